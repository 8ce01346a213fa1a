"""vdn.normal_metrics, vdn.vis.colorize_normals and vdn.steps.evaluate_normals_step on the device (csrc/normal_metrics.hip)
against the CPU restatement tests/normal_angle_ref.py, at the shapes where the kernels can go wrong.

Bars (against the restatement, float64 numpy):
  n         equal.
  map       |got - want| <= 2^-23 want + 1e-30: one float32 rounding of an fp64 value that two libms may leave a few fp64 ulp
            apart; NaN where and only where the restatement has one.
  mean,     <= 1e-8 degrees: the worst-case error of an fp64 sum of n <= 66820 angles up to 180 is n 2^-53 180 = 1.4e-9; an
  rmse      error of float32 kind is 1e-5 or more.
  median    <= 2^-23 want: one float32 ulp, for an fp64 angle that the two sides round to float32 across a boundary.
  shares    equal; the test first asserts, on the restatement, that no kept angle lies within 1e-6 degrees of a threshold (a
            condition on the seeded inputs, not a tolerance).
  picture   byte for byte; the test first asserts that no v_c of the restatement lies within 1e-9 of a half-integer (but for
            components that are exactly zero, whose v_c is exactly 127.5 on both sides).
Inputs are normal_angle_ref.make_case: exactly rounded operations, predictions turned 0 .. 58.7 degrees from the target."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import normal_angle_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL32 = 2.0 ** -23


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def case(seed, shape, keep_rate=0.7):
    """Seeded inputs, shared between tests and never written."""
    c = A.make_case(seed, shape, keep_rate)
    for a in c.values():
        a.setflags(write=False)
    return c


def restate(pred, target, mask, from_depth=False, erode=True):
    """-> (angles with NaN at dropped pixels, rows), after the condition on the inputs that makes the shares exact."""
    ang, keep = A.angle_map_ref(pred, target, mask, from_depth, erode)
    kept = ang[keep]
    kept = kept[~np.isnan(kept)]
    for t in A.THRESHOLDS:
        assert kept.size == 0 or np.abs(kept - t).min() > 1e-6, f"an angle within 1e-6 of {t}: choose another seed"
    return ang, A.stats_ref(ang, keep)


def run(pred, target, mask, from_depth=False, erode=True):
    """-> (map float32 [B, T, H, W], rows float64 [1 + B + B T, 9]) as numpy, from the public functions."""
    from vdn import normal_metrics as M
    kw = dict(from_depth=from_depth, erode=erode)
    m = M.angular_error_map(pred, target, mask, **kw)
    r = M.angular_error(pred, target, mask, **kw)
    B, T = m.shape[:2]
    assert m.dtype == torch.float32 and m.is_cuda and tuple(m.shape) == tuple(pred.shape[:2]) + tuple(pred.shape[3:])
    assert set(r) == {"batch", "items", "frames"} and all(v.dtype == torch.float64 and v.is_cuda for v in r.values())
    assert tuple(r["batch"].shape) == (9,) and tuple(r["items"].shape) == (B, 9) and tuple(r["frames"].shape) == (B, T, 9)
    rows = torch.cat([r["batch"][None], r["items"], r["frames"].reshape(B * T, 9)]).cpu().numpy()
    return m.cpu().numpy(), rows


def agree(got, want, what):
    """The bars of the module's docstring on (map, rows); prints the figures before asserting."""
    (gmap, grows), (wang, wrows) = got, want
    nan = np.isnan(wang)
    g, w = gmap.astype(np.float64)[~nan], wang[~nan]
    map_excess = float((np.abs(g - w) - (REL32 * w + 1e-30)).max()) if w.size else -1.0
    rn = np.isnan(wrows)
    diff = np.where(rn, 0.0, np.abs(grows - np.where(rn, 0.0, wrows)))
    print(f"[{what}] n {grows[:3, 0].tolist()} map worst rel {float((np.abs(g - w) / np.maximum(w, 1e-300)).max()) if w.size else 0:.2e} "
          f"mean {diff[:, 1].max():.2e} median rel {float((diff[:, 2] / np.where(rn[:, 2], 1.0, np.maximum(wrows[:, 2], 1e-300))).max()):.2e} "
          f"rmse {diff[:, 3].max():.2e} shares {diff[:, 4:].max():.2e}")
    assert np.array_equal(np.isnan(gmap), nan)
    assert map_excess <= 0.0
    assert np.array_equal(np.isnan(grows), rn)
    assert np.array_equal(grows[:, 0], wrows[:, 0])
    assert diff[:, 1].max() <= 1e-8 and diff[:, 3].max() <= 1e-8
    assert (diff[:, 2] <= REL32 * np.where(rn[:, 2], 0.0, wrows[:, 2])).all()
    assert diff[:, 4:].max() == 0.0


def check(pred, target, mask, what, from_depth=False, erode=True):
    want = restate(pred, target, mask, from_depth, erode)
    got = run(dev(pred), dev(target), None if mask is None else dev(mask), from_depth, erode)
    agree(got, want, what)
    return got, want


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("from_depth", [False, True], ids=["stored", "from_depth"])
@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (1, 1, 3, 5)], ids=lambda s: "x".join(map(str, s)))
def test_smallest(shape, from_depth):
    """Even and odd n, the reflect pad at its minimum; no mask."""
    c = case(2, shape)
    (_, rows), _ = check(c["pred"], c["depth"] if from_depth else c["target"], None, f"smallest {shape}", from_depth)
    assert rows[0, 0] == shape[2] * shape[3]


@pytest.mark.parametrize("shape", [(1, 2, 7, 9), (1, 2, 6, 10)], ids=lambda s: "x".join(map(str, s)))
def test_ragged_pointer_strided_target_float_mask(shape):
    """A prediction that starts one float past a 16-byte boundary, a target that is a strided view and a float mask: the same
    bits as the aligned contiguous call (H W odd: one pixel per lane; H W a multiple of 4: four, by a load each)."""
    from vdn import normal_metrics as M
    c = case(5, shape, 0.9)
    mask = c["mask"].astype(np.float32)
    (gmap, grows), _ = check(c["pred"], c["target"], mask, f"ragged {shape}")
    flat = torch.empty(c["pred"].size + 1, dtype=torch.float32, device=DEV)
    pred = flat[1:].view(c["pred"].shape)
    pred.copy_(dev(c["pred"]))
    assert pred.data_ptr() % 16 == 4 and pred.is_contiguous()
    wide = torch.zeros(c["target"].shape[:-1] + (2 * shape[3],), dtype=torch.float32, device=DEV)
    target = wide[..., ::2]
    target.copy_(dev(c["target"]))
    assert not target.is_contiguous()
    omap, orows = run(pred, target, dev(mask))
    assert omap.tobytes() == gmap.tobytes() and orows.tobytes() == grows.tobytes()
    dmap = M.angular_error_map(pred, dev(c["depth"]), dev(mask), from_depth=True).cpu().numpy()
    amap = M.angular_error_map(dev(c["pred"]), dev(c["depth"]), dev(mask), from_depth=True).cpu().numpy()
    assert dmap.tobytes() == amap.tobytes()


@pytest.mark.parametrize("from_depth", [False, True], ids=["stored", "from_depth"])
def test_past_one_trip(from_depth):
    """260 x 257 = 66820 pixels, a multiple of 4: more than the 65536 that one trip of a frame's 64 blocks covers at four
    pixels per lane, and more than one trip of the select's grid."""
    c = case(7, (1, 1, 260, 257), 0.9)
    check(c["pred"], c["depth"] if from_depth else c["target"], c["mask"], "past one trip", from_depth)


@pytest.mark.parametrize("shape", [(1, 300, 4, 5), (300, 1, 3, 4)], ids=lambda s: "x".join(map(str, s)))
def test_many_frames_and_items(shape):
    """More frames, and more items, than the 256 lanes of the one-block fold; B T rows."""
    c = case(13, shape, 0.9)
    (_, rows), _ = check(c["pred"], c["target"], c["mask"], f"many {shape}", erode=False)
    assert rows.shape == (1 + shape[0] + shape[0] * shape[1], 9)
    check(c["pred"], c["target"], None, f"many {shape} eroded")


# ------------------------------------------------------------------------------------------------ masks, NaN
@functools.lru_cache(maxsize=None)
def masked_case():
    """[2, 3, 12, 14] at keep rate 0.7: frame (0, 1) and item 1 all dropped, NaN and inf under dropped pixels."""
    c = case(11, (2, 3, 12, 14))
    mask = c["mask"].copy()
    mask[0, 1] = False
    mask[1] = False
    keep = A.R.erode_ref(mask)
    pred, target = c["pred"].copy(), c["target"].copy()
    drop = np.broadcast_to(~mask[:, :, None], pred.shape)               # dropped before the erosion: dropped either way
    pred[drop & (np.arange(pred.size).reshape(pred.shape) % 3 == 0)] = np.nan
    target[drop & (np.arange(pred.size).reshape(pred.shape) % 3 == 1)] = np.inf
    for a in (pred, target, mask, keep):
        a.setflags(write=False)
    return pred, target, mask, keep


def test_masks_empty_sets_and_poison_under_dropped_pixels():
    pred, target, mask, keep = masked_case()
    (gmap, rows), _ = check(pred, target, mask, "masks")
    B, T = 2, 3
    assert rows[1 + B + 1, 0] == 0 and np.isnan(rows[1 + B + 1, 1:]).all()          # frame (0, 1)
    assert rows[2, 0] == 0 and np.isnan(rows[2, 1:]).all()                          # item 1
    assert np.isnan(rows[1 + B + 3:, 1:]).all() and (rows[1 + B + 3:, 0] == 0).all()
    for r in (0, 1, 1 + B, 1 + B + 2):
        assert rows[r, 0] > 0 and not np.isnan(rows[r]).any()
    assert np.array_equal(rows[0], rows[1])                                        # the batch is item 0
    (pmap, plain), _ = check(pred, target, mask, "masks, erode=False", erode=False)
    assert plain[0, 0] > rows[0, 0] and plain[0, 0] == mask.sum()                   # the erosion drops border and neighbour pixels
    assert np.array_equal(pmap[keep], gmap[keep])


def test_nan_under_a_kept_pixel_poisons_its_sets_alone():
    pred, target, mask, keep = masked_case()
    _, clean = run(dev(pred), dev(target), dev(mask))
    y, x = np.argwhere(keep[0, 2])[0]
    poisoned = pred.copy()
    poisoned[0, 2, 1, y, x] = np.nan
    (_, rows), _ = check(poisoned, target, mask, "NaN kept")
    B = 2
    bad = [0, 1, 1 + B + 2]                                                        # the batch, item 0, frame (0, 2)
    assert np.array_equal(rows[:, 0], clean[:, 0])
    assert np.isnan(rows[bad, 1:]).all() and not np.isnan(clean[bad]).any()
    rest = np.setdiff1d(np.arange(rows.shape[0]), bad)
    assert rows[rest].tobytes() == clean[rest].tobytes()


@pytest.mark.parametrize("kind", ["zero degrees", "180 degrees", "zero vector", "equal angles"])
def test_constant_fields_select_with_every_key_tied(kind):
    shape = (1, 2, 5, 6)
    c = case(17, shape)
    target = c["target"]
    if kind == "zero degrees":
        pred, angle = target * np.float32(2.0), 0.0
    elif kind == "180 degrees":
        pred, angle = target * np.float32(-0.5), 180.0
    elif kind == "zero vector":
        pred, angle = np.zeros_like(target), 90.0
    else:
        pred, target = np.empty_like(target), np.empty_like(target)
        pred[:], target[:] = np.float32([1, 2, 2]).reshape(3, 1, 1), np.float32([2, -1, 3]).reshape(3, 1, 1)
        angle = None
    (gmap, rows), (wang, _) = check(pred, target, None, kind)
    kept = ~np.isnan(wang)
    assert kept.all()
    if angle is not None:
        assert (gmap[kept] == np.float32(angle)).all()
        assert rows[0, 1] == angle and rows[0, 2] == angle and abs(rows[0, 3] - angle) <= 1e-13 * max(angle, 1.0)
    assert np.unique(gmap[kept]).size == 1 and (rows[:, 2] == np.float64(gmap[kept][0])).all()


def test_tiny_angles_keep_their_digits():
    """target + a perturbation of 1e-7: angles of about 1e-5 degrees, where acos of a cosine returns 0 or noise. The map's
    relative error stays within 2^-22."""
    from vdn import normal_metrics as M
    c = case(19, (1, 2, 9, 11))
    target = c["target"]
    pred = (target.astype(np.float64) + 1e-7 * (c["pred"].astype(np.float64) - 0.5)).astype(np.float32)
    want, keep = A.angle_map_ref(pred, target, None, erode=False)
    assert keep.all() and want.max() < 1e-3 and (want > 0).sum() > 0.9 * want.size
    got = M.angular_error_map(dev(pred), dev(target), None, erode=False).cpu().numpy().astype(np.float64)
    rel = np.abs(got - want)[want > 0] / want[want > 0]
    print(f"tiny angles {want.min():.3e} .. {want.max():.3e} degrees: worst relative error {rel.max():.3e}")
    assert rel.max() <= 2.0 ** -22 and (got[want == 0] == 0).all()


def test_from_depth_against_the_stored_unit_normals():
    """from_depth equals the restatement (bars above) and agrees with the explicit target normal_vector(depth) to 1e-4
    degrees, not to the bit: that target was rounded to float32."""
    from vdn.normals import normal_vector
    c = case(23, (1, 2, 11, 13), 0.9)
    (gmap, rows), _ = check(c["pred"], c["depth"], c["mask"], "from_depth", from_depth=True)
    stored = normal_vector(dev(c["depth"])[:, :, None])
    smap, srows = run(dev(c["pred"]), stored, dev(c["mask"]))
    kept = ~np.isnan(gmap)
    worst = float(np.abs(gmap[kept].astype(np.float64) - smap[kept]).max())
    print(f"from_depth vs stored normals: map {worst:.2e} degrees, mean {abs(rows[0, 1] - srows[0, 1]):.2e}")
    assert np.array_equal(np.isnan(smap), ~kept) and worst <= 1e-4 and np.abs(rows[:, 1:4] - srows[:, 1:4]).max() <= 1e-4


# ------------------------------------------------------------------------------------------------ runs, values
def test_two_runs_give_the_same_bits_and_values_are_lists():
    from vdn import normal_metrics as M, vis
    c = case(11, (2, 3, 12, 14))
    args = (dev(c["pred"]), dev(c["target"]), dev(c["mask"]))
    a, b = run(*args), run(*args)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    vals = M.angular_error_values(*args)
    assert isinstance(vals["batch"], list) and len(vals["batch"]) == 9 and len(vals["items"]) == 2 and len(vals["frames"][1]) == 3
    assert np.array(vals["batch"]).tobytes() == a[1][0].tobytes() and np.array(vals["frames"]).tobytes() == a[1][3:].tobytes()
    p = args[0].clone().requires_grad_(True)                                       # a score: detached, nothing recorded
    r = M.angular_error(p, args[1], args[2])
    assert not r["batch"].requires_grad and r["batch"].cpu().numpy().tobytes() == a[1][0].tobytes()
    x = dev(c["pred"]).view(6, 3, 12, 14)
    assert vis.colorize_normals(x).cpu().numpy().tobytes() == vis.colorize_normals(x).cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ the picture
def picture_inputs(x, from_depth):
    """The restatement's bytes, after the condition on the inputs that makes them exact: no v_c within 1e-9 of a half-integer.
    A component that is exactly zero is left out of the condition: its v_c is 0 / |a| * 0.5 + 0.5 = 127.5 with no rounding on
    either side (every border column and row of a from_depth picture is one: the reflect pad makes Ix or Iy zero there)."""
    want, v = A.colorize_ref(x, from_depth)
    a = np.moveaxis(A.depth_normal_ref(x) if from_depth else np.asarray(x, np.float64), 1, -1)
    frac = np.abs(v - np.floor(v) - 0.5)[(a != 0) & ~np.isnan(v)]
    assert frac.min() > 1e-9, "a v_c within 1e-9 of a half-integer: choose another seed"
    assert (want[(a == 0) & ~np.isnan(v)] == 128).all()
    return want


@pytest.mark.parametrize("shape", [(2, 7, 9), (3, 6, 10), (1, 64, 67)], ids=lambda s: "x".join(map(str, s)))
def test_picture_bytes(shape):
    from vdn import vis
    N, H, W = shape
    c = case(29, (1, N, H, W))
    x = c["pred"][0].copy()
    x[0, :, 0, 0] = 0.0                                                             # a zero vector, NaN and inf: grey
    x[0, 1, 1, 1] = np.nan
    x[N - 1, 2, H - 1, W - 1] = -np.inf
    want = picture_inputs(x, False)
    assert want[0, 0, 0].tolist() == [128] * 3 and want[0, 1, 1].tolist() == [128] * 3 and want[N - 1, H - 1, W - 1].tolist() == [128] * 3
    got = vis.colorize_normals(dev(x))
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (N, H, W, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(vis.colorize_normals(dev(x), order="bgr").cpu().numpy(), want[..., ::-1])
    five = vis.colorize_normals(dev(x)[None])
    assert tuple(five.shape) == (1, N, H, W, 3) and np.array_equal(five[0].cpu().numpy(), want)
    flat = torch.empty(x.size + 1, dtype=torch.float32, device=DEV)               # one float past 16 bytes
    off = flat[1:].view(x.shape)
    off.copy_(dev(x))
    assert np.array_equal(vis.colorize_normals(off).cpu().numpy(), want)
    depth = c["depth"][0]
    dwant = picture_inputs(depth, True)
    dgot = vis.colorize_normals(dev(depth), from_depth=True)
    assert tuple(dgot.shape) == (N, H, W, 3) and np.array_equal(dgot.cpu().numpy(), dwant)
    assert np.array_equal(vis.colorize_normals(dev(depth)[None, :, None], from_depth=True)[0].cpu().numpy(), dwant)


def test_picture_from_depth_against_stored_normals():
    """colorize_normals(from_depth) against colorize_normals(normal_vector(depth)): the bytes differ only where the float32
    rounding of the stored normals crosses a half-integer, fewer than 1e-4 of them."""
    from vdn import vis
    from vdn.normals import normal_vector
    depth = dev(A.make_depth(29, (1, 2, 64, 67)))
    a = vis.colorize_normals(depth, from_depth=True).cpu().numpy()
    b = vis.colorize_normals(normal_vector(depth[:, :, None])).cpu().numpy()
    differ = int((a != b).sum())
    print(f"bytes that differ: {differ} of {a.size}")
    assert a.shape == b.shape == (1, 2, 64, 67, 3) and differ <= 1e-4 * a.size
    assert int(np.abs(a.astype(int) - b.astype(int)).max()) <= 1


# ------------------------------------------------------------------------------------------------ the loop body
def test_evaluate_normals_step_and_meter():
    from vdn import normal_metrics as M, steps
    from vdn.normals import sobel_ix_iy
    B, S, H, W = 2, 3, 10, 12

    def model(d, rgb):
        ix, iy = sobel_ix_iy(d[:, :, None])
        return d, torch.cat([-ix, -iy, torch.ones_like(ix)], dim=2)

    rng = np.random.default_rng(31)
    batches = []
    for _ in range(2):
        b = {"rgb": rng.uniform(0, 1, (B, S, 3, H, W)).astype(np.float32),
             "depth_anything_v2": rng.uniform(0.5, 10.0, (B, S, 1, H, W)).astype(np.float32),
             "depth": rng.uniform(0.5, 20.0, (B, S, 1, H, W)).astype(np.float32),
             "mask": rng.random((B, S, 1, H, W)) < 0.9}
        batches.append({k: torch.from_numpy(v).to(DEV) for k, v in b.items()})
    meter = steps.MetricMeter()
    rows, want = [], []
    for batch in batches:
        r = steps.evaluate_normals_step(model, batch, meter=meter)
        assert r.dtype == torch.float64 and r.is_cuda and tuple(r.shape) == (B, 9)
        rows.append(r.cpu().numpy())
        t = steps.prepare_batch(batch)
        _, normals = model(t["input_depth"], t["rgb"])
        want.append(M.angular_error(normals, t["gt"], t["mask"], from_depth=True)["items"].cpu().numpy())
        ang, keep = A.angle_map_ref(normals.cpu().numpy(), t["gt"].cpu().numpy(), t["mask"].cpu().numpy(), from_depth=True)
        ref = A.stats_ref(ang, keep)[1:1 + B]
        assert np.array_equal(rows[-1][:, 0], ref[:, 0]) and np.abs(rows[-1][:, 1:4] - ref[:, 1:4]).max() <= 1e-5
    rows, want = np.concatenate(rows), np.concatenate(want)
    assert rows.tobytes() == want.tobytes() and not np.isnan(rows).any() and (rows[:, 0] > 0).all()
    plain = steps.evaluate_normals_step(model, batches[0], erode=False).cpu().numpy()
    assert (plain[:, 0] > rows[:B, 0]).all()
    got, mean = meter.means(), np.nanmean(rows, axis=0)
    assert len(got) == 9 and meter.rows == 2 * B
    for g, w in zip(got, mean):
        print(f"{g!r} vs {w!r}")
        assert abs(g - w) <= 2 * np.spacing(abs(w))
