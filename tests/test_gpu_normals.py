"""vdn.normals on the device (csrc/normals.hip) against the CPU restatement tests/normal_ref.py at the shapes where the
kernels can go wrong, and against the reference's recorded values (tests/golden/normal_cases.npz).

Bars. Against the restatement: the loss and each per-frame mean within 1e-9 absolute (a naive fp64 sum of 1.1e6 terms in
[-1, 1] has a worst-case mean error of about 1.2e-10), counts exact, NaN meets NaN. Against the recorded reference values:
2e-6 (the reference computes in float32; tests/test_normals_host.py). normal_vector and sobel_ix_iy: equal to the fp64
restatement rounded to float32, allowing 1 ulp. VideoNormalLoss.forward returns a float32 tensor, whose rounding alone (up to
3e-8 at a loss of 0.5) is above 1e-9: the fp64 value of the same launch is read through normal_loss, and forward's tensor
must be that value rounded to float32.
tools/normal_bench.py measures the differences behind these bars and writes them to profiles/normal_eval.md."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import normal_ref as R
from test_normals_host import CASES, LOSS_ATOL, case_inputs, normals_bar, recorded_normals

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL = 1e-9
# the reflect pad at its smallest | 3 x 3 | odd, less than a wave | one pixel per lane over several blocks (H * W odd) |
# four pixels per lane, odd width: quads and stencil rows straddle rows and blocks | the model's frame | the large frame
SHAPES = [(1, 2, 2), (2, 3, 3), (2, 5, 7), (2, 37, 53), (3, 64, 257), (1, 224, 224), (1, 518, 518)]


@functools.lru_cache(maxsize=None)
def inputs(shape, masked):
    """Seeded inputs, shared between tests and never written."""
    F, H, W = shape
    c = R.make_case(5000 + F + H + W, (1, F, H, W), "bool" if masked else "none", "scaled",
                    false_rate=0.15 if H * W < 64 else 0.05)
    for a in c.values():
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(shape, masked, from_depth):
    c = inputs(shape, masked)
    return R.normal_loss_ref(c["pred"], c["depth"] if from_depth else c["target"], c["mask"] if masked else None, from_depth)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def agree(got, want, what):
    """The issue's bar on (loss, per-frame mean, per-frame count); prints the figures before asserting."""
    loss, mean, count = got[0], got[1].numpy(), got[2].numpy()
    nan = np.isnan(want[1])
    worst = float(np.abs(mean[~nan] - want[1][~nan]).max()) if (~nan).any() else 0.0
    print(f"[{what}] loss {loss!r} vs {want[0]!r}: diff {abs(loss - want[0]):.2e}; per-frame mean max diff {worst:.2e}; "
          f"counts {count.ravel().tolist()}")
    assert mean.dtype == np.float64 and count.dtype == np.int64
    assert np.array_equal(count, want[2])
    assert np.array_equal(np.isnan(mean), nan)
    assert abs(loss - want[0]) <= ATOL and worst <= ATOL


def run(c, from_depth, masked=True, **kw):
    from vdn import normals as N
    fn = N.normal_loss_from_depth if from_depth else N.normal_loss
    return fn(dev(c["pred"]), dev(c["depth"] if from_depth else c["target"]), dev(c["mask"]) if masked else None, **kw)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("from_depth", [False, True], ids=["normals", "depth"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_matches_the_restatement(shape, from_depth, masked):
    got = run(inputs(shape, masked), from_depth, masked, per_frame=True)
    agree(got, reference(shape, masked, from_depth), f"{shape} depth={from_depth} mask={masked}")
    if shape == (1, 2, 2) and not masked:
        assert got[2].item() == 4                       # all four pixels of the smallest frame are kept


@pytest.mark.parametrize("c", CASES, ids=lambda c: f"seed{c['seed']}-{c['mask_kind']}-{c['target_kind']}")
def test_loss_matches_the_recorded_reference(c):
    from vdn import normals as N
    case = case_inputs(c)
    pred, target, depth, mask = (dev(case[k]) for k in ("pred", "target", "depth", "mask"))
    out = N.VideoNormalLoss()(pred, target, mask)["normal_loss"]
    assert out.is_cuda and out.dim() == 0 and out.dtype == torch.float32
    stored, from_depth = float(out), N.normal_loss_from_depth(pred, depth, mask)
    print(f"forward {stored!r} vs {c['expected']!r}: {stored - c['expected']:+.2e}; from depth {from_depth!r} vs "
          f"{c['expected_depth']!r}: {from_depth - c['expected_depth']:+.2e}")
    assert abs(stored - c["expected"]) <= LOSS_ATOL and abs(from_depth - c["expected_depth"]) <= LOSS_ATOL
    want = R.normal_loss_ref(case["pred"], case["depth"], case["mask"], True)[0]
    assert abs(from_depth - want) <= ATOL
    if c["mask_kind"] == "none":                         # absent = all true
        assert N.normal_loss_from_depth(pred, depth, None) == from_depth


def test_misaligned_planes_take_the_one_pixel_path():
    """H * W is a multiple of 4 but pred starts 4 bytes past a 16-byte boundary: float loads, same result to the bar."""
    from vdn import normals as N
    shape = (3, 64, 257)
    c = inputs(shape, True)
    flat = torch.empty(c["pred"].size + 1, dtype=torch.float32, device=DEV)
    pred = flat[1:].view(c["pred"].shape)
    pred.copy_(dev(c["pred"]))
    assert pred.data_ptr() % 16 == 4 and pred.is_contiguous()
    for from_depth in (False, True):
        got = (N.normal_loss_from_depth if from_depth else N.normal_loss)(
            pred, dev(c["depth"] if from_depth else c["target"]), dev(c["mask"]), per_frame=True)
        agree(got, reference(shape, True, from_depth), f"misaligned depth={from_depth}")


def test_erosion_geometry():
    from vdn import normals as N
    H, W = 6, 9
    loss = N.VideoNormalLoss()
    ones = torch.ones(1, 4, H, W, dtype=torch.bool, device=DEV)
    m = ones.clone()
    m[0, 1, 0, 0] = m[0, 2, 0, 4] = m[0, 3, 3, 4] = False      # a corner, an edge, the interior
    keep = loss.eroded_mask(m)
    assert keep.dtype == torch.bool and keep.shape == m.shape and keep.is_cuda
    assert np.array_equal(keep.cpu().numpy(), R.erode_ref(m.cpu().numpy()))
    assert (~keep).sum((-1, -2)).ravel().tolist() == [0, 4, 6, 9]
    assert bool(loss.eroded_mask(ones).all())                   # an all-true mask keeps the whole border
    c = R.make_case(77, (1, 4, H, W))
    _, _, count = N.normal_loss_from_depth(dev(c["pred"]), dev(c["depth"]), m, per_frame=True)
    assert count.ravel().tolist() == [H * W, H * W - 4, H * W - 6, H * W - 9]
    for kind in (torch.float32, torch.uint8, torch.int64):      # non-zero = use, whatever the type
        assert torch.equal(loss.eroded_mask(m.to(kind) * 3), keep)


def test_empty_masks():
    from vdn import normals as N
    shape = (4, 37, 53)
    c = inputs(shape, True)
    zero = torch.zeros(1, *shape, dtype=torch.bool, device=DEV)
    for from_depth in (False, True):
        loss, mean, count = run(dict(c, mask=zero.cpu().numpy()), from_depth, per_frame=True)
        assert loss == 1.0 and count.sum().item() == 0 and bool(mean.isnan().all())
    assert float(N.VideoNormalLoss()(dev(c["pred"]), dev(c["target"]), zero)["normal_loss"]) == 1.0
    # one fully masked frame of several: its mean is NaN, and the loss is that of the other frames
    mask = c["mask"].copy()
    mask[0, 2] = False
    for from_depth in (False, True):
        got = run(dict(c, mask=mask), from_depth, per_frame=True)
        agree(got, R.normal_loss_ref(c["pred"], c["depth"] if from_depth else c["target"], mask, from_depth), "one empty frame")
        assert bool(got[1][0, 2].isnan()) and got[2][0, 2].item() == 0
        rest = [0, 1, 3]
        sub = {k: np.ascontiguousarray(v[:, rest]) for k, v in dict(c, mask=mask).items()}
        assert run(sub, from_depth) == got[0]           # adding a frame's 0.0 changes no bit of the sum


def test_non_finite_values_under_dropped_pixels_reach_nothing():
    from vdn import normals as N
    shape = (2, 37, 53)
    c = inputs(shape, True)
    keep = R.erode_ref(c["mask"])
    assert 0.25 < keep.mean() < 0.9
    pred, depth, target = c["pred"].copy(), c["depth"].copy(), c["target"].copy()
    poison = np.array([np.nan, np.inf, -np.inf], np.float32)
    drop = np.broadcast_to(~keep[:, :, None], pred.shape)
    pred[drop] = poison[np.arange(drop.sum()) % 3]
    target[drop] = poison[(1 + np.arange(drop.sum())) % 3]
    unused = ~c["mask"]                                  # a kept pixel's stencil reads eroded neighbours, never masked ones
    depth[unused] = poison[np.arange(unused.sum()) % 3]
    for from_depth in (False, True):
        clean = run(c, from_depth, per_frame=True)
        dirty = run(dict(c, pred=pred, depth=depth, target=target), from_depth, per_frame=True)
        assert np.isfinite(clean[0]) and dirty[0] == clean[0]
        assert torch.equal(dirty[1], clean[1]) and torch.equal(dirty[2], clean[2])
    # under a kept pixel a NaN is a NaN
    y, x = np.argwhere(keep[0, 1])[0]
    bad = c["pred"].copy()
    bad[0, 1, 2, y, x] = np.nan
    loss, mean, _ = run(dict(c, pred=bad), True, per_frame=True)
    assert np.isnan(loss) and bool(mean[0, 1].isnan()) and not bool(mean[0, 0].isnan())
    bad_depth = c["depth"].copy()
    bad_depth[0, 1, y, x + 1 if x + 1 < shape[2] else x - 1] = np.nan
    assert np.isnan(run(dict(c, depth=bad_depth), True))


def test_zero_prediction_vector_contributes_cosine_zero():
    from vdn import normals as N
    c = R.make_case(78, (1, 1, 2, 2))
    for from_depth in (False, True):
        loss, mean, count = run(dict(c, pred=np.zeros_like(c["pred"])), from_depth, masked=False, per_frame=True)
        assert loss == 1.0 and mean.item() == 0.0 and count.item() == 4
    shape = (2, 37, 53)
    c = inputs(shape, False)
    pred = c["pred"].copy()
    pred[0, 0, :, 10:20, 7:30] = 0.0
    agree(run(dict(c, pred=pred), True, masked=False, per_frame=True),
          R.normal_loss_ref(pred, c["depth"], None, True), "zero vectors")


def one_ulp(got, want64, what):
    want = want64.astype(np.float32)
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    exact = float((got == want).mean())
    print(f"[{what}] {exact:.4%} of the values equal the rounded restatement; max diff {diff.max():.2e}")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert (diff <= np.spacing(np.abs(want)).astype(np.float64)).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_normal_vector_and_sobel_match_the_restatement(shape):
    from vdn import normals as N
    d = inputs(shape, False)["depth"]
    img = dev(d)[:, :, None]
    n = N.normal_vector(img)
    assert n.shape == (1, shape[0], 3, *shape[1:]) and n.is_cuda
    one_ulp(n.cpu().numpy(), R.normal_vector_ref(d), f"normal_vector {shape}")
    ix, iy = N.sobel_ix_iy(img)
    assert ix.shape == iy.shape == img.shape
    wx, wy = R.sobel_ref(d)
    one_ulp(ix.cpu().numpy()[:, :, 0], wx, f"Ix {shape}")
    one_ulp(iy.cpu().numpy()[:, :, 0], wy, f"Iy {shape}")


def test_normal_vector_arguments_and_recorded_normals():
    from vdn import normals as N
    d = inputs((2, 37, 53), False)["depth"]
    img = dev(d)[:, :, None]
    for kw in (dict(normalize_kernel=False), dict(scale_xy=2.5, scale_z=0.3), dict(eps=1e-2, scale_z=0.0),
               dict(normalize_kernel=False, scale_xy=0.1, scale_z=4.0, eps=0.5)):
        one_ulp(N.normal_vector(img, **kw).cpu().numpy(), R.normal_vector_ref(d, **kw), f"normal_vector {kw}")
    wx, wy = R.sobel_ref(d, normalize_kernel=False)
    ix, iy = N.sobel_ix_iy(img, normalize_kernel=False)
    one_ulp(ix.cpu().numpy()[:, :, 0], wx, "Ix, kernel not divided")
    one_ulp(iy.cpu().numpy()[:, :, 0], wy, "Iy, kernel not divided")
    for depth, args, want in recorded_normals():
        got = N.normal_vector(dev(depth)[:, :, None], **args).cpu().numpy()
        diff = float(np.abs(got - want).max())
        print(f"recorded normals {depth.shape}: max abs diff {diff:.2e}, bar {normals_bar(depth):.2e}")
        assert diff <= normals_bar(depth)


def test_forward_equals_the_fused_path():
    """Given vdn.normals.normal_vector(gt) as target, the stored-target path differs from the fused one only by the float32
    rounding of the stored target: 3 * 2^-24 per cosine at most, of either sign. The bar is on the mean, where n independent
    roundings shrink as 1 / sqrt(n), so the shapes are the two with tens of thousands of kept pixels."""
    from vdn import normals as N
    for shape in ((3, 64, 257), (1, 224, 224)):
        c = inputs(shape, True)
        pred, depth, mask = dev(c["pred"]), dev(c["depth"]), dev(c["mask"])
        target = N.normal_vector(depth[:, :, None])
        fused = N.normal_loss_from_depth(pred, depth, mask)
        stored = N.normal_loss(pred, target, mask)
        out = N.VideoNormalLoss()(pred, target, mask)["normal_loss"]
        print(f"{shape}: fused {fused!r} stored {stored!r} diff {abs(fused - stored):.2e}; forward {float(out)!r}")
        assert abs(fused - stored) <= ATOL
        assert out.dtype == torch.float32 and out.is_cuda and float(out) == float(np.float32(stored))


def test_batches_views_and_untouched_inputs():
    from vdn import normals as N
    B, T, H, W = 2, 3, 37, 53
    c = R.make_case(79, (B, T, H, W), "bool", "scaled")
    want = R.normal_loss_ref(c["pred"], c["depth"], c["mask"], True)
    want_stored = R.normal_loss_ref(c["pred"], c["target"], c["mask"])
    agree(N.normal_loss_from_depth(dev(c["pred"]), dev(c["depth"]), dev(c["mask"]), per_frame=True), want, "B = 2")
    agree(N.normal_loss_from_depth(dev(c["pred"]), dev(c["depth"])[:, :, None], dev(c["mask"]), per_frame=True), want, "[B,T,1,H,W]")
    # channels-last storage, a cropped depth and a strided mask: views that are not contiguous
    pred = dev(c["pred"]).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    target = dev(c["target"]).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    wide = torch.full((B, T, H, W + 5), -777.0, device=DEV)
    wide[..., 2:W + 2] = dev(c["depth"])
    depth = wide[..., 2:W + 2]
    two = torch.zeros(B, T, H, 2 * W, dtype=torch.bool, device=DEV)
    two[..., ::2] = dev(c["mask"])
    mask = two[..., ::2]
    assert not (pred.is_contiguous() or depth.is_contiguous() or mask.is_contiguous())
    keep = [t.clone() for t in (pred, target, wide, two)]
    agree(N.normal_loss_from_depth(pred, depth, mask, per_frame=True), want, "views, from depth")
    agree(N.normal_loss(pred, target, mask, per_frame=True), want_stored, "views, stored target")
    out = N.VideoNormalLoss()(pred, target, mask)["normal_loss"]
    assert float(out) == float(np.float32(N.normal_loss(pred, target, mask)))
    one_ulp(N.normal_vector(depth[:, :, None]).cpu().numpy(), R.normal_vector_ref(c["depth"]), "normal_vector of a view")
    for before, after in zip(keep, (pred, target, wide, two)):
        assert torch.equal(before, after)
    # host tensors are copied once and give the same bits
    assert N.normal_loss_from_depth(torch.from_numpy(c["pred"]), torch.from_numpy(c["depth"]), torch.from_numpy(c["mask"])) == \
        N.normal_loss_from_depth(dev(c["pred"]), dev(c["depth"]), dev(c["mask"]))


def test_two_runs_give_the_same_bits():
    from vdn import normals as N
    for shape in ((3, 64, 257), (1, 518, 518)):
        c = inputs(shape, True)
        for from_depth in (False, True):
            a, b = run(c, from_depth, per_frame=True), run(c, from_depth, per_frame=True)
            assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    d = dev(inputs((3, 64, 257), False)["depth"])[:, :, None]
    assert torch.equal(N.normal_vector(d), N.normal_vector(d))


def test_errors_on_device_tensors():
    from vdn import normals as N
    p, d, m = torch.ones(1, 2, 3, 4, 5, device=DEV), torch.ones(1, 2, 4, 5, device=DEV), torch.ones(1, 2, 4, 5, device=DEV)
    with pytest.raises(ValueError, match="at least 2"):
        N.normal_loss_from_depth(p[:, :, :, :1], d[:, :, :1], m[:, :, :1])
    with pytest.raises(ValueError, match="at least 2"):
        N.normal_vector(d[:, :, None, :1])
    with pytest.raises(ValueError, match="target"):
        N.VideoNormalLoss()(p, p[..., :4], m)
    with pytest.raises(ValueError, match="mask"):
        N.VideoNormalLoss()(p, p, m[:, :1])
    with pytest.raises(NotImplementedError):
        N.VideoNormalLoss(reduction="image-based")
