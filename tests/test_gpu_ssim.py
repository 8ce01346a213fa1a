"""The SSIM term of the depth criterion on the device (csrc/ssim.hip, vdn.loss) against the CPU restatement tests/ssim_ref.py
at the sizes where the kernels can go wrong, then the classes at the 161-pixel cases of tests/golden/ssim_cases.npz. The
sizes: frames around one tile, then (PAST_ONE_RING) frames whose inner tiles have all four neighbours, frames past one trip
of the sweeps on either path with rows that end inside a lane's quad, more tiles than the fold has lanes, and an item's
maximum on a lane's second trip. Tile and trip are the library's own figures (vdn.loss.ssim_tile, vdn.loss.trip_pixels).

Bars.
Value: |got - want| <= 1e-10, for the loss and every frame's cs. A cs pixel is a quotient whose denominator is at least C2 =
9e-4 and whose terms are fp64 sums of 121 products of values in [0, 1]: about 50 ulp(1) / C2 = 6e-12 per pixel, which the mean
does not grow. An error of float32 kind is 1e-7.
Gradient, per element: |got - want| <= 4 * 2^-24 * mag + 8 * floor * parts + 1e-30. mag = |sc g_x / max_val| + |sc * the
maximum's term| + |fit correction| (+ |prior| when accumulating): the float32 roundings of the result, two of them and a
factor 2, as in tests/test_gpu_loss_grad.py. floor * parts is what fp64 leaves of the adjoint's cancelling parts: parts is the
sum of their magnitudes (through the fit also what the item-wide sums G0 and G1 carry of them into the pixel's correction),
and floor is measured per case, not fixed: the restatement is evaluated in the two summation orders, H then W against W then
H, and the largest difference relative to parts is taken (ssim_ref.fp64_floor); 8 times it is allowed. Measured on these
cases: between 9e-16 and 8e-13, 1e-14 typically (profiles/ssim_loss.md; 2.6e-15 to 9.2e-15 on the cases of PAST_ONE_RING,
profiles/criteria_edges.md); a case whose two orders happen to agree more closely than 2^-50 is
given 2^-50, four ulp, the least that 121-term sums in two orders can be asked to agree to."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import loss_ref as R
import ssim_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = (16, 32)   # asserted against vdn.loss.ssim_tile() below: module-level sizes cannot ask the device


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def frames_at_tile_edges():
    th, tw = TILE
    return [(th + 10 + dy, tw + 10 + dx) for dy, dx in ((-1, -1), (0, 0), (1, 1), (-1, 1), (1, -1))]


def inverse_case():
    """[1, 2, 30, 45]: frame 1 is the contrast inverse of its target (cs = -0.87 on the CPU) and holds the item's maximum, a
    kept prediction; frame 0 is an ordinary frame."""
    c = S.make_case(31, (1, 2, 30, 45), 0.875)
    yy, xx = np.meshgrid(np.linspace(0, 1, 30), np.linspace(0, 1, 45), indexing="ij")
    t = 0.5 + 0.4 * np.sin(40 * xx) * np.sin(33 * yy)
    c["target"][0, 1], c["pred"][0, 1] = t.astype(np.float32), (1 - t).astype(np.float32)
    c["target"][0, 0] /= np.float32(4)
    c["pred"][0, 0] /= np.float32(4)
    c["pred"][0, 1, 3, 4], c["mask"][0, 1, 3, 4] = np.float32(1.5), True
    return c


def negative_case():
    """Every kept value negative and of the clamp's size: the maximum is a dropped pixel's zero, max_val the clamp's 1e-8."""
    c = S.make_case(32, (1, 2, 13, 17), 0.75)
    c["pred"], c["target"] = (-2.0 ** -29 * c["pred"]).astype(np.float32), (-2.0 ** -29 * c["target"]).astype(np.float32)
    return c


def zero_item_case():
    c = S.make_case(33, (2, 2, 12, 14), 0.875, gain=1.5)
    c["pred"][0], c["target"][0], c["mask"][0] = 0, 0, True
    return c


def tie_case():
    c = S.make_case(34, (1, 2, 14, 15), 0.875, gain=1.5)
    k = c["mask"][0].ravel()
    top = c["pred"][0].ravel()[k].max()
    c["target"][0, 1, 2, 3], c["mask"][0, 1, 2, 3] = top, True
    return c


def det0_case():
    """Item 0 keeps one pixel: the fit's determinant is exactly 0, scale = shift = 0, the aligned prediction is 0 everywhere."""
    c = S.make_case(35, (2, 2, 13, 16), 0.875, gain=1.5)
    c["mask"][0] = False
    c["mask"][0, 1, 5, 6] = True
    return c


def trip(wide):
    """The pixels of a frame that one trip of the sweeps covers: the library's own figure, which needs no device."""
    from vdn import loss as L
    return L.trip_pixels(wide)


def interior_frame(dy, dx):
    """(H, W) of 3 tiles + 10 + (dy, dx): at (1, 1) the outputs make 4 x 4 tiles with a ragged last row and column of one
    output, at (0, 0) exactly 3 x 3; the pixels make 4 x 4 tiles either way. The inner tiles have all four neighbours: their
    whole halo comes from inside the frame, and the adjoint's from staged outputs without a zero."""
    th, tw = TILE
    return 3 * th + 10 + dy, 3 * tw + 10 + dx


def strip_shape(odd):
    """[1, 2, H, 13] with 256 + 2 tiles in one column, outputs and pixels alike: lanes 0 and 1 of the fold that adds a frame's
    tiles take a second row. 53 612 pixels (odd: 53 599), past one trip of either sweep, and no row holds whole quads."""
    return (1, 2, 257 * TILE[0] + 12 - odd, 13)


def placed(name):
    """The frame-0 indices at which a holder case puts the item's maximum. trip + 7: block 0, lane 1, on its second trip.
    trip - 4 * 256 + 5: the last block of the first trip, lane 1. The fold meets block 0 first; the lower index must win."""
    second = trip(True) + 7
    return (second,) if name == "holder-second-trip" else (trip(True) - 4 * 256 + 5, second)


def holder_case(name):
    c = S.make_case(66, strip_shape(0), 0.875, gain=1.5)
    top = np.float32(4.5)
    assert top > c["pred"].max() and top > c["target"].max()
    for i in placed(name):
        c["pred"][0, 0].reshape(-1)[i], c["mask"][0, 0].reshape(-1)[i] = top, True
    return c


#        name                 (case maker, aligned, expected holder per item, expected gated frames)
CASES = {
    "one-output": (lambda: S.make_case(41, (1, 1, 11, 11), 0.875, gain=1.5), False, ("prediction",), 0),
    "odd-width": (lambda: S.make_case(42, (2, 3, 12, 37), 0.875), False, ("target", "target"), 0),
    "odd-width-aligned": (lambda: S.make_case(42, (2, 3, 12, 37), 0.875), True, None, 0),
    **{f"tile-edge-{h}x{w}": (functools.partial(S.make_case, 43, (1, 2, h, w), 0.875, (), 1.5), h % 2 == 0, None, 0)
       for h, w in frames_at_tile_edges()},
    "many-frames": (lambda: S.make_case(44, (1, 300, 11, 13), 0.875, gain=1.5), False, ("prediction",), 0),
    "many-items-aligned": (lambda: S.make_case(45, (300, 1, 11, 12), 0.875, gain=1.5), True, None, 0),
    "inverse-frame": (inverse_case, False, ("prediction",), 1),
    "inverse-frame-aligned": (inverse_case, True, None, None),
    "target-holds": (lambda: S.make_case(46, (1, 2, 14, 15), 0.875), False, ("target",), 0),
    "dropped-zero": (negative_case, False, ("dropped",), 0),
    "clamp": (zero_item_case, False, ("clamp", "prediction"), 0),
    "tie": (tie_case, False, ("tie",), 0),
    "det-zero-aligned": (det0_case, True, None, 0),
    # past one ring of tiles and past one trip of the sweeps (reach() states what each is there for)
    "interior-tile": (lambda: S.make_case(61, (1, 2) + interior_frame(1, 1), 0.875, gain=1.5), False, ("prediction",), 0),
    "interior-tile-quads-aligned": (lambda: S.make_case(62, (1, 2) + interior_frame(0, 0), 0.875, gain=1.5), True, None, 0),
    "strip-quads-aligned": (lambda: S.make_case(63, strip_shape(0), 0.875, gain=1.5), True, None, 0),
    "strip-single": (lambda: S.make_case(64, strip_shape(1), 0.875, gain=1.5), False, ("prediction",), 0),
    "strip-gated-aligned": (lambda: S.make_case(65, strip_shape(0), 0.875, ((0, 1),), 1.5), True, ("prediction",), 1),
    "holder-second-trip": (functools.partial(holder_case, "holder-second-trip"), False, ("prediction",), 0),
    "holder-tie-across-blocks": (functools.partial(holder_case, "holder-tie-across-blocks"), False, ("prediction",), 0),
}
PAST_ONE_RING = [n for n in CASES if n.startswith(("interior-", "strip-", "holder-"))]


def reach(name, shape):
    """What a case of PAST_ONE_RING is there for, in terms of the tile and the trip the library reports: a change of either
    fails here and cannot quietly take the coverage away."""
    from vdn import loss as L
    th, tw = L.ssim_tile()
    H, W = shape[2:]
    wide = H * W % 4 == 0
    out, px = (-(-(H - 10) // th), -(-(W - 10) // tw)), (-(-H // th), -(-W // tw))
    assert W % 4 != 0                                            # on the quad path a lane's quad spans a row's end
    if name.startswith("interior-"):
        assert wide == (name == "interior-tile-quads-aligned")
        assert out == ((4, 4) if name == "interior-tile" else (3, 3)) and px == (4, 4)       # inner tiles have four neighbours
        assert ((H - 10) % th, (W - 10) % tw) == ((1, 1) if name == "interior-tile" else (0, 0))
    else:
        assert wide == (name != "strip-single") and H * W > L.trip_pixels(wide)              # the lanes come round again
        assert out[0] * out[1] > 256 and px[0] * px[1] > 256                                 # and so do the fold's
        assert H * W >= L.trip_pixels(False)                                                 # every block of a frame owns pixels


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Inputs, the fit where the case is aligned, the restatement and the measured floor: computed once, shared, never written."""
    make, aligned, holders, gated = CASES[name]
    c = make()
    fit = R.fit_ref(c["pred"], c["target"], c["mask"]) if aligned else None
    r = S.ssim_grad_ref(c["pred"], c["target"], c["mask"], fit)
    floor = max(S.fp64_floor(c["pred"], c["target"], c["mask"], fit), 2.0 ** -50)
    for a in list(c.values()) + [r["grad"], r["mag"], r["parts"]]:
        a.setflags(write=False)
    return c, fit, r, floor


def ratio_to_bound(got, r, floor):
    bound = 4.0 * 2.0 ** -24 * r["mag"] + 8.0 * floor * r["parts"] + 1e-30
    return float((np.abs(got.astype(np.float64) - r["grad"]) / bound).max())


def same_bits(a, b):
    a, b = (x.detach().cpu().numpy() for x in (a, b))
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_tile_shape_is_the_one_the_cases_sit_on():
    from vdn import loss as L
    assert L.ssim_tile() == TILE


@pytest.mark.parametrize("name", list(CASES))
def test_value_and_gradient_match_the_restatement(name):
    from vdn import loss as L
    _, aligned, holders, gated = CASES[name]
    c, fit, r, floor = oracle(name)
    f = r["fwd"]
    # the case takes the branch it is named for
    if holders is not None:
        assert tuple(S.HOLDERS[int(h)] for h in f["holder"]) == holders
    if gated is not None:
        assert f["gated"] == gated
    if name == "det-zero-aligned":
        assert fit[0][0] == 0 and fit[1][0] == 0 and fit[0][1] != 0 and not r["grad"][0].any()
    if name == "clamp":
        assert f["cs"][0, 0] == 1.0 and f["max_val"][0] == np.float32(1e-8) and not r["grad"][0].any()
    if name == "inverse-frame":
        assert f["cs"][0, 1] < -0.8 and f["index"][0] == 30 * 45 + 3 * 45 + 4 and r["hold"][0] != 0
    if name in PAST_ONE_RING:
        reach(name, c["pred"].shape)
    if name == "strip-gated-aligned":
        assert f["cs"][0, 1] < 0 < f["cs"][0, 0] and r["hold"][0] != 0 and not c["mask"][0, 1].any()
    if name.startswith("holder-"):
        at = placed(name)
        flat = lambda n: c[n][0, 0].reshape(-1)
        assert all(flat("mask")[i] and flat("pred")[i].tobytes() == flat("pred")[at[0]].tobytes() for i in at)
        assert f["index"][0] == min(at) and flat("pred")[at[0]] == f["max_val"][0] and r["hold"][0] != 0
    p, t, k = (dev(c[n]) for n in ("pred", "target", "mask"))
    if name in PAST_ONE_RING and c["pred"][0, 0].size % 4 == 0:
        assert p.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0     # the quad path is the one that runs
    got = L.ssim_loss(p, t, k, aligned=aligned)
    err = max(abs(got["ssim_loss"] - f["loss"]), float(np.abs(got["cs"].numpy() - f["cs"]).max()))
    print(f"[{name}] loss {got['ssim_loss']:.12f}, |value - restatement| {err:.2e}, holder {[S.HOLDERS[int(h)] for h in got['holder']][:4]}, "
          f"gated {got['gated']}, floor {floor:.2e}")
    assert err <= 1e-10
    assert got["gated"] == f["gated"] and got["holder"].tolist() == f["holder"].tolist() and got["index"].tolist() == f["index"].tolist()
    assert got["weight"].tolist() == f["weight"].tolist() and got["max_val"].numpy().astype(np.float32).tobytes() == f["max_val"].tobytes()
    g = L.ssim_loss_grad(p, t, k, aligned=aligned)
    assert g.dtype == torch.float32 and g.is_cuda and tuple(g.shape) == c["pred"].shape
    gh = g.cpu().numpy()
    worst = ratio_to_bound(gh, r, floor)
    print(f"[{name}] largest |got - want| / bound {worst:.3f}; max |g| {np.abs(r['grad']).max():.3g}")
    assert np.isfinite(gh).all() and worst <= 1.0
    if name == "inverse-frame":
        frame = gh[0, 1].copy()
        assert frame[3, 4] != 0 and abs(frame[3, 4] - r["hold"][0]) <= 4 * 2.0 ** -24 * abs(r["hold"][0])   # the holder still receives its term
        frame[3, 4] = 0
        assert not frame.any() and not np.signbit(frame).any()                        # the gated frame's direct gradient: +0.0
    if name in ("clamp", "det-zero-aligned"):
        assert not gh[0].any()


def test_two_runs_give_the_same_bits():
    from vdn import loss as L
    for name in ("odd-width-aligned", "inverse-frame", "strip-quads-aligned"):
        c, _, _, _ = oracle(name)
        aligned = CASES[name][1]
        p, t, k = (dev(c[n]) for n in ("pred", "target", "mask"))
        a, b = L.ssim_loss(p, t, k, aligned=aligned), L.ssim_loss(p, t, k, aligned=aligned)
        assert a["ssim_loss"] == b["ssim_loss"] and a["cs"].numpy().tobytes() == b["cs"].numpy().tobytes()
        same_bits(L.ssim_loss_grad(p, t, k, aligned=aligned), L.ssim_loss_grad(p, t, k, aligned=aligned))


def test_misaligned_and_strided_inputs_give_the_same_bits():
    """Through stage: a prediction one float past a 16-byte boundary, a target that is a strided view, a float mask."""
    from vdn import loss as L
    c, _, _, _ = oracle("tile-edge-26x42")                   # H * W is a multiple of 4: the aligned call reads quads
    shape = c["pred"].shape
    p, t, k = (dev(c[n]) for n in ("pred", "target", "mask"))
    off = torch.empty(p.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(shape)
    off.copy_(p)
    wide = torch.zeros(shape[:3] + (2 * shape[3],), dtype=torch.float32, device=DEV)
    wide[..., ::2] = t
    assert off.data_ptr() % 16 == 4 and not wide[..., ::2].is_contiguous()
    a = L.ssim_loss(p, t, k)
    b = L.ssim_loss(off, wide[..., ::2], k.to(torch.float32))
    assert a["ssim_loss"] == b["ssim_loss"] and a["cs"].numpy().tobytes() == b["cs"].numpy().tobytes()
    same_bits(L.ssim_loss_grad(p, t, k), L.ssim_loss_grad(off, wide[..., ::2], k.to(torch.float32)))
    # with the fit the values agree to the bar, not to the bit: vdn_depth_loss sums a misaligned tensor in another order
    c_al, fit, r, floor = oracle("tile-edge-26x42")
    assert CASES["tile-edge-26x42"][1]
    g = L.ssim_loss_grad(off, wide[..., ::2], k.to(torch.float32), aligned=True)
    assert ratio_to_bound(g.cpu().numpy(), r, floor) <= 1.0


@pytest.mark.parametrize("name", ["odd-width", "odd-width-aligned", "inverse-frame"])
def test_accumulate_adds_to_the_prior_gradient_with_one_rounding(name):
    from vdn import loss as L
    c, fit, _, floor = oracle(name)
    aligned = CASES[name][1]
    prior = (S._hash01(9, c["pred"].size).reshape(c["pred"].shape) - 0.5).astype(np.float32) * np.float32(1e-3)
    r = S.ssim_grad_ref(c["pred"], c["target"], c["mask"], fit, coeff=0.3, prior=prior)
    p, t, k = (dev(c[n]) for n in ("pred", "target", "mask"))
    before = dev(prior)
    got = L.ssim_loss_grad(p, t, k, aligned=aligned, coeff=0.3, prior=before)
    same_bits(before, dev(prior))                                               # the prior itself is left as it is
    worst = ratio_to_bound(got.cpu().numpy(), r, floor)
    print(f"[{name}] accumulate: largest |got - want| / bound {worst:.3f}")
    assert worst <= 1.0
    # against accumulate = 0 plus the prior, added in float64 and rounded once
    alone = L.ssim_loss_grad(p, t, k, aligned=aligned, coeff=0.3).cpu().numpy().astype(np.float64)
    diff = np.abs(got.cpu().numpy().astype(np.float64) - (alone + prior.astype(np.float64)))
    assert (diff <= 2.0 ** -24 * (np.abs(alone) + np.abs(prior)) * 2).all()


def test_misaligned_prediction_past_one_trip_gives_the_same_bits():
    """strip-quads-aligned with the prediction one float past a 16-byte boundary: the forward's maximum then reads a pixel per
    lane and the backward four pixels per lane with scalar loads, both past one trip. A maximum has no order and the backward
    picks its order from the shape alone, so without the fit every value and the gradient keep their bits; with the fit
    (which vdn_depth_loss sums in another order for a misaligned tensor) the gradient keeps to the bar."""
    from vdn import loss as L
    c, fit, r, floor = oracle("strip-quads-aligned")
    shape = c["pred"].shape
    p, t, k = (dev(c[n]) for n in ("pred", "target", "mask"))
    off = torch.empty(p.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(shape)
    off.copy_(p)
    assert off.data_ptr() % 16 == 4 and p.data_ptr() % 16 == 0 and shape[2] * shape[3] % 4 == 0 and shape[2] * shape[3] > L.trip_pixels(True)
    a, b = L.ssim_loss(p, t, k), L.ssim_loss(off, t, k)
    assert a["ssim_loss"] == b["ssim_loss"] and a["gated"] == b["gated"]
    for n in ("cs", "max_val", "holder", "index", "weight"):
        assert a[n].numpy().tobytes() == b[n].numpy().tobytes(), n
    same_bits(L.ssim_loss_grad(p, t, k), L.ssim_loss_grad(off, t, k))
    worst = ratio_to_bound(L.ssim_loss_grad(off, t, k, aligned=True).cpu().numpy(), r, floor)
    print(f"[strip-quads-aligned] misaligned prediction, through the fit: largest |got - want| / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["interior-tile-quads-aligned", "strip-quads-aligned"])
def test_accumulate_across_row_ends_and_past_one_trip(name):
    """The accumulating write on the quad path where a lane's quad spans a row's end, and on its second trip: a prior gradient
    of the size a training step holds, N(0, 1), under the file's bound with its |prior| term."""
    from vdn import loss as L
    c, fit, _, floor = oracle(name)
    assert CASES[name][1]
    reach(name, c["pred"].shape)
    prior = np.random.default_rng(17).standard_normal(c["pred"].shape).astype(np.float32)
    r = S.ssim_grad_ref(c["pred"], c["target"], c["mask"], fit, coeff=0.85, prior=prior)
    p, t, k = (dev(c[n]) for n in ("pred", "target", "mask"))
    before = dev(prior)
    got = L.ssim_loss_grad(p, t, k, aligned=True, coeff=0.85, prior=before)
    same_bits(before, dev(prior))
    gh = got.cpu().numpy()
    worst = ratio_to_bound(gh, r, floor)
    moved = float((gh != prior).mean())
    print(f"[{name}] accumulate: largest |got - want| / bound {worst:.3f}; share of elements the term moved {moved:.3f}")
    assert np.isfinite(gh).all() and worst <= 1.0


# ------------------------------------------------------------------------------------------------ the classes, at 161 pixels
def fixture():
    import test_ssim_host as Hs
    return Hs


@pytest.mark.parametrize("name", ["plain", "gated", "sparse"])
def test_depth_shallow_ssim_loss_against_the_fixture(name):
    """Fails without the feature: the class does not exist."""
    from vdn import loss as L
    Hs = fixture()
    c, r, Z = Hs.case(name), Hs.alone(name), Hs.Z
    p, t, k = (dev(c[n]) for n in ("pred", "target", "mask"))
    crit = L.DepthShallowSSIMLoss()
    with torch.no_grad():
        plain = crit(p, t, k)
    assert plain.dtype == torch.float32 and plain.dim() == 0 and plain.is_cuda and not plain.requires_grad
    q = p.clone().requires_grad_()
    v = crit(q, t, k)
    same_bits(v.detach(), plain)
    v.backward()
    same_bits(q.grad, L.ssim_loss_grad(p, t, k))
    v32, v64 = (float(x) for x in Z[f"{name}_alone_value"])
    dv, dg = (float(x) for x in Z[f"{name}_alone_yardstick"])
    assert float(v.detach()) == float(np.float32(r["fwd"]["loss"]))                              # the float64 value, rounded once
    assert abs(float(v.detach()) - v32) <= 4 * dv + 2.0 ** -24
    g = q.grad.cpu().numpy().astype(np.float64).ravel()
    at = Z[f"{name}_at"]
    per = float(Z[f"{name}_alone_norm"][1]) / np.sqrt(g.size)
    rel = float(np.sqrt(((g[at] - Z[f"{name}_alone_grad32"].astype(np.float64)) ** 2).mean())) / per
    floor = max(S.fp64_floor(c["pred"], c["target"], c["mask"]), 2.0 ** -50)
    worst = ratio_to_bound(q.grad.cpu().numpy(), r, floor)
    print(f"[{name}] alone: value {float(v.detach()):.9f} (f32 run {v32:.9f}); gradient rel-L2 at the samples vs the f32 run {rel:.2e} "
          f"(f32 vs f64 {dg:.2e}); vs the restatement {worst:.3f} of the bound, floor {floor:.2e}")
    assert rel <= 4 * dg and worst <= 1.0


@pytest.mark.parametrize("name", ["plain", "gated", "sparse"])
def test_ssim_video_depth_loss_against_the_fixture(name):
    from vdn import loss as L
    Hs = fixture()
    c, w, Z = Hs.case(name), Hs.whole(name), Hs.Z
    i = Hs.NAMES.index(name)
    alpha, ss, scale = float(Z["alpha"][i]), float(Z["stable_scale"][i]), float(Z["ssim_scale"])
    p, t, k = (dev(c[n]) for n in ("pred", "target", "mask"))
    crit = L.SSIMVideoDepthLoss(alpha, 4, 0.0, ss, scale)
    with torch.no_grad():
        plain = crit(p, t, k)
    keys = [str(x) for x in Z[f"{name}_whole_keys"]]
    assert list(plain) == keys == list(crit.keys)
    q = p.clone().requires_grad_()
    d = crit(q, t, k)
    for key in keys:
        same_bits(d[key].detach(), plain[key])
    d32, d64 = Z[f"{name}_whole_dict"]
    for key, a, b in zip(keys, d32, d64):
        tol = 4 * max(abs(float(a) - float(b)), 2.0 ** -24 * abs(float(b)))
        print(f"[{name}] {key}: device {float(d[key].detach()):.9f} f32 run {float(a):.9f} f64 run {float(b):.9f}")
        assert abs(float(d[key].detach()) - float(a)) <= tol and abs(float(d[key].detach()) - w["values"][key]) <= 2.0 ** -22 * abs(w["values"][key]), key
    total = plain["spatial_loss"] + (plain["stable_loss"] * ss if ss > 0 else 0) + plain["ssim_loss"] * scale
    same_bits(plain["total_loss"], total)                                              # the float32 sum, as the reference forms it
    d["total_loss"].backward()
    g = q.grad.cpu().numpy()
    dg = float(Z[f"{name}_whole_yardstick"][1])
    at = Z[f"{name}_at"]
    per = float(Z[f"{name}_whole_norm"][1]) / np.sqrt(g.size)
    rel = float(np.sqrt(((g.astype(np.float64).ravel()[at] - Z[f"{name}_whole_grad32"].astype(np.float64)) ** 2).mean())) / per
    base, term = w["base"], w["term"]
    floor = max(S.fp64_floor(c["pred"], c["target"], c["mask"], w["fit"], scale), 2.0 ** -50)
    bound = 4.0 * 2.0 ** -24 * (base["mag_a"] + base["mag_fit"] + term["mag"]) + 8.0 * floor * term["parts"] + 1e-30
    worst = float((np.abs(g.astype(np.float64) - w["grad"]) / bound).max())
    print(f"[{name}] whole: gradient rel-L2 at the samples vs the f32 run {rel:.2e} (f32 vs f64 {dg:.2e}); vs the restatement "
          f"{worst:.3f} of the bound")
    assert rel <= 4 * dg and worst <= 1.0
    # the term's share is ssim_loss_grad's, added to the other terms' gradient with one rounding
    rest = L.depth_loss_grad(p, t, k, alpha=alpha, stable_scale=ss)
    same_bits(q.grad, L.ssim_loss_grad(p, t, k, aligned=True, coeff=scale, prior=rest))


def test_without_the_term_it_is_the_trimmed_criterion_bit_for_bit():
    from vdn import loss as L
    c = S.make_case(51, (2, 3, 20, 22), 0.875)
    p, t, k = (dev(c[n]) for n in ("pred", "target", "mask"))
    for trim in (0.0, 0.2):
        mine, theirs = L.SSIMVideoDepthLoss(0.5, 4, trim, 10, 0.0), L.TrimmedVideoDepthLoss(0.5, 4, trim, 10)
        q, r = p.clone().requires_grad_(), p.clone().requires_grad_()
        a, b = mine(q, t, k), theirs(r, t, k)
        assert list(a) == list(b)
        for key in a:
            same_bits(a[key], b[key])
        a["total_loss"].backward()
        b["total_loss"].backward()
        same_bits(q.grad, r.grad)


def test_validate_step_carries_the_terms_key():
    from vdn import loss as L
    from vdn import steps
    rng = np.random.default_rng(3)
    shape = (1, 2, 1, 161, 162)
    batch = {"rgb": torch.zeros((1, 2, 3, 161, 162), device=DEV),
             "depth_anything_v2": dev(rng.uniform(0.5, 10.0, shape).astype(np.float32)),
             "depth": dev(rng.uniform(0.5, 20.0, shape).astype(np.float32)), "mask": dev(rng.random(shape) < 0.8)}
    crit = L.SSIMVideoDepthLoss(ssim_loss_scale=0.1)
    meter = steps.LossMeter()
    losses = steps.validate_step(lambda depth: depth * 0.75 + 0.125, batch, crit, with_rgb=False, meter=meter)
    assert list(losses) == list(crit.keys) and "ssim_loss" in losses
    got = meter.averages()
    assert list(got) == list(crit.keys) and got["ssim_loss"] == float(losses["ssim_loss"]) and 0 < got["ssim_loss"] <= 1
