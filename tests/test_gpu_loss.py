"""vdn.loss on the device (csrc/loss.hip) against the CPU restatement tests/loss_ref.py, on the recorded cases of
tests/golden/loss_cases.npz: the smallest shapes at which each piece can go wrong (odd sizes and one pixel per lane, whole
quads, grids that collapse to a point, empty frames and items, medians of exactly 0, a negative scale, targets around the
bounds of absRel, alpha = 0, stable_scale = 0, bool and uint8 masks), and on the constructed cases of
tests/test_loss_host.py (EXTRA): quads that span a row's end, and frames past one trip of the sweep on both paths.

Bars. Both sides are fp64 over the same float32 operands and differ in summation order only: spatial_loss, stable_loss,
absRel_loss, d1, data, every g_k and every per-frame s within 1e-9 absolute (the bar of tests/test_gpu_normals.py; the
largest sum of a recorded case has 9216 terms below 100, whose fp64 sum is good to 1e-10 in any order; a constructed case
takes the mean of n <= 107 117 terms, which any order gives to n * 2^-53 times the mean of their magnitudes: 1.2e-11 times a
mean that is below 10 in every term of these cases), total_loss within (1 + stable_scale) * 1e-9; every median, count and
fit exactly equal. forward's float32 tensors must be the fp64 values of the same inputs rounded once."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import loss_ref as R
from test_loss_host import CASES, EXTRA, EXTRA_ARGS, KEYS, case_id, case_inputs, extra

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL = 1e-9


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs and restatement of recorded case i, computed once, shared and never written."""
    c = CASES[i]
    case = case_inputs(c)
    for a in case.values():
        a.setflags(write=False)
    return case, R.depth_loss_ref(case["pred"], case["target"], case["mask"], alpha=c["alpha"], stable_scale=c["stable_scale"])


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def run(case, c, **kw):
    from vdn import loss as L
    args = dict(alpha=c["alpha"], stable_scale=c["stable_scale"])
    args.update(kw)
    return L.depth_loss(dev(case["pred"]), dev(case["target"]), dev(case["mask"]), **args)


def agree(got, want, stable_scale, what):
    """The bars of this file on one result of depth_loss; prints the figures before asserting."""
    worst = {}
    for k in KEYS + ("data",):
        if k == "stable_loss" and not stable_scale > 0:
            assert k not in got and k not in want
            continue
        worst[k] = abs(got[k] - want[k])
    n = len(want["g"])
    worst["g"] = float(np.abs(got["g"].numpy()[:n] - want["g"]).max())
    for k in ("s_pred", "s_target"):
        worst[k] = float(np.abs(got[k].numpy() - want[k]).max())
    print(f"[{what}] " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k in ("m_pred", "m_target", "count"):
        assert np.array_equal(got[k].numpy(), want[k].astype(np.float64 if k != "count" else np.int64)), k
    assert np.array_equal(got["M"].numpy()[:n], want["M"]) and not got["M"].numpy()[n:].any()
    for k in ("d1_hits", "absrel_count"):
        assert got[k] == want[k], k
    if stable_scale > 0:
        assert got["stable_count"] == want["stable_count"]
    for k, v in worst.items():
        assert v <= (ATOL * (1 + stable_scale) if k == "total_loss" else ATOL), (k, v)


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = (np.asarray(v.numpy() if isinstance(v, torch.Tensor) else v) for v in (a[k], b[k]))
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: case_id(CASES[i]))
def test_values_match_the_restatement(i):
    from vdn import loss as L
    c = CASES[i]
    case, want = _case(i)
    got = run(case, c)
    agree(got, want, c["stable_scale"], case_id(c))
    out = L.VideoDepthLoss(alpha=c["alpha"], stable_scale=c["stable_scale"])(dev(case["pred"]), dev(case["target"]), dev(case["mask"]))
    assert tuple(out) == tuple(k for k in KEYS if k != "stable_loss" or c["stable_scale"] > 0)
    for k, v in out.items():
        assert v.is_cuda and v.dim() == 0 and v.dtype == torch.float32
        assert float(v) == float(np.float32(got[k])), k        # the fp64 value rounded once


@pytest.mark.parametrize("name", list(EXTRA))
def test_constructed_cases_match_the_restatement(name):
    """The values, medians, scales, counts and the fit at quads that span a row's end and past one trip of the sweep."""
    from vdn import loss as L
    case, want = extra(name)
    B, T, H, W = case["pred"].shape
    wide = H * W % 4 == 0
    assert W % 4 != 0 and wide == (name != "two-trips-single")
    if name != "quads-cross-rows":
        assert H * W > L.trip_pixels(wide)                       # every lane of block 0 comes round its stride loop again
    if wide:
        assert all(dev(case[k]).data_ptr() % 16 == 0 for k in ("pred", "target"))   # the four-pixel path is the one that runs
    agree(run(case, EXTRA_ARGS), want, EXTRA_ARGS["stable_scale"], name)
    # the fit alone, on frame 1 of every item, bit for bit
    p, t, m = (case[k][:, 1] for k in ("pred", "target", "mask"))
    scale, shift = L.compute_scale_and_shift(dev(p), dev(t), dev(m))
    fit = R.fit_ref(p, t, m)
    print("scale", scale.tolist(), fit[0].tolist(), "shift", shift.tolist(), fit[1].tolist())
    assert scale.cpu().numpy().tobytes() == fit[0].tobytes() and shift.cpu().numpy().tobytes() == fit[1].tobytes()
    if B > 1:
        assert fit[0][0] != fit[0][1]


@pytest.mark.parametrize("i", [0, 9], ids=lambda i: case_id(CASES[i]))
def test_fit_is_the_restatements_float32_pair(i):
    """compute_scale_and_shift on [B, H, W] (one frame of every item, so the items' fits differ; case 9 has an empty item)."""
    from vdn import loss as L
    case, _ = _case(i)
    p, t, m = (case[k][:, 1] for k in ("pred", "target", "mask"))
    scale, shift = L.compute_scale_and_shift(dev(p), dev(t), dev(m))
    want = R.fit_ref(p, t, m)
    assert scale.dtype == torch.float32 and scale.is_cuda and tuple(scale.shape) == (p.shape[0],)
    print("scale", scale.tolist(), want[0].tolist(), "shift", shift.tolist(), want[1].tolist())
    assert scale.cpu().numpy().tobytes() == want[0].tobytes() and shift.cpu().numpy().tobytes() == want[1].tobytes()


def test_two_runs_give_the_same_bits():
    from vdn import loss as L
    for i in (0, 5):
        case, _ = _case(i)
        same_bits(run(case, CASES[i]), run(case, CASES[i]))
        crit = L.VideoDepthLoss()
        args = [dev(case[k]) for k in ("pred", "target", "mask")]
        a, b = crit(*args), crit(*args)
        same_bits({k: v.cpu() for k, v in a.items()}, {k: v.cpu() for k, v in b.items()})


def test_nan_and_inf_under_dropped_pixels_change_no_bit():
    # plain, an empty frame, an empty item; then quads that span a row's end past one trip, where the finest grid's right-hand
    # neighbour comes from the lane's own quad: a dropped one must reach nothing there either
    for case, args in [(_case(i)[0], CASES[i]) for i in (0, 8, 9)] + [(extra("two-trips-quads-cross-rows")[0], EXTRA_ARGS)]:
        drop = case["mask"] == 0
        poisoned = dict(case)
        for k, vals in (("pred", (np.nan, np.inf)), ("target", (-np.inf, np.nan))):
            a = case[k].copy()
            a[drop] = np.where(np.arange(drop.sum()) % 2 == 0, vals[0], vals[1]).astype(np.float32)
            poisoned[k] = a
        assert drop.any() and np.isnan(poisoned["pred"]).any() and np.isinf(poisoned["target"]).any()
        same_bits(run(case, args), run(poisoned, args))


def test_temporal_term_stays_inside_an_item():
    """[2, 2, H, W]: the temporal term equals that of the two items run alone, recombined by their counts (a difference taken
    from the last frame of item 0 to the first of item 1 would add a third pair)."""
    c = R.make_case(71, (2, 2, 17, 13), 0.8)
    both = run(c, dict(alpha=0.5, stable_scale=10))
    alone = [run({k: v[b:b + 1] for k, v in c.items()}, dict(alpha=0.5, stable_scale=10)) for b in range(2)]
    n = [a["stable_count"] for a in alone]
    want = (alone[0]["stable_loss"] * n[0] + alone[1]["stable_loss"] * n[1]) / (n[0] + n[1])
    print(f"stable {both['stable_loss']!r} vs {want!r}: {both['stable_loss'] - want:+.1e}; counts {n} / {both['stable_count']}")
    assert min(n) > 0 and both["stable_count"] == n[0] + n[1]
    assert abs(both["stable_loss"] - want) <= ATOL


def test_gradient_terms_stay_inside_a_frame():
    """A clip of a frame, its vertical flip and its horizontal flip has the fit of each of its frames alone (the same sums;
    checked on the restatement first), so its gradient terms equal those of the three frames run alone with T = 1, recombined
    by M_k. A neighbour read across a row end or into the next frame would break that."""
    c = R.make_case(61, (1, 1, 17, 13), 0.8)
    frames = [{k: v for k, v in c.items()}, {k: v[:, :, ::-1].copy() for k, v in c.items()}, {k: v[:, :, :, ::-1].copy() for k, v in c.items()}]
    clip = {k: np.concatenate([f[k] for f in frames], 1) for k in c}
    fit = R.fit_ref(clip["pred"], clip["target"], clip["mask"])
    for f in frames:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(fit, R.fit_ref(f["pred"], f["target"], f["mask"])))
    whole = run(clip, dict(alpha=0.5, stable_scale=0))
    alone = [run(f, dict(alpha=0.5, stable_scale=0)) for f in frames]
    M = np.stack([a["M"].numpy() for a in alone])
    g = np.stack([a["g"].numpy() for a in alone])
    want = (g * M).sum(0) / M.sum(0)
    print("g", whole["g"].tolist(), "recombined", want.tolist(), "M", M.sum(0).tolist())
    assert np.array_equal(whole["M"].numpy(), M.sum(0)) and (M.sum(0) > 0).all()
    assert np.abs(whole["g"].numpy() - want).max() <= ATOL
    data = sum(a["data"] * int(a["count"].sum()) for a in alone) / int(whole["count"].sum())
    assert abs(whole["data"] - data) <= ATOL


def test_views_and_mask_types_give_the_same_values():
    from vdn import loss as L
    case, want = _case(2)                                         # [1, 4, 16, 16]: whole quads
    base = run(case, CASES[2])
    p, t, m = (dev(case[k]) for k in ("pred", "target", "mask"))
    wide = torch.zeros(1, 4, 16, 32, device=DEV)
    views = []
    for x in (p, t):
        w = wide.clone()
        w[..., ::2] = x
        views.append(w[..., ::2])
    assert not views[0].is_contiguous()
    same_bits(base, L.depth_loss(views[0], views[1], m))
    for mask in (m.to(torch.uint8), m.float() * 3.0, m.cpu()):
        same_bits(base, L.depth_loss(p, t, mask))
    # both planes 4 bytes past a 16-byte boundary: one pixel per lane, another summation order, the same bars
    off = [torch.empty(p.numel() + 1, device=DEV)[1:].view(p.shape).copy_(x) for x in (p, t)]
    assert all(o.data_ptr() % 16 == 4 and o.is_contiguous() for o in off)
    agree(L.depth_loss(off[0], off[1], m), want, CASES[2]["stable_scale"], "misaligned")
    # the same past one trip, with rows that end inside what would be a quad: five trips of one pixel per lane
    case, want = extra("two-trips-quads-cross-rows")
    p, t, m = (dev(case[k]) for k in ("pred", "target", "mask"))
    off = [torch.empty(p.numel() + 1, device=DEV)[1:].view(p.shape).copy_(x) for x in (p, t)]
    assert all(o.data_ptr() % 16 == 4 and o.is_contiguous() for o in off) and p.shape[2] * p.shape[3] > L.trip_pixels(False)
    agree(L.depth_loss(off[0], off[1], m, **EXTRA_ARGS), want, EXTRA_ARGS["stable_scale"], "misaligned two-trips-quads-cross-rows")
