"""The trimmed depth criterion on the device (vdn_depth_loss_trimmed and its backward, vdn.loss.TrimmedVideoDepthLoss) against
the CPU restatement tests/loss_trim_ref.py, which tests/test_loss_trim_host.py holds to the reference's recorded values and
gradients: on the recorded cases and on constructed ones the reference is not consulted for, then the properties the kernels
promise.

Arithmetic restated (include/vdn.h): per term (data |an - tn| over kept pixels, stable |pg - tg| over counted pairs, absRel
|(a - t) / t| over counted pixels) with n counted residuals, k = floor(n * keep), keep = 1.0 - trim computed once on the host in
double; the key of a residual is the bit pattern of its float32 rounding (a NaN sorts after +inf, uncounted elements have no
key); thr = the key of rank k - 1, n_less = #{key < thr}, n_tied = #{key == thr}, w = (k - n_less) / n_tied; term = (sum below
thr + w * sum at thr) / n; the gradient weighs each counted element by 1, w or 0.

Bars. Values: 1e-9 absolute, the bar of tests/test_gpu_loss.py ((1 + stable_scale) * 1e-9 for total_loss): both sides take
the same fp64 steps from the same float32 samples and differ in the order of their sums. k, n_less, n_tied and thr are
compared exactly; every case used here passes loss_trim_ref.data_selection_is_stable, so the data term's selection does not
hang on the last bits of a per-frame scale (the stable and absRel residuals are exact functions of float32 values).
Gradients: the per-element bar of tests/test_gpu_loss_grad.py, 4 * 2^-24 * (|sc * g_a| + |fit correction|) + 1e-30."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import loss_ref as R
import loss_trim_ref as TR
from test_gpu_loss_grad import ratio_to_bound, same_bits
from test_loss_trim_host import CASES, case_id, oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
VALUES = ("spatial_loss", "stable_loss", "absRel_loss", "d1", "total_loss", "data")
# The histogram kernel's grid is (min(64, blocks of a frame), frames): a frame's pixels go round its blocks' stride loop.
EXTRA = {"tie": "loss_trim_ref.make_tie_case: many residuals on every threshold, 0 < w < 1",
         "last-pass": "loss_trim_ref.make_last_pass_case: the absRel keys share their top 22 bits",
         "grid-rounds": "[2, 3, 128, 96]: 73 728 elements in one selection set, six frames of 12 blocks each (four pixels a lane)",
         "frame-rounds": "[1, 2, 260, 256]: 66 560 pixels a frame: a second trip of a frame's 64 blocks x 256 lanes x 4 pixels, and"
                         " a third of the 32 blocks of the sums",
         "single-pixel": "[1, 2, 131, 127]: H * W = 16 637, no multiple of 4: one pixel per lane, a second trip of a frame's 64 blocks",
         "empty-frame-and-item": "[2, 3, 17, 13], frame 1 of item 0 and all of item 1 dropped",
         "nothing-kept": "[1, 2, 9, 11] under a mask that keeps nothing: every count and every value is 0"}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def extra(name, weights=(1.0, 0.0, 0.0, 0.0)):
    """A constructed case: inputs, trim and the restatement, computed once, shared and never written."""
    trim = 0.2
    if name == "tie":
        case = TR.make_tie_case()
    elif name == "last-pass":
        case = TR.make_last_pass_case()
    elif name == "grid-rounds":
        case = R.make_case(161, (2, 3, 128, 96), 0.8)
    elif name == "frame-rounds":
        case = R.make_case(162, (1, 2, 260, 256), 0.8)
    elif name == "single-pixel":
        case = R.make_case(163, (1, 2, 131, 127), 0.8)
    elif name == "empty-frame-and-item":
        case = R.make_case(164, (2, 3, 17, 13), 0.8, empty_frames=(1,), empty_items=(1,))
    else:
        case = R.make_case(165, (1, 2, 9, 11), 0.8)
        case["mask"][:] = False
    assert TR.data_selection_is_stable(case["pred"], case["target"], case["mask"], trim=trim), f"{name}: choose another seed"
    r = TR.depth_loss_trim_grad_ref(case["pred"], case["target"], case["mask"], weights=weights, trim=trim)
    for a in list(case.values()) + [r["grad"], r["mag_a"], r["mag_fit"]]:
        a.setflags(write=False)
    return case, r, trim


def forward(case, trim, alpha=0.5, stable_scale=10):
    from vdn import loss as L
    return L.depth_loss(dev(case["pred"]), dev(case["target"]), dev(case["mask"]), alpha=alpha, stable_scale=stable_scale, trim=trim)


def grad(case, trim, alpha=0.5, stable_scale=10, **kw):
    from vdn import loss as L
    return L.depth_loss_grad(dev(case["pred"]), dev(case["target"]), dev(case["mask"]), alpha=alpha, stable_scale=stable_scale,
                             trim=trim, **kw)


def check_values(got, want, stable_scale, what):
    for k in VALUES:
        if k not in want:
            assert k == "stable_loss" and k not in got
            continue
        bar = (1 + stable_scale) * 1e-9 if k == "total_loss" else 1e-9
        print(f"[{what}] {k}: {got[k]!r} vs {want[k]!r} diff {got[k] - want[k]:+.2e} (bar {bar:.1e})")
        assert abs(got[k] - want[k]) <= bar, k
    for k in ("trim_k", "trim_less", "trim_tied"):
        print(f"[{what}] {k}: {got[k].tolist()} vs {want[k].tolist()}")
        assert got[k].dtype == torch.int64 and got[k].tolist() == want[k].tolist(), k
    assert got["trim_threshold"].dtype == torch.float64 and got["trim_threshold"].numpy().tobytes() == want["trim_threshold"].tobytes()
    assert np.abs(got["trim_weight"].numpy() - want["trim_weight"]).max() <= 1e-15
    for k in ("stable_count", "absrel_count", "d1_hits"):
        assert got[k] == want.get(k, 0), k
    assert got["M"].tolist() == want["M"].tolist() and np.abs(got["g"].numpy() - want["g"]).max() <= 1e-9


def check_grad(got, case, r, what):
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == case["pred"].shape
    g = got.cpu().numpy()
    worst = ratio_to_bound(g, r)
    print(f"[{what}] largest |got - want| / bound {worst:.3f}; max |g| {np.abs(r['grad']).max():.3g}")
    drop = case["mask"] == 0
    assert not g[drop].any() and not np.signbit(g[drop]).any()       # +0.0 under every dropped pixel
    assert worst <= 1.0


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_recorded_cases_match_the_restatement(c):
    """Values, selection and gradient of the recorded cases: trim 0.05, 0.2, 0.5 on three shapes, k == 0, emptiness, alpha = 0 and
    stable_scale = 0."""
    case, r = oracle(c["index"])
    got = forward(case, c["trim"], c["alpha"], c["stable_scale"])
    check_values(got, r["fwd"], c["stable_scale"], case_id(c))
    if c["trim"] == 0.999:
        assert got["data"] == 0.0 and got["stable_loss"] == 0.0 and got["absRel_loss"] == 0.0 and got["spatial_loss"] > 0
    check_grad(grad(case, c["trim"], c["alpha"], c["stable_scale"]), case, r, case_id(c))


@pytest.mark.parametrize("name", list(EXTRA))
def test_constructed_cases_match_the_restatement(name):
    """The gradient is that of total_loss, except in the last-pass case, where it is total_loss + absRel_loss: that case is about
    the absRel selection, and its mirrored pairs make the fit's sums G0 and G1 of total_loss alone cancel to exactly 0 in real
    arithmetic, so that the bar's |fit correction| would be the restatement's own rounding residue (1e-18) at the pixels whose
    g_a is exactly 0."""
    weights = (1.0, 0.0, 0.0, 1.0) if name == "last-pass" else (1.0, 0.0, 0.0, 0.0)
    case, r, trim = extra(name, weights)
    f = r["fwd"]
    B, T, H, W = case["pred"].shape
    if name == "tie":
        assert (f["trim_tied"] > 1).all() and ((0 < f["trim_weight"]) & (f["trim_weight"] < 1)).all()
    elif name == "last-pass":
        assert f["trim_tied"][2] == 1 and f["trim_threshold"][2] == 1 + 202 * 2.0 ** -23
    elif name == "grid-rounds":
        assert B * T * H * W > 4 * 64 * 256 and H * W % 4 == 0
    elif name == "frame-rounds":
        assert H * W > 64 * 256 * 4 and H * W % 4 == 0
    elif name == "single-pixel":
        assert H * W % 4 != 0 and H * W > 64 * 256
    elif name == "empty-frame-and-item":
        assert f["count"].ravel().tolist()[1] == 0 and not f["count"][1].any() and f["count"][0, 0] > 0
    else:
        assert not f["count"].any()
    got = forward(case, trim)
    check_values(got, f, 10, name)
    if name == "nothing-kept":
        assert all(got[k] == 0.0 for k in VALUES) and not got["trim_k"].any() and not got["trim_threshold"].any()
        assert not grad(case, trim).cpu().numpy().any()
        return
    check_grad(grad(case, trim, weights=weights), case, r, name)


@pytest.mark.parametrize("key,weights", [("spatial_loss", (0.0, 1.0, 0.0, 0.0)), ("stable_loss", (0.0, 0.0, 1.0, 0.0)),
                                         ("absRel_loss", (0.0, 0.0, 0.0, 1.0))])
def test_each_coefficient_alone_matches_the_restatement(key, weights):
    """On two recorded cases (trim 0.2 and 0.5). The constructed cases are left to the total: their mirrored values make single
    products of the fit chain cancel exactly at some pixels, where the bar would be the restatement's rounding residue."""
    for i in (1, 5):
        case, r = oracle(i, weights)
        assert CASES[i]["trim"] in (0.2, 0.5) and np.abs(r["grad"]).max() > 0
        check_grad(grad(case, CASES[i]["trim"], weights=weights), case, r, f"{case_id(CASES[i])} {key}")


def test_tied_weights_sum_to_the_kept_share():
    """In the tie case the gradient of absRel alone is w / (t * n) in magnitude at a tied pixel before the frame and fit chains;
    here on the restatement's weights, which the device's gradient was just held to: they sum to k - n_less over the tied set.
    On the device the same is read off out[20..34]: w * n_tied is k - n_less."""
    case, r, trim = extra("tie")
    got = forward(case, trim)
    for i, term in enumerate(TR.TERMS):
        s = r["fwd"]["sel"][term]
        tied = (s["u"] > 0) & (s["u"] < 1)
        assert tied.sum() == s["n_tied"] == int(got["trim_tied"][i]) and abs(s["u"][tied].sum() - (s["k"] - s["n_less"])) < 1e-12
        assert abs(float(got["trim_weight"][i]) * int(got["trim_tied"][i]) - (int(got["trim_k"][i]) - int(got["trim_less"][i]))) < 1e-12


def test_autograd_gives_depth_loss_grads_bits():
    from vdn import loss as L
    case, _ = oracle(1)
    trim = CASES[1]["trim"]
    p, t, k = (dev(case[n]) for n in ("pred", "target", "mask"))
    crit = L.TrimmedVideoDepthLoss(trim=trim)
    plain = crit(p, t, k)
    want = forward(case, trim)
    assert tuple(plain) == crit.keys and all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda and v.grad_fn is None for v in plain.values())
    for n in crit.keys:
        assert float(plain[n]) == float(np.float32(want[n])), n
    q = p.clone().requires_grad_()
    out = crit(q, t, k)
    for n in crit.keys:
        same_bits(out[n], plain[n])
    out["total_loss"].backward()
    same_bits(q.grad, L.depth_loss_grad(p, t, k, trim=trim))
    assert (q.grad != L.depth_loss_grad(p, t, k)).any()       # and it is not the untrimmed gradient
    q = p.clone().requires_grad_()
    out = crit(q, t, k)
    (3 * out["total_loss"] + 2 * out["absRel_loss"] + 5 * out["d1"]).backward()
    same_bits(q.grad, L.depth_loss_grad(p, t, k, weights=(3, 0, 0, 2), trim=trim))
    with pytest.raises(NotImplementedError, match="target"):
        crit(q, t.clone().requires_grad_(), k)
    # two criteria evaluated before either backward: each reads the state it saved
    other, _ = oracle(11)
    assert other["pred"].shape == case["pred"].shape
    args = [[dev(c[n]) for n in ("pred", "target", "mask")] for c in (case, other)]
    qs = [x[0].clone().requires_grad_() for x in args]
    outs = [crit(q, x[1], x[2]) for q, x in zip(qs, args)]
    for o in outs:
        o["total_loss"].backward()
    for q, x in zip(qs, args):
        same_bits(q.grad, L.depth_loss_grad(*x, trim=trim))


def test_two_runs_give_the_same_bits_and_dropped_pixels_reach_nothing():
    from vdn import loss as L
    for i in (1, 10, 11):                                     # plain, an empty frame, an empty item
        case, _ = oracle(i)
        c = CASES[i]
        args = [dev(case[k]) for k in ("pred", "target", "mask")]
        launch = lambda a: L._launch(*a, c["alpha"], 4, c["stable_scale"], DEV, True, keep=1.0 - c["trim"])[1].clone()
        base, gbase = launch(args), grad(case, c["trim"], c["alpha"], c["stable_scale"])
        same_bits(base, launch(args))
        same_bits(gbase, grad(case, c["trim"], c["alpha"], c["stable_scale"]))
        drop = case["mask"] == 0
        poisoned = dict(case)
        for k, vals in (("pred", (np.nan, np.inf)), ("target", (-np.inf, np.nan))):
            x = case[k].copy()
            x[drop] = np.where(np.arange(drop.sum()) % 2 == 0, vals[0], vals[1]).astype(np.float32)
            poisoned[k] = x
        assert drop.any() and np.isnan(poisoned["pred"]).any() and np.isinf(poisoned["target"]).any()
        same_bits(base, launch([dev(poisoned[k]) for k in ("pred", "target", "mask")]))
        same_bits(gbase, grad(poisoned, c["trim"], c["alpha"], c["stable_scale"]))


def test_an_items_gradient_stays_inside_the_item():
    """The fit, the frame chain and the temporal pairs belong to one item; the selection is the batch's. Item 1's prediction
    moves by a relative 1e-6 per pixel, little enough that no residual crosses a threshold (asserted on the restatement: the
    same counts and the same weight u on every element of both items; a threshold that item 1 owns may move with it; targets
    and masks, which every count depends on, stay). Item 0's gradient then keeps its bits, and item 1's does not."""
    case, r = oracle(1, (1.0, 0.0, 0.0, 1.0))                 # [2, 3, 17, 13], trim 0.2
    trim = CASES[1]["trim"]
    other = dict(case)
    other["pred"] = case["pred"].copy()
    other["pred"][1] *= (1 + 1e-6 * np.random.default_rng(5).standard_normal(case["pred"][1].shape)).astype(np.float32)
    assert (other["pred"][1] != case["pred"][1]).mean() > 0.5
    moved = TR.depth_loss_trim_ref(other["pred"], other["target"], other["mask"], trim=trim)
    for k in ("trim_k", "trim_less", "trim_tied", "trim_weight"):
        assert np.array_equal(moved[k], r["fwd"][k]), f"{k}: the move changed the selection; choose a smaller one"
    assert moved["trim_tied"].tolist() == [1, 1, 1]
    for term in TR.TERMS:
        assert np.array_equal(r["fwd"]["sel"][term]["u"], moved["sel"][term]["u"]), term
    a, b = grad(case, trim, weights=(1, 0, 0, 1)), grad(other, trim, weights=(1, 0, 0, 1))
    same_bits(a[0], b[0])
    assert (a[1] != b[1]).any()


def test_trim_zero_is_the_untrimmed_criterion_bit_for_bit():
    from vdn import loss as L
    case, _ = oracle(1)
    p, t, k = (dev(case[n]) for n in ("pred", "target", "mask"))
    a, b = L.TrimmedVideoDepthLoss(trim=0.0)(p, t, k), L.VideoDepthLoss()(p, t, k)
    assert a.keys() == b.keys()
    for n in a:
        same_bits(a[n], b[n])
    same_bits(L.depth_loss_grad(p, t, k, trim=0.0), L.depth_loss_grad(p, t, k))
    q0, q1 = p.clone().requires_grad_(), p.clone().requires_grad_()
    L.TrimmedVideoDepthLoss(trim=0)(q0, t, k)["total_loss"].backward()
    L.VideoDepthLoss()(q1, t, k)["total_loss"].backward()
    same_bits(q0.grad, q1.grad)
    plain, zero = L.depth_loss(p, t, k), L.depth_loss(p, t, k, trim=0.0)
    assert plain.keys() == zero.keys() and "trim_k" not in zero and all(plain[n] == zero[n] for n in VALUES)
