"""The normal criterion's gradient on the device (csrc/normals_grad.hip, vdn.normals) against the CPU restatement
tests/normal_grad_ref.py: on the recorded cases of tests/golden/normal_grad_cases.npz (whose reference gradients
tests/test_normal_grad_host.py holds the restatement to), against a stored target and against a depth target, and on shapes
the reference is not consulted for; then through autograd, in the training step beside VideoDepthLoss, and the properties the
kernel promises: saved state, determinism, dropped pixels, locality, views and mask types.

Bar, per element: |got - want| <= 2^-23 * |want| + 2^-40 * mag + 1e-30, mag = |coeff| / (N n) * (|that_c| + |p . that| / n *
|p_c| / |p|) as the restatement returns it. Both sides take the same fp64 steps from the same float32 samples. The device
rounds once to float32, an error of at most 2^-24 |want|; the fp64 cancellation in that_c - (..) p_c / |p| is below 2^-50 mag.
The bar allows twice the former and a wide margin on the latter. It is derived, not measured."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import normal_grad_ref as G
import normal_ref as R
from test_normal_grad_host import CASES, KINDS, RECORDED, SPECIAL, case_id, inputs, oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
#         name               (B, T, H, W)
SHAPES = {"min-reflect": (1, 1, 2, 2),         # reflect pad at its minimum, every pixel on two borders
          "quads-cross-rows": (1, 2, 6, 6),    # H * W % 4 == 0 and W % 4 != 0: quads cross row ends
          "single-narrow": (1, 2, 7, 5),       # an odd pixel count: the one-pixel path; W < 6: no quad could share columns
          "quads-in-rows": (2, 2, 9, 12),      # every quad inside one row
          "two-trips-quads": (1, 1, 259, 256),  # one frame larger than one trip of the grid, on the four-pixel path
          "two-trips-single": (1, 1, 259, 257)}  # one more column: the one-pixel path, five trips


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def same_bits(a, b):
    a, b = (x.detach().cpu().numpy() for x in (a, b))
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def grad(case, kind="stored", masked=True, **kw):
    from vdn import normals as N
    return N.normal_loss_grad(dev(case["pred"]), dev(case["depth" if kind == "depth" else "target"]),
                              dev(case["mask"]) if masked else None, from_depth=kind == "depth", **kw)


def dropped(case, masked=True):
    keep = R.erode_ref(case["mask"]) if masked else np.ones(case["mask"].shape, bool)
    return np.broadcast_to(~keep[:, :, None], case["pred"].shape)


def check(got, case, want, mag, what, masked=True):
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == case["pred"].shape
    g = got.cpu().numpy()
    bound = 2.0 ** -23 * np.abs(want) + 2.0 ** -40 * mag + 1e-30
    worst = float((np.abs(g.astype(np.float64) - want) / bound).max())
    print(f"[{what}] largest |got - want| / bound {worst:.3f}; max |g| {np.abs(want).max():.3g}")
    drop = dropped(case, masked)
    assert not g[drop].any() and not np.signbit(g[drop]).any()      # +0.0 under every dropped pixel
    assert worst <= 1.0


@functools.lru_cache(maxsize=None)
def extra(name, kind, masked):
    """An oracle-only case and the restatement on it, computed once, shared and never written."""
    shape = SHAPES[name]
    case = R.make_case(100 + list(SHAPES).index(name), shape, "bool", "scaled", false_rate=0.06)
    grad_, mag = G.normal_loss_grad_ref(case["pred"], case["depth" if kind == "depth" else "target"], case["mask"] if masked else None,
                                        kind == "depth")
    for a in list(case.values()) + [grad_, mag]:
        a.setflags(write=False)
    return case, grad_, mag


@pytest.mark.parametrize("i,kind", RECORDED, ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_gradient_matches_the_restatement(i, kind):
    case, want, mag = oracle(i, kind)
    nomask = i != SPECIAL and CASES[i]["mask_kind"] == "none"      # an all-true mask, given as None: the NULL mask
    check(grad(case, kind, masked=not nomask), case, want, mag, f"{case_id(i)} {kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_oracle_only_shapes(name, kind):
    from vdn import normals as N
    B, T, H, W = SHAPES[name]
    wide = H * W % 4 == 0
    if name.startswith("two-trips"):
        assert N.grad_trip_pixels(True) == 65536 and N.grad_trip_pixels(False) == 16384   # what the shapes above were chosen for
        assert H * W > N.grad_trip_pixels(wide) and wide == (name == "two-trips-quads")
    elif name == "quads-cross-rows":
        assert wide and W % 4 != 0
    elif name == "single-narrow":
        assert not wide and W < 6
    elif name == "quads-in-rows":
        assert W % 4 == 0 and W >= 6
    for masked in (False, True):
        case, want, mag = extra(name, kind, masked)
        if wide:
            assert dev(case["pred"]).data_ptr() % 16 == 0
        if masked and name != "min-reflect":
            keep = R.erode_ref(case["mask"])
            assert keep.any() and not keep.all()
        check(grad(case, kind, masked), case, want, mag, f"{name} {kind} {'masked' if masked else 'no mask'}", masked)


def test_autograd_gives_normal_loss_grads_bits():
    """Fails without the feature: forward's value then has no grad_fn."""
    from vdn import normals as N
    case = inputs(1)
    p, t, d, k = (dev(case[n]) for n in ("pred", "target", "depth", "mask"))
    crit = N.VideoNormalLoss()
    q = p.clone().requires_grad_()
    out = crit(q, t, k)
    v = out["normal_loss"]
    assert list(out) == ["normal_loss"] and v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda
    assert v.grad_fn is not None
    v.backward()
    assert q.grad.dtype == torch.float32 and q.grad.shape == q.shape
    same_bits(q.grad, N.normal_loss_grad(p, t, k))
    q = p.clone().requires_grad_()
    (3 * crit(q, t, k)["normal_loss"]).backward()
    same_bits(q.grad, N.normal_loss_grad(p, t, k, coeff=3))
    # no double backward: asked for with create_graph=True the gradient is the same and carries no graph, so a second
    # derivative raises instead of coming out as a silent zero
    q = p.clone().requires_grad_()
    g, = torch.autograd.grad(crit(q, t, k)["normal_loss"], q, create_graph=True)
    same_bits(g, N.normal_loss_grad(p, t, k))
    assert g.grad_fn is None and not g.requires_grad
    with pytest.raises(RuntimeError, match="does not require grad"):
        g.sum().backward()
    with pytest.raises(NotImplementedError, match="target"):
        crit(q, t.clone().requires_grad_(), k)
    with pytest.raises(NotImplementedError, match="gt_depth"):
        crit.forward_from_depth(q, d.clone().requires_grad_(), k)
    # the target made on the fly
    for depth in (d, d[:, :, None]):
        q = p.clone().requires_grad_()
        out = crit.forward_from_depth(q, depth, k)
        assert list(out) == ["normal_loss"] and out["normal_loss"].grad_fn is not None
        assert out["normal_loss"].item() == pytest.approx(N.normal_loss_from_depth(p, d, k), abs=1e-7)
        out["normal_loss"].backward()
        same_bits(q.grad, N.normal_loss_grad(p, d, k, from_depth=True))


def test_the_training_step():
    """scripts/train.py:441-447 with both criteria from this package on one clip. The coefficient 0.7 reaches the normal
    criterion's backward as the float32 tensor autograd makes of it (grad_output * 0.7 in the loss's dtype) and crosses to the
    kernel widened to float64, which is exact; normal_loss_grad(coeff=0.7) rounds its coefficient to float32 the same way."""
    import loss_ref
    from vdn import loss as L, normals as N
    shape = (1, 3, 16, 20)
    dc, nc = loss_ref.make_case(95, shape, 0.95), R.make_case(96, shape, "bool")
    mask = dev(dc["mask"])
    pd, td, pn, tn = dev(dc["pred"]), dev(dc["target"]), dev(nc["pred"]), dev(nc["target"])
    pred_depths, pred_normals = pd.clone().requires_grad_(), pn.clone().requires_grad_()
    depth_loss_dict = L.VideoDepthLoss()(pred_depths, td, mask)
    normal_loss_dict = N.VideoNormalLoss()(pred_normals, tn, mask)
    total_loss = depth_loss_dict["total_loss"] + normal_loss_dict["normal_loss"] * 0.7
    total_loss.backward()
    assert pred_depths.grad is not None and pred_normals.grad is not None and pred_normals.grad.abs().max().item() > 0
    same_bits(pred_depths.grad, L.depth_loss_grad(pd, td, mask))
    same_bits(pred_normals.grad, N.normal_loss_grad(pn, tn, mask, coeff=0.7))
    want, mag = G.normal_loss_grad_ref(nc["pred"], nc["target"], dc["mask"], coeff=0.7)
    check(pred_normals.grad, dict(nc, mask=dc["mask"]), want, mag, "training step, coeff 0.7")


def test_without_a_gradient_forward_is_what_it_was():
    from vdn import normals as N
    case = inputs(1)
    p, t, d, k = (dev(case[n]) for n in ("pred", "target", "depth", "mask"))
    crit = N.VideoNormalLoss()
    for fn, tgt in ((crit, t), (crit.forward_from_depth, d)):
        base = fn(p, tgt, k)["normal_loss"]
        assert base.grad_fn is None and not base.requires_grad
        with torch.no_grad():
            quiet = fn(p.clone().requires_grad_(), tgt, k)["normal_loss"]
        tracked = fn(p.clone().requires_grad_(), tgt, k)["normal_loss"]
        assert quiet.grad_fn is None and tracked.grad_fn is not None
        same_bits(base, quiet)
        same_bits(base, tracked.detach())
    assert float(crit(p, t, k)["normal_loss"]) == pytest.approx(N.normal_loss(p, t, k), abs=1e-7)


def test_backward_reads_its_own_saved_state():
    """Two criteria evaluated on different inputs before either backward: the runtime's result buffer holds the second call's
    count by then. The two cases keep different numbers of pixels."""
    from vdn import normals as N
    a, b = inputs(1), inputs(2)
    assert R.erode_ref(a["mask"]).sum() != R.erode_ref(b["mask"]).sum()
    args = [[dev(c[n]) for n in ("pred", "target", "mask")] for c in (a, b)]
    alone = [N.normal_loss_grad(*x) for x in args]
    qs = [x[0].clone().requires_grad_() for x in args]
    outs = [N.VideoNormalLoss()(q, x[1], x[2]) for q, x in zip(qs, args)]
    for o in outs:
        o["normal_loss"].backward()
    for q, want in zip(qs, alone):
        same_bits(q.grad, want)


def test_two_runs_give_the_same_bits_and_dropped_pixels_reach_nothing():
    """NaN and inf under the pixels the erosion drops, in prediction and stored target; in the depth under the pixels the mask
    itself drops (a pixel that only the erosion drops has a kept neighbour, whose stencil reads its depth, here as in the
    reference). The gradient keeps its bits and is +0.0 there."""
    for i in (1, 4):                                          # a bool mask; B = 2 with a frame that keeps nothing
        case = inputs(i)
        drop = ~R.erode_ref(case["mask"])
        drop3 = np.broadcast_to(drop[:, :, None], case["pred"].shape)
        raw = case["mask"] == 0
        poisoned = dict(case)
        for k, where, vals in (("pred", drop3, (np.nan, np.inf)), ("target", drop3, (-np.inf, np.nan)), ("depth", raw, (np.nan, -np.inf))):
            x = case[k].copy()
            x[where] = np.where(np.arange(where.sum()) % 2 == 0, vals[0], vals[1]).astype(np.float32)
            poisoned[k] = x
        assert drop.any() and raw.any() and np.isnan(poisoned["pred"]).any() and np.isinf(poisoned["target"]).any()
        for kind in KINDS:
            base = grad(case, kind)
            same_bits(base, grad(case, kind))
            got = grad(poisoned, kind)
            same_bits(base, got)
            g = got.cpu().numpy()
            assert np.isfinite(g).all() and not g[drop3].any() and not np.signbit(g[drop3]).any()


def test_nothing_kept_gives_positive_zeros():
    """An all-false mask, and a mask whose every third column is false, which keeps nothing after the erosion although two
    thirds of it are true: N = 0, the loss is sum * 0 and the gradient +0.0 everywhere, not 0 / 0."""
    from vdn import normals as N
    case = dict(inputs(1))
    thirds = np.ones(case["mask"].shape, bool)
    thirds[..., 1::3] = False
    assert thirds.mean() > 0.6 and not R.erode_ref(thirds).any()
    for mask in (np.zeros_like(thirds), thirds):
        case["mask"] = mask
        for kind in KINDS:
            g = grad(case, kind).cpu().numpy()
            assert not np.isnan(g).any() and not g.any() and not np.signbit(g).any()
        q = dev(case["pred"]).requires_grad_()
        out = N.VideoNormalLoss()(q, dev(case["target"]), dev(mask))["normal_loss"]
        assert out.item() == 1.0
        out.backward()
        assert not q.grad.cpu().numpy().any() and not np.signbit(q.grad.cpu().numpy()).any()


def test_a_frames_gradient_stays_inside_the_frame():
    """Nothing but the batch's count ties the frames together. Two frames with one mask double N, so each frame's gradient in
    the pair is exactly half of its gradient alone; a neighbour read across the frame's end would break that."""
    x, y = R.make_case(111, (1, 1, 10, 12), "bool"), R.make_case(112, (1, 1, 10, 12), "bool")
    y["mask"] = x["mask"]
    pair = {k: np.concatenate([x[k], y[k]], 1) for k in x}
    for kind in KINDS:
        both = grad(pair, kind)
        for f, one in enumerate((x, y)):
            alone = grad(one, kind)
            assert alone.abs().max().item() > 0
            same_bits(both[:, f:f + 1], alone * 0.5)


def test_views_mask_types_and_dtypes():
    from vdn import normals as N
    case, want, mag = oracle(2, "stored")                     # [1, 2, 24, 18]: whole quads, a float mask
    p, t, d, m = (dev(case[k]) for k in ("pred", "target", "depth", "mask"))
    H, W = p.shape[-2:]
    assert H * W % 4 == 0 and p.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0
    base, base_d = N.normal_loss_grad(p, t, m), N.normal_loss_grad(p, d, m, from_depth=True)
    # both tensors 4 bytes past a 16-byte boundary: a load per pixel, where the aligned tensors take 16-byte loads and stores
    off = [torch.empty(x.numel() + 1, device=DEV)[1:].view(x.shape).copy_(x) for x in (p, t)]
    assert all(o.data_ptr() % 16 == 4 and o.is_contiguous() for o in off)
    single = N.normal_loss_grad(off[0], off[1], m)
    check(single, case, want, mag, "a load per pixel")
    same_bits(single, base)
    same_bits(N.normal_loss_grad(off[0], d, m, from_depth=True), base_d)
    # the same through autograd: the prediction a 4-byte-offset view, then a non-contiguous one (channels last in memory)
    q = off[0].detach().requires_grad_()
    N.VideoNormalLoss()(q, off[1], m)["normal_loss"].backward()
    same_bits(q.grad, base)
    q = p.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3).detach().requires_grad_()
    assert not q.is_contiguous() and q.shape == p.shape
    N.VideoNormalLoss().forward_from_depth(q, d, m)["normal_loss"].backward()
    assert q.grad.shape == q.shape
    same_bits(q.grad.contiguous(), base_d)
    for mask in (m.to(torch.uint8), m.float() * 3.0, m != 0):
        same_bits(base, N.normal_loss_grad(p, t, mask))
    q = p.half().requires_grad_()
    N.VideoNormalLoss()(q, t, m)["normal_loss"].backward()
    assert q.grad.dtype == torch.float16 and q.grad.shape == q.shape
    same_bits(q.grad, N.normal_loss_grad(q.detach().float(), t, m).half())
