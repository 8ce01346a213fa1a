"""The depth criterion's gradient on the device (csrc/loss_grad.hip, vdn.loss) against the CPU restatement
tests/loss_grad_ref.py: on the 14 recorded cases of tests/golden/loss_cases.npz (whose reference gradients
tests/test_loss_grad_host.py holds the restatement to) and on four cases the reference is not consulted for, then through
autograd, and the properties the kernels promise: saved state, determinism, views and mask types, locality.

Bar, per element: |got - want| <= 4 * 2^-24 * (|sc * g_a| + |fit correction|) + 1e-30. Both sides take the same fp64 steps
from the same float32 samples and differ in the order of the per-frame and per-item sums (1e-16 relative); the device then
rounds g_p = sc * g_a + fit correction to float32 once, an error of at most 2^-24 * |g_p| <= 2^-24 * (|sc * g_a| + |fit
correction|). The bar allows two such roundings and a factor 2 over that."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import loss_grad_ref as G
import loss_ref as R
from test_loss_grad_host import oracle
from test_loss_host import CASES, case_id

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXTRA = ("flat-frame", "two-trips-quads", "two-trips-single", "quads-cross-rows")


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def ratio_to_bound(got, r):
    """The largest |got - want| over the bar of this file, for a float32 gradient `got` and the restatement's dictionary."""
    bound = 4.0 * 2.0 ** -24 * (r["mag_a"] + r["mag_fit"]) + 1e-30
    return float((np.abs(got.astype(np.float64) - r["grad"]) / bound).max())


@functools.lru_cache(maxsize=None)
def extra(name):
    """The oracle-only cases: inputs, arguments and the restatement, computed once, shared and never written.
    flat-frame        the kept predictions of frame 1 are all equal: s_raw = 0 < 1e-6, the clamp's branch with g_s = 0; every
                      kept pixel shares the median's value, so the lowest index holds it;
    two-trips-quads   [1, 2, 184, 180]: 33 120 pixels a frame, above the 32 768 that 32 blocks x 256 lanes x 4 pixels cover in
                      one trip, so the lanes' stride loop runs a second time on the four-pixel path;
    two-trips-single  [1, 2, 181, 183]: 33 123 pixels, not a multiple of 4: the same on the one-pixel path, which runs five trips;
    quads-cross-rows  [1, 2, 6, 6]: H * W is a multiple of 4 and W is not, so every second quad of a lane spans a row's end (as at
                      518 x 518): the stencil must take each pixel's own row and column, not its quad's."""
    if name == "flat-frame":
        case = R.make_case(81, (1, 3, 9, 11), 0.8)
        case["pred"][0, 1] = np.float32(2.5)
    elif name == "quads-cross-rows":
        case = R.make_case(84, (1, 2, 6, 6), 0.8)
    else:
        case = R.make_case(82 if name == "two-trips-quads" else 83, (1, 2, 184, 180) if name == "two-trips-quads" else (1, 2, 181, 183), 0.8)
    r = G.depth_loss_grad_ref(case["pred"], case["target"], case["mask"])
    for a in list(case.values()) + [r["grad"], r["mag_a"], r["mag_fit"]]:
        a.setflags(write=False)
    return case, r


def grad(case, alpha=0.5, stable_scale=10, **kw):
    from vdn import loss as L
    return L.depth_loss_grad(dev(case["pred"]), dev(case["target"]), dev(case["mask"]), alpha=alpha, stable_scale=stable_scale, **kw)


def same_bits(a, b):
    a, b = (x.detach().cpu().numpy() for x in (a, b))
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(got, case, r, what):
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == case["pred"].shape
    g = got.cpu().numpy()
    worst = ratio_to_bound(g, r)
    print(f"[{what}] largest |got - want| / bound {worst:.3f}; max |g| {np.abs(r['grad']).max():.3g}")
    drop = case["mask"] == 0
    assert not g[drop].any() and not np.signbit(g[drop]).any()       # +0.0 under every dropped pixel
    assert worst <= 1.0


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: case_id(CASES[i]))
def test_gradient_matches_the_restatement(i):
    c = CASES[i]
    case, r = oracle(i)
    check(grad(case, c["alpha"], c["stable_scale"]), case, r, case_id(c))


@pytest.mark.parametrize("key", ["spatial_loss", "stable_loss", "absRel_loss"])
def test_each_entry_alone_matches_the_restatement(key):
    from test_loss_grad_host import KEYS
    for i in (0, 11) + ((5,) if key == "absRel_loss" else ()):   # seeds 41 and 52, and 46 for absRel (recorded alone too)
        c = CASES[i]
        assert c["seed"] in (41, 52, 46)
        case, r = oracle(i, key)
        check(grad(case, c["alpha"], c["stable_scale"], weights=KEYS[key]), case, r, f"{case_id(c)} {key}")


@pytest.mark.parametrize("name", EXTRA)
def test_oracle_only_cases(name):
    case, r = extra(name)
    if name == "flat-frame":
        keep1 = case["mask"][0, 1] != 0
        assert r["g_s"][0, 1] == 0 and r["fwd"]["s_pred"][0, 1] == 1e-6 and r["holder"][0, 1] == np.flatnonzero(keep1.ravel())[0]
        assert r["g_s"][0, 0] != 0 and r["g_m"][0, 1] != 0
    elif name == "quads-cross-rows":
        H, W = case["pred"].shape[2:]
        assert H * W % 4 == 0 and W % 4 != 0 and dev(case["pred"]).data_ptr() % 16 == 0
    else:
        H, W = case["pred"].shape[2:]
        from vdn import loss as L
        assert H * W > L.trip_pixels(True) and (H * W % 4 == 0) == (name == "two-trips-quads")   # one trip of the wider sweep
    check(grad(case), case, r, name)


def test_autograd_gives_depth_loss_grads_bits():
    """Fails without the feature: forward's values then have no grad_fn."""
    from vdn import loss as L
    case, _ = oracle(0)
    p, t, k = (dev(case[n]) for n in ("pred", "target", "mask"))
    crit = L.VideoDepthLoss()
    q = p.clone().requires_grad_()
    out = crit(q, t, k)
    assert tuple(out) == crit.keys and all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in out.values())
    assert out["total_loss"].grad_fn is not None
    out["total_loss"].backward()
    assert q.grad.dtype == torch.float32 and q.grad.shape == q.shape
    same_bits(q.grad, L.depth_loss_grad(p, t, k))
    # 3 * total + 2 * absRel, with d1 in the sum: the coefficients, and the zero for d1
    q = p.clone().requires_grad_()
    out = crit(q, t, k)
    (3 * out["total_loss"] + 2 * out["absRel_loss"] + 5 * out["d1"]).backward()
    same_bits(q.grad, L.depth_loss_grad(p, t, k, weights=(3, 0, 0, 2)))
    # no double backward: asked for with create_graph=True the gradient is the same and carries no graph, so a second
    # derivative raises instead of coming out as a silent zero
    q = p.clone().requires_grad_()
    g, = torch.autograd.grad(crit(q, t, k)["total_loss"], q, create_graph=True)
    same_bits(g, L.depth_loss_grad(p, t, k))
    assert g.grad_fn is None and not g.requires_grad
    with pytest.raises(RuntimeError, match="does not require grad"):
        g.sum().backward()
    with pytest.raises(NotImplementedError, match="target"):
        crit(q, t.clone().requires_grad_(), k)


def test_without_a_gradient_forward_is_what_it_was():
    from vdn import loss as L
    case, _ = oracle(0)
    p, t, k = (dev(case[n]) for n in ("pred", "target", "mask"))
    crit = L.VideoDepthLoss()
    base = crit(p, t, k)
    assert all(v.grad_fn is None and not v.requires_grad for v in base.values())
    with torch.no_grad():
        quiet = crit(p.clone().requires_grad_(), t, k)
    tracked = crit(p.clone().requires_grad_(), t, k)
    assert all(v.grad_fn is None for v in quiet.values()) and all(v.grad_fn is not None for v in tracked.values())
    for other in (quiet, tracked):
        assert other.keys() == base.keys()
        for n in base:
            same_bits(base[n], other[n])


def test_backward_reads_its_own_saved_state():
    """Two criteria evaluated on different inputs before either backward: the runtime's result buffer holds the second call's
    state by then."""
    from vdn import loss as L
    a, b = (oracle(i)[0] for i in (0, 9))                     # the same shape, different inputs; case 9 has an empty item
    args = [[dev(c[n]) for n in ("pred", "target", "mask")] for c in (a, b)]
    alone = [L.depth_loss_grad(*x) for x in args]
    qs = [x[0].clone().requires_grad_() for x in args]
    outs = [L.VideoDepthLoss()(q, x[1], x[2]) for q, x in zip(qs, args)]
    for o in outs:
        o["total_loss"].backward()
    for q, want in zip(qs, alone):
        same_bits(q.grad, want)


def test_two_runs_give_the_same_bits_and_dropped_pixels_reach_nothing():
    for i in (0, 8, 9):                                       # plain, an empty frame, an empty item
        case, _ = oracle(i)
        c = CASES[i]
        base = grad(case, c["alpha"], c["stable_scale"])
        same_bits(base, grad(case, c["alpha"], c["stable_scale"]))
        drop = case["mask"] == 0
        poisoned = dict(case)
        for k, vals in (("pred", (np.nan, np.inf)), ("target", (-np.inf, np.nan))):
            x = case[k].copy()
            x[drop] = np.where(np.arange(drop.sum()) % 2 == 0, vals[0], vals[1]).astype(np.float32)
            poisoned[k] = x
        assert drop.any() and np.isnan(poisoned["pred"]).any() and np.isinf(poisoned["target"]).any()
        got = grad(poisoned, c["alpha"], c["stable_scale"])
        same_bits(base, got)
        g = got.cpu().numpy()
        assert not g[drop].any() and not np.signbit(g[drop]).any()


def test_views_mask_types_and_dtypes():
    from vdn import loss as L
    case, r = oracle(2)                                       # [1, 4, 16, 16]: whole quads
    p, t, m = (dev(case[k]) for k in ("pred", "target", "mask"))
    base = L.depth_loss_grad(p, t, m)
    # both planes 4 bytes past a 16-byte boundary: a load per pixel, where the aligned tensors take 16-byte loads. A lane owns
    # the same four pixels either way, so the gradient has the same bits.
    off = [torch.empty(p.numel() + 1, device=DEV)[1:].view(p.shape).copy_(x) for x in (p, t)]
    assert all(o.data_ptr() % 16 == 4 and o.is_contiguous() for o in off) and p.data_ptr() % 16 == 0
    single = L.depth_loss_grad(off[0], off[1], m)
    check(single, case, r, "a load per pixel")
    same_bits(single, base)
    # the same through autograd: the prediction a 4-byte-offset view, its gradient the aligned tensor's bits
    q = off[0].detach().requires_grad_()
    L.VideoDepthLoss()(q, off[1], m)["total_loss"].backward()
    same_bits(q.grad, base)
    for mask in (m.to(torch.uint8), m.float() * 3.0):
        same_bits(base, L.depth_loss_grad(p, t, mask))
    q = p.half().requires_grad_()
    L.VideoDepthLoss()(q, t, m)["total_loss"].backward()
    assert q.grad.dtype == torch.float16 and q.grad.shape == q.shape
    same_bits(q.grad, L.depth_loss_grad(q.detach().float(), t, m).half())


def test_an_items_gradient_stays_inside_the_item():
    """The fit and the temporal pairs belong to one item. Item 1's prediction changes; its target and mask stay, because the
    counts that divide every term (kept pixels, grid points, temporal pairs, absRel pixels) are sums over the whole batch and
    depend on targets and masks alone. Item 0's gradient keeps its bits."""
    case, _ = oracle(0)                                       # [2, 3, 17, 13]
    other = dict(case)
    other["pred"] = case["pred"].copy()
    other["pred"][1] = R.make_case(91, case["pred"].shape, 0.8)["pred"][1]
    a, b = grad(case, weights=(1, 0, 0, 1)), grad(other, weights=(1, 0, 0, 1))
    same_bits(a[0], b[0])
    assert (a[1] != b[1]).any()


def test_a_frames_gradient_stays_inside_the_frame():
    """stable_scale = 0 and T = 1 items: every frame has its own fit, and nothing but the batch's counts ties the frames
    together. Two frames with one mask double every count, so each frame's gradient in the pair is exactly half of its
    gradient alone; a neighbour read across the frame's end would break that."""
    x, y = R.make_case(92, (1, 1, 17, 13), 0.8), R.make_case(93, (1, 1, 17, 13), 0.8)
    y["mask"] = x["mask"]
    pair = {k: np.concatenate([x[k], y[k]], 0) for k in x}
    both = grad(pair, stable_scale=0)
    for b, one in enumerate((x, y)):
        alone = grad(one, stable_scale=0)
        assert alone.abs().max().item() > 0
        same_bits(both[b:b + 1], alone * 0.5)
