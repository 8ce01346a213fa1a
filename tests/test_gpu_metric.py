"""The metric-depth criterion and scores on the device (csrc/metric.hip, vdn.metric, vdn.steps) against the numpy restatement
tests/metric_ref.py, which tests/test_metric_host.py holds to what the reference's own functions recorded.

Bars. n and d1 d2 d3: equal bits (the same float32 operations on both sides). The six fp64 metrics and the loss: 1e-9 relative,
test_gpu_eval.py's bar with its reasoning: both sides are fp64 with different summation orders, and n * 2^-53 <= 9e-11 at the
largest shape here (786 432 pixels); the rest is margin for log and sqrt. The gradient: within one float32 ulp of
float32(restated gradient), which is rounded once from fp64 on both sides, and exactly +0.0 at dropped pixels. NaN meets NaN.

test_past_one_grid_pass takes its sizes from the kernels' own launch constants: vdn_metric_trip(wide) = MT_BPI (256 blocks per
item) * 256 lanes * 4 or 1 elements, of which a lane issues MT_INFLIGHT = 4 trips together before its loop comes round."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import metric_ref as R
from test_metric_host import MAX_DEPTH, MIN_DEPTH, RECORDED, case_id, case_inputs, same_f32_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 1e-9
INFLIGHT = 4     # MT_INFLIGHT of csrc/metric.hip


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def same_bits(a, b):
    a, b = (x.detach().cpu().numpy() for x in (a, b))
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_rows(got, want):
    """got: the device's float64 [B, 10]; want: metric_ref's."""
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == want.shape
    g = got.cpu().numpy()
    assert np.array_equal(g[:, 0], want[:, 0]), (g[:, 0], want[:, 0])
    same_f32_bits(g[:, 1:4], want[:, 1:4])
    assert np.array_equal(g[:, 1:4].astype(np.float32).astype(np.float64), g[:, 1:4], equal_nan=True)   # float32 quotients
    a, b = g[:, 4:], want[:, 4:]
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    ok = ~np.isnan(b)
    rel = np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), np.finfo(np.float64).tiny)
    rel = np.where(a[ok] == b[ok], 0.0, rel)
    print(f"rows {want.shape[0]}, n {want[:, 0].astype(int).tolist()}: six metrics max rel {rel.max(initial=0.0):.2e}")
    assert (rel <= BAR).all(), (rel.max(), a, b)


def check_loss(got, want):
    """got: vdn.metric.silog_loss's dict; want: metric_ref.silog_ref's [4]."""
    assert got["n"] == int(want[1])
    for a, b in ((got["loss"], want[0]), (got["sum"], want[2]), (got["sum_sq"], want[3])):
        assert np.isnan(a) == np.isnan(b), (got, want)
        if not np.isnan(b):
            print(f"loss state {a!r} against {b!r}")
            assert abs(a - b) <= BAR * abs(b), (a, b)


def check_grad(got, want, keep):
    """got: the device's float32 gradient; want: metric_ref's float64 one."""
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == want.shape
    g, w = got.cpu().numpy(), want.astype(np.float32)
    assert not g[~keep].any() and not np.signbit(g[~keep]).any()          # exactly +0.0 at dropped pixels
    assert np.array_equal(np.isnan(g), np.isnan(w))
    ok = ~np.isnan(w)
    ulps = np.abs(g[ok].astype(np.float64) - w[ok].astype(np.float64)) / np.spacing(np.abs(w[ok])).astype(np.float64)
    print(f"gradient {want.shape}: {int((ulps > 0).sum())} of {int(ok.sum())} elements off float32(restated), worst {ulps.max(initial=0.0):.2f} ulp")
    assert (ulps <= 1.0).all()


@functools.lru_cache(maxsize=None)
def extra(shape, mask="bool", special="plain", seed=700, lambd=0.5, pshape=None):
    """A case the reference is not consulted for and the restatement on it, computed once, shared and never written."""
    c = R.case_dict(seed, shape, mask, special, lambd)
    case = R.make_case(c, pshape)
    keep = R.keep_mask(case["mask"], case["depth"], MIN_DEPTH, MAX_DEPTH)
    rows = R.eval_rows(case["pred"], case["depth"], case["mask"], MIN_DEPTH, MAX_DEPTH)
    state = grad = None
    if pshape is None:
        state = R.silog_ref(case["pred"], case["depth"], keep, lambd)
        grad = R.silog_grad_ref(case["pred"], case["depth"], keep, lambd)
    for a in (case["pred"], case["depth"], case["mask"], keep, rows, state, grad):
        if a is not None:
            a.setflags(write=False)
    return c, case, keep, rows, state, grad


def check_everything(c, case, keep, rows, state, grad):
    """The metrics, the loss (fused mask and precomposed mask) and the gradient (autograd and silog_loss_grad) of one case."""
    from vdn import metric
    p, d, m = dev(case["pred"]), dev(case["depth"]), dev(case["mask"])
    check_rows(metric.eval_depth_batch(p, d, m, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH), rows)
    check_loss(metric.silog_loss(p, d, m, c["lambd"], min_depth=MIN_DEPTH, max_depth=MAX_DEPTH), state)
    crit = metric.SiLogLoss(c["lambd"])
    fused = crit.forward_from_valid(p, d, m, MIN_DEPTH, MAX_DEPTH)
    assert fused.dtype == torch.float32 and fused.dim() == 0 and fused.is_cuda and fused.grad_fn is None
    plain = crit(p, d, dev(keep))
    same_bits(fused, plain)                                          # the fused mask is the composed mask
    same_f32_bits(fused.cpu().numpy(), np.float32(metric.silog_loss(p, d, dev(keep), c["lambd"])["loss"]))
    pg = p.clone().requires_grad_(True)
    loss = crit.forward_from_valid(pg, d, m, MIN_DEPTH, MAX_DEPTH)
    same_bits(loss.detach(), fused)
    loss.backward()
    check_grad(pg.grad, grad, keep)
    same_bits(metric.silog_loss_grad(p, d, m, c["lambd"], min_depth=MIN_DEPTH, max_depth=MAX_DEPTH), pg.grad)
    same_bits(metric.silog_loss_grad(p, d, dev(keep), c["lambd"]), pg.grad)


@pytest.mark.parametrize("rec", RECORDED, ids=case_id)
def test_recorded_cases(rec):
    """Every case of the fixture, the edge rows of include/vdn.h among them: no kept pixel (NaN, zero gradient), pred == target
    (0, NaN at kept pixels), a negative radicand (NaN, NaN at kept pixels), the bounds and their neighbours, mask values other
    than 0 and 1, thresh exactly at a threshold, items of 9 and 10 pixels."""
    _, c, checksum, want = rec
    case = case_inputs(c, checksum)
    keep = R.keep_mask(case["mask"], case["depth"], MIN_DEPTH, MAX_DEPTH)
    rows = R.eval_rows(case["pred"], case["depth"], case["mask"], MIN_DEPTH, MAX_DEPTH)
    state = R.silog_ref(case["pred"], case["depth"], keep, c["lambd"])
    grad = R.silog_grad_ref(case["pred"], case["depth"], keep, c["lambd"])
    check_everything(c, case, keep, rows, state, grad)
    sp = c["special"]
    if sp == "empty_all":
        assert np.isnan(state[0]) and not grad.any()
    if sp in ("equal", "negative_radicand"):
        assert (state[0] == 0.0 if sp == "equal" else np.isnan(state[0])) and np.isnan(grad[keep]).all()


#                                  less than a wave; small and odd; several blocks per item, odd width, two items; one real frame
@pytest.mark.parametrize("shape,mask", [((1, 2, 3), "bool"), ((3, 5, 7), "uint8"), ((2, 64, 257), "float"), ((1, 768, 1024), "bool")],
                         ids=str)
def test_shapes(shape, mask):
    c, case, keep, rows, state, grad = extra(shape, mask)
    if shape[0] > 1:                    # the items of a batch differ, so mixing them up shows
        assert len({tuple(r) for r in rows.tolist()}) == shape[0]
    check_everything(c, case, keep, rows, state, grad)


@pytest.mark.parametrize("wide", [True, False], ids=["quads", "single"])
def test_past_one_grid_pass(wide):
    """An item longer than the MT_INFLIGHT trips of the grid whose loads a lane issues together, so that the first lanes go
    round their outer loop again, by one quad (five elements on the one-element path): a lost tail changes n."""
    from vdn import metric
    n = INFLIGHT * metric.trip_elements(wide) + (4 if wide else 5)
    assert metric.trip_elements(wide) == 256 * 256 * (4 if wide else 1) and (n % 4 == 0) == wide
    c, case, keep, rows, state, grad = extra((1, 1, n), "uint8", seed=701)
    check_everything(c, case, keep, rows, state, grad)
    tail = np.zeros_like(case["mask"])
    tail[0, 0, -3:] = 1                  # the last three elements alone: only the second round of the loop sees them
    d = np.clip(case["depth"], 0.05, 19.0)
    got = metric.eval_depth_batch(dev(case["pred"]), dev(d), dev(tail), min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
    check_rows(got, R.eval_rows(case["pred"], d, tail, MIN_DEPTH, MAX_DEPTH))
    assert got[0, 0].item() == 3


@pytest.mark.parametrize("src,dst", [((4, 6), (5, 7)), ((1, 1), (5, 7)), ((37, 53), (64, 257)), ((518, 518), (768, 1024))], ids=str)
def test_resampled_prediction(src, dst):
    """A prediction of another size is sampled at the ground truth's pixels, align-corners, and the metrics of the restated
    blend come out: d1 d2 d3 bit for bit. (1, 1): a single source pixel, scale 0."""
    from vdn import metric
    B = 2 if dst[0] < 768 else 1
    c, case, keep, rows, _, _ = extra((B,) + dst, "bool", seed=702, pshape=src)
    assert case["pred"].shape == (B,) + src
    got = metric.eval_depth_batch(dev(case["pred"]), dev(case["depth"]), dev(case["mask"]), min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
    check_rows(got, rows)
    up = dev(R.resample_ac(case["pred"], *dst))          # the restated map, written out: the same-size kernel on it agrees
    same_bits(metric.eval_depth_batch(up, dev(case["depth"]), dev(case["mask"]), min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)[:, :4],
              got[:, :4])


def test_eval_depth_has_the_reference_signature():
    from vdn import metric
    c, case, keep, rows, _, _ = extra((3, 5, 7), "uint8")
    p, t = case["pred"][0][keep[0]], case["depth"][0][keep[0]]
    got = metric.eval_depth(dev(p), dev(t))
    assert tuple(got) == R.KEYS and all(isinstance(v, float) for v in got.values())
    check_rows(torch.tensor([[float(p.size)] + list(got.values())], dtype=torch.float64, device=DEV), rows[:1])
    again = metric.eval_depth(torch.from_numpy(case["pred"][:1].copy()), torch.from_numpy(case["depth"][:1].copy()))     # any shape, host tensors
    assert again == metric.eval_depth(dev(case["pred"][0].reshape(-1)), dev(case["depth"][0].reshape(-1)))


def test_mask_types_views_and_misaligned_pointers():
    from vdn import metric
    c, case, keep, rows, state, grad = extra((2, 16, 16), "bool", seed=703)
    p, d, m = dev(case["pred"]), dev(case["depth"]), dev(case["mask"])
    kw = dict(min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
    base = metric.eval_depth_batch(p, d, m, **kw)
    check_rows(base, rows)
    gbase = metric.silog_loss_grad(p, d, m, **kw)
    u8 = m.to(torch.uint8)
    twos = torch.where(m, u8, torch.full_like(u8, 2))             # a uint8 mask is used in place: a byte of 2 drops
    for mask in (u8, twos, m.float(), torch.where(m, 1.0, 0.5).to(DEV), m.cpu(), m.to(torch.int64)):
        same_bits(metric.eval_depth_batch(p, d, mask, **kw), base)
        same_bits(metric.silog_loss_grad(p, d, mask, **kw), gbase)
    wide = torch.zeros(2, 16, 32, device=DEV)
    wide[..., ::2] = p
    assert not wide[..., ::2].is_contiguous()
    same_bits(metric.eval_depth_batch(wide[..., ::2], d, m, **kw), base)
    same_bits(metric.eval_depth_batch(p.double(), d.cpu(), m, **kw), base)
    bufs = [torch.empty(p.numel() + 4, dtype=torch.float32, device=DEV) for _ in range(2)]
    mbuf = torch.empty(m.numel() + 4, dtype=torch.bool, device=DEV)
    off = 1 + (-(bufs[0].data_ptr() // 4) % 4)                    # 4 bytes past a 16-byte boundary: the one-element path
    ps = bufs[0][off:off + p.numel()].view(p.shape).copy_(p)
    ds = bufs[1][off:off + d.numel()].view(d.shape).copy_(d)
    ms = mbuf[1:1 + m.numel()].view(m.shape).copy_(m)
    assert ps.data_ptr() % 16 == 4 and ms.data_ptr() % 4 == 1
    for args in ((ps, ds, ms), (p, d, ms), (ps, d, m)):
        check_rows(metric.eval_depth_batch(*args, **kw), rows)
        same_bits(metric.eval_depth_batch(*args, **kw)[:, :4], base[:, :4])
        same_bits(metric.silog_loss_grad(*args, **kw), gbase)


def test_two_runs_give_the_same_bits():
    from vdn import metric
    kw = dict(min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
    for shape, pshape in (((2, 64, 257), None), ((2, 64, 257), (37, 53)), ((1, 768, 1024), None)):
        c, case, *_ = extra(shape, "float" if shape[0] == 2 and pshape is None else "bool", seed=702 if pshape else 700, pshape=pshape)
        p, d, m = dev(case["pred"]), dev(case["depth"]), dev(case["mask"])
        same_bits(metric.eval_depth_batch(p, d, m, **kw), metric.eval_depth_batch(p, d, m, **kw))
        if pshape is None:
            a, b = metric.silog_loss(p, d, m, **kw), metric.silog_loss(p, d, m, **kw)
            assert a == b
            same_bits(metric.silog_loss_grad(p, d, m, **kw), metric.silog_loss_grad(p, d, m, **kw))


def test_nan_and_inf_under_dropped_pixels_reach_nothing():
    from vdn import metric
    c, case, keep, rows, state, grad = extra((2, 64, 257), "float")
    p, d = case["pred"].copy(), case["depth"].copy()
    drop = np.argwhere(np.asarray(case["mask"]) != 1)[:6]
    for k, (b, y, x) in enumerate(drop):
        p[b, y, x] = (np.nan, np.inf, -1.0)[k % 3]
        d[b, y, x] = (1.0, np.nan, 0.0)[k % 3] if k < 3 else d[b, y, x]
    kw = dict(min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
    m = dev(case["mask"])
    got = metric.eval_depth_batch(dev(p), dev(d), m, **kw)
    same_bits(got, metric.eval_depth_batch(dev(case["pred"]), dev(case["depth"]), m, **kw))
    check_rows(got, rows)
    g = metric.silog_loss_grad(dev(p), dev(d), m, **kw)
    same_bits(g, metric.silog_loss_grad(dev(case["pred"]), dev(case["depth"]), m, **kw))
    check_grad(g, grad, keep)


def test_a_non_positive_prediction_gives_what_log_gives():
    from vdn import metric
    c, case, keep, _, _, _ = extra((3, 5, 7), "uint8")
    p = case["pred"].copy()
    b, y, x = np.argwhere(keep)[0]
    p[b, y, x] = -1.0
    rows = R.eval_rows(p, case["depth"], case["mask"], MIN_DEPTH, MAX_DEPTH)
    assert np.isnan(rows[b, 7:]).all() and not np.isnan(rows[b, 1:7]).any()
    check_rows(metric.eval_depth_batch(dev(p), dev(case["depth"]), dev(case["mask"]), min_depth=MIN_DEPTH, max_depth=MAX_DEPTH), rows)


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 16, 16)], ids=str)
def test_canaries_around_the_outputs_are_untouched(shape):
    """The output rows and the gradient sit inside larger buffers of a canary value: the bytes before and after them stay."""
    from vdn.normals import _runtime_for
    c, case, keep, rows, state, grad = extra(shape, "uint8", seed=703 if shape == (2, 16, 16) else 700)
    rt = _runtime_for(DEV)
    p, d, m = dev(case["pred"]), dev(case["depth"]), dev(case["mask"])
    B, n = shape[0], p.numel()
    CAN = -12345.678
    obuf = torch.full(((B + 2) * 10,), CAN, dtype=torch.float64, device=DEV)
    out = obuf[10:10 + B * 10].view(B, 10)
    rt.metric_eval(p, d, m, out, (MIN_DEPTH, MAX_DEPTH))
    check_rows(out, rows)
    assert (obuf[:10] == CAN).all() and (obuf[-10:] == CAN).all()
    sbuf = torch.full((12,), CAN, dtype=torch.float64, device=DEV)
    rt.silog_loss(p, d, m, sbuf[4:8], 0.5, (MIN_DEPTH, MAX_DEPTH))
    assert (sbuf[:4] == CAN).all() and (sbuf[8:] == CAN).all() and sbuf[5].item() == state[1]
    coeff = torch.ones(1, dtype=torch.float32, device=DEV)
    for pad in (4, 5):                                   # the gradient on a 16-byte boundary (quads where n allows) and off it
        gbuf = torch.full((n + 2 * pad,), CAN, dtype=torch.float32, device=DEV)
        g = gbuf[pad:pad + n].view(p.shape)
        rt.silog_loss_backward(p, d, m, sbuf[4:8], coeff, g, 0.5, (MIN_DEPTH, MAX_DEPTH))
        check_grad(g, grad, keep)
        assert (gbuf[:pad] == np.float32(CAN)).all() and (gbuf[-pad:] == np.float32(CAN)).all()


def test_backward_scales_with_the_incoming_gradient():
    from vdn import metric
    c, case, keep, _, _, _ = extra((2, 64, 257), "float")
    p, d, m = dev(case["pred"]), dev(case["depth"]), dev(case["mask"])
    pg = p.clone().requires_grad_(True)
    (metric.SiLogLoss().forward_from_valid(pg, d, m, MIN_DEPTH, MAX_DEPTH) * 3.0).backward()
    check_grad(pg.grad, R.silog_grad_ref(case["pred"], case["depth"], keep, 0.5, 3.0), keep)
    same_bits(pg.grad, metric.silog_loss_grad(p, d, m, weight=3.0, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH))
    with pytest.raises(NotImplementedError):
        metric.SiLogLoss()(pg, d.clone().requires_grad_(True), dev(keep))
    with torch.no_grad():
        assert metric.SiLogLoss()(pg, d, dev(keep)).grad_fn is None


def test_validate_step_and_meter():
    """metric_validate_step with a stub model gives eval_depth_batch's rows, and the meter drops exactly the items with fewer
    than 10 kept pixels: an item of 9, one of 10 (the fixture's nine_ten case), an empty one and full ones."""
    from vdn import metric
    from vdn.steps import DepthMetricMeter, metric_validate_step
    c, case, keep, rows, _, _ = extra((2, 64, 257), "bool", seed=702, pshape=(37, 53))
    small = dev(case["pred"])
    seen = []

    def model(img):
        seen.append(tuple(img.shape))
        assert img.is_cuda and img.dtype == torch.float32
        return small

    sample = {"image": torch.zeros(2, 3, 37, 53), "depth": dev(case["depth"]), "valid_mask": dev(case["mask"])}
    meter = DepthMetricMeter()
    got = metric_validate_step(model, sample, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, meter=meter)
    assert seen == [(2, 3, 37, 53)]
    same_bits(got, metric.eval_depth_batch(small, sample["depth"], sample["valid_mask"], min_depth=MIN_DEPTH, max_depth=MAX_DEPTH))
    check_rows(got, rows)
    nt = R.make_case(R.case_dict(35, (2, 16, 16), "bool", "nine_ten", 0.5))
    empty = np.zeros_like(nt["mask"])
    later = []
    for mask in (nt["mask"], empty):
        s = {"image": torch.zeros(2, 3, 16, 16), "depth": dev(nt["depth"]), "valid_mask": dev(mask)}
        later.append(metric_validate_step(lambda img: dev(nt["pred"]), s, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, meter=meter))
        check_rows(later[-1], R.eval_rows(nt["pred"], nt["depth"], mask, MIN_DEPTH, MAX_DEPTH))
    assert later[0][:, 0].tolist() == [9, 10] and later[1][:, 0].tolist() == [0, 0]
    state = meter.state()
    assert state.is_cuda and state[-1].item() == 3            # the two full items and the one of 10
    means = meter.means()
    want = got[0, 1:] + got[1, 1:] + later[0][1, 1:]
    want = want / torch.full_like(want, 3.0)
    assert tuple(means) == R.KEYS and list(means.values()) == want.cpu().tolist()
