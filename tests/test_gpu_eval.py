"""vdn.eval on the device (csrc/eval.hip) against the reference's recorded values (tests/golden/eval_cases.npz) and
against the CPU restatement tests/eval_ref.py at the shapes where the kernels can go wrong.

Tolerance: delta1..3 are equal as float32. The other four metrics are within 1e-9 relative: each is built from sums of
non-negative fp64 terms over fewer than 6e5 elements, for which the summation order costs at most about 7e-11; the rest is
margin for the conditioning of the 2 x 2 fit. NaN must meet NaN. tools/eval_bench.py measures the differences and writes them to profiles/eval_metrics.md."""
from __future__ import annotations

import functools
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval_ref as R
from test_eval_host import CASES, case_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-9
CANARY = -777.0
# one gradient row and less than a wave | small odd sizes | no gradient row: TGM is NaN | several blocks per frame, odd
# width | a real frame
SHAPES = [(1, 2, 3), (3, 5, 7), (1, 1, 9), (4, 64, 257), (2, 518, 518)]


@functools.lru_cache(maxsize=None)
def clip(shape, domain, with_mask, empty=(), constant=False):
    """Seeded inputs, shared between tests and never written. Shapes too small for make_case's random invalid pixels to leave
    anything get an all-valid gt with one pixel out of range."""
    T, H, W = shape
    if H * W < 64:
        rng = np.random.default_rng(H * W)
        gt = (1.0 + 6.0 * rng.random(shape)).astype(np.float32)
        gt.reshape(T, -1)[:, -1] = 80.0
        for f in empty:
            gt[f] = 0.0
        pred = (3.0 / np.maximum(gt, 0.5) + 0.2 if domain == "depth" else 0.5 * gt + 1.0).astype(np.float32)
        pred += (0.05 * rng.standard_normal(shape)).astype(np.float32)
        pred.reshape(T, -1)[:, 0] = -1.0
        mask = None
        if with_mask:
            mask = np.ones(shape, bool)
            mask.reshape(T, -1)[:, 1] = False
    else:
        pred, gt, mask = R.make_case(1000 + T + H + W, shape, domain, with_mask, empty)
    if constant:
        pred = np.full(shape, 0.3, np.float32)
    return pred, gt, mask


@functools.lru_cache(maxsize=None)
def reference(shape, domain, with_mask, empty=(), constant=False, tgm_over_time=False, seq_len=98):
    pred, gt, mask = clip(shape, domain, with_mask, empty, constant)
    return tuple(R.eval_ref(pred, gt, seq_len, domain, mask=mask, tgm_over_time=tgm_over_time))


def agree(got, want, what):
    """The issue's bar; returns the largest relative difference of the four fp64 metrics."""
    worst = 0.0
    for i in R.F64_IDX:
        if np.isnan(want[i]) or np.isnan(got[i]):
            assert np.isnan(want[i]) and np.isnan(got[i]), (what, R.eval_metrics[i], got[i], want[i])
            continue
        rel = abs(got[i] - want[i]) / abs(want[i])
        worst = max(worst, rel)
    print(f"[{what}] fp64 metrics max rel diff {worst:.2e}; got {list(got)}")
    assert worst <= RTOL, (what, got, want)
    for i in R.DELTA_IDX:
        assert got[i] == float(np.float32(got[i])), "a delta accuracy is a float32 value"
        assert struct.pack("f", got[i]) == struct.pack("f", want[i]) or (np.isnan(got[i]) and np.isnan(want[i])), \
            (what, R.eval_metrics[i], got[i], want[i])
    return worst


def run(pred, gt, mask, **kw):
    from vdn.eval import eval_single_by_data
    out = eval_single_by_data(pred, gt, mask=mask, **kw)
    assert len(out) == 7 and all(isinstance(v, float) for v in out)
    return out


@pytest.mark.parametrize("c", CASES, ids=lambda c: f"seed{c['seed']}-{c['domain']}")
def test_fixture_cases_match_the_reference(c):
    pred, gt, mask = case_inputs(c)
    got = run(pred, gt, mask, domain=c["domain"], dataset_min_depth=c["dmin"], dataset_max_depth=c["dmax"])
    agree(got, c["expected"], f"reference seed {c['seed']}")


@pytest.mark.parametrize("tgm_over_time", [False, True], ids=["rows", "frames"])
@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("domain", ["depth", "disp"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_eval_ref(shape, domain, with_mask, tgm_over_time):
    pred, gt, mask = clip(shape, domain, with_mask)
    want = reference(shape, domain, with_mask, tgm_over_time=tgm_over_time)
    if shape[1] == 1 and not tgm_over_time or shape[0] == 1 and tgm_over_time:
        assert np.isnan(want[2])            # no gradient row, or no pair of frames
    got = run(pred, gt, mask, domain=domain, tgm_over_time=tgm_over_time)
    agree(got, want, f"{shape} {domain} mask={with_mask} over_time={tgm_over_time}")


@pytest.mark.parametrize("tgm_over_time", [False, True], ids=["rows", "frames"])
@pytest.mark.parametrize("empty", [(0,), (3,), (1,), (0, 2)], ids=lambda e: "empty" + "".join(map(str, e)))
@pytest.mark.parametrize("shape", [(4, 5, 7), (4, 64, 257)], ids=lambda s: "x".join(map(str, s)))
def test_frames_without_a_valid_pixel_are_dropped(shape, empty, tgm_over_time):
    pred, gt, mask = clip(shape, "depth", True, empty)
    want = reference(shape, "depth", True, empty, tgm_over_time=tgm_over_time)
    agree(run(pred, gt, mask, tgm_over_time=tgm_over_time), want, f"{shape} empty={empty} over_time={tgm_over_time}")


def test_no_valid_pixel_at_all_gives_seven_nan():
    pred, gt, _ = clip((3, 5, 7), "depth", False)
    out = run(pred, np.zeros_like(gt), None)
    assert all(np.isnan(v) for v in out), out


@pytest.mark.parametrize("seq_len,frames_of_gt", [(3, 4), (2, 3), (1, 4)])
def test_seq_len_shorter_than_the_clip(seq_len, frames_of_gt):
    shape = (4, 64, 257)
    pred, gt, mask = clip(shape, "disp", True)
    want = reference(shape, "disp", True, seq_len=seq_len)
    got = run(pred, gt[:frames_of_gt], mask[:frames_of_gt], domain="disp", seq_len=seq_len)
    agree(got, want, f"seq_len={seq_len}")


@pytest.mark.parametrize("domain", ["depth", "disp"])
@pytest.mark.parametrize("shape", [(3, 5, 7), (4, 64, 257)], ids=lambda s: "x".join(map(str, s)))
def test_constant_prediction_takes_the_minimum_norm_fit(shape, domain):
    from vdn import _abi
    from vdn.eval import _runtime
    pred, gt, mask = clip(shape, domain, False, (), True)
    want = reference(shape, domain, False, (), True)
    agree(run(pred, gt, mask, domain=domain), want, f"{shape} {domain} constant")
    rt = _runtime(torch.device(DEV))
    coef = torch.full((2,), 9.0, dtype=torch.float64, device=DEV)
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    rt.eval_fit(p, g, None, 1e-3, 70.0, _abi.EVAL_DEPTH if domain == "depth" else _abi.EVAL_DISP, coef)
    valid = (gt > np.float32(1e-3)) & (gt < np.float32(70))
    g64 = gt.astype(np.float64)[valid]
    t = g64 if domain == "disp" else 1.0 / (g64 + 1e-8)
    A = np.stack([np.full(t.size, float(np.float32(0.3))), np.ones(t.size)], 1)
    lstsq = np.linalg.lstsq(A, t, rcond=None)[0]
    assert np.allclose(coef.cpu().numpy(), lstsq, rtol=1e-12, atol=0), (coef, lstsq)


def _placed(values: np.ndarray, dtype, off: int, pad: int = 8):
    """`values` at element offset `off` of a canary-filled device allocation: (whole buffer, the [T, H, W] view)."""
    fill = CANARY if dtype == torch.float32 else 0xA5
    n = values.size
    buf = torch.full((off + n + pad,), fill, dtype=dtype, device=DEV)
    view = buf[off:off + n].view(values.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(dtype))
    return buf, view, fill


@pytest.mark.parametrize("tgm_over_time", [False, True], ids=["rows", "frames"])
@pytest.mark.parametrize("shape", [(3, 5, 7), (4, 64, 257)], ids=lambda s: "x".join(map(str, s)))
def test_inputs_at_a_one_element_offset_between_canaries(shape, tgm_over_time):
    """Device tensors are used in place, 4 bytes (mask: 1 byte) past a 16-byte boundary; nothing outside or inside the
    inputs is written."""
    pred, gt, mask = clip(shape, "depth", True)
    want = reference(shape, "depth", True, tgm_over_time=tgm_over_time)
    placed = [_placed(pred, torch.float32, 1), _placed(gt, torch.float32, 1), _placed(mask, torch.uint8, 1)]
    before = [b.clone() for b, _, _ in placed]
    assert all(v.data_ptr() % 16 == v.element_size() for _, v, _ in placed)
    got = run(placed[0][1], placed[1][1], placed[2][1], tgm_over_time=tgm_over_time)
    agree(got, want, f"{shape} offset over_time={tgm_over_time}")
    for (buf, view, fill), b in zip(placed, before):
        assert torch.equal(buf, b)
        assert bool((buf[:1] == fill).all()) and bool((buf[1 + view.numel():] == fill).all())


def test_two_runs_give_identical_bits():
    pred, gt, mask = clip((4, 64, 257), "depth", True)
    p, g, m = (torch.from_numpy(a).to(DEV) for a in (pred, gt, mask))
    for over_time in (False, True):
        a = run(p, g, m, tgm_over_time=over_time)
        junk = torch.full((1 << 20,), 3.0, device=DEV)   # other work in between, other addresses after it
        del junk
        b = run(p.clone(), g.clone(), m.clone(), tgm_over_time=over_time)
        assert struct.pack("7d", *a) == struct.pack("7d", *b)


@pytest.mark.parametrize("src,dst", [((5, 7), (11, 13)), ((37, 53), (19, 20)), ((518, 518), (518, 518))],
                         ids=["up", "down", "identity"])
def test_resize_half_pixel_bilinear(src, dst):
    """Against F.interpolate(align_corners=False). Both compute the source coordinate and the two weights per axis with
    the same float32 operations (the coordinate is one fused multiply-add in both), so what can differ is the rounding of the blend hy0 (wx0 a + wx1 b) + hy1 (wx0 c + wx1 d):
    three roundings per level, two levels, with or without fused multiply-adds, on terms that sum to at most max|x|.
    Bar: 8 * 2^-24 * max|x|. The identity resize has weights 1 and 0 and is exact."""
    from vdn.eval import _runtime
    rt = _runtime(torch.device(DEV))
    rng = np.random.default_rng(src[0] * dst[1])
    x = torch.from_numpy((10.0 * rng.standard_normal((2, *src))).astype(np.float32))
    want = F.interpolate(x[:, None], size=dst, mode="bilinear", align_corners=False)[:, 0]
    n = want.numel()
    buf = torch.full((1 + n + 8,), CANARY, dtype=torch.float32, device=DEV)
    out = buf[1:1 + n].view(2, *dst)
    rt.resize_bilinear_hp(x.to(DEV), out)
    assert bool((buf[:1] == CANARY).all()) and bool((buf[1 + n:] == CANARY).all())
    err = float((out.cpu() - want).abs().max())
    bar = 8 * 2.0 ** -24 * float(x.abs().max())
    print(f"[resize {src}->{dst}] max abs diff {err:.3e} (bar {bar:.3e})")
    if src == dst:
        assert torch.equal(out.cpu(), x)
    assert err <= bar


def test_a_smaller_prediction_is_resized_to_gt():
    """The wrapper's resize path is the resize kernel followed by the same evaluation."""
    from vdn.eval import _runtime
    _, gt, mask = clip((4, 64, 257), "depth", True)
    rng = np.random.default_rng(5)
    small = torch.from_numpy((0.2 + rng.random((4, 37, 53))).astype(np.float32)).to(DEV)
    full = torch.empty(4, 64, 257, device=DEV)
    _runtime(torch.device(DEV)).resize_bilinear_hp(small, full)
    a, b = run(small, gt, mask), run(full, gt, mask)
    assert struct.pack("7d", *a) == struct.pack("7d", *b) and not any(np.isnan(a))
