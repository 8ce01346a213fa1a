"""The hand-written kernels of the video models (csrc/stitch.hip, refine.hip with the median on select.hpp, hiera.hip,
dn_head.hip's prologue and tail, points.hip) where their unit tests do not go: past the first trip of every grid-stride
loop, at the tails and heads next to it, in every template branch and at every guard. References are the restatements of
tests/video_kernels_ref.py (held to what they restate by tests/test_video_kernels_ref_host.py): float64 where the bar is a
tolerance, float32 with one rounding per operation where it is "the same bits". Every bar is the one the kernel's unit test
already holds (test_gpu_ops.py, test_gpu_dn_head.py, test_gpu_hiera.py, test_gpu_refiner23.py, test_gpu_metric_model.py),
except the stitch fit's one float32 ulp, derived at its test. Every shape is the smallest that reaches its branch and each
test asserts that it does. Outputs are fresh allocations, NaN-filled (canary-filled where compared for equality) with a
canary pad behind them that is checked afterwards; every output element is compared."""
import math

import numpy as np
import pytest
import torch

import hiera_ref as HR
import test_gpu_refiner23 as R23
import video_kernels_ref as V
from common import rel_l2, worst_px
from test_gpu_ops import close, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD, CANARY = 64, -777.0
NAN = float("nan")
EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3   # enum vdn_status (include/vdn.h)
CAP = 16384 * 256                            # lanes of a launch capped at 16384 blocks


def _runtime(half, split):
    from vdn.runtime import Runtime
    from vdn import _abi
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    assert _abi.lib.vdn_arch_ok() == 1, "not a gfx950 device"
    return Runtime(torch.device("cuda:0"), half, split)


@pytest.fixture(scope="module")
def rt():
    return _runtime(torch.float16, False)


@pytest.fixture(scope="module")
def rt3():
    return _runtime(torch.float16, True)


@pytest.fixture(scope="module")
def rtb3():
    return _runtime(torch.bfloat16, True)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fresh(shape, fill=CANARY, dtype=torch.float32):
    """(whole allocation, the output the kernel gets): `shape` filled with `fill`, PAD canaries behind it."""
    n = math.prod(shape)
    buf = torch.full((n + PAD,), CANARY, dtype=dtype, device=DEV)
    buf[:n] = fill
    return buf, buf[:n].view(shape)


def _pad_intact(*bufs):
    torch.cuda.synchronize()
    return all(bool((b[-PAD:] == torch.full_like(b[-PAD:], CANARY)).all()) for b in bufs)


def _untouched(*bufs):
    torch.cuda.synchronize()
    return all(bool((b == torch.full_like(b, CANARY)).all()) for b in bufs)


def _planes(shape, dtype, split=True):
    from vdn.runtime import HL
    (hb, hi), (lb, lo) = _fresh(shape, dtype=dtype), _fresh(shape, dtype=dtype)
    return (hb, lb) if split else (hb,), HL(hi, lo if split else None)


def _same(a, b):
    """equal values; a NaN equals a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ================================================================================================ 1. vdn_stitch_fit
@pytest.mark.parametrize("shape,r", [((262144 + 4 * 5,), 0), ((262144 + 4 * 5 + 3,), 3), ((2, 363, 363), 2)], ids=["r0", "r3", "2x363x363"])
def test_stitch_fit_second_trip_and_tail(rt, shape, r):
    """align_partial_kernel reads float4s on 256 x 256 lanes: n / 4 > 65536 gives block 0 a second trip, and with n % 4 != 0
    its first lanes take the tail elements as well. Reference: the closed form in float64 from exactly rounded sums. Bar: one
    float32 ulp of each coefficient. The device's fp64 sums of at most 3e5 same-sign terms are off by less than 3e5 * 2^-53 =
    3e-11 relative; with det >= 0.05 s0 s2 (asserted on the reference) the solution moves by less than 1e-8 relative, a sixth
    of a float32 half-ulp, so only a tie of the final conversion is left."""
    n = math.prod(shape)
    assert n // 4 > 256 * 256 and n % 4 == r
    pred = rnd(*shape, seed=1100).abs() + 0.1
    target = 1.7 * pred + 0.3 + 0.05 * rnd(*shape, seed=1101)
    scale, shift, det, s0, s2 = V.stitch_fit(pred.numpy(), target.numpy())
    assert det >= 0.05 * s0 * s2, (det, s0 * s2)
    cbuf, coef = _fresh((2,), NAN)
    rt.stitch_fit(pred.to(DEV), target.to(DEV), coef)
    got = coef.cpu().numpy().astype(np.float64)
    assert _pad_intact(cbuf)
    for g, want in zip(got, (scale, shift)):
        ulp = float(np.spacing(np.float32(abs(want))))
        print(f"[stitch_fit n={n}] got {g!r} reference {want!r}: {abs(g - want) / ulp:.3f} ulp")
        assert abs(g - want) <= ulp


# ================================================================================================ 2. vdn_stitch_apply
def _apply_case(rt, T, hw, align_len, overlap, ref_frame, seed):
    interp = overlap - align_len
    win = rnd(T, hw, seed=seed)                          # both signs: the clamp cuts about half of scale * d + shift
    old = rnd(interp, hw, seed=seed + 1).abs()
    scale, shift = np.float32(1.3), np.float32(-0.2)
    want_tail, want_new, want_ref = V.stitch_apply(win.numpy(), scale, shift, old.numpy(), align_len, overlap, ref_frame)
    assert (want_new == 0).any() and (want_new > 0).any()
    (tb, tail), (nb, new), (rb, ref1) = _fresh((interp, hw)), _fresh((T - overlap, hw)), _fresh((hw,))
    tail.copy_(old)
    coef = torch.tensor([float(scale), float(shift)], dtype=torch.float32, device=DEV)
    rt.stitch_apply(win.to(DEV), coef, tail, new, ref1, align_len, overlap, ref_frame)
    got = [t.cpu().numpy() for t in (tail, new, ref1)]
    assert _pad_intact(tb, nb, rb)
    for name, g, w in zip(("out_tail", "out_new", "ref1"), got, (want_tail, want_new, want_ref)):
        assert np.array_equal(g, w), (name, int((g != w).sum()), float(np.abs(g - w).max()))


def test_stitch_apply_second_trip_is_the_float32_expression(rt):
    """32-frame windows of 374 x 374 as DeviceStitcher passes them: 30 * hw elements, more than 16384 blocks of 256. out_tail,
    out_new and ref1 equal the float32 numpy expression vdn.h promises, value for value. (A fit fused into one fma, as the
    kernel once had it, leaves about 8 % of the values one ulp off.)"""
    from vdn import util
    T, hw, align_len = util.INFER_LEN, 374 * 374, util.OVERLAP - util.INTERP_LEN
    assert (T, align_len, util.OVERLAP, util.KEYFRAMES[1]) == (32, 2, 10, 12)
    assert (T - align_len) * hw > CAP
    _apply_case(rt, T, hw, align_len, util.OVERLAP, util.KEYFRAMES[1], seed=1200)


def test_stitch_apply_two_blend_frames(rt):
    """interp = 2, the least vdn_stitch_apply takes: the weights are 0 and 1 and no step is taken; hw = 5."""
    _apply_case(rt, 5, 5, 1, 3, 4, seed=1210)


@pytest.mark.parametrize("T,align_len,overlap,ref_frame", [(10, 2, 10, 9), (32, 9, 10, 12), (32, 2, 10, 1), (32, 2, 10, 32)],
                         ids=["T<=overlap", "interp<2", "ref<align", "ref>=T"])
def test_stitch_apply_rejects(rt, T, align_len, overlap, ref_frame):
    from vdn import _abi
    hw = 5
    win, coef = torch.ones(T, hw, device=DEV), torch.ones(2, device=DEV)
    (tb, tail), (nb, new), (rb, ref1) = _fresh((8, hw)), _fresh((32, hw)), _fresh((hw,))
    rc = _abi.lib.vdn_stitch_apply(win.data_ptr(), coef.data_ptr(), tail.data_ptr(), new.data_ptr(), ref1.data_ptr(), hw, T, align_len,
                                   overlap, ref_frame, _stream())
    assert rc == EINVAL and _untouched(tb, nb, rb)


# ================================================================================================ 3. vdn_frame_median
def _median(rt, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    mbuf, med = _fresh((x.shape[0],))
    rt.frame_median(torch.from_numpy(x).to(DEV), med)
    got = med.cpu().numpy()
    assert _pad_intact(mbuf)
    return got


def _check_median(rt, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    got, want = _median(rt, x), V.frame_median(x)
    quant = torch.quantile(torch.from_numpy(x), 0.5, dim=-1).numpy()
    assert _same(got, want), (got, want)
    assert _same(got, quant), (got, quant)


@pytest.mark.parametrize("n", [33, 34])
@pytest.mark.parametrize("F_", [65, 130])
def test_frame_median_many_frames(rt, F_, n):
    """median_final_kernel has 64 lanes a block: 65 frames reach its second, 130 its third; 130 / 260 scan blocks. Every frame
    has values of its own, so one that reads its neighbour's state shows."""
    assert (F_ + 63) // 64 == {65: 2, 130: 3}[F_]
    x = rnd(F_, n, seed=1300) * (1.0 + torch.arange(F_)[:, None]) + torch.arange(F_)[:, None]
    x[::7] = torch.round(x[::7])
    med = torch.quantile(x, 0.5, dim=-1)
    assert len(set(med.tolist())) == F_
    _check_median(rt, x.numpy())


def _v(bin1, bin2):
    """the float in [1, 1.25) whose pass-1 and pass-2 bins are these (mantissa bits 20..10 and 9..0)"""
    return np.array([0x3F800000 | (bin1 << 10) | bin2], dtype=np.uint32).view(np.float32)[0]


# name: (a, b, pass, place of a's bin in its lane's run, place of b's). a and b are the two middle order statistics of a
# frame; select_scan_kernel gives each of its 256 lanes a run of 8 bins on passes 0 and 1 and of 4 bins on pass 2.
RANK_BINS = {
    "pass0_last_of_run": (1.8, 1.9, 0, 7, 7),            # [1.75, 2): bin 1024 + 4 * 127 + 3, the last of its lane's run
    "pass0_first_of_run": (2.1, 2.2, 0, 0, 0),           # [2, 2.5): the first bin of the next lane
    "pass0_two_lanes": (1.9, 2.1, 0, 7, 0),              # slot 0 ends one lane's run, slot 1 begins the next
    "pass1_bin0": (_v(0, 5), _v(0, 9), 1, 0, 0),
    "pass1_last_of_run": (_v(7, 1), _v(7, 2), 1, 7, 7),
    "pass1_first_of_run": (_v(8, 1), _v(8, 2), 1, 0, 0),
    "pass1_two_lanes": (_v(7, 1000), _v(8, 3), 1, 7, 0),
    "pass1_last_bin": (_v(2047, 1), _v(2047, 2), 1, 7, 7),
    "pass2_bin0": (_v(5, 0), _v(5, 1), 2, 0, 1),
    "pass2_last_of_run": (_v(5, 2), _v(5, 3), 2, 2, 3),
    "pass2_two_lanes": (_v(5, 3), _v(5, 4), 2, 3, 0),
    "pass2_first_of_run": (_v(5, 4), _v(5, 5), 2, 0, 1),
    "pass2_last_bin": (_v(5, 1022), _v(5, 1023), 2, 2, 3),
    "pass2_same_key": (_v(5, 1023), _v(5, 1023), 2, 3, 3),
}


def _frame_around(a, b, n, rs):
    """n shuffled positive values whose middle order statistics are a and b: the others lie below a and above b by relative
    steps of 2^-1 .. 2^-20, so that some share a's or b's leading key bits and some do not."""
    below = (n - 1) // 2
    above = n - 2 - below
    lo = np.float32(a) * (1 - np.exp2(-rs.randint(1, 21, below))).astype(np.float32)
    hi = np.float32(b) * (1 + np.exp2(-rs.randint(1, 21, above))).astype(np.float32)
    f = np.concatenate([lo, hi, np.array([a, b], dtype=np.float32)]).astype(np.float32)
    s = np.sort(f)
    assert s[(n - 1) // 2] == np.float32(a) and s[n // 2] == np.float32(a if n & 1 else b) and (lo < a).all() and (hi > b).all()
    return rs.permutation(f)


@pytest.mark.parametrize("n", [40, 41])
def test_frame_median_rank_in_every_lane_position(rt, n):
    """The bin that holds the rank at the first and the last place of a scan lane's run, in bin 0 and in the last bin of
    passes 1 and 2, and in different lanes for the floor and the ceil rank; one frame per case, all in one call."""
    rs = np.random.RandomState(1310 + n)
    for name, (a, b, p, place_a, place_b) in RANK_BINS.items():
        ba, bb, per = V.pass_bins(a), V.pass_bins(b), 4 if p == 2 else 8
        assert ba[:p] == bb[:p], name                                   # the earlier passes do not tell them apart
        assert (ba[p] % per, bb[p] % per) == (place_a, place_b), (name, ba, bb)
        if name.endswith("two_lanes"):
            assert bb[p] // per == ba[p] // per + 1
        if name.endswith("bin0"):
            assert ba[p] == 0
        if name.endswith("last_bin") or name.endswith("same_key"):
            assert bb[p] == (1023 if p == 2 else 2047)
    _check_median(rt, np.stack([_frame_around(a, b, n, rs) for a, b, *_ in RANK_BINS.values()]))


def test_frame_median_shared_key_prefixes(rt):
    """Keys that share their top 22 bits (1 + j 2^-23, j < 1024: only pass 2 tells them apart), keys that share their top 11
    bits only ([1, 1.25)), and a frame of equal values."""
    rs = np.random.RandomState(1320)
    low = (1.0 + rs.permutation(1024) * 2.0 ** -23).astype(np.float32)
    assert len({V.pass_bins(v)[:2] for v in low}) == 1 and len({V.pass_bins(v)[2] for v in low}) == 1024
    mid = (0x3F800000 | rs.randint(0, 1 << 21, 1024).astype(np.uint32)).view(np.float32)
    assert len({V.pass_bins(v)[0] for v in mid}) == 1 and len({V.pass_bins(v)[1] for v in mid}) > 256
    _check_median(rt, np.stack([low, mid, np.full(1024, 3.25, dtype=np.float32)]))
    _check_median(rt, np.stack([low[:1023], mid[:1023]]))


def test_frame_median_special_values(rt):
    """Signed zeros, (-x, +x), subnormals, the largest finite values and infinities with odd and even counts: NaN or inf
    exactly where torch.quantile gives one. The rows of tests/video_kernels_ref.py without a NaN, one call per length."""
    rows = [r for r in V.MEDIAN_ROWS if not np.isnan(np.array(r, dtype=np.float32)).any()]
    assert [-0.0, 0.0] in rows and [-7.5, 7.5] in rows
    for n in sorted({len(r) for r in rows}):
        _check_median(rt, np.array([r for r in rows if len(r) == n], dtype=np.float32))


def test_frame_median_of_a_frame_with_a_nan_is_nan(rt):
    """A frame that holds a NaN of either sign gets a NaN median, as torch.quantile gives it, and the frames next to it keep
    theirs. Without the rule the select passed a NaN over (it sorts beyond the infinity of its sign): 4.0 for
    [1, 2, nan, 4, 5] and 2.0 with the NaN's sign bit set."""
    x = np.array([[1, 2, V.NAN, 4, 5], [1, 2, 3, 4, 5], [1, 2, V.NEG_NAN, 4, 5], [9, 8, 7, 6, 5], [V.NAN, V.NAN, V.NEG_NAN, 1, 2],
                  [V.NAN] * 5, [-V.INF, V.INF, V.NEG_NAN, 0, 1]], dtype=np.float32)
    assert np.signbit(x[2, 2]) and not np.signbit(x[0, 2])
    got = _median(rt, x)
    print(f"[frame_median NaN] medians {got.tolist()}")
    assert np.isnan(got[[0, 2, 4, 5, 6]]).all(), got
    assert got[1] == 3.0 and got[3] == 7.0
    _check_median(rt, x)
    for n in sorted({len(r) for r in V.MEDIAN_ROWS}):                   # and every special row that holds one, among the others
        _check_median(rt, np.array([r for r in V.MEDIAN_ROWS if len(r) == n], dtype=np.float32))
    big = rnd(3, 70001, seed=1330).numpy()                              # one NaN among many blocks' worth, in the middle frame
    big[1, 65537] = V.NEG_NAN
    got = _median(rt, big)
    assert np.isnan(got[1]) and not np.isnan(got[[0, 2]]).any()
    _check_median(rt, big)
    _check_median(rt, rnd(3, 70001, seed=1330).numpy())                 # the same workspace right after: no flag is left behind


def test_frame_median_second_trip_of_the_histogram_blocks(rt):
    """A frame's keys are counted by 64 blocks of 256 lanes: n = 64 * 256 + 1 gives the first lane a second element."""
    n = 64 * 256 + 1
    x = rnd(1, n, seed=1340) * 3.0
    x[0, -1] = 1e6                                                      # the element of the second trip is the largest
    _check_median(rt, x.numpy())
    x[0, -1] = float(torch.quantile(x[0, :-1], 0.5))                    # ... and then the median itself
    _check_median(rt, x.numpy())


# ================================================================================================ 4. vdn_refine_*
def test_refine_scale_second_trip(rt):
    """2 frames of 257 x 257: more than 256 blocks of 256 pixels per frame. Different medians per frame; 1e-6 against float64
    as test_refiner_scale_pack_finish_kernels; scale_out is one float per frame and nothing behind it."""
    F_, H, W = 2, 257, 257
    assert H * W > 256 * 256
    g = torch.Generator().manual_seed(1400)
    x = torch.rand(F_, H, W, generator=g) * 60000.0 + 100.0
    x[1] *= 0.5
    med = torch.quantile(x.reshape(F_, -1), 0.5, dim=-1)
    assert float(med[0]) > 1.5 * float(med[1])
    want, s = V.refine_scale(x.reshape(F_, -1).numpy(), med.numpy(), 0.7, -0.2, 1.0, 65535.0)
    (ob, out), (sb, sc) = _fresh((F_, H, W), NAN), _fresh((F_,), NAN)
    rt.refine_scale(x.to(DEV), med.to(DEV), 0.7, -0.2, 1.0, 65535.0, out, sc)
    close(sc, torch.from_numpy(s), 1e-6)
    close(out, torch.from_numpy(want).reshape(F_, H, W), 1e-6)
    assert _pad_intact(ob, sb)


@pytest.mark.parametrize("F_,H,W", [(3, 2, 2), (3, 2, 7), (3, 7, 2), (17, 497, 497)])
def test_refine_pack_smallest_maps_and_second_trip(rt, F_, H, W):
    """H = 2 and W = 2, where both reflected neighbours of a pixel are the same pixel, and 17 frames of 497 x 497, past 16384
    blocks of 256 pixels. 2e-6 against the float64 Sobel restatement as test_refiner_scale_pack_finish_kernels; without
    normals all three planes are d, bit for bit."""
    if F_ == 17:
        assert F_ * H * W > CAP
    d = torch.rand(F_, H, W, generator=torch.Generator().manual_seed(1410 + H + W)) * 2.0
    dd = d.to(DEV)
    pb, packed = _fresh((F_, 3, H, W), NAN)
    rt.refine_pack(dd, packed, normals=True)
    close(packed, torch.from_numpy(V.sobel_pack(d.numpy())), 2e-6)
    assert _pad_intact(pb)
    pb, packed = _fresh((F_, 3, H, W))
    rt.refine_pack(dd, packed, normals=False)
    assert torch.equal(packed.cpu(), d[:, None].expand(-1, 3, -1, -1)) and _pad_intact(pb)


@pytest.mark.parametrize("H,W", [(1, 8), (8, 1)])
def test_refine_pack_rejects_one_pixel_wide_maps(rt, H, W):
    from vdn import _abi
    d = torch.ones(2, H, W, device=DEV)
    pb, packed = _fresh((2, 3, H, W))
    for normals in (1, 0):
        assert _abi.lib.vdn_refine_pack(d.data_ptr(), packed.data_ptr(), 2, H, W, normals, _stream()) == EINVAL
    assert _untouched(pb)


@pytest.mark.parametrize("residual", [True, False])
def test_refine_finish_second_trip(rt, residual):
    """n = 4 194 304 + 5: five lanes of the first block take a second element. 1e-6 against float64."""
    n = CAP + 5
    g = torch.Generator().manual_seed(1420)
    scaled, depth = torch.rand(n, generator=g), torch.rand(n, generator=g)
    ob, out = _fresh((n,), NAN)
    rt.refine_finish(scaled.to(DEV) if residual else None, depth.to(DEV), 1.3, 0.05, 65535.0, residual, out)
    want = V.refine_finish(scaled.numpy() if residual else None, depth.numpy(), 1.3, 0.05, 65535.0, residual)
    close(out, torch.from_numpy(want), 1e-6)
    assert _pad_intact(ob)


@pytest.mark.parametrize("tail", [0, 2])
def test_refine_mix_and_normalize_vector_body_second_trip(rt, tail):
    """4 (16384 * 256 + 7) + 3 floats behind a one-float offset: a 3-float head and a float4 body of 7 more lanes than a launch
    has, which therefore take a second trip; with two floats more, a tail behind the body as well. The cases and the bars
    (2e-6 of max |out| against float64 and NaN in, NaN out; bit-equal to torch.div) are test_gpu_refiner23.py's own."""
    n, offs = 4 * (CAP + 7) + 3 + tail, (1, 1, 1)
    head = (16 - 4 * offs[0]) // 4
    assert head == 3 and (n - head) // 4 > CAP and n - head - 4 * ((n - head) // 4) == tail
    R23.test_refine_mix_against_fp64(rt, n, offs)
    R23.test_refine_normalize_is_torch_div(rt, n, offs)


# ================================================================================================ 5. vdn_hiera_embed
def _embed_case(run, F_, ldk, dtype, split, seed):
    from vdn.runtime import HL
    img = torch.randn(F_, 3, 224, 224, generator=torch.Generator().manual_seed(seed))   # every frame its own values
    bufs, rows = _planes((F_ * 3136, ldk), dtype, split)
    run.hiera_embed(img.to(DEV), rows, F_, ldk)
    want = HL.from_float(torch.from_numpy(V.hiera_embed_rows(img.numpy())), dtype, split)
    for got, w in ((rows.hi, want.hi),) + (((rows.lo, want.lo),) if split else ()):
        got = got.cpu()
        for f in range(F_):                                                              # all rows of every frame, frame by frame
            assert torch.equal(got[f * 3136:(f + 1) * 3136, :147], w[f * 3136:(f + 1) * 3136]), f
        assert not got[:, 147:].any()
    assert _pad_intact(*bufs)


def test_hiera_embed_56_frames(rt3):
    """56 frames at ldk 192 in fp16 split planes: 56 * 3136 * 24 lanes of 8 columns, more than 16384 blocks of 256, so the last
    frames are gathered on the second trip. hi and lo planes equal unfold in unrolled order, bit for bit, for every frame."""
    assert 56 * 3136 * (192 // 8) > CAP and 54 * 3136 * (192 // 8) < CAP
    _embed_case(rt3, 56, 192, torch.float16, True, 1500)


def test_hiera_embed_single_plane_bf16_and_ldk_256(rt, rtb3, rt3):
    """rows_lo = NULL, the bf16 instance and a longer zero tail, one frame each."""
    _embed_case(rt, 1, 192, torch.float16, False, 1510)
    _embed_case(rtb3, 1, 192, torch.bfloat16, True, 1511)
    _embed_case(rt3, 1, 256, torch.float16, True, 1512)


def test_hiera_embed_rejects_ldk_152_and_an_unaligned_plane(rt):
    from vdn import _abi
    img = torch.ones(1, 3, 224, 224, device=DEV)
    rb, rows = _fresh((3136 + 1, 192), dtype=torch.float16)
    assert _abi.lib.vdn_hiera_embed(_abi.F16, img.data_ptr(), rows.data_ptr(), None, 1, 152, _stream()) == EALIGN
    assert _abi.lib.vdn_hiera_embed(_abi.F16, img.data_ptr(), rows.data_ptr() + 2, None, 1, 192, _stream()) == EALIGN
    assert _abi.lib.vdn_hiera_embed(_abi.F16, img.data_ptr(), rows.data_ptr(), rows.data_ptr() + 2, 1, 192, _stream()) == EALIGN
    assert _untouched(rb)


# ================================================================================================ 6. vdn_hiera_pool / _reroll
def test_hiera_pool_second_trip(rt):
    """F = 2, n = 8200, C = 1024: 4 198 400 float4 outputs, past 16384 blocks of 256. Integer-valued data made on the device
    (a multiplicative scramble of the index below 2^24, exact in float32); exact against the restatement and torch.max."""
    F_, n, C = 2, 8200, 1024
    assert F_ * n * (C // 4) > CAP
    x = ((torch.arange(F_ * 4 * n * C, device=DEV) * 7919) % 1000003).float().reshape(F_, 4 * n, C)
    yb, y = _fresh((F_, n, C))
    rt.hiera_pool(x, y, F_, n, C)
    xc, got = x.cpu(), y.cpu()
    assert _pad_intact(yb)
    assert torch.equal(got, torch.from_numpy(V.hiera_pool(xc.numpy(), n)))
    assert torch.equal(got, xc.reshape(F_, 4, n, C).max(1).values)


def test_hiera_pool_four_channels_and_nan(rt):
    """C = 4, one float4 per token. A NaN in one group of one token: the kernel's fmaxf drops it where Hiera's torch.max /
    MaxPool would hand it on (include/vdn.h states the departure); four NaNs give a NaN."""
    F_, n, C = 3, 5, 4
    x = rnd(F_, 4 * n, C, seed=1600)
    x[1, 2 * n + 3, 1] = NAN                                   # group 2 of token 3 of frame 1
    x[2, torch.arange(4) * n + 1, 2] = NAN                     # all four groups of token 1 of frame 2
    yb, y = _fresh((F_, n, C))
    rt.hiera_pool(x.to(DEV), y, F_, n, C)
    got, tmax = y.cpu(), x.reshape(F_, 4, n, C).max(1).values
    assert _pad_intact(yb)
    others = torch.stack([x[1, g * n + 3, 1] for g in (0, 1, 3)]).max()
    print(f"[hiera_pool NaN] fmaxf gives {float(got[1, 3, 1])}, torch.max gives {float(tmax[1, 3, 1])}")
    assert bool(torch.isnan(tmax[1, 3, 1])) and got[1, 3, 1] == others
    assert bool(torch.isnan(got[2, 1, 2])) and bool(torch.isnan(tmax[2, 1, 2]))
    assert _same(got.numpy(), V.hiera_pool(x.numpy(), n))
    tmax[1, 3, 1] = others
    assert _same(got.numpy(), tmax.numpy())


def test_hiera_pool_rejects_six_channels(rt):
    from vdn import _abi
    x = torch.ones(1, 4 * 5, 6, device=DEV)
    yb, y = _fresh((1, 5, 6))
    assert _abi.lib.vdn_hiera_pool(x.data_ptr(), y.data_ptr(), 1, 5, 6, _stream()) == EALIGN
    assert _untouched(yb)


def test_hiera_reroll_56_frames(rt):
    """Stage 0 at C = 96 and 56 frames: 56 * 3136 * 24 float4s, the last frames on the second trip. Exact against hiera_ref."""
    F_, C = 56, 96
    assert F_ * 3136 * (C // 4) > CAP
    x = torch.randn(F_, 3136, C, generator=torch.Generator().manual_seed(1610))
    ob, out = _fresh((F_, 56, 56, C))
    rt.hiera_reroll(x.to(DEV), out, F_, 0, C)
    got = out.cpu()
    assert _pad_intact(ob)
    assert torch.equal(got, HR.reroll(x, 0)) and np.array_equal(got.numpy(), V.hiera_reroll(x.numpy(), 0))


# ================================================================================================ 7. vdn_dn_prologue
def _prologue_inputs(frames, C, hw, S, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(frames * hw, C, generator=g), torch.randn(frames * hw, C, generator=g), torch.randn(S, C, generator=g))


def test_dn_prologue_second_trip(rt3):
    """14 frames of 96 x 3136: 4 214 784 elements, past 16384 blocks of 256, with b and an APE of S = 4 rows, so that f % S
    wraps three times. The f32 rows and the fp16 hi / lo planes equal the torch composition, bit for bit."""
    from vdn.runtime import HL
    frames, C, hw, S = 14, 96, 3136, 4
    assert frames * C * hw > CAP and (frames - 1) // S == 3
    a, b, ape = _prologue_inputs(frames, C, hw, S, 1700)
    want = V.dn_prologue(a, b, frames, C, hw, ape, S)
    fb, xf = _fresh((frames * hw, C))
    hbufs, xh = _planes((frames * hw, C), torch.float16)
    rt3.dn_prologue(a.to(DEV), b.to(DEV), frames, C, hw, ape=ape.to(DEV), S=S, out_f=xf, out_h=xh)
    assert torch.equal(xf.cpu(), want)
    wh = HL.from_float(want, torch.float16, True)
    assert torch.equal(xh.hi.cpu(), wh.hi) and torch.equal(xh.lo.cpu(), wh.lo)
    assert _pad_intact(fb, *hbufs)


def test_dn_prologue_bf16_f32_alone_and_one_input(rt, rtb3):
    """The bf16 instance (split planes), out_f without 16-bit planes, and a alone with an APE into one fp16 plane."""
    from vdn.runtime import HL
    frames, C, hw, S = 5, 8, 7, 2
    a, b, ape = _prologue_inputs(frames, C, hw, S, 1710)
    ad, bd, aped = a.to(DEV), b.to(DEV), ape.to(DEV)
    want = V.dn_prologue(a, b, frames, C, hw, ape, S)
    hbufs, xh = _planes((frames * hw, C), torch.bfloat16)
    rtb3.dn_prologue(ad, bd, frames, C, hw, ape=aped, S=S, out_h=xh)
    wh = HL.from_float(want, torch.bfloat16, True)
    assert torch.equal(xh.hi.cpu(), wh.hi) and torch.equal(xh.lo.cpu(), wh.lo) and _pad_intact(*hbufs)
    fb, xf = _fresh((frames * hw, C))
    rt.dn_prologue(ad, bd, frames, C, hw, ape=aped, S=S, out_f=xf)
    assert torch.equal(xf.cpu(), want) and _pad_intact(fb)
    hbufs, xh = _planes((frames * hw, C), torch.float16, split=False)
    rt.dn_prologue(ad, None, frames, C, hw, ape=aped, S=S, out_h=xh)
    assert torch.equal(xh.hi.cpu(), V.dn_prologue(a, None, frames, C, hw, ape, S).half()) and _pad_intact(*hbufs)


def test_dn_prologue_rejects_missing_outputs(rt):
    from vdn import _abi
    a = torch.ones(2 * 5, 8, device=DEV)
    lb, lo = _fresh((2 * 5, 8), dtype=torch.float16)
    fb, xf = _fresh((2 * 5, 8))
    assert _abi.lib.vdn_dn_prologue(_abi.F16, a.data_ptr(), None, 2, 8, 5, None, 1, None, None, None, _stream()) == EINVAL
    assert _abi.lib.vdn_dn_prologue(_abi.F16, a.data_ptr(), None, 2, 8, 5, None, 1, xf.data_ptr(), None, lo.data_ptr(), _stream()) == EINVAL
    assert _untouched(lb, fb)


# ================================================================================================ 8. vdn_dn_tail
TAIL_CASES = {   # F, IH, IW, Cin, OH, OW, residual, relu, outputs
    "cin128_same_size": (1, 5, 6, 128, 5, 6, False, False, "all"),
    "cin128_resized": (1, 5, 6, 128, 9, 11, True, True, "all"),
    "cin1": (2, 4, 5, 1, 7, 9, True, False, "all"),
    "ih1": (2, 1, 7, 8, 3, 9, False, True, "all"),
    "iw1": (2, 6, 1, 8, 9, 4, True, True, "all"),
    "ih1_same_size": (2, 1, 7, 8, 1, 7, False, False, "all"),
    "oh1_ow1": (2, 4, 5, 8, 1, 1, True, False, "all"),
    "oh1": (2, 4, 5, 8, 1, 7, False, False, "raw"),
    "ow1": (2, 4, 5, 8, 6, 1, True, True, "depth"),
    "one_axis": (2, 5, 6, 8, 5, 9, False, True, "all"),
    "down_scale": (2, 9, 8, 8, 4, 5, True, False, "all"),
    "257_pixels_same_size": (1, 257, 1, 4, 257, 1, True, True, "all"),
    "257_pixels_resized": (1, 4, 40, 8, 1, 257, False, False, "all"),
    "raw_only": (2, 6, 7, 8, 9, 10, False, False, "raw"),
    "depth_and_normal_only": (2, 6, 7, 8, 9, 10, True, True, "depth"),
}


@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_dn_tail_edges(rt, case):
    """The LDS table's limit of 128 input channels and a single one; maps one pixel high or wide, where every tap but the
    centre row or column is outside; outputs one pixel high or wide, where the align_corners scale is 0 and every output reads
    source 0; a resize on one axis; a down-scale; 257 output pixels, one of them in a second block; raw alone and depth +
    normal alone. Against the float64 conv3x3 + bilinear restatement at test_dn_tail_vs_fp64's bars: 1e-5 on the rel-L2 of
    every output and on depth's worst pixel."""
    F_, IH, IW, Cin, OH, OW, residual, relu, outputs = TAIL_CASES[case]
    if case.startswith("257"):
        assert F_ * OH * OW == 257
    g = torch.Generator().manual_seed(1800 + sum(TAIL_CASES[case][:6]))
    x = torch.relu(torch.randn(F_, IH, IW, Cin, generator=g))
    w = torch.randn(3, Cin, 3, 3, generator=g) * 0.05
    bias = torch.randn(3, generator=g) * 0.1
    din = torch.randn(F_, OH, OW, generator=g).abs() * 0.1
    y, d, nrm = V.dn_tail(x.numpy(), w.numpy(), bias.numpy(), OH, OW, din.numpy() if residual else None, relu)
    if relu:
        assert (d > 0).any()
    (rb, raw), (db, depth), (nb, normal) = _fresh((F_, 3, OH, OW), NAN), _fresh((F_, OH, OW), NAN), _fresh((F_, 3, OH, OW), NAN)
    rt.dn_tail(x.to(DEV), F_, IH, IW, Cin, w.to(DEV), bias.to(DEV), OH, OW, depth_in=din.to(DEV) if residual else None, relu=relu,
               raw=raw if outputs != "depth" else None, depth=depth if outputs != "raw" else None,
               normal=normal if outputs != "raw" else None)
    assert _pad_intact(rb, db, nb)
    if outputs != "depth":
        e = rel_l2(raw.cpu(), y)
        print(f"[dn_tail {case}] raw rel-L2 {e:.2e}")
        assert bool(torch.isfinite(raw).all()) and e < 1e-5
    else:
        assert bool(torch.isnan(raw).all())
    if outputs != "raw":
        e, wp, en = rel_l2(depth.cpu(), d), worst_px(depth.cpu(), d), rel_l2(normal[:, :2].cpu(), nrm[:, :2])
        print(f"[dn_tail {case}] depth rel-L2 {e:.2e} worst pixel {wp:.2e} normal rel-L2 {en:.2e}")
        assert bool(torch.isfinite(depth).all()) and e < 1e-5 and wp < 1e-5
        assert bool(torch.isfinite(normal).all()) and en < 1e-5 and bool(torch.all(normal[:, 2] == 1))
    else:
        assert bool(torch.isnan(depth).all()) and bool(torch.isnan(normal).all())


def test_dn_tail_rejects(rt):
    """129 input channels: VDN_EUNSUPPORTED. depth without normal, normal without depth, neither raw nor depth, depth_in
    without depth: VDN_EINVAL each."""
    from vdn import _abi
    F_, H, W = 1, 4, 5
    x, w, bias = torch.ones(F_, H, W, 129, device=DEV), torch.ones(3, 129, 3, 3, device=DEV), torch.ones(3, device=DEV)
    (rb, raw), (db, depth), (nb, normal) = _fresh((F_, 3, H, W)), _fresh((F_, H, W)), _fresh((F_, 3, H, W))
    din = torch.ones(F_, H, W, device=DEV)

    def call(Cin, depth_in, r, d, n_):
        return _abi.lib.vdn_dn_tail(x.data_ptr(), F_, H, W, Cin, w.data_ptr(), bias.data_ptr(), H, W, depth_in, 0, r, d, n_, _stream())

    assert call(129, None, raw.data_ptr(), depth.data_ptr(), normal.data_ptr()) == EUNSUPPORTED
    assert call(8, None, raw.data_ptr(), depth.data_ptr(), None) == EINVAL
    assert call(8, None, raw.data_ptr(), None, normal.data_ptr()) == EINVAL
    assert call(8, None, None, None, None) == EINVAL
    assert call(8, din.data_ptr(), raw.data_ptr(), None, None) == EINVAL
    assert _untouched(rb, db, nb)


# ================================================================================================ 9. vdn_depth_to_points
def test_depth_to_points_second_trip_and_odd_last_pixel(rt):
    """One 1449 x 1449 map: 2 099 601 pixels, an odd count, in more pairs than 4096 blocks of 256 lanes. Points and colours
    equal the numpy expression bit for bit, as test_depth_to_points_is_numpy_bit_for_bit; the last pixel has no partner."""
    h = w = 1449
    n = h * w
    assert n % 2 == 1 and n > 2 * 4096 * 256
    rs = np.random.RandomState(1900)
    depth = (rs.rand(h, w) * 20.0).astype(np.float32)
    depth[0, 0], depth[h // 2, w // 3], depth[1, 2] = 0.0, 3.0e38, 1.0e-40
    rgb = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    rgb[-1, -1] = (255, 0, 254)
    wp, wc = V.depth_to_points(depth, rgb, 470.4, 431.7)
    (pb, pts), (cb, col) = _fresh((n, 3), dtype=torch.float64), _fresh((n, 3), dtype=torch.float64)
    rt.depth_to_points(torch.from_numpy(depth).to(DEV), torch.from_numpy(rgb).to(DEV), 470.4, 431.7, pts, col)
    gp, gc = pts.cpu().numpy(), col.cpu().numpy()
    assert _pad_intact(pb, cb)
    z = float(depth[-1, -1])
    assert gp[-1].tolist() == [(w - 1 - w / 2) / 470.4 * z, (h - 1 - h / 2) / 431.7 * z, z] and gc[-1].tolist() == [1.0, 0.0, 254 / 255.0]
    assert np.array_equal(gp, wp) and np.array_equal(gc, wc)
