"""The normalisation, elementwise and spatial kernels (csrc/norm.hip, csrc/spatial.hip) where the unit tests of
test_gpu_ops.py do not go: past the first round of a persistent or grid-stride launch, at the channel counts next to every
guard, at the tile switch of dwconv7, in bf16 and in split planes, and at the shapes the entry points reject. References are
the float64 restatements of tests/elementwise_ref.py on the same rounded inputs; bars are that file's (1e-5 for a float32
output, 1e-3 for fp16, 1.5e-2 for bf16) unless a test says otherwise. Every shape is the smallest that reaches its branch."""
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as E
from elementwise_ref import close64

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {torch.float32: 1e-5, torch.float16: 1e-3, torch.bfloat16: 1.5e-2}
EINVAL, EALIGN = -1, -3   # enum vdn_status (include/vdn.h)


@pytest.fixture(scope="module")
def rt():
    from vdn.runtime import Runtime
    from vdn import _abi
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    assert _abi.lib.vdn_arch_ok() == 1, "not a gfx950 device"
    return Runtime(torch.device("cuda:0"), torch.float16)


@pytest.fixture(scope="module")
def rt3():
    from vdn.runtime import Runtime
    return Runtime(torch.device("cuda:0"), torch.float16, split=True)


@pytest.fixture(scope="module")
def rtb():
    from vdn.runtime import Runtime
    return Runtime(torch.device("cuda:0"), torch.bfloat16)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def planes(n, *shape):
    """Fresh split-plane output (not from the arena: a test must not see what an earlier one left there)."""
    from vdn.runtime import HL
    return HL(*(torch.full(shape, float("nan"), device=DEV, dtype=torch.float16) for _ in range(n)))


# ================================================================================================ 3.1 LayerNorm
@pytest.mark.parametrize("C", [64, 1024, 2048])
def test_layernorm_persistent_rounds(rt, C):
    """rows = 2.5 x (8 blocks per CU x 4 rows per block) + 3: whatever the occupancy query admits (at most 8 blocks per CU),
    every wave walks 2 or 3 rows and the last round is partial; nxt -> cur hand-over, the prefetch guard and, with out_group,
    the compaction across rounds. Every output row is compared."""
    rows = 4 * 8 * cus() * 5 // 2 + 3
    x = E.tagged(rows, C, seed=300 + C) * 3 + 1
    w, b = E.noise(C, seed=301), E.noise(C, seed=302)
    vec, tab = E.noise(C, seed=303), E.noise(5, C, seed=304)
    ref = E.layer_norm(x, w, b, 1e-6).to(DEV)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    of = torch.full((rows, C), float("nan"), device=DEV)
    oh = torch.full((rows, C), float("nan"), device=DEV, dtype=torch.float16)
    rt.layernorm(xd, rows, C, wd, bd, 1e-6, out_h=oh, out_f=of)
    print("ln persistent", C, "f32", close64(of, ref, 1e-5), "f16", close64(oh, ref, 1e-3))
    # cls-row compaction in groups of 11
    nout = rows - -(-rows // 11)
    oc = torch.full((nout, C), float("nan"), device=DEV)
    rt.layernorm(xd, rows, C, wd, bd, 1e-6, out_f=oc, out_group=11)
    keep = (torch.arange(rows) % 11 != 0).to(DEV)
    assert int(keep.sum()) == nout
    print("ln persistent", C, "out_group", close64(oc, ref[keep], 1e-5))
    # + alpha * vec + tab[(row // 7) % 5]
    of.fill_(float("nan"))
    rt.layernorm(xd, rows, C, wd, bd, 1e-6, out_f=of, addvec=vec.to(DEV), alpha=0.5, addtab=tab.to(DEV), tab_div=7, tab_mod=5)
    idx = ((torch.arange(rows) // 7) % 5).to(DEV)
    print("ln persistent", C, "vec+tab", close64(of, ref + 0.5 * vec.double().to(DEV) + tab.double().to(DEV)[idx], 1e-5))


@pytest.mark.parametrize("xdt", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("C", [4, 36, 260, 516, 1028, 1536, 2044, 2048])
def test_layernorm_channel_guards(rt, rtb, C, xdt):
    """The `c < C` guard at one lane (4), inside a 256-channel step away from a multiple of 64 (36, 260, 516, 1028, 2044), at the
    first step of NV = 8 (1028) and with every step full (1536 of NV = 8 leaves two empty, 2048 none); every input type, fp16 and
    bf16 outputs."""
    rows = 37
    x = (E.tagged(rows, C, seed=310 + C) * 3 + 1).to(xdt)
    w, b = E.noise(C, seed=311), E.noise(C, seed=312)
    ref = E.layer_norm(x.float(), w, b, 1e-6)
    for r, hdt in ((rt, torch.float16), (rtb, torch.bfloat16)):
        of = torch.full((rows, C), float("nan"), device=DEV)
        oh = torch.full((rows, C), float("nan"), device=DEV, dtype=hdt)
        r.layernorm(x.to(DEV), rows, C, w.to(DEV), b.to(DEV), 1e-6, out_h=oh, out_f=of)
        print("ln guards", C, xdt, "f32", close64(of, ref, 1e-5, f"f32 out, {hdt} runtime"), hdt, close64(oh, ref, TOL[hdt], f"{hdt} out"))
    # the compaction and the table next to the guard
    oc = torch.full((rows - 4, C), float("nan"), device=DEV)
    tab = E.noise(5, C, seed=313)
    rt.layernorm(x.to(DEV), rows, C, w.to(DEV), b.to(DEV), 1e-6, out_f=oc, out_group=11, addtab=tab.to(DEV), tab_div=7, tab_mod=5)
    close64(oc, E.layer_norm(x.float(), w, b, 1e-6, tab=tab, tab_div=7, tab_mod=5, out_group=11), 1e-5)


@pytest.mark.parametrize("kt", [False, True], ids=["rowmajor", "ktile"])
def test_layernorm_6bit_planes_persistent(rt3, kt):
    """The X6 instantiation past its own grid cap (3 blocks per CU by its LDS): 2.5 rounds, so the staging buffer of a wave is
    reused by its next row. Checked as test_layernorm_8bit_planes_and_k_tile_major checks one round: against the split-plane
    output of the plain instantiation pushed through vdn_pack_x8, and that against float64 (2e-6: two planes, ~21 bits)."""
    from vdn import pack
    from vdn.runtime import HL
    from test_gpu_ops import _check_x6, _same_rows, _unkt16
    rows, C = 4 * 3 * cus() * 5 // 2 + 3, 64
    x = E.tagged(rows, C, seed=320) * 3 + 1
    w, b = E.noise(C, seed=321), E.noise(C, seed=322)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    ref = planes(2, rows, C)
    rt3.layernorm(xd, rows, C, wd, bd, 1e-6, out_h=ref)
    close64(ref.float(), E.layer_norm(x, w, b, 1e-6), 2e-6)
    oh = HL(torch.zeros(rows, C, dtype=torch.float16, device=DEV))
    o8 = torch.zeros(2, rows, C, dtype=torch.uint8, device=DEV)
    rt3.layernorm(xd, rows, C, wd, bd, 1e-6, out_h=oh, out8=o8, kt=kt)
    assert torch.equal(_unkt16(oh.hi, rows, C) if kt else oh.hi, ref.hi)
    _same_rows(o8, pack.planes8(ref, pack.ORDER_NATURAL, kt=kt))
    _check_x6(o8, ref, rows, C, pack.ORDER_NATURAL, kt=kt)


# ================================================================================================ 3.2 GroupNorm
GN_SHAPES = [(2, 50, 8, 1), (1, 3, 64, 32), (1, 1, 64, 32), (2, 100, 264, 33), (1, 130, 2048, 64), (2, 361, 1024, 1)]


@pytest.mark.parametrize("F_,HW,C,groups", GN_SHAPES)
def test_groupnorm_shapes(rt, rt3, F_, HW, C, groups):
    """One group and 64 of them (the size of the apply kernel's table), C = 8 (256 pixel lanes) and 2048 (one), 33 channel
    vectors (25 idle threads), fewer pixels than splits (empty splits), one pixel. fp16 planes at 1e-3 and split planes at 5e-6
    (the bar of test_x3_temporal_norms_upsample_headout), inputs of mean / std ratio 0.25."""
    x = E.noise(F_, HW, C, seed=330 + C) + 0.25
    w, b = E.noise(C, seed=331), E.noise(C, seed=332)
    xh = x.half()
    y = torch.full((F_, HW, C), float("nan"), device=DEV, dtype=torch.float16)
    rt.groupnorm(xh.to(DEV), y, F_, HW, C, groups, w.to(DEV), b.to(DEV), 1e-6)
    print("gn shape", (F_, HW, C, groups), "f16", close64(y, E.group_norm(xh.float(), groups, w, b, 1e-6), 1e-3))
    hi, lo, val = E.gn_input(F_, HW, C, 0.25, seed=333 + C)
    from vdn.runtime import HL
    y3 = planes(2, F_, HW, C)
    rt3.groupnorm(HL(hi.to(DEV), lo.to(DEV)), y3, F_, HW, C, groups, w.to(DEV), b.to(DEV), 1e-6)
    print("gn shape", (F_, HW, C, groups), "planes", close64(y3.float(), E.group_norm(val, groups, w, b, 1e-6), 5e-6))


@pytest.mark.parametrize("nsplit", [1, 64])
def test_groupnorm_nsplit_through_abi(rt3, nsplit):
    """One split, and 64 over 50 pixels (14 of them empty), through the C-ABI with a poisoned workspace."""
    from vdn import _abi
    F_, HW, C, groups = 2, 50, 192, 32
    hi, lo, val = E.gn_input(F_, HW, C, 0.25, seed=340)
    w, b = E.noise(C, seed=341).to(DEV), E.noise(C, seed=342).to(DEV)
    hid, lod = hi.to(DEV), lo.to(DEV)
    y = planes(2, F_, HW, C)
    part = torch.full((F_, nsplit, groups, 2), float("nan"), device=DEV)
    rc = _abi.lib.vdn_groupnorm(_abi.F16, hid.data_ptr(), lod.data_ptr(), y.hi.data_ptr(), y.lo.data_ptr(), F_, HW, C, groups,
                                w.data_ptr(), b.data_ptr(), 1e-6, part.data_ptr(), nsplit, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    close64(y.float(), E.group_norm(val, groups, w.cpu(), b.cpu(), 1e-6), 5e-6)
    assert bool(torch.isfinite(part).all())   # every split wrote its slot, the empty ones too


@pytest.mark.parametrize("k", [0.25, 4, 16, 64, 256])
@pytest.mark.parametrize("HW,C", [(361, 256), (1369, 256), (361, 1024)])
def test_groupnorm_accuracy_against_torch_fp32(rt3, HW, C, k):
    """Inputs N(k, 1), k = mean / std of a group up to 256, in and out as split planes (about 22 bits). The kernel's rel-L2 and
    worst-element errors against float64 must stay within max(4 x the same error of torch's float32 CPU group_norm, 4e-7): the
    factor 4 is a margin for another fixed summation order and the toward-zero split (2^-22 per value), 4e-7 that split's floor.
    tests/test_elementwise_ref_host.py holds torch's side below 1e-4, so the bound is never loose.
    A variance taken as q / n - mean^2 from one pass of fp32 sums fails this from k = 4 or 16 on (3.6e-4 at k = 64, 6e-3 at 256:
    profiles/elementwise_edges.md)."""
    from vdn.runtime import HL
    F_, groups = 2, 32
    w, b = 1 + 0.25 * E.noise(C, seed=21), 0.25 * E.noise(C, seed=22)
    hi, lo, val = E.gn_input(F_, HW, C, k, seed=23)
    ref = E.group_norm(val, groups, w, b, 1e-6)
    t_err, t_mx = E.errors64(F.group_norm(val.permute(0, 2, 1), groups, w, b, 1e-6).permute(0, 2, 1), ref)
    y = planes(2, F_, HW, C)
    rt3.groupnorm(HL(hi.to(DEV), lo.to(DEV)), y, F_, HW, C, groups, w.to(DEV), b.to(DEV), 1e-6)
    assert bool(torch.isfinite(y.float()).all())
    err, mx = E.errors64(y.float(), ref)
    print(f"gn accuracy HW={HW} C={C} k={k}: kernel rel-L2 {err:.2e} worst {mx:.2e} | torch fp32 rel-L2 {t_err:.2e} worst {t_mx:.2e}")
    assert err <= max(4 * t_err, 4e-7) and mx <= max(4 * t_mx, 4e-7), (err, mx, t_err, t_mx)


# ================================================================================================ 3.3 above the block cap
def test_add_vec_above_cap(rt):
    """5003 x 772 floats = 965 579 vectors > 2048 blocks x 256 lanes; 772 = 4 x 193 is no power of two, so the vector index wraps
    inside a grid stride. One fused multiply-add per value: 1e-6."""
    rows, C = 5003, 772
    assert rows * C // 4 > 2048 * 256
    x, vec = E.tagged(rows, C, seed=350), E.tagged(1, C, seed=351)[0]
    y = torch.full((rows, C), float("nan"), device=DEV)
    rt.add_vec(x.to(DEV), vec.to(DEV), 0.1, y, rows, C)
    print("add_vec", close64(y, E.add_vec(x, vec, 0.1), 1e-6))


@pytest.mark.parametrize("rows,C", [(9001, 1028), (37, 36)])
def test_addtab_cast(rt, rt3, rtb, rows, C):
    """9001 x 1028 floats = 2 313 257 vectors > 8192 x 256, table row (row // 1370) % 3 (the pos-embed of 1370-token images);
    fp16, split planes (hi + lo at 1e-6), bf16, and without a table."""
    x, tab = E.tagged(rows, C, seed=360), E.noise(3, C, seed=361)
    if rows > 1000:
        assert rows * C // 4 > 8192 * 256
    xd, td = x.to(DEV), tab.to(DEV)
    ref = E.addtab_cast(x, tab, 1370, 3).to(DEV)
    for r, dt in ((rt, torch.float16), (rtb, torch.bfloat16)):
        y = torch.full((rows, C), float("nan"), device=DEV, dtype=dt)
        r.addtab_cast(xd, td, 1370, 3, y, rows, C)
        print("addtab_cast", rows, dt, close64(y, ref, TOL[dt]))
    y3 = planes(2, rows, C)
    rt3.addtab_cast(xd, td, 1370, 3, y3, rows, C)
    print("addtab_cast", rows, "planes", close64(y3.float(), ref, 1e-6))
    y = torch.full((rows, C), float("nan"), device=DEV, dtype=torch.float16)
    rt.addtab_cast(xd, None, 1, 1, y, rows, C)
    assert torch.equal(y.cpu(), x.half())   # no table: the conversion alone, to nearest


@pytest.mark.parametrize("ydt", [torch.float16, torch.bfloat16, torch.float32], ids=["to_f16", "to_bf16", "to_f32"])
@pytest.mark.parametrize("xdt", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
def test_cast_bitwise_all_pairs(rt, xdt, ydt):
    """1 500 007 elements > 4096 x 256: every pair of types must give the bits of tensor.to(dtype) (round to nearest even,
    subnormals kept, overflow to inf, -0 kept); NaN is compared as NaN."""
    n = 1_500_007
    x = E.cast_input(n, seed=370).to(xdt)
    want = x.to(ydt)
    y = torch.empty(n, device=DEV, dtype=ydt)
    y.view(torch.int32 if ydt == torch.float32 else torch.int16).fill_(0x5a5a)
    rt.cast(x.to(DEV), y)
    got = y.cpu()
    assert torch.equal(got.isnan(), want.isnan())
    iv = torch.int32 if ydt == torch.float32 else torch.int16
    ok = want.isnan() | (got.view(iv) == want.view(iv))
    assert bool(ok.all()), (int((~ok).sum()), x[~ok][:8].tolist(), got[~ok][:8].tolist(), want[~ok][:8].tolist())


def _grid(B, H, W, C, seed, dtype=torch.float32):
    return E.tagged(B * H * W, C, seed=seed, dtype=dtype).reshape(B, H, W, C)


@pytest.mark.parametrize("B,ih,iw,oh,ow,C", [(1, 150, 150, 300, 300, 384), (2, 5, 7, 11, 9, 8), (1, 19, 13, 37, 30, 136)])
def test_upsample_above_cap_and_channel_counts(rt, B, ih, iw, oh, ow, C):
    """300 x 300 x 48 vectors = 4 320 000 > 16384 x 256; one channel vector per pixel (8) and 17 (136: no power of two)."""
    if C == 384:
        assert B * oh * ow * (C // 8) > 16384 * 256
    x = _grid(B, ih, iw, C, 380, torch.float16)
    y = torch.full((B, oh, ow, C), float("nan"), device=DEV, dtype=torch.float16)
    rt.upsample(x.half().to(DEV), y, B, ih, iw, oh, ow, C)
    print("upsample", C, close64(y, E.bilinear_ac(x, oh, ow), 1e-3))


def test_upsample_bf16_and_planes(rtb, rt3):
    B, ih, iw, oh, ow, C = 2, 19, 13, 37, 30, 136
    x = _grid(B, ih, iw, C, 381, torch.bfloat16)
    y = torch.full((B, oh, ow, C), float("nan"), device=DEV, dtype=torch.bfloat16)
    rtb.upsample(x.bfloat16().to(DEV), y, B, ih, iw, oh, ow, C)
    print("upsample bf16", close64(y, E.bilinear_ac(x, oh, ow), 1.5e-2))
    xf = _grid(B, ih, iw, C, 382)
    xs = rt3.to_half(xf.to(DEV))
    y3 = planes(2, B, oh, ow, C)
    rt3.upsample(xs, y3, B, ih, iw, oh, ow, C)
    print("upsample planes", close64(y3.float(), E.bilinear_ac(xs.float().cpu(), oh, ow), 3e-6))   # the bar of test_x3_temporal_norms_upsample_headout


def test_upsample_f32_above_cap(rt):
    """2 x 777 x 700 = 1 087 800 outputs > 4096 x 256, with the ReLU."""
    B, ih, iw, oh, ow = 2, 390, 350, 777, 700
    assert B * oh * ow > 4096 * 256
    x = _grid(B, ih, iw, 1, 383)[..., 0] - 1.5
    y = torch.full((B, oh, ow), float("nan"), device=DEV)
    rt.upsample_f32(x.to(DEV), y, B, ih, iw, oh, ow, relu=True)
    ref = E.bilinear_ac(x, oh, ow).clamp(min=0)
    assert 0.2 < float((ref == 0).double().mean()) < 0.8   # the ReLU cuts a real share of the map
    print("upsample_f32", close64(y, ref, 1e-5))


def test_bicubic_above_cap(rt):
    """74 x 74 x 384 = 2 102 784 outputs > 4096 x 256; the pos-embed's scale_factor semantics (oh + 0.1) / 37."""
    gs, oh, ow, C = 37, 74, 74, 384
    assert oh * ow * C > 4096 * 256
    g = _grid(1, gs, gs, C, 390)[0]
    sy, sx = (oh + 0.1) / gs, (ow + 0.1) / gs
    ref = F.interpolate(g.double().permute(2, 0, 1)[None], scale_factor=(sy, sx), mode="bicubic")[0].permute(1, 2, 0)
    assert ref.shape[:2] == (oh, ow)
    y = torch.full((oh, ow, C), float("nan"), device=DEV)
    rt.bicubic(g.to(DEV), y, gs, gs, oh, ow, C, sy, sx)
    print("bicubic", close64(y, ref, 1e-5))


@pytest.mark.parametrize("C", [8, 64])
def test_head_out_above_cap(rt, rt3, rtb, C):
    """M = 2 100 003 > 8192 x 256 pixels, at the two edges of the kernel's 64-entry weight table: 8 channels and 64; ReLU on and
    off; split planes at C = 64 (the lo plane reads the same table), bf16 at C = 8."""
    M = 2_100_003
    assert M > 8192 * 256
    w = E.noise(C, seed=400)
    wd = w.to(DEV)
    f = (E.tagged(M, C, seed=401) - 1.0).half().float()
    fd = f.half().to(DEV)
    for relu in (False, True):
        d = torch.full((M,), float("nan"), device=DEV)
        rt.head_out(fd, wd, -0.3, d, M, C, relu=relu)
        ref = E.head_out(f, w, -0.3, relu)
        if relu:
            assert 0.05 < float((ref == 0).double().mean()) < 0.95
        print("head_out", C, "relu" if relu else "plain", close64(d, ref, 1e-5))
    del fd
    if C == 64:
        ff = E.tagged(M, C, seed=402) - 1.0
        fs = rt3.to_half(ff.to(DEV))
        d = torch.full((M,), float("nan"), device=DEV)
        rt3.head_out(fs, wd, -0.3, d, M, C, relu=False)
        print("head_out", C, "planes", close64(d, E.head_out(fs.float().cpu(), w, -0.3, False), 1e-5))
    else:
        fb = (E.tagged(M, C, seed=403) - 1.0).bfloat16()
        d = torch.full((M,), float("nan"), device=DEV)
        rtb.head_out(fb.to(DEV), wd, -0.3, d, M, C, relu=True)
        print("head_out", C, "bf16", close64(d, E.head_out(fb.float(), w, -0.3, True), 1e-5))


def test_patchify_above_cap(rt3):
    """20 images of 518 x 518: 27 380 rows x 80 vectors = 2 190 400 > 8192 x 256, split planes. The planes hold the pixel to
    2^-22 (1e-6, as test_x3_temporal_norms_upsample_headout); the 52 pad columns are zero in both."""
    B, H, W, ldk = 20, 518, 518, 640
    nrows = B * 37 * 37
    assert nrows * (ldk // 8) > 8192 * 256
    img = E.tagged(B * 3 * H, W, seed=410).reshape(B, 3, H, W)
    rows = planes(2, nrows, ldk)
    rt3.patchify(img.to(DEV), rows, B, H, W, ldk)
    print("patchify", close64(rows.float()[:, :588], E.patchify(img.double()), 1e-6))
    assert float(rows.hi[:, 588:].float().abs().max()) == 0.0 and float(rows.lo[:, 588:].float().abs().max()) == 0.0


def test_patchify_ldk_704(rt, rt3, rtb):
    """A row stride of 704 (the next multiple of 64 after 640): 116 pad columns, all three operand modes."""
    B, H, W, ldk = 1, 28, 42, 704
    img = E.tagged(B * 3 * H, W, seed=411).reshape(B, 3, H, W)
    ref = E.patchify(img.double())
    for r, dt in ((rt, torch.float16), (rtb, torch.bfloat16)):
        rows = torch.full((6, ldk), float("nan"), device=DEV, dtype=dt)
        r.patchify(img.to(DEV), rows, B, H, W, ldk)
        assert torch.equal(rows[:, :588].cpu(), ref.float().to(dt))   # one rounding to nearest of the pixel itself
        assert float(rows[:, 588:].float().abs().max()) == 0.0
    rows = planes(2, 6, ldk)
    rt3.patchify(img.to(DEV), rows, B, H, W, ldk)
    print("patchify 704 planes", close64(rows.float()[:, :588], ref, 1e-6))
    assert float(rows.hi[:, 588:].float().abs().max()) == 0.0 and float(rows.lo[:, 588:].float().abs().max()) == 0.0


def test_mask_down1_above_cap(rt):
    """16 maps of 518 x 518 -> 259 x 259: 1 073 296 outputs > 4096 x 256. The reference of test_mask_downsampler_stages (sigmoid ->
    conv 3 x 3 stride 2 -> LayerNorm2d -> GELU -> conv 1 x 1), in float64."""
    from oracle import ref_cpu as O
    B, H, W = 16, 518, 518
    depth = F.relu(E.tagged(B * H, W, seed=420).reshape(B, 1, H, W) - 1.0)
    e0 = dict(w0=E.noise(4, 1, 3, 3, seed=421), b0=E.noise(4, seed=422), lw=E.noise(4, seed=423) + 1, lb=E.noise(4, seed=424),
              w3=E.noise(1, 4, 1, 1, seed=425), b3=E.noise(1, seed=426))
    d = {k: v.double() for k, v in e0.items()}
    m = F.conv2d(torch.sigmoid(depth.double()), d["w0"], d["b0"], stride=2, padding=1)
    ref = F.conv2d(F.gelu(O.layer_norm_2d(m, d["lw"], d["lb"])), d["w3"], d["b3"])[:, 0]
    oh, ow = ref.shape[-2:]
    assert B * oh * ow > 4096 * 256
    flat = torch.cat([e0[k].reshape(-1) for k in ("w0", "b0", "lw", "lb", "w3", "b3")]).to(DEV)
    o1 = torch.full((B, oh, ow), float("nan"), device=DEV)
    rt.mask_down1(depth[:, 0].contiguous().to(DEV), o1, B, H, W, oh, ow, flat)
    print("mask_down1", close64(o1, ref, 1e-5))


# ================================================================================================ 3.4 dwconv7
@pytest.mark.parametrize("B,H,W,C", [(1, 9, 72, 32), (1, 8, 73, 32), (2, 1, 64, 64), (1, 7, 65, 32), (1, 17, 128, 32), (1, 3, 129, 64)])
def test_dwconv7_tile_switch(rt, B, H, W, C):
    """W = 72 is the widest whole-row tile ((49 x 32 + 14 x 78 x 36) x 4 = 163 520 of 163 840 bytes of LDS), 73 the first map in
    64-column tiles (a 9-column last tile); 64 / 65 and 128 / 129 put the tile edge on and one past the map's; fewer rows than
    a tile's 8, one row, one channel block."""
    x = _grid(B, H, W, C, 430)
    w, b = E.noise(49, C, seed=431, scale=0.15), E.noise(C, seed=432)
    y = torch.full((B, H, W, C), float("nan"), device=DEV)
    rt.dwconv7(x.to(DEV), y, B, H, W, C, w.to(DEV), b.to(DEV))
    print("dwconv7", (B, H, W, C), close64(y, E.dwconv7(x, w, b), 1e-5))


# ================================================================================================ 3.5 rejected shapes
SENTINEL = -7.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _untouched(*ts):
    torch.cuda.synchronize()
    for t in ts:
        assert bool((t.float() == SENTINEL).all())


@pytest.mark.parametrize("C", [6, 2052])
def test_layernorm_rejects_channel_counts(rt, C):
    """C must be a multiple of 4 and at most 2048 (NV = 8 steps of 256): VDN_EALIGN, nothing launched."""
    from vdn import _abi
    rows = 5
    x, w, b = torch.ones(rows, C, device=DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    of = torch.full((rows, C), SENTINEL, device=DEV)
    oh = torch.full((rows, C), SENTINEL, device=DEV, dtype=torch.float16)
    rc = _abi.lib.vdn_layernorm(x.data_ptr(), _abi.F32, rows, C, w.data_ptr(), b.data_ptr(), 1e-6, None, 1.0, None, 1, 1, 0,
                                oh.data_ptr(), None, _abi.F16, of.data_ptr(), None, 0, _stream())
    assert rc == EALIGN
    _untouched(of, oh)


@pytest.mark.parametrize("C,groups", [(130 * 8, 65), (100, 32)])
def test_groupnorm_rejects_group_counts(rt, C, groups):
    """More than 64 groups (the apply kernel's table) and a channel count the groups do not divide: VDN_EINVAL."""
    from vdn import _abi
    F_, HW = 1, 4
    x = torch.ones(F_, HW, C, device=DEV, dtype=torch.float16)
    w, b = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    y = torch.full((F_, HW, C), SENTINEL, device=DEV, dtype=torch.float16)
    part = torch.full((F_, 4, groups, 2), SENTINEL, device=DEV)
    rc = _abi.lib.vdn_groupnorm(_abi.F16, x.data_ptr(), None, y.data_ptr(), None, F_, HW, C, groups, w.data_ptr(), b.data_ptr(), 1e-6,
                                part.data_ptr(), 4, _stream())
    assert rc == EINVAL
    _untouched(y, part)


def test_head_out_rejects_72_channels(rt):
    """The weight table holds 64 entries: VDN_EINVAL."""
    from vdn import _abi
    M, C = 10, 72
    f = torch.ones(M, C, device=DEV, dtype=torch.float16)
    w = torch.ones(C, device=DEV)
    d = torch.full((M,), SENTINEL, device=DEV)
    assert _abi.lib.vdn_head_out(_abi.F16, f.data_ptr(), None, w.data_ptr(), 0.0, d.data_ptr(), M, C, 0, _stream()) == EINVAL
    _untouched(d)


def test_patchify_rejects_ldk_600(rt):
    """The row stride must be a multiple of 64 (the GEMM's K tile) and at least 588: VDN_EALIGN."""
    from vdn import _abi
    img = torch.ones(1, 3, 28, 28, device=DEV)
    rows = torch.full((4, 640), SENTINEL, device=DEV, dtype=torch.float16)
    assert _abi.lib.vdn_patchify(_abi.F16, img.data_ptr(), rows.data_ptr(), None, 1, 28, 28, 600, _stream()) == EALIGN
    _untouched(rows)
