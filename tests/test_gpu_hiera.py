"""Native Hiera trunk on the MI355X: the kernels of csrc/hiera.hip and the trunk's attention (csrc/lane_attn.hip) against
torch computations made here (tests/hiera_ref.py), the trunk against the fixtures tools/make_golden_hiera.py took from the `transformers` port of the
model, and the depth + normal model on native trunks against the imported reference wrapper's fixture."""
import os

import numpy as np
import pytest
import torch

import dn_fixture as DF
import hiera_ref as HR
from common import rel_l2, worst_px

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-3
DEV = torch.device("cuda:0")
NAMES = {(1, 2, 7, 2): "hiera_tiny_224", (1, 2, 11, 2): "hiera_small_224", (2, 3, 16, 3): "hiera_base_224"}


def _rt(split=True, half=torch.float16):
    from vdn.runtime import Runtime
    return Runtime(DEV, half, split)


def _load(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _frames(n):
    from vdn import synth
    return torch.from_numpy(synth.normalize_frames(synth.frames_u8(DF.SEED, n, 224, 224)))


# ------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("heads,W,Lkv,qs", [(1, 49, 64, 1), (2, 49, 64, 4), (2, 49, 16, 1), (4, 49, 16, 4), (4, 1, 196, 1),
                                            (8, 1, 196, 4), (8, 1, 49, 1)])
def test_hiera_attn_vs_fp64(heads, W, Lkv, qs, split):
    """Every row of the shape table, fp64 reference on the values the planes hold."""
    rt = _rt(split)
    F, C = 3, heads * 96
    rows = F * W * Lkv
    g = torch.Generator().manual_seed(heads * 100 + Lkv + qs)
    qkv = rt.to_half((torch.randn(rows, 3 * C, generator=g) * 1.2).to(DEV))
    out = rt.hbuf("a", (rows // qs, C))
    rt.hiera_attn(qkv, out, F, heads, W, Lkv, qs, 96 ** -0.5)
    ref = HR.attn_rows(qkv.float().cpu().double().reshape(F, W * Lkv, 3 * C), heads, W, Lkv, qs).reshape(rows // qs, C)
    got = out.float().cpu()
    tol = 1e-5 if split else 2e-3
    print(f"hiera_attn heads={heads} W={W} Lkv={Lkv} qs={qs} split={split}: rel-L2 {rel_l2(got, ref):.2e} worst {worst_px(got, ref):.2e}")
    assert rel_l2(got, ref) < tol
    assert worst_px(got, ref) < 10 * tol


def test_hiera_attn_bf16_planes():
    rt = _rt(True, torch.bfloat16)
    F, heads, W, Lkv, qs = 2, 2, 49, 64, 4
    C, rows = heads * 96, F * W * Lkv
    qkv = rt.to_half(torch.randn(rows, 3 * C, generator=torch.Generator().manual_seed(3)).to(DEV))
    out = rt.hbuf("a", (rows // qs, C))
    rt.hiera_attn(qkv, out, F, heads, W, Lkv, qs, 96 ** -0.5)
    ref = HR.attn_rows(qkv.float().cpu().double().reshape(F, W * Lkv, 3 * C), heads, W, Lkv, qs).reshape(rows // qs, C)
    assert rel_l2(out.float().cpu(), ref) < 1e-4


def test_hiera_pool_exact():
    rt = _rt()
    F, n, C = 3, 196, 384
    x = torch.randn(F, 4 * n, C, generator=torch.Generator().manual_seed(1))
    y = torch.empty(F, n, C, device=DEV)
    rt.hiera_pool(x.to(DEV), y, F, n, C)
    assert torch.equal(y.cpu(), x.reshape(F, 4, n, C).max(1).values)


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
def test_hiera_reroll_exact(stage):
    rt = _rt()
    F, side, C = 2, 56 >> stage, 96 << stage
    x = torch.randn(F, side * side, C, generator=torch.Generator().manual_seed(stage))
    out = torch.empty(F, side, side, C, device=DEV)
    rt.hiera_reroll(x.to(DEV), out, F, stage, C)
    assert torch.equal(out.cpu(), HR.reroll(x, stage))
    with np.load(os.path.join(GOLD, "hiera_tiny_f2.npz")) as z:   # and against the oracle's own reroll of an arange
        ar = torch.arange(side * side, dtype=torch.float32).reshape(1, -1, 1).expand(1, -1, 4).contiguous()
        o = torch.empty(1, side, side, 4, device=DEV)
        rt.hiera_reroll(ar.to(DEV), o, 1, stage, 4)
        assert np.array_equal(o[..., 0].reshape(-1).long().cpu().numpy(), z[f"reroll{stage}"])


def test_hiera_embed_rows_exact_and_projection():
    """The gathered rows equal unfold(7, stride 4, pad 3) in unrolled order, value for value (hi + lo planes hold an f32 input
    to 2^-21); the projection + pos_embed on vdn_gemm equals the convolution to 1e-6."""
    import torch.nn.functional as Fn
    from vdn import pack
    from vdn.runtime import HL
    rt = _rt()
    F = 2
    img = _frames(F)
    rows = rt.hbuf("rows", (F * 3136, 192))
    rt.hiera_embed(img.to(DEV), rows, F, 192)
    cols = Fn.unfold(img, 7, padding=3, stride=4).transpose(1, 2)[:, HR.unroll_index(3)].reshape(F * 3136, 147)
    want = HL.from_float(cols, torch.float16, True)
    assert torch.equal(rows.hi[:, :147].cpu(), want.hi) and torch.equal(rows.lo[:, :147].cpu(), want.lo)
    assert not rows.hi[:, 147:].any() and not rows.lo[:, 147:].any()
    g = torch.Generator().manual_seed(9)
    sd = {"patch_embed.proj.weight": torch.randn(96, 3, 7, 7, generator=g) / 12, "patch_embed.proj.bias": torch.randn(96, generator=g) * 0.1,
          "pos_embed": torch.randn(1, 3136, 96, generator=g) * 0.3}
    ref = HR.embed({k: v.double() for k, v in sd.items()}, img.double()).reshape(F * 3136, 96)
    x = rt.fbuf("x", (F * 3136, 96))
    tab = sd["pos_embed"][0][HR.unroll_index(3)].contiguous().to(DEV)
    rt.gemm(rows, pack.patch_embed(sd["patch_embed.proj.weight"].to(DEV), rt.prec), F * 3136, 96, 192,
            bias=sd["patch_embed.proj.bias"].to(DEV), tab=tab, tab_mod=3136, out=x)
    print(f"hiera_embed projection rel-L2 {rel_l2(x.cpu(), ref):.2e} worst {worst_px(x.cpu(), ref):.2e}")
    # split planes hold each operand to 2^-21 (hi + lo of 11 bits each, nearest): two operands per product, 2 * 2^-21 ~ 1e-6
    # is the worst case per term and the bound for both figures (random signs leave about a third of it)
    assert rel_l2(x.cpu(), ref) < 1e-6 and worst_px(x.cpu(), ref) < 1e-6


# ------------------------------------------------------------------------------------------------------ fixtures
def _check(got, ref, names, where):
    for n in names:
        raw, mr, wraw, wmr = DF.metrics(got, ref, n)
        print(f"{where}:{n} rel-L2 {raw:.2e} mean-removed {mr:.2e} worst {wraw:.2e} / {wmr:.2e} (bar {TOL:.1e})")
        assert raw < TOL and mr < TOL and wraw < TOL and wmr < TOL, (where, n, raw, mr, wraw, wmr)


def _summary(name, t, n):
    N, C = t.shape[0], t.shape[-1]
    return DF.summarise(name, t.reshape(N, -1, C).permute(0, 2, 1), n)


def _trunk(z, precision=None):
    import vdn
    F, depths = int(z["meta"][0]), tuple(int(v) for v in z["meta"][1:])
    enc = vdn.HieraImageEncoder(NAMES[depths])
    enc.load_state_dict(DF.state_dict(enc), strict=True)
    enc = enc.to(DEV).eval()
    if precision:
        enc.set_precision(precision)
    return enc, _frames(F).to(DEV), F


def _run_fixture(name, precision=None):
    z = _load(name)
    enc, x, F = _trunk(z, precision)
    cls_out, maps = enc(x, taps=True)
    assert cls_out is None and len(maps) == 4
    got = {}
    for s, m in enumerate(maps):
        assert m.shape == (F, 56 >> s, 56 >> s, 96 << s) and m.dtype == torch.float32 and m.is_contiguous()
        got.update(_summary(f"map{s}", m, int(z["map0_idx"].size)))
    taps = ["embed"] + [f"first{s}" for s in range(4)]
    for k in taps:
        T = int(z[f"{k}_per"])
        got.update(_summary(k, enc._taps[k].reshape(F, T, -1), int(z[f"{k}_idx"].size)))
    where = name + (f"[{precision}]" if precision else "")
    _check(got, z, taps, where)                              # tap by tap, in the order the stream passes them
    _check(got, z, [f"map{s}" for s in range(4)], where)


@pytest.mark.parametrize("name", ["hiera_tiny_f2", "hiera_base_f2", "hiera_base_f8"])
def test_trunk_fixture(name):
    _run_fixture(name)


def test_trunk_fixture_bf16x3():
    _run_fixture("hiera_tiny_f2", "bf16x3")


def test_trunk_repeat_is_bitwise_equal_and_allocates_no_workspace():
    z = _load("hiera_tiny_f2")
    enc, x, _ = _trunk(z)
    a = [m.clone() for m in enc(x)[1]]
    rt = enc._eng["rt"]
    nbufs = len(rt._bufs)
    b = enc(x)[1]
    assert len(rt._bufs) == nbufs
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_trunk_forward_runs_no_aten_kernel():
    """Between forward's input and its four outputs torch only allocates: the device activity of a forward consists of
    this library's kernels alone (the fp32, contiguous, device-resident input needs no conversion)."""
    from torch.profiler import ProfilerActivity, profile
    z = _load("hiera_tiny_f2")
    enc, x, _ = _trunk(z)
    enc(x)   # engines packed, arena warm
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        enc(x)
        torch.cuda.synchronize()
    compute = [e.name for e in prof.events() if e.name.startswith("aten::") and not e.name.startswith(
        ("aten::empty", "aten::to", "aten::_to_copy", "aten::contiguous", "aten::view", "aten::reshape", "aten::detach", "aten::alias"))]
    assert compute == [], sorted(set(compute))
    copies = [e.name for e in prof.events() if e.name in ("aten::_to_copy", "aten::copy_", "aten::clone")]
    assert copies == [], sorted(set(copies))
    kernels = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    print("device kernels of one trunk forward:", sorted(kernels))
    assert not any(k.startswith(("void at::", "at::", "Cijk", "void rocprim")) for k in kernels), sorted(kernels)
    assert kernels, "the profiler reported no device activity"
    assert any("lane_attn_kernel" in k for k in kernels), sorted(kernels)


# ------------------------------------------------------------------------------------------------------ wrapper
def test_model_on_native_trunks_vs_reference_wrapper():
    import vdn
    z = _load("dn_model_native")
    B, S, H, W, seq = (int(v) for v in z["meta"])
    m = vdn.VideoDepthEstimationModel.with_native_trunks(seq, attention_feature_levels=[int(v) for v in z["levels"]])
    m.load_state_dict(DF.state_dict(m), strict=True)
    m = m.to(DEV).eval()
    depth, img = (torch.from_numpy(t).to(DEV) for t in DF.wrapper_inputs(B, S, H, W))
    d, n = m(depth, img)
    assert d.shape == (B, S, H, W) and n.shape == (B, S, 3, H, W) and torch.all(n[:, :, 2] == 1)
    got = DF.summarise_wrapper(d, n)
    for lvl in (2, 3):
        C, (h, w) = DF.CHANNELS[lvl], DF.SIZES[lvl]
        got.update(DF.summarise(f"tap{lvl}", DF.tokens_as_maps(m._taps[lvl].float(), B * S, C, h * w), DF.N_TAP))
    for k in ("tap2", "tap3", "depth", "dx", "dy"):
        tol = max(TOL, 3 * float(z[f"{k}_cond"])) if f"{k}_cond" in z else TOL   # as tests/test_gpu_dn_head.py: the head's measured conditioning
        raw, mr, wraw, wmr = DF.metrics(got, z, k)
        print(f"dn_model_native:{k} rel-L2 {raw:.2e} mean-removed {mr:.2e} worst {wraw:.2e} / {wmr:.2e} (bar {tol:.1e})")
        assert raw < tol and mr < tol and wraw < tol and wmr < tol, (k, raw, mr, wraw, wmr)


def test_outer_load_state_dict_after_a_forward_repacks_the_trunks():
    """Run, load different weights through the OUTER model, run again: the result must be that of a fresh model with the new
    weights (the trunks' packed planes follow the load), and loading the first weights back must give the first result."""
    import vdn

    def build(seed_shift):
        m = vdn.VideoDepthEstimationModel.with_native_trunks(4, encoder="hiera_tiny_224")
        sd = DF.state_dict(m)
        if seed_shift:   # other trunk weights: the two branches' trunks swapped and the qkv weights rescaled
            sd = {k: v.clone() for k, v in sd.items()}
            for k in list(sd):
                if k.startswith("encoder."):
                    o = "img_" + k
                    sd[k], sd[o] = sd[o], sd[k]
            for k in sd:
                if k.endswith("attn.qkv.weight") and "encoder" in k:
                    sd[k] = sd[k] * 0.8
        return m, sd

    depth, img = (torch.from_numpy(t).to(DEV) for t in DF.wrapper_inputs(1, 4, 224, 224))
    m, sd0 = build(False)
    m.load_state_dict(sd0, strict=True)
    m = m.to(DEV).eval()
    d0, n0 = (t.clone() for t in m(depth, img))
    _, sd1 = build(True)
    m.load_state_dict(sd1, strict=True)          # after a forward, through the outer model only
    d1, n1 = (t.clone() for t in m(depth, img))
    fresh, _ = build(True)
    fresh.load_state_dict(sd1, strict=True)
    fresh = fresh.to(DEV).eval()
    df, nf = fresh(depth, img)
    assert torch.equal(d1, df) and torch.equal(n1, nf)
    assert rel_l2(n1[:, :, :2].cpu(), n0[:, :, :2].cpu()) > 1e-3   # the new weights move the result by more than the parity bar
    m.load_state_dict(sd0, strict=True)
    d2, n2 = m(depth, img)
    assert torch.equal(d2, d0) and torch.equal(n2, n0)
