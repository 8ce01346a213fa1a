"""Depth + normal model on the MI355X: its kernels (csrc/dn_head.hip, csrc/lane_attn.hip) against fp64 torch, and the head / wrapper
against the fixtures the imported reference wrote (tools/make_golden_dn.py)."""
import os

import numpy as np
import pytest
import torch

import dn_fixture as DF
from common import rel_l2, worst_px

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-3
DEV = torch.device("cuda:0")


def _rt(split=True):
    from vdn.runtime import Runtime
    return Runtime(DEV, torch.float16, split)


# ------------------------------------------------------------------------------------------------------ kernels
def _attn_ref(qkv, B, S, hw, C, temporal):
    """fp64 nn.MultiheadAttention core on the token rows [(b s hw), 3C]."""
    x = qkv.double().reshape(B, S, hw, 3, 8, C // 8)
    if temporal:
        x = x.permute(0, 2, 3, 4, 1, 5)            # b, hw, 3, head, S, dh
    else:
        x = x.permute(0, 1, 3, 4, 2, 5)            # b, S, 3, head, hw, dh
    q, k, v = x.unbind(2)
    a = torch.softmax(q @ k.transpose(-1, -2) * (C // 8) ** -0.5, dim=-1) @ v
    if temporal:
        return a.permute(0, 3, 1, 2, 4).reshape(B * S * hw, C)   # b, S, hw, head, dh
    return a.permute(0, 1, 3, 2, 4).reshape(B * S * hw, C)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("C,hw,S,B,temporal", [
    (96, 3136, 2, 1, False), (192, 784, 2, 1, False), (384, 196, 4, 2, False), (768, 49, 4, 2, False),
    (96, 56, 4, 2, True), (192, 40, 32, 1, True), (384, 196, 4, 2, True), (768, 49, 32, 1, True)])
def test_dn_attn_vs_fp64(C, hw, S, B, temporal, split):
    rt = _rt(split)
    rows = B * S * hw
    g = torch.Generator().manual_seed(C + hw + S)
    qkv32 = torch.randn(rows, 3 * C, generator=g) * 1.2
    qkv = rt.to_half(qkv32.to(DEV))
    out = rt.hbuf("a", (rows, C))
    if temporal:
        rt.dn_attn(qkv, out, rows, C, 8, L=S, estride=hw, n0=hw, s0=1, n1=B, s1=S * hw, scale=(C // 8) ** -0.5)
    else:
        rt.dn_attn(qkv, out, rows, C, 8, L=hw, estride=1, n0=1, s0=0, n1=B * S, s1=hw, scale=(C // 8) ** -0.5)
    ref = _attn_ref(qkv.float().cpu(), B, S, hw, C, temporal)
    got = out.float().cpu()
    tol = 1e-5 if split else 2e-3
    assert rel_l2(got, ref) < tol, rel_l2(got, ref)
    assert worst_px(got, ref) < 10 * tol


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("frames,heads,W,Lkv", [(2, 2, 49, 16),    # windowed: the stride translation
                                                (3, 1, 1, 196)])   # global: partial last query tile and last key tile
def test_dn_and_hiera_entries_agree_bitwise(frames, heads, W, Lkv, split):
    """vdn_dn_attn and vdn_hiera_attn are one kernel (csrc/lane_attn.hip) behind two argument lists: on a geometry both can
    express (q_stride 1) the same planes give the same bytes."""
    rt = _rt(split)
    C, rows = heads * 96, frames * W * Lkv
    g = torch.Generator().manual_seed(frames * 1000 + W + Lkv)
    qkv = rt.to_half((torch.randn(rows, 3 * C, generator=g) * 1.2).to(DEV))
    a, b = rt.hbuf("a", (rows, C)), rt.hbuf("b", (rows, C))
    rt.hiera_attn(qkv, a, frames, heads, W, Lkv, 1, 96 ** -0.5)
    rt.dn_attn(qkv, b, rows, C, heads, L=Lkv, estride=W, n0=W, s0=1 if W > 1 else 0, n1=frames, s1=W * Lkv, scale=96 ** -0.5)
    assert torch.equal(a.hi, b.hi)
    assert (a.lo is None) == (b.lo is None) == (not split)
    if split:
        assert torch.equal(a.lo, b.lo)
    assert bool(torch.isfinite(a.hi.float()).all()) and float(a.hi.float().abs().max()) > 0   # both ran on real values


def test_dn_prologue_bitwise():
    """view + add + APE + split, bitwise against torch (the same fp32 operations in the same order)."""
    from vdn.runtime import HL
    rt = _rt(True)
    B, S, h, w, C = 2, 3, 7, 9, 192
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(B * S, h, w, C, generator=g), torch.randn(B * S, h, w, C, generator=g)
    ape = torch.randn(8, C, generator=g)
    ref = (a + b).view(B, S, C, h, w) + ape[:S][None, :, :, None, None]
    ref = ref.permute(0, 1, 3, 4, 2).reshape(-1, C)
    xf = rt.fbuf("x", (B * S * h * w, C))
    xh = rt.hbuf("xh", (B * S * h * w, C))
    rt.dn_prologue(a.to(DEV), b.to(DEV), B * S, C, h * w, ape=ape.to(DEV), S=S, out_f=xf, out_h=xh)
    assert torch.equal(xf.cpu(), ref)
    want = HL.from_float(ref, torch.float16, True)
    assert torch.equal(xh.hi.cpu(), want.hi) and torch.equal(xh.lo.cpu(), want.lo)
    one = rt.hbuf("one", (B * S * h * w, C))   # one trunk, no APE (a non-attention level of the depth-only model)
    rt.dn_prologue(a.to(DEV), None, B * S, C, h * w, out_h=one)
    assert torch.equal(one.hi.cpu(), a.view(B, S, C, h, w).permute(0, 1, 3, 4, 2).reshape(-1, C).half())


@pytest.mark.parametrize("OH,OW,residual,relu", [(32, 40, False, False), (45, 61, True, True)])
def test_dn_tail_vs_fp64(OH, OW, residual, relu):
    import torch.nn.functional as Fn
    rt = _rt(True)
    F, IH, IW, Cin = 3, 32, 40, 48
    g = torch.Generator().manual_seed(OH)
    x = torch.relu(torch.randn(F, IH, IW, Cin, generator=g))
    w = torch.randn(3, Cin, 3, 3, generator=g) * 0.05
    bias = torch.randn(3, generator=g) * 0.1
    din = torch.randn(F, OH, OW, generator=g).abs()
    y = Fn.conv2d(x.double().permute(0, 3, 1, 2), w.double(), bias.double(), padding=1)
    if (OH, OW) != (IH, IW):
        y = Fn.interpolate(y, size=(OH, OW), mode="bilinear", align_corners=True)
    d = y[:, 0] + (din.double() if residual else 0)
    if relu:
        d = torch.relu(d)
    raw = torch.empty(F, 3, OH, OW, device=DEV)
    depth = torch.empty(F, OH, OW, device=DEV)
    normal = torch.empty(F, 3, OH, OW, device=DEV)
    rt.dn_tail(x.to(DEV).contiguous(), F, IH, IW, Cin, w.to(DEV), bias.to(DEV), OH, OW,
               depth_in=din.to(DEV) if residual else None, relu=relu, raw=raw, depth=depth, normal=normal)
    assert rel_l2(raw.cpu(), y) < 1e-5
    assert rel_l2(depth.cpu(), d) < 1e-5 and worst_px(depth.cpu(), d) < 1e-5
    assert rel_l2(normal[:, :2].cpu(), -y[:, 1:]) < 1e-5
    assert torch.all(normal[:, 2] == 1)


# ------------------------------------------------------------------------------------------------------ fixtures
def _load(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _check(got, ref, names, where):
    """Every metric <= 1e-3; a stage tap whose 16 blocks amplify fp32 rounding (the fixture's measured `_cond`: rel-L2 move
    under a 1e-7 input perturbation, tools/make_golden_dn.py) gets 3x that instead when it is larger."""
    for n in names:
        tol = max(TOL, 3 * float(ref[f"{n}_cond"])) if f"{n}_cond" in ref else TOL
        raw, mr, wraw, wmr = DF.metrics(got, ref, n)
        print(f"{where}:{n} rel-L2 {raw:.2e} mean-removed {mr:.2e} worst {wraw:.2e} / {wmr:.2e} (bar {tol:.1e})")
        assert raw < tol and mr < tol and wraw < tol and wmr < tol, (where, n, raw, mr, wraw, wmr)


def _taps(model, ref, levels, F):
    got = {}
    for lvl in (2, 3):
        if lvl in levels:
            C = DF.CHANNELS[lvl]
            h, w = DF.SIZES[lvl]
            got.update(DF.summarise(f"tap{lvl}", DF.tokens_as_maps(model._taps[lvl].float(), F, C, h * w), DF.N_TAP))
    return got


def _head(name):
    import vdn
    z = _load(name)
    _, S, seq = (int(v) for v in z["meta"])
    levels = [int(v) for v in z["levels"]]
    head = vdn.VideoDepthAnythingHeadV2(sequence_length=seq, attention_feature_levels=levels)
    head.load_state_dict(DF.state_dict(head), strict=True)
    head = head.to(DEV).eval()
    feats = [torch.from_numpy(f).to(DEV) for f in DF.head_inputs(1, S)]
    return z, head, feats, levels, S


@pytest.mark.parametrize("name", ["dn_head_s4", "dn_head_s32", "dn_head_s2_all"])
def test_head_fixture(name):
    z, head, feats, levels, S = _head(name)
    out = head(feats)
    assert out.shape == (1, S, 3, 224, 224)
    _check(DF.summarise_head(out), z, ["out"], name)
    _check(_taps(head, z, levels, S), z, [f"tap{l}" for l in (2, 3) if l in levels], name)


def _wrapper(z):
    import vdn
    from vdn import synth
    B, S, H, W, seq = (int(v) for v in z["meta"])
    res, relu, use_d, use_rgb, ape = (bool(v) for v in z["flags"])
    m = vdn.VideoDepthEstimationModel(seq, attention_feature_levels=[int(v) for v in z["levels"]], use_residual=res,
                                      use_final_relu=relu, use_depth_feature=use_d, use_rgb_feature=use_rgb,
                                      trunk=synth.dn_trunk(), img_trunk=synth.dn_trunk(), pe="ape" if ape else "none")
    m.load_state_dict(DF.state_dict(m), strict=True)
    depth, img = DF.wrapper_inputs(B, S, H, W)
    return m.to(DEV).eval(), torch.from_numpy(depth).to(DEV), torch.from_numpy(img).to(DEV), res


@pytest.mark.parametrize("name", ["dn_model_b2", "dn_model_nope"])
def test_model_fixture(name):
    z = _load(name)
    m, depth, img, res = _wrapper(z)
    d, n = m(depth, img)
    B, S, H, W = depth.shape
    assert d.shape == (B, S, H, W) and n.shape == (B, S, 3, H, W)
    assert torch.all(n[:, :, 2] == 1)
    got = DF.summarise_wrapper(d, n, depth if res else None)
    _check(got, z, ["depth", "dx", "dy"] + (["dres"] if res else []), name)
    _check(_taps(m, z, [int(v) for v in z["levels"]], B * S), z, [f"tap{l}" for l in (2, 3) if f"tap{l}_mean" in z], name)


def test_batch_of_two_clips_matches_each_alone():
    z = _load("dn_model_b2")
    m, depth, img, _ = _wrapper(z)
    d, n = m(depth, img)
    d, n = d.clone(), n.clone()
    for b in range(depth.shape[0]):
        d1, n1 = m(depth[b:b + 1].contiguous(), img[b:b + 1].contiguous())
        assert rel_l2(d1.cpu(), d[b:b + 1].cpu()) < 1e-6 and rel_l2(n1.cpu(), n[b:b + 1].cpu()) < 1e-6


def test_repeat_call_allocates_nothing_and_is_bitwise_equal():
    z = _load("dn_model_b2")
    m, depth, img, _ = _wrapper(z)
    d0, n0 = (t.clone() for t in m(depth, img))
    rt = m._eng["rt"]
    nbufs, nbytes = len(rt._bufs), rt.workspace_bytes()
    torch.cuda.synchronize()
    reserved = torch.cuda.memory_reserved(DEV)
    d1, n1 = m(depth, img)
    torch.cuda.synchronize()
    assert len(rt._bufs) == nbufs and rt.workspace_bytes() == nbytes
    assert torch.cuda.memory_reserved(DEV) == reserved
    assert torch.equal(d0, d1) and torch.equal(n0, n1)
