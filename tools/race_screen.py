#!/usr/bin/env python3
"""Race screen (GPU box): the counted-vmcnt ping-pong GEMM and the pipelined attention, many repetitions at
several sizes, every run compared bit for bit with the first (an ordering mistake shows up as rare differing tiles)."""
import os, sys, math
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
import torch
from vdn.runtime import Runtime, ceil_to
from vdn import pack, _abi

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rt = Runtime(torch.device("cuda:0"), torch.float16, split=True)
torch.manual_seed(0)
bad = 0
for bm in ("256", "192", "128"):
    _abi.set_tuning(force_bm=int(bm))
    for (M, N, K) in ((10960, 4096, 1024), (5480, 1024, 4096), (1370, 3072, 1024), (2050, 512, 96)):
        a = rt.to_half(torch.randn(M, K, device="cuda"))
        w = pack._pad_k(torch.randn(N, K, device="cuda") / math.sqrt(K), rt.prec)
        bias = torch.randn(N, device="cuda")
        out = rt.hbuf(f"rs_{M}_{N}", (M, N))
        rt.gemm(a, w, M, N, K, out=out, bias=bias, act=_abi.ACT_GELU)
        h0, l0 = out.hi.clone(), out.lo.clone()
        diff = 0
        for _ in range(reps):
            rt.gemm(a, w, M, N, K, out=out, bias=bias, act=_abi.ACT_GELU)
            diff += int(not (torch.equal(out.hi, h0) and torch.equal(out.lo, l0)))
        bad += diff
        print(f"gemm BM={bm} M={M} N={N} K={K}: {diff} of {reps} runs differ", flush=True)
_abi.set_tuning(force_bm=0)
# 8-bit cross-term kernel (5-slot ring, counted waits in units, two tile heights): K-tile-major planes, the three hot flavours
from vdn.runtime import HL


def kt16(t, rows, K):
    return t.reshape(rows, K // 32, 32).permute(1, 0, 2).contiguous()


def kt8(t, rows, K):
    return t.reshape(rows, K // 64, 64).permute(1, 0, 2).contiguous()


for bm in (256, 192):
    _abi.set_tuning(force_bm=bm)
    for (M, N, K) in ((10960, 4096, 1024), (5480, 1024, 4096), (10960, 1024, 64), (4100, 3072, 192)):
        a = rt.to_half(torch.randn(M, K, device="cuda"))
        w = pack.linear(torch.randn(N, K, device="cuda") / math.sqrt(K), rt.prec)
        ak, a8k = HL(kt16(a.hi, M, K)), pack.planes8(a, kt=True)
        x8 = pack.X8(w)
        bias = torch.randn(N, device="cuda")
        kt = dict(a8=a8k, w8=x8.p8, a_kt=True, w_kt=True)
        oh, o8 = HL(torch.zeros(M, N, dtype=torch.float16, device="cuda")), torch.zeros(2, M, N, dtype=torch.uint8, device="cuda")
        res0 = torch.randn(M, N, device="cuda")
        res = res0.clone()

        def run():
            rt.gemm(ak, HL(x8.hi), M, N, K, out=oh, out8=o8, out_kt=True, bias=bias, act=_abi.ACT_GELU, **kt)
            res.copy_(res0)
            rt.gemm(ak, HL(x8.hi), M, N, K, out=res, bias=bias, gamma=bias, res1=res, **kt)

        run()
        h0, p0, r0 = oh.hi.clone(), o8.clone(), res.clone()
        diff = 0
        for _ in range(reps // 2):
            run()
            diff += int(not (torch.equal(oh.hi, h0) and torch.equal(o8, p0) and torch.equal(res, r0)))
        bad += diff
        print(f"gemm_x8 BM={bm} M={M} N={N} K={K} (GELU planes + residual): {diff} of {reps // 2} runs differ", flush=True)
    # head-split epilogues of the cross-term kernel: lane-half swap of the 8-bit planes, and the RoPE'd flavour
    side, Bh, Hh, K = 37, 4, 4, 256
    P, C = side * side, Hh * 64
    tp, M = ceil_to(P, 64), Bh * P
    a = rt.to_half(torch.randn(M, K, device="cuda"))
    ws, bs = [torch.randn(C, K, device="cuda") / math.sqrt(K) for _ in range(3)], [torch.randn(C, device="cuda") for _ in range(3)]
    cs = pack.rope_table(side, side, 64, device="cuda")
    a8 = pack.planes8(a)
    for rope in (0, 1):
        wp, bp = pack.cat_proj(ws, bs, [rope, rope, 0], rt.prec)
        w8 = pack.planes8(wp)
        q, k = rt.hbuf(f"rs_q{rope}", (Bh * Hh, tp, 64), zero=True), rt.hbuf(f"rs_k{rope}", (Bh * Hh, tp, 64), zero=True)
        vt = rt.hbuf(f"rs_vt{rope}", (Bh * Hh, 64, tp), zero=True)
        q8, k8 = rt.qk8(f"rs_q8{rope}", Bh * Hh, tp), rt.qk8(f"rs_k8{rope}", Bh * Hh, tp)
        hd = dict(dst=[q, k, vt], dst8=[q8, k8, None], transposed=[0, 0, 1], heads=Hh, tokens=P, tpad=tp)
        if rope:
            hd.update(rope=[1, 1, 0], rope_cs=cs, rope_mod=P)

        def run_h():
            rt.gemm(a, wp, M, 3 * C, K, bias=bp, store=_abi.ST_HEADS, heads=hd, a8=a8, w8=w8)

        run_h()
        ref = [t.clone() for t in (q.hi, k.hi, vt.hi, q8, k8)]
        diff = 0
        for _ in range(reps // 2):
            run_h()
            diff += int(not all(torch.equal(x, y) for x, y in zip((q.hi, k.hi, vt.hi, q8, k8), ref)))
        bad += diff
        print(f"gemm_x8 BM={bm} head split{' + RoPE' if rope else ''} M={M} N={3 * C} K={K}: {diff} of {reps // 2} runs differ", flush=True)
_abi.set_tuning(force_bm=0)
for (B, H, nq, nk) in ((8, 16, 1370, 1370), (4, 16, 1369, 8214), (2, 6, 150, 200), (1, 16, 361, 1369)):
    qp, kp = ceil_to(nq, 64), ceil_to(nk, 64)
    q = rt.to_half(torch.randn(B * H, qp, 64, device="cuda"))
    k = rt.to_half(torch.randn(B * H, kp, 64, device="cuda"))
    v = rt.to_half(torch.randn(B * H, 64, kp, device="cuda"))
    o = rt.hbuf(f"rs_o{nq}_{nk}", (B * nq, H * 64))

    def planes8(t):  # the 8-bit planes the projection epilogue would have written (score cross terms on the e5m2 MFMA)
        return torch.cat([t.float().to(torch.float8_e5m2).view(torch.uint8),
                          (t.lo.float() * 1024.0).to(torch.float8_e5m2).view(torch.uint8)], dim=-1).contiguous()

    for tag, kw in (("3-product scores", {}), ("8-bit cross terms", dict(q8=planes8(q), k8=planes8(k)))):
        rt.flash_attn(q, k, v, o, B, H, nq, qp, nk, kp, 0.125, **kw)
        h0, l0 = o.hi.clone(), o.lo.clone()
        diff = 0
        for _ in range(reps):
            rt.flash_attn(q, k, v, o, B, H, nq, qp, nk, kp, 0.125, **kw)
            diff += int(not (torch.equal(o.hi, h0) and torch.equal(o.lo, l0)))
        bad += diff
        print(f"attn ({tag}) B={B} H={H} nq={nq} nk={nk}: {diff} of {reps} runs differ", flush=True)
# fused depth tail (LDS-DMA source patch + register-resident weights) and the persistent LayerNorm
x = torch.randn(8 * 296 * 296, 128, device="cuda")
w = pack.conv3x3_taps(torch.randn(32, 128, 3, 3, device="cuda") / math.sqrt(9 * 128), rt.prec)
b2, w1 = torch.randn(32, device="cuda") * 0.1, torch.randn(32, device="cuda") * 0.3
d = torch.empty(8, 518, 518, device="cuda")
rt.depth_tail(x, w, b2, w1, 0.2, d, 8, 296, 296, 128, 518, 518, True)
d0 = d.clone()
diff = 0
for _ in range(reps // 4):
    rt.depth_tail(x, w, b2, w1, 0.2, d, 8, 296, 296, 128, 518, 518, True)
    diff += int(not torch.equal(d, d0))
bad += diff
print(f"depth_tail B=8 296->518: {diff} of {reps // 4} runs differ", flush=True)
# output_conv1's combine pass (LDS-staged source patch, plain stores, no atomics)
z = torch.randn(4 * 148 * 148, 9 * 128, device="cuda")
b1 = torch.randn(128, device="cuda")
o = torch.empty(4 * 296 * 296, 128, device="cuda")
rt.oc1_combine(z, b1, o, 4, 148, 148, 296, 296, 128)
o0 = o.clone()
diff = 0
for _ in range(reps // 4):
    rt.oc1_combine(z, b1, o, 4, 148, 148, 296, 296, 128)
    diff += int(not torch.equal(o, o0))
bad += diff
print(f"oc1_combine B=4 148->296: {diff} of {reps // 4} runs differ", flush=True)
del z, o, o0
# sub-pixel convolution (ConvTranspose + layer_rn as one implicit GEMM; ragged K per phase on the ping-pong / lock-step loops)
for Ci, k in ((256, 4), (512, 2)):
    wsp = pack.subpixel_conv(torch.randn(Ci, Ci, k, k, device="cuda") / math.sqrt(Ci), torch.randn(Ci, device="cuda"),
                             torch.randn(256, Ci, 3, 3, device="cuda") / math.sqrt(9 * Ci), rt.prec)
    pm = rt.to_half(torch.randn(8 * 37 * 37, Ci, device="cuda"))
    o = rt.hbuf(f"rs_sp{k}", (8 * 37 * 37 * k * k, 256))
    args = dict(store=_abi.ST_CONVT, out=o, conv=dict(B=8, H=37, W=37, C=Ci, OH=37, OW=37, stride=1, korder=1),
                convt=dict(k=k, cout=256, B=8, H=37, W=37), subpix_bias=wsp[1])
    rt.gemm(pm, wsp[0], 8 * 37 * 37, k * k * 256, 4 * Ci, **args)
    h0, l0 = o.hi.clone(), o.lo.clone()
    diff = 0
    for _ in range(reps // 4):
        rt.gemm(pm, wsp[0], 8 * 37 * 37, k * k * 256, 4 * Ci, **args)
        diff += int(not (torch.equal(o.hi, h0) and torch.equal(o.lo, l0)))
    bad += diff
    print(f"subpixel conv k={k} Ci={Ci} B=8 37x37: {diff} of {reps // 4} runs differ", flush=True)
    del wsp, pm, o, h0, l0
# Hiera trunk kernels (csrc/hiera.hip): the LDS-staged key / value tiles of the attention (a pooled-query windowed shape and
# the 196-key global one, which takes four tiles), then the gather, pool and reroll passes
for (F, heads, W, Lkv, qs) in ((8, 2, 49, 64, 4), (8, 4, 1, 196, 1), (8, 8, 1, 196, 4)):
    C = heads * 96
    qkv = rt.to_half(torch.randn(F * W * Lkv, 3 * C, device="cuda"))
    o = rt.hbuf(f"rs_hi{heads}_{qs}", (F * W * Lkv // qs, C))
    rt.hiera_attn(qkv, o, F, heads, W, Lkv, qs, 96 ** -0.5)
    h0, l0 = o.hi.clone(), o.lo.clone()
    diff = 0
    for _ in range(reps):
        rt.hiera_attn(qkv, o, F, heads, W, Lkv, qs, 96 ** -0.5)
        diff += int(not (torch.equal(o.hi, h0) and torch.equal(o.lo, l0)))
    bad += diff
    print(f"hiera_attn F={F} heads={heads} W={W} Lkv={Lkv} q_stride={qs}: {diff} of {reps} runs differ", flush=True)
img = torch.randn(8, 3, 224, 224, device="cuda")
hr = rt.hbuf("rs_hi_rows", (8 * 3136, 192))
px, py = torch.randn(8 * 3136, 192, device="cuda"), torch.empty(8 * 784, 192, device="cuda")
pm = torch.empty(8, 28, 28, 192, device="cuda")


def run_hiera():
    rt.hiera_embed(img, hr, 8, 192)
    rt.hiera_pool(px, py, 8, 784, 192)
    rt.hiera_reroll(py, pm, 8, 1, 192)


run_hiera()
ref = [t.clone() for t in (hr.hi, hr.lo, py, pm)]
diff = 0
for _ in range(reps // 4):
    run_hiera()
    diff += int(not all(torch.equal(x, y) for x, y in zip((hr.hi, hr.lo, py, pm), ref)))
bad += diff
print(f"hiera embed + pool + reroll F=8: {diff} of {reps // 4} runs differ", flush=True)
del img, hr, px, py, pm, ref
t = torch.randn(10960, 1024, device="cuda")
g, be = torch.randn(1024, device="cuda"), torch.randn(1024, device="cuda")
oh = rt.hbuf("rs_ln", (10960, 1024))
rt.layernorm(t, 10960, 1024, g, be, 1e-6, out_h=oh)
h0, l0 = oh.hi.clone(), oh.lo.clone()
diff = 0
for _ in range(reps):
    rt.layernorm(t, 10960, 1024, g, be, 1e-6, out_h=oh)
    diff += int(not (torch.equal(oh.hi, h0) and torch.equal(oh.lo, l0)))
bad += diff
print(f"layernorm 10960 x 1024: {diff} of {reps} runs differ", flush=True)
print("RACE SCREEN", "CLEAN" if bad == 0 else f"FAILED ({bad})")
sys.exit(1 if bad else 0)
