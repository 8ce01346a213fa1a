#!/usr/bin/env python3
"""Time the DPT tail alone at the ViT-L size (GPU box): vdn_depth_tail, and in front of it output_conv1 both ways — the
three launches of the materialised path (refinenet1.out_conv at 148 x 148, the 148 -> 296 resize, the 3x3 conv on the 296 x 296
map) and the two that replace them (one GEMM for all nine taps at 148 x 148, vdn_oc1_combine). B = frames (argv[1], default 8;
a bench lane is 4). VDN_LIB selects a variant library."""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
import torch
from vdn.runtime import Runtime
from vdn import pack
rt = Runtime(torch.device("cuda:0"), torch.float16, split=True)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
IH, C, OH, F, LH = 296, 128, 518, 256, 148


def timed(fn, reps=12):
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record()
        torch.cuda.synchronize(); ts.append(s.elapsed_time(e))
    ts = sorted(ts[2:])
    return ts[len(ts) // 2] * 1e3   # us


x = torch.randn(B * IH * IH, C, device="cuda")
w = pack.conv3x3_taps(torch.randn(32, C, 3, 3, device="cuda") / math.sqrt(9 * C), rt.prec)
b2, w1 = torch.randn(32, device="cuda") * 0.1, torch.randn(32, device="cuda") * 0.3
d = torch.empty(B, OH, OH, device="cuda")
us = timed(lambda: rt.depth_tail(x, w, b2, w1, 0.2, d, B, IH, IH, C, OH, OH, True))
fl = 2.0 * B * OH * OH * 32 * 9 * C
print(f"depth_tail B={B} {IH}->{OH} C={C}: median {us:.1f} us  ({fl/us/1e6:.1f} TF/s algorithmic)  lib={os.environ.get('VDN_LIB','default')}")

# output_conv1, materialised: out_conv (1x1) at 148 x 148 -> resize to 296 x 296 (hi + lo planes) -> conv3x3 F -> F/2, fp32 out
M1, M0 = B * LH * LH, B * IH * IH
W1, b1 = torch.randn(C, F, 3, 3, device="cuda") / math.sqrt(9 * F), torch.randn(C, device="cuda") * 0.1
Wo, bo = torch.randn(F, F, 1, 1, device="cuda") / math.sqrt(F), torch.randn(F, device="cuda") * 0.1
u = rt.to_half(torch.randn(M1, F, device="cuda"))
wo_p, w1_p = pack.conv1x1(Wo, rt.prec), pack.conv3x3(W1, rt.prec)
v, p1, o1 = rt.hbuf("tb_v", (M1, F)), rt.hbuf("tb_path1", (M0, F)), rt.fbuf("tb_out1", (M0, C))
conv = dict(B=B, H=IH, W=IH, C=F, OH=IH, OW=IH, stride=1)
t_oc = timed(lambda: rt.gemm(u, wo_p, M1, F, F, bias=bo, out=v))
t_up = timed(lambda: rt.upsample(v, p1, B, LH, LH, IH, IH, F))
t_c3 = timed(lambda: rt.gemm(p1, w1_p, M0, C, 9 * F, out=o1, bias=b1, conv=conv))
print(f"materialised B={B}: out_conv {t_oc:.1f} us + resize {t_up:.1f} us + output_conv1 {t_c3:.1f} us = {t_oc + t_up + t_c3:.1f} us")

# output_conv1 at the low resolution: one GEMM N = 9 F/2, fp32 out, then the combine
wc, bc = pack.lowres_oc1(W1, Wo, bo, rt.prec)
z, o1b = rt.fbuf("tb_z", (M1, 9 * C)), rt.fbuf("tb_out1b", (M0, C))
t_g = timed(lambda: rt.gemm(u, wc, M1, 9 * C, F, bias=bc, out=z))
t_cb = timed(lambda: rt.oc1_combine(z, b1, o1b, B, LH, LH, IH, IH, C))
gb_g, gb_c = (z.numel() * 4 + M1 * F * 4) / 1e9, (z.numel() * 4 + o1b.numel() * 4) / 1e9
print(f"low resolution B={B}: gemm N={9 * C} {t_g:.1f} us ({2.0 * M1 * 9 * C * F / t_g / 1e6:.0f} TF/s algorithmic, {gb_g / t_g * 1e3:.2f} TB/s of "
      f"{gb_g:.2f} GB) + combine {t_cb:.1f} us ({gb_c / t_cb * 1e3:.2f} TB/s of {gb_c:.2f} GB) = {t_g + t_cb:.1f} us")
print(f"out1 low resolution vs materialised: rel-L2 {float((o1b - o1).double().norm() / o1.double().norm()):.2e}")
