#!/usr/bin/env python3
"""The cross-term kernel on plain-A problems of the RCU convolution shapes (M = 8 (H+2)^2, N = 256, K = 2304) against the
three-product kernels (plain GEMM of the same shape, and the 3x3 implicit-GEMM launches of an RCU), interleaved rounds in one
process (GPU box): the measurement behind profiles/rcu_x8.md step 0."""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
import torch
from vdn.runtime import Runtime, HL
from vdn import pack, _abi

rt = Runtime(torch.device("cuda:0"), torch.float16, split=True)
torch.manual_seed(0)
N, C = 256, 256
K = 9 * C


def kt16(t, rows, K):
    return t.reshape(rows, K // 32, 32).permute(1, 0, 2).contiguous()


for label, B, H in (("148^2", 8, 148), ("74^2", 8, 74)):
    Mp, Mu = B * (H + 2) * (H + 2), B * H * H
    a = rt.to_half(torch.randn(Mp, K, device="cuda"))
    w = pack.linear(torch.randn(N, K, device="cuda") / math.sqrt(K), rt.prec)
    ak, a8k = HL(kt16(a.hi, Mp, K)), pack.planes8(a, kt=True)
    x8 = pack.X8(w, pack.ORDER_GEMM)
    bias = torch.randn(N, device="cuda")
    # conv operands
    xc = rt.to_half(torch.randn(Mu, C, device="cuda"))
    wc = pack.conv3x3(torch.randn(N, C, 3, 3, device="cuda") / math.sqrt(K), rt.prec)
    conv = dict(B=B, H=H, W=H, C=C, OH=H, OW=H, stride=1)
    res = rt.to_half(torch.randn(Mu, N, device="cuda"))
    resp = rt.to_half(torch.randn(Mp, N, device="cuda"))
    o3 = rt.hbuf("o3" + label, (Mp, N))
    oc = rt.hbuf("oc" + label, (Mu, N))
    o8 = HL(rt.buf("o8" + label, (Mp, N), torch.float16))
    o88 = rt.buf("o88" + label, (2, Mp, N), torch.uint8)
    o8h = rt.hbuf("o8h" + label, (Mp, N))
    runs = {
        "x3 plain  bias+relu -> hi/lo": lambda: rt.gemm(a, w, Mp, N, K, out=o3, bias=bias, act=_abi.ACT_RELU),
        "x3 conv1  relu_a bias relu": lambda: rt.gemm(xc, wc, Mu, N, K, out=oc, bias=bias, act=_abi.ACT_RELU, relu_a=True, conv=conv),
        "x3 conv2  bias res1 res2": lambda: rt.gemm(xc, wc, Mu, N, K, out=oc, bias=bias, res1=res, res2=res, conv=conv),
        "x8 plain  bias+gelu -> kt planes+x6": lambda: rt.gemm(ak, HL(x8.hi), Mp, N, K, a8=a8k, w8=x8.p8, a_kt=True, w_kt=True,
                                                              out=o8, out8=o88, out_kt=True, bias=bias, act=_abi.ACT_GELU),
        "x8 plain  bias res1 -> hi/lo": lambda: rt.gemm(ak, HL(x8.hi), Mp, N, K, a8=a8k, w8=x8.p8, a_kt=True, w_kt=True,
                                                        out=o8h, bias=bias, res1=resp),
    }
    for bm in (0, 192, 256):
        key = "x8 plain  bias+gelu -> kt planes+x6"
        if bm:
            def f(bm=bm, g=runs[key]):
                old = _abi.set_tuning(force_bm=bm)
                try:
                    g()
                finally:
                    _abi.restore_tuning(old)
            runs[f"x8 same, BM={bm}"] = f
    times = {}
    for rnd in range(9):
        for name, fn in runs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record(); torch.cuda.synchronize()
            if rnd >= 2:
                times.setdefault(name, []).append(s.elapsed_time(e))
    for name in runs:
        ts = sorted(times[name]); med = ts[len(ts) // 2]
        M = Mu if "conv" in name else Mp
        line = f"{label:6s} {name:40s} M={M:7d} | {med*1e3:7.1f} us (min {ts[0]*1e3:6.1f}) {2.0*M*N*K/med/1e9:6.1f} TF/s alg"
        print(line, flush=True)
    del a, w, ak, a8k, xc, res, resp
