#!/usr/bin/env python3
"""Dump the raw bytes of every output plane the GEMM epilogues (csrc/gemm_kernels.hpp, csrc/gemm_x8.hip) and the element-wise
producers of the same planes (vdn_layernorm, vdn_groupnorm, vdn_addtab_cast, vdn_upsample_bilinear, vdn_patchify, vdn_pack_x8,
vdn_pack_x8_f32, vdn_depth_tail) write, for a byte-for-byte comparison of two builds of the library
(profiles/gemm_epilogue_refactor.md is such a comparison):

    python tools/gemm_dump.py DIR                          # this tree's library
    VDN_LIB=<other tree>/lib/libvdn_hip.so python tools/gemm_dump.py DIR2      # then cmp every file of the two DIRs

Seeded CPU generators make the inputs; every case is one call through a fresh Runtime; outputs are pre-filled so that an
element a kernel does not write is the same in both dumps; each output plane is written as DIR/<case>.<name>.bin.
Families: the 4-wave tile kernels (single planes) and gemm_x3_kernel (split planes) at (77, 32, 64) and (300, 192, 200), fp16 and
bf16; the 8-wave kernels forced by force_bm = 128 / 192 / 256 and p8 = 1 / 2 at (513, 200, 96) and (724, 1152, 384); split-K
with its four reduce flavours at (361, 256, 2048); the 8-bit cross-term kernel at both M tiles at (4099, 448, 64) and
(2817, 3072, 384). Flavours: plain rows to f32, hi-only and split planes with row_group; [bias] [ReLU] split planes; one / two
split residuals; the f32 LayerScale residual; bias + GELU planes (with out8 / out_kt on the 8-bit kernel); GEGLU with GELU and
SiLU; the head split without / with RoPE, V^T, without / with dst8 and dst_lo; ConvTranspose scatter; the sub-pixel
convolution. A case a build rejects prints SKIP and the reason. Not a test: it asserts nothing."""
import hashlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))

import torch  # noqa: E402


def main():
    out_dir = sys.argv[1]
    os.makedirs(out_dir, exist_ok=True)
    from vdn import _abi, pack
    from vdn.runtime import HL, Runtime, ceil_to
    dev = torch.device("cuda:0")
    seed = [9000]
    count = [0]

    def randn(*shape, scale=1.0):
        seed[0] += 1
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed[0])) * scale

    def dump(case, **tensors):
        torch.cuda.synchronize()
        for name, t in sorted(tensors.items()):
            if t is None:
                continue
            raw = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
            with open(os.path.join(out_dir, f"{case}.{name}.bin"), "wb") as f:
                f.write(raw)
            count[0] += 1
            print(f"{case}.{name}.bin {len(raw)} {hashlib.sha256(raw).hexdigest()[:16]}", flush=True)

    def full(shape, dt, fill=-7.0):
        return torch.full(shape, fill, dtype=dt, device=dev)

    def planes(shape, dt, lo=True):
        return HL(full(shape, dt), full(shape, dt) if lo else None)

    def case(name, fn):
        try:
            fn()
        except (_abi.VdnError, AssertionError, TypeError, ValueError, AttributeError, KeyError) as e:   # a shape / flavour a family does not take
            print(f"SKIP {name}: {e}", flush=True)

    def kt16(t, rows, K):
        return t.reshape(rows, K // 32, 32).permute(1, 0, 2).contiguous()

    def gemm_flavours(tag, dt, split, M, N, K, tuning, x8=False):
        """Every epilogue flavour the shape admits, one fresh Runtime per call."""
        a, w = randn(M, K), randn(N, K, scale=1 / math.sqrt(K))
        b, g = randn(N).to(dev), randn(N).to(dev)
        r1, r2 = randn(M, N), randn(M, N)

        def run(name, make_out, **kw):
            def go():
                _abi.restore_tuning(None)
                if tuning:
                    _abi.set_tuning(**tuning)
                rt = Runtime(dev, dt, split=split)
                A, W = rt.to_half(a.to(dev)), pack.linear(w.to(dev), rt.prec)
                args = dict(kw)
                if x8:
                    X = pack.X8(W)
                    A, W = HL(kt16(A.hi, M, K)), HL(X.hi)
                    args.update(a8=pack.planes8(rt.to_half(a.to(dev)), kt=True), w8=X.p8, a_kt=True, w_kt=True)
                for k_ in ("res1", "res2"):
                    if isinstance(args.get(k_), torch.Tensor) and args[k_].dtype == torch.float32 and args[k_].device.type == "cpu":
                        args[k_] = rt.to_half(args[k_].to(dev)) if split else args[k_].to(dt).to(dev)
                outs = make_out(rt, args)
                rt.gemm(A, W, M, N, K, **args)
                flat = {}
                for nm, t in outs.items():
                    if isinstance(t, HL):
                        flat[nm], flat[nm + "_lo"] = t.hi, t.lo
                    else:
                        flat[nm] = t
                dump(f"{tag}_{M}x{N}x{K}_{name}", **flat)
                _abi.restore_tuning(None)
            case(f"{tag}_{M}x{N}x{K}_{name}", go)

        def out_as(kind, rows=M, cols=N):
            def mk(rt, args):
                o = full((rows, cols), torch.float32) if kind == "f32" else planes((rows, cols), dt, lo=kind == "split")
                args["out"] = o if kind != "hi" else o.hi
                return dict(out=o if kind != "hi" else o.hi)
            return mk

        run("plain_f32_gelu", out_as("f32"), bias=b, act=_abi.ACT_GELU)
        run("plain_hi", out_as("hi"), bias=b)
        P = 7 if M % 7 == 0 else 10 if M % 10 == 0 else 0
        if P:
            run("plain_split_rowgroup", out_as("split", rows=(M // P) * (P + 1)), bias=b, act=_abi.ACT_GELU, row_group=P, row_skip=1)
        if split or x8:
            run("half", out_as("split"), bias=b)
            run("half_relu", out_as("split"), bias=b, act=_abi.ACT_RELU)
            run("reshalf1", out_as("split"), bias=b, res1=r1)
            run("reshalf2", out_as("split"), bias=b, res1=r1, res2=r2)
            run("fc1", out_as("split"), bias=b, act=_abi.ACT_GELU)

        def res_inplace(rt, args):
            o = r1.clone().to(dev)
            args.update(out=o, res1=o)
            return dict(out=o)
        run("res", res_inplace, bias=b, gamma=g)
        if x8 and N % 64 == 0:
            def fc1_kt(rt, args):
                o, o8 = HL(full((M, N), dt)), torch.full((2, M, N), 0xA5, dtype=torch.uint8, device=dev)
                args.update(out=o, out8=o8, out_kt=True)
                return dict(out=o.hi, out8=o8)
            run("fc1_out8_kt", fc1_kt, bias=b, act=_abi.ACT_GELU)
        if N % 32 == 0:
            wg, bg = randn(N, K, scale=1 / math.sqrt(K)), randn(N)
            for nm, act, kind in (("geglu_gelu_split", _abi.ACT_NONE, "split" if (split or x8) else "hi"), ("geglu_silu_f32", _abi.ACT_SILU, "f32")):
                def go(nm=nm, act=act, kind=kind):
                    _abi.restore_tuning(None)
                    if tuning:
                        _abi.set_tuning(**tuning)
                    rt = Runtime(dev, dt, split=split)
                    wp, bp = pack.geglu(wg.to(dev), bg.to(dev), rt.prec)
                    A, args = rt.to_half(a.to(dev)), {}
                    if x8:
                        X = pack.X8(wp)
                        args.update(a8=pack.planes8(A, kt=True), w8=X.p8, a_kt=True, w_kt=True)
                        A, wp = HL(kt16(A.hi, M, K)), HL(X.hi)
                    o = full((M, N // 2), torch.float32) if kind == "f32" else planes((M, N // 2), dt, lo=kind == "split")
                    rt.gemm(A, wp, M, N, K, bias=bp, act=act, store=_abi.ST_GEGLU, out=o if kind != "hi" else o.hi, **args)
                    dump(f"{tag}_{M}x{N}x{K}_{nm}", **(dict(out=o) if kind == "f32" else dict(out=o.hi, out_lo=o.lo)))
                    _abi.restore_tuning(None)
                case(f"{tag}_{M}x{N}x{K}_{nm}", go)
        if N % 192 == 0:   # fused Q / K / V projection: heads = N / 192
            Hh = N // 192
            B = 3 if M % 3 == 0 else 2
            T = M // B
            if B * T == M:
                tp, side = ceil_to(T, 64), 8
                for nm, rope, with8, with_lo in (("heads", 0, False, True), ("heads_dst8", 0, True, False), ("heads_dst8_lo", 0, True, True),
                                                 ("heads_rope", 1, False, True), ("heads_rope_dst8", 1, True, False), ("heads_rope_dst8_lo", 1, True, True)):
                    if with8 and not (split and dt == torch.float16):
                        continue

                    def mk(rt, args, rope=rope, with8=with8, with_lo=with_lo):
                        lo = with_lo and (split or x8)
                        q, k = planes((B * Hh, tp, 64), dt, lo), planes((B * Hh, tp, 64), dt, lo)
                        vt = planes((B * Hh, 64, tp), dt, lo)
                        q8 = torch.full((B * Hh, tp, 128), 0xA5, dtype=torch.uint8, device=dev) if with8 else None
                        k8 = torch.full((B * Hh, tp, 128), 0xA5, dtype=torch.uint8, device=dev) if with8 else None
                        args.update(store=_abi.ST_HEADS, heads=dict(
                            dst=[q, k, vt], dst8=[q8, k8, None], transposed=[0, 0, 1], rope=[rope, rope, 0],
                            rope_cs=pack.rope_table(side, side, 64, device=dev) if rope else None, rope_mod=side * side, heads=Hh,
                            tokens=T, tok_off=0, tpad=tp))
                        return dict(q=q, k=k, vt=vt, q8=q8, k8=k8)
                    run(nm, mk, bias=b)

    # ---- 4-wave tile kernels (single planes) and gemm_x3_kernel (split planes)
    for dt, dn in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
        for split in (False, True):
            for M, N, K in ((77, 32, 64), (300, 192, 200)):
                gemm_flavours(f"w4_{dn}_{'x3' if split else 'x1'}", dt, split, M, N, K, None)

        def convt(dt=dt, dn=dn):
            k, Ci, Co, B, H, W = 2, 96, 96, 2, 5, 7
            rt = Runtime(dev, dt, split=False)
            x, w, b = randn(B * H * W, Ci), randn(Ci, Co, k, k, scale=1 / math.sqrt(Ci)), randn(Co)
            wp, bp = pack.conv_transpose(w.to(dev), b.to(dev), rt.prec)
            out = full((B, H * k, W * k, Co), dt)
            rt.gemm(x.to(dt).to(dev), wp, B * H * W, k * k * Co, Ci, out=out, bias=bp, store=_abi.ST_CONVT, convt=dict(k=k, cout=Co, B=B, H=H, W=W))
            dump(f"w4_{dn}_convt", out=out)
        case(f"w4_{dn}_convt", convt)
    # ---- 8-wave kernels, every tile height and both ping-pong variants; split-K; sub-pixel convolution
    for dt, dn in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
        for tuning, tn in (({"force_bm": 128}, "bm128"), ({"force_bm": 192}, "bm192"), ({"force_bm": 256}, "bm256"),
                           ({"force_bm": 256, "p8": 1}, "p8_1"), ({"force_bm": 192, "p8": 2}, "p8_2")):
            for M, N, K in ((513, 200, 96), (724, 1152, 384)):
                gemm_flavours(f"w8_{dn}_{tn}", dt, True, M, N, K, tuning)

            def subpix(dt=dt, dn=dn, tuning=tuning, tn=tn):
                Ci, k, F, B, h, w = 512, 2, 256, 1, 5, 7
                _abi.restore_tuning(None)
                _abi.set_tuning(**tuning)
                rt = Runtime(dev, dt, split=True)
                wt, bt, wr = randn(Ci, Ci, k, k, scale=Ci ** -0.5).to(dev), randn(Ci).to(dev), randn(F, Ci, 3, 3, scale=(9 * Ci) ** -0.5).to(dev)
                p = rt.to_half(randn(B * h * w, Ci).to(dev))
                packed = pack.subpixel_conv(wt, bt, wr, rt.prec)
                out = planes((B * k * h * k * w, F), dt)
                rt.gemm(p, packed[0], B * h * w, k * k * F, 4 * Ci, store=_abi.ST_CONVT, out=out,
                        conv=dict(B=B, H=h, W=w, C=Ci, OH=h, OW=w, stride=1, korder=1), convt=dict(k=k, cout=F, B=B, H=h, W=w), subpix_bias=packed[1])
                dump(f"w8_{dn}_{tn}_subpix", out=out.hi, out_lo=out.lo)
                _abi.restore_tuning(None)
            case(f"w8_{dn}_{tn}_subpix", subpix)
        gemm_flavours(f"splitk_{dn}", dt, True, 361, 256, 2048, None)
    # ---- the 8-bit cross-term kernel at both M tiles
    for bm in (192, 256):
        for M, N, K in ((4099, 448, 64), (2817, 3072, 384)):
            gemm_flavours(f"x8_bm{bm}", torch.float16, True, M, N, K, {"force_bm": bm}, x8=True)
    _abi.restore_tuning(None)

    # ---- element-wise producers
    for xdt, xn in ((torch.float32, "f32"), (torch.float16, "f16"), (torch.bfloat16, "bf16")):
        for C in (64, 384, 1024):
            rows, grp = 30, 10
            x, w, b = randn(rows, C).to(xdt).to(dev), randn(C).to(dev), randn(C).to(dev)
            for dt, dn in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
                def ln(dt=dt, dn=dn):
                    rt = Runtime(dev, dt, split=True)
                    o, of = planes((rows, C), dt), full((rows, C), torch.float32)
                    rt.layernorm(x, rows, C, w, b, 1e-6, out_h=o, out_f=of)
                    oh = full((rows, C), dt)
                    rt.layernorm(x, rows, C, w, b, 1e-6, out_h=oh)
                    og = planes((rows - rows // grp, C), dt)
                    rt.layernorm(x, rows, C, w, b, 1e-6, out_h=og, out_group=grp)
                    dump(f"ln_{xn}_{dn}_{C}", out=o.hi, out_lo=o.lo, out_f=of, hi_only=oh, group=og.hi, group_lo=og.lo)
                    if dt == torch.float16:
                        for kt in (False, True):
                            ok, o8 = planes((rows, C), dt), torch.full((2, rows, C), 0xA5, dtype=torch.uint8, device=dev)
                            rt.layernorm(x, rows, C, w, b, 1e-6, out_h=ok, out8=o8, kt=kt)
                            dump(f"ln_{xn}_{dn}_{C}_out8_kt{int(kt)}", out=ok.hi, out_lo=ok.lo, out8=o8)
                case(f"ln_{xn}_{dn}_{C}", ln)
    for dt, dn in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
        def elementwise(dt=dt, dn=dn):
            rt = Runtime(dev, dt, split=True)
            F_, HW, C = 3, 50, 64
            x = rt.to_half(randn(F_ * HW, C).to(dev))
            y = planes((F_ * HW, C), dt)
            rt.groupnorm(x, y, F_, HW, C, 32, randn(C).to(dev), randn(C).to(dev), 1e-5)
            dump(f"groupnorm_{dn}", out=y.hi, out_lo=y.lo)
            xa, tab = randn(20, 64).to(dev), randn(4, 64).to(dev)
            ya = planes((20, 64), dt)
            rt.addtab_cast(xa, tab, 5, 4, ya, 20, 64)
            dump(f"addtab_cast_{dn}", out=ya.hi, out_lo=ya.lo)
            xu = rt.to_half(randn(1 * 10 * 10, 64).to(dev))
            yu = planes((1, 23, 17, 64), dt)
            rt.upsample(xu, yu, 1, 10, 10, 23, 17, 64)
            dump(f"upsample_{dn}", out=yu.hi, out_lo=yu.lo)
            img, rows = randn(1, 3, 28, 28).to(dev), planes((4, 640), dt)
            rt.patchify(img, rows, 1, 28, 28, 640)
            dump(f"patchify_{dn}", out=rows.hi, out_lo=rows.lo)
        case(f"elementwise_{dn}", elementwise)

    def x8_packs():
        rt = Runtime(dev, torch.float16, split=True)
        rows, C = 77, 384
        t = rt.to_half((randn(rows, C) * 3.0).to(dev))
        for order in (0, 1, 2):
            hi_kt, p8 = full((rows, C), torch.float16), torch.full((2, rows, C), 0xA5, dtype=torch.uint8, device=dev)
            rt.pack_x8(t, hi_kt, p8, order)
            dump(f"pack_x8_order{order}", hi_kt=hi_kt, p8=p8, rowmajor=pack.planes8(t, order, kt=False))
        hi_kt, p8 = full((rows, C), torch.float16), torch.full((2, rows, C), 0xA5, dtype=torch.uint8, device=dev)
        rt.pack_x8_f32((randn(rows, C) * 3.0).to(dev), hi_kt, p8)
        dump("pack_x8_f32", hi_kt=hi_kt, p8=p8)
        B, IH, IW, C, OH, OW = 1, 40, 24, 64, 70, 42
        x = randn(B * IH * IW, C).to(dev).contiguous()
        wt = pack.conv3x3_taps(randn(32, C, 3, 3, scale=1 / math.sqrt(9 * C)).to(dev), rt.prec)
        b2, w1 = randn(32, scale=0.1).to(dev), randn(32, scale=0.3).to(dev)
        for relu in (False, True):
            d = full((B, OH, OW), torch.float32)
            rt.depth_tail(x, wt, b2, w1, 0.2, d, B, IH, IW, C, OH, OW, relu=relu)
            dump(f"depth_tail_relu{int(relu)}", out=d)
    case("x8_packs", x8_packs)
    print(f"files {count[0]}", flush=True)


if __name__ == "__main__":
    main()
