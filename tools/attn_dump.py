#!/usr/bin/env python3
"""Dump the raw bytes of every output plane of every kernel vdn_flash_attn can reach (flash_attn_kernel in its six
instantiations, flash_attn2_kernel in its two, csrc/attn.hip), for a byte-for-byte comparison of two builds of the library
(profiles/attn_refactor.md is such a comparison):

    python tools/attn_dump.py DIR                          # this tree's library
    VDN_LIB=<other tree>/lib/libvdn_hip.so python tools/attn_dump.py DIR2      # then cmp every file of the two DIRs

Seeded CPU generators make the inputs; every case is one call through a fresh Runtime; each output plane is written as
DIR/<case>.<name>.bin. All at B = 1, H = 2; (nq, nk) = (37, 64) one tile, (130, 130) three tiles with a ragged last one and two
query blocks, (129, 321) six tiles (the first, even, odd and last iteration), (40, 449) one key more than a whole number of
tiles, and (129, 321) again with Q scaled by 6 so that the running maximum moves and O is rescaled. K pad rows are NaN, as in
the tests; outputs are pre-filled so that an element a kernel does not write is the same in both dumps. Not a test: it asserts
nothing."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))

import torch  # noqa: E402

SHAPES = ((37, 64, 1.0), (130, 130, 1.0), (129, 321, 1.0), (40, 449, 1.0), (129, 321, 6.0))
# (name, dtype, split, pv, 8-bit Q / K planes, out8, out_kt)
KERNELS = (("f16_single", torch.float16, False, 1, False, False, False),
           ("bf16_single", torch.bfloat16, False, 1, False, False, False),
           ("f16_split_pv3", torch.float16, True, 3, False, False, False),
           ("f16_split_pv2", torch.float16, True, 2, False, False, False),
           ("bf16_split_pv3", torch.bfloat16, True, 3, False, False, False),
           ("bf16_split_pv2", torch.bfloat16, True, 2, False, False, False),
           ("f16_qk8_pv2", torch.float16, True, 2, True, False, False),
           ("f16_qk8_pv1", torch.float16, True, 1, True, False, False),
           ("f16_qk8_pv1_out8", torch.float16, True, 1, True, True, False),
           ("f16_qk8_pv1_out8_kt", torch.float16, True, 1, True, True, True))


def main():
    out_dir = sys.argv[1]
    os.makedirs(out_dir, exist_ok=True)
    from vdn.runtime import HL, Runtime, ceil_to
    dev = torch.device("cuda:0")
    H, dh, scale = 2, 64, 0.125
    nan = float("nan")
    seed = [7000]

    def randn(*shape):
        seed[0] += 1
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed[0]))

    def dump(case, **tensors):
        torch.cuda.synchronize()
        for name, t in sorted(tensors.items()):
            raw = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
            with open(os.path.join(out_dir, f"{case}.{name}.bin"), "wb") as f:
                f.write(raw)
            print(f"{case}.{name}.bin {len(raw)} {hashlib.sha256(raw).hexdigest()[:16]}", flush=True)

    for nq, nk, gain in SHAPES:
        q, k, v = randn(H, nq, dh) * gain, randn(H, nk, dh), randn(H, nk, dh)
        qp, kp = ceil_to(nq, 64), ceil_to(nk, 64)
        for name, dt, split, pv, qk8, out8, out_kt in KERNELS:
            def padded(x, rows, fill):   # [H, n, 64] -> planes [H, rows, 64], pad rows `fill`
                P = HL.from_float(x, dt, split)
                planes = []
                for p in (P.hi, P.lo):
                    if p is not None:
                        t = torch.full((H, rows, dh), fill, dtype=dt)
                        t[:, :x.shape[1]] = p
                        planes.append(t.to(dev))
                return HL(*planes)

            qd, kd = padded(q, qp, 0.0), padded(k, kp, nan)
            vt = v.transpose(1, 2).contiguous()
            V = HL.from_float(vt, dt, split)
            if split and pv == 1:  # the one-product P V reads the hi plane alone: rounded to nearest, as the projection writes it
                V = HL(vt.to(dt), (vt - vt.to(dt).float()).to(dt))
            planes = []
            for p in (V.hi, V.lo):
                if p is not None:
                    t = torch.zeros(H, dh, kp, dtype=dt)
                    t[:, :, :nk] = p
                    planes.append(t.to(dev))
            vd = HL(*planes)
            q8 = k8 = None
            if qk8:
                def planes8(t):  # HL [H, pad, 64] -> u8 [H, pad, 128]: e5m2(value) | e5m2(remainder * 2^10)
                    return torch.cat([t.float().to(torch.float8_e5m2).view(torch.uint8),
                                      (t.lo.float() * 1024.0).to(torch.float8_e5m2).view(torch.uint8)], dim=-1).contiguous()
                q8, k8 = planes8(qd), planes8(kd)
            hi = torch.full((nq, H * dh), nan, dtype=dt, device=dev)
            lo = torch.full((nq, H * dh), nan, dtype=dt, device=dev) if split and not out_kt else None
            o8 = torch.full((2, nq, H * dh), 0xA5, dtype=torch.uint8, device=dev) if out8 else None
            rt = Runtime(dev, dt, split=split)
            rt.pv_products = pv
            rt.flash_attn(qd, kd, vd, HL(hi, lo), 1, H, nq, qp, nk, kp, scale, q8=q8, k8=k8, out8=o8, out_kt=out_kt)
            outs = dict(out=hi)
            if lo is not None:
                outs["out_lo"] = lo
            if o8 is not None:
                outs["out8"] = o8
            dump(f"{name}_{nq}x{nk}" + ("_gain6" if gain != 1.0 else ""), **outs)
            del rt


if __name__ == "__main__":
    main()
