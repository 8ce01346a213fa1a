#!/usr/bin/env python3
"""Dump the raw bytes of everything the kernels that share csrc/resample.hpp produce, for a byte-for-byte comparison of two
builds of the library (profiles/resample_refactor.md is such a comparison):

    python tools/resample_dump.py DIR                          # this tree's library
    VDN_LIB=<other tree>/lib/libvdn_hip.so python tools/resample_dump.py DIR2      # then cmp every file of the two DIRs

Seeded CPU generators make the inputs; every touched entry is called once per case through Runtime, at sizes with tile tails
and more than one block; each output is written as DIR/<case>.<name>.bin. Not a test: it asserts nothing."""
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
    from vdn import pack
    from vdn.runtime import Runtime
    dev = torch.device("cuda:0")
    seed = [2000]

    def gen():
        seed[0] += 1
        return torch.Generator().manual_seed(seed[0])

    def randn(*shape):
        return torch.randn(*shape, generator=gen())

    def empty(*shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=dev)

    def dump(case, **tensors):
        torch.cuda.synchronize()
        for name, t in sorted(tensors.items()):
            raw = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
            with open(os.path.join(out_dir, f"{case}.{name}.bin"), "wb") as f:
                f.write(raw)
            print(f"{case}.{name}.bin {len(raw)} {hashlib.sha256(raw).hexdigest()[:16]}", flush=True)

    # ---- bilinear, align_corners, 16-bit planes: single plane and split, both half types
    for half, hname in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
        for split in (False, True):
            rt = Runtime(dev, half, split)
            B, IH, IW, OH, OW, C = 2, 37, 76, 65, 133, 24
            x = rt.to_half(randn(B * IH * IW, C).to(dev))
            y = rt.hbuf("up", (B * OH * OW, C))
            rt.upsample(x, y, B, IH, IW, OH, OW, C)
            planes = dict(hi=y.hi) if y.lo is None else dict(hi=y.hi, lo=y.lo)
            dump(f"upsample_{hname}_{'split' if split else 'single'}", **planes)
    rt = Runtime(dev, torch.float16, True)
    for (B, IH, IW, OH, OW) in ((2, 70, 112, 60, 100), (1, 259, 462, 540, 960), (1, 6, 7, 1, 5)):
        for relu in (False, True):
            y = empty(B, OH, OW)
            rt.upsample_f32((randn(B, IH, IW) * 2.5).to(dev), y, B, IH, IW, OH, OW, relu=relu)
            dump(f"upsample_f32_{IH}x{IW}_{OH}x{OW}_relu{int(relu)}", out=y)

    # ---- oc1 combine: exact 2x and the head's 2x - 1 shape, tile tails
    for (B, IH, IW, OH, OW, Co) in ((1, 37, 37, 74, 74, 32), (2, 20, 33, 39, 65, 16)):
        z, bias, out = randn(B * IH * IW, 9 * Co).to(dev), randn(Co).to(dev), empty(B * OH * OW, Co)
        rt.oc1_combine(z, bias, out, B, IH, IW, OH, OW, Co)
        dump(f"oc1_combine_{IH}x{IW}_{OH}x{OW}_c{Co}", out=out)

    # ---- fused depth tail: both half types, 1 and 2 channel passes, tile tails in both directions
    for half, hname in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
        rth = Runtime(dev, half, True)
        for (B, IH, IW, C, OH, OW) in ((2, 76, 76, 32, 133, 133), (1, 40, 24, 64, 70, 42)):
            x = randn(B * IH * IW, C).to(dev)
            wt = pack.conv3x3_taps((randn(32, C, 3, 3) / math.sqrt(9 * C)).to(dev), rth.prec)
            b2, w1 = (randn(32) * 0.1).to(dev), (randn(32) * 0.3).to(dev)
            for relu in (False, True):
                d = empty(B, OH, OW)
                rth.depth_tail(x, wt, b2, w1, 0.2, d, B, IH, IW, C, OH, OW, relu=relu)
                dump(f"depth_tail_{hname}_{IH}x{IW}_c{C}_relu{int(relu)}", out=d)

    # ---- depth + normal tail, with and without resize
    F, IH, IW, Cin = 2, 38, 52, 48
    x, w, bias = randn(F, IH, IW, Cin).to(dev), (randn(3, Cin, 3, 3) / math.sqrt(9 * Cin)).to(dev), randn(3).to(dev)
    for (OH, OW) in ((IH, IW), (67, 91), (30, 41)):
        raw, depth, normal = empty(F, 3, OH, OW), empty(F, OH, OW), empty(F, 3, OH, OW)
        rt.dn_tail(x, F, IH, IW, Cin, w, bias, OH, OW, depth_in=randn(F, OH, OW).to(dev), relu=True, raw=raw, depth=depth,
                   normal=normal)
        dump(f"dn_tail_{IH}x{IW}_{OH}x{OW}", raw=raw, depth=depth, normal=normal)

    # ---- cubic: the position-embedding resize (explicit scale factors) and the u8 pre-processing
    ih, iw, C = 37, 37, 48
    for (oh, ow) in ((19, 27), (66, 90)):
        dst = empty(oh * ow, C)
        rt.bicubic(randn(ih * iw, C).to(dev), dst, ih, iw, oh, ow, C, (oh + 0.1) / ih, (ow + 0.1) / iw)
        dump(f"bicubic_{oh}x{ow}", out=dst)
    for (n, h, w, H, W) in ((2, 60, 100, 70, 112), (1, 300, 180, 238, 140), (1, 37, 53, 518, 742)):
        fr = torch.randint(0, 256, (n, h, w, 3), generator=gen(), dtype=torch.uint8).to(dev)
        for swap in (False, True):
            out = rt.preprocess_u8(fr, H, W, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), swap)
            dump(f"preprocess_u8_{h}x{w}_{H}x{W}_swap{int(swap)}", out=out)

    # ---- half-pixel bilinear, down and up
    for (T, IH, IW, OH, OW) in ((2, 37, 53, 19, 20), (1, 40, 30, 97, 71)):
        y = empty(T, OH, OW)
        rt.resize_bilinear_hp(randn(T, IH, IW).to(dev), y)
        dump(f"resize_bilinear_hp_{IH}x{IW}_{OH}x{OW}", out=y)


if __name__ == "__main__":
    main()
