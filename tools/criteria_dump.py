#!/usr/bin/env python3
"""Dump the raw bytes of everything the criteria that share csrc/frame_sums.hpp produce (loss, loss_grad, ssim,
normals, normals_grad, eval, metric), for a byte-for-byte comparison of two builds of the library (profiles/criteria_refactor.md is
such a comparison):

    python tools/criteria_dump.py DIR                          # this tree's library
    VDN_LIB=<other tree>/lib/libvdn_hip.so python tools/criteria_dump.py DIR2      # then cmp every file of the two DIRs

Seeded CPU generators make the inputs; every entry is called once per case through a fresh Runtime; each output is written
as DIR/<case>.<name>.bin. Every reported sum is fp64, so no workspace is dumped. The shapes are the smallest that reach each
path: one pixel per lane, quads, quads whose rows are not whole quads, one size past the first round of a block's stride
loop per unit and path, float planes one float off a 16-byte boundary, an empty frame and an empty item. Not a test: it
asserts nothing."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))

import torch  # noqa: E402


def main():
    out_dir = sys.argv[1]
    os.makedirs(out_dir, exist_ok=True)
    from vdn import _abi
    from vdn.runtime import Runtime
    dev = torch.device("cuda:0")
    seed = [3000]

    def gen():
        seed[0] += 1
        return torch.Generator().manual_seed(seed[0])

    def randn(*shape):
        return torch.randn(*shape, generator=gen())

    def rand(*shape):
        return torch.rand(*shape, generator=gen())

    def empty(*shape, dtype=torch.float32, off=False):
        if not off:
            return torch.empty(*shape, dtype=dtype, device=dev)
        n = 1
        for s in shape:
            n *= s
        return torch.empty(n + 1, dtype=dtype, device=dev)[1:].view(*shape)  # one float past a 16-byte boundary

    def put(t, off=False):
        """t on the device; off: every float plane of it starts one float past a 16-byte boundary."""
        if not off or t.dtype != torch.float32:
            return t.to(dev)
        d = empty(*t.shape, off=True)
        d.copy_(t)
        return d

    live = []  # the Runtimes whose launches may still run: their workspaces stay allocated until the next dump has synchronised

    def fresh():
        live.append(Runtime(dev))
        return live[-1]

    def dump(case, **tensors):
        torch.cuda.synchronize()
        live.clear()
        for name, t in sorted(tensors.items()):
            raw = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
            with open(os.path.join(out_dir, f"{case}.{name}.bin"), "wb") as f:
                f.write(raw)
            print(f"{case}.{name}.bin {len(raw)} {hashlib.sha256(raw).hexdigest()[:16]}", flush=True)

    f64 = torch.float64

    # ---- depth criterion: forward, the fit alone, trimmed, and the two backward passes
    def depth(case, B, T, H, W, off=False, holes=False):
        target = rand(B, T, H, W) * 10.0 + 0.5
        pred = put(target * 0.7 + 0.3 + randn(B, T, H, W) * 0.2, off)
        mask = (rand(B, T, H, W) > 0.2).to(torch.uint8)
        if holes:  # an empty frame in an item that keeps others, and an empty item
            mask[0, 1] = 0
            mask[B - 1] = 0
        target, mask = put(target, off), mask.to(dev)
        coeff = torch.tensor([1.0, 0.5, 0.25], device=dev)
        args = dict(alpha=0.5, scales=4, stable_scale=10.0)

        def state(n):
            return (empty(n, dtype=f64), empty(B, 2), empty(B * T, 4, dtype=f64), empty(B * T, dtype=torch.int64))

        out, ss, fs, fc = state(20)
        fresh().depth_loss(pred, target, mask, out, scale_shift=ss, frame_stats=fs, frame_counts=fc, **args)
        dump(f"depth_loss_{case}", out=out, scale_shift=ss, frame_stats=fs, frame_counts=fc)
        fit = empty(B, 2)
        fresh().depth_loss(pred, target, mask, None, scale_shift=fit, **args)
        dump(f"depth_loss_{case}_fit_alone", scale_shift=fit)
        grad = empty(B, T, H, W, off=off)
        fresh().depth_loss_backward(pred, target, mask, 0.5, 4, 10.0, ss, fs, fc, out, coeff, grad)
        dump(f"depth_loss_backward_{case}", grad=grad)
        out, ss, fs, fc = state(40)
        fresh().depth_loss(pred, target, mask, out, scale_shift=ss, frame_stats=fs, frame_counts=fc, keep=0.8, **args)
        dump(f"depth_loss_trimmed_{case}", out=out, scale_shift=ss, frame_stats=fs, frame_counts=fc)
        grad = empty(B, T, H, W, off=off)
        fresh().depth_loss_backward(pred, target, mask, 0.5, 4, 10.0, ss, fs, fc, out, coeff, grad, keep=0.8)
        dump(f"depth_loss_trimmed_backward_{case}", grad=grad)

    depth("2x3x5x7", 2, 3, 5, 7)
    depth("1x2x16x16", 1, 2, 16, 16)
    depth("1x2x6x6", 1, 2, 6, 6)
    depth("1x2x184x180", 1, 2, 184, 180)   # quads, past the first round of 32 x 256 x 4 pixels
    depth("1x2x91x91", 1, 2, 91, 91)       # one pixel per lane, past the first round of 32 x 256
    depth("1x2x16x16_offset", 1, 2, 16, 16, off=True)
    depth("2x3x5x7_holes", 2, 3, 5, 7, holes=True)

    # ---- normal criterion: both target kinds, with and without a mask, and the backward pass
    def unit(t):
        return t / t.norm(dim=1, keepdim=True)

    def normals(case, F, H, W, off=False):
        pred = put(unit(randn(F, 3, H, W)) * (rand(F, 1, H, W) + 0.5), off)
        stored, dmap = put(unit(randn(F, 3, H, W)), off), put(rand(F, H, W) * 10.0 + 0.5, off)
        m = (rand(F, H, W) > 0.1).to(torch.uint8).to(dev)
        coeff = torch.tensor([0.7], dtype=f64, device=dev)
        for tgt, gname in ((stored, "stored"), (dmap, "depth")):
            for mask, mname in ((None, "nomask"), (m, "mask")):
                out, fs, fc = empty(2, dtype=f64), empty(F, dtype=f64), empty(F, dtype=torch.int64)
                fresh().normal_eval(pred, tgt, mask, out, fs, fc)
                dump(f"normal_eval_{case}_{gname}_{mname}", out=out, frame_sums=fs, frame_counts=fc)
                grad = empty(F, 3, H, W, off=off)
                fresh().normal_loss_backward(pred, tgt, mask, out[1:2].clone(), coeff, grad)
                dump(f"normal_loss_backward_{case}_{gname}_{mname}", grad=grad)

    normals("2x5x7", 2, 5, 7)
    normals("2x16x16", 2, 16, 16)
    normals("2x6x6", 2, 6, 6)
    normals("1x259x256", 1, 259, 256)      # quads, past the first round of 64 x 256 x 4 pixels
    normals("1x259x257", 1, 259, 257)      # one pixel per lane, past the first round
    normals("2x16x16_offset", 2, 16, 16, off=True)

    # ---- clip evaluation: both domains, both TGM kinds
    def clip(case, T, H, W, off=False):
        gt = put(rand(T, H, W) * 60.0 + 0.5, off)
        pred = put(rand(T, H, W) * 2.0 + 0.05, off)
        m = (rand(T, H, W) > 0.2).to(torch.uint8)
        m[:, 0, :4] = 1
        m = m.to(dev)
        for domain, dname in ((_abi.EVAL_DEPTH, "depth"), (_abi.EVAL_DISP, "disp")):
            for tgm, tname in ((_abi.EVAL_TGM_ROWS, "rows"), (_abi.EVAL_TGM_FRAMES, "frames")):
                for mask, mname in ((None, "nomask"), (m, "mask")):
                    rt = fresh()
                    coef, out = empty(2, dtype=f64), empty(7, dtype=f64)
                    rt.eval_fit(pred, gt, mask, 1e-3, 70.0, domain, coef)
                    rt.eval_metrics(pred, gt, mask, 1e-3, 70.0, domain, tgm, coef, out)
                    dump(f"eval_{case}_{dname}_{tname}_{mname}", coef=coef, out=out)

    clip("3x5x7", 3, 5, 7)
    clip("3x91x91", 3, 91, 91)             # past the first round of 32 x 256 pixels
    clip("3x16x16_offset", 3, 16, 16, off=True)

    # ---- metric-depth scores: same size and resampled; SiLog and its backward pass
    def metric(case, B, H, W, ph, pw, off=False):
        depth_gt = put(rand(B, H, W) * 9.0 + 0.5, off)
        valid = (rand(B, H, W) > 0.2).to(torch.uint8).to(dev)
        for (h, w), rname in (((H, W), "same"), ((ph, pw), "resampled")):
            pred = put(rand(B, h, w) * 9.0 + 0.5, off)
            for mask, bounds, mname in ((None, None, "all"), (valid, (1.0, 9.0), "bounded")):
                out = empty(B, 10, dtype=f64)
                fresh().metric_eval(pred, depth_gt, mask, out, bounds)
                dump(f"metric_eval_{case}_{rname}_{mname}", out=out)

    def silog(case, n, off=False):
        target, pred = put(rand(n) * 9.0 + 0.5, off), put(rand(n) * 9.0 + 0.5, off)
        m = (rand(n) > 0.2).to(torch.uint8).to(dev)
        coeff = torch.tensor([0.3], device=dev)
        for mask, bounds, mname in ((None, None, "all"), (m, (1.0, 9.0), "bounded")):
            out, grad = empty(4, dtype=f64), empty(n, off=off)
            fresh().silog_loss(pred, target, mask, out, 0.5, bounds)
            fresh().silog_loss_backward(pred, target, mask, out, coeff, grad, 0.5, bounds)
            dump(f"silog_{case}_{mname}", out=out, grad=grad)

    wide_n, single_n = _abi.lib.vdn_metric_trip(1) * 4 + 12, _abi.lib.vdn_metric_trip(0) * 4 + 12  # past a lane's trips in flight
    metric("2x5x7", 2, 5, 7, 3, 4)
    metric("1x16x16", 1, 16, 16, 7, 9)
    metric(f"1x4x{wide_n // 4}", 1, 4, wide_n // 4, 3, 1000)
    metric(f"1x4x{single_n // 4}_offset", 1, 4, single_n // 4, 3, 1000, off=True)  # off the boundary: one element per lane
    silog("35", 35)
    silog("256", 256)
    silog(str(wide_n), wide_n)
    silog(f"{single_n}_offset", single_n, off=True)

    # ---- the SSIM term: alone and on the aligned prediction, forward, backward and the accumulating backward. Last, so that
    # the seeds of the cases above stay what they were.
    def ssim(case, B, T, H, W, off=False):
        target = rand(B, T, H, W) * 2.0 + 0.5
        pred = put(target * 0.7 + 0.3 + randn(B, T, H, W) * 0.2, off)
        mask = (rand(B, T, H, W) > 0.2).to(torch.uint8).to(dev)
        target = put(target, off)
        coeff = torch.tensor([0.3], device=dev)
        fit = empty(B, 2)
        fresh().depth_loss(pred, target, mask, None, scale_shift=fit)
        for ss, sname in ((None, "alone"), (fit, "aligned")):
            out, cs, im = empty(4, dtype=f64), empty(B * T, dtype=f64), empty(B, 4, dtype=f64)
            fresh().ssim_loss(pred, target, mask, ss, out, cs, im)
            grad = empty(B, T, H, W, off=off)
            fresh().ssim_loss_backward(pred, target, mask, ss, out, cs, im, coeff, grad)
            added = put(randn(B, T, H, W) * 1e-3, off)
            fresh().ssim_loss_backward(pred, target, mask, ss, out, cs, im, coeff, added, accumulate=True)
            dump(f"ssim_{case}_{sname}", out=out, frame_cs=cs, item_max=im, grad=grad, grad_accumulated=added)

    ssim("2x3x12x37", 2, 3, 12, 37)
    ssim("1x2x26x42", 1, 2, 26, 42)            # one tile of outputs and a second row and column of tiles of pixels
    ssim("1x2x27x43_offset", 1, 2, 27, 43, off=True)
    ssim("1x300x11x13", 1, 300, 11, 13)        # more frames than the lanes of the one-block folds


if __name__ == "__main__":
    main()
