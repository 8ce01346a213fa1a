#!/usr/bin/env python3
"""Time the depth refiners' clip driver (`refine_video_depth`, v5 ViT-L) on one MI355X and write a markdown report
(profiles/refine_clip.md is a run of this tool):

    python tools/refine_clip_bench.py --out profiles/refine_clip.md [--append SECTION.md]

Cases: a 256-frame 518 x 518 depth clip (12 windows, 384 window slots over 256 distinct frames) and the 64-frame 1024 x 1024 clip
of BASELINE configs[4] (3 windows, 96 slots over 64 frames). Per case, on the same seeded clip resident on the GPU:
  * driver:   `refine_video_depth` (front once per distinct frame, clip-level tap cache, fused window tail, device stitcher,
              pinned copy), frames/s by a host clock that ends in the blocking device-to-host copy;
  * baseline: what the code before this driver offers a user: `forward` of every window's 32 gathered frames pushed through
              `DeviceStitcher`, the same range check and pinned copy; frames/s the same way. The two alternate in one process;
  * tail:     vdn_refine_window_tail on one window against the launches it fuses (index_select by slots, then
              vdn_upsample_bilinear_f32(relu), then vdn_refine_finish), HIP events, median of --iters, after a torch.equal check.
The two clips are compared (rel-L2, worst pixel) before anything is timed. Reports, not gates; --append adds a prepared section
(the asm_diff of the three kernels that now share their pixel functions with the tail) to the report."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = [(256, 518, 518), (64, 1024, 1024)]


def make_clip(n, H, W, device):
    """A seeded depth clip [n,H,W] in (0, 65535): eight synthetic frames, repeated with a slow per-frame gain."""
    from vdn import synth
    base = torch.from_numpy(synth.depth_clip(1234, 8, H, W)).to(device)
    gain = 1.0 - 0.002 * torch.arange(n, device=device, dtype=torch.float32)
    return (base[torch.arange(n, device=device) % 8] * gain[:, None, None]).contiguous()


def clock_fps(fns, n, warmup, iters):
    """Alternate the callables `fns` (each ends in a blocking copy); -> per callable (median frames/s, best frames/s)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    times = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[i].append(time.perf_counter() - t0)
    return [(n / statistics.median(t), n / min(t)) for t in times]


def event_us(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) * 1e3)
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3, help="timed clips per variant")
    ap.add_argument("--tail-iters", type=int, default=50)
    ap.add_argument("--encoder", default="vitl")
    ap.add_argument("--cases", default=None, help="e.g. 50x36x52 (frames x H x W), comma-separated; default: the two report cases")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", default=None)
    a = ap.parse_args()

    import vdn
    from vdn import synth, util
    from vdn.video_depth import DeviceStitcher
    from vdn.video_depth_model_v5 import VideoDepthAnything as RefinerV5
    assert torch.cuda.is_available(), "this tool times the MI355X; there is no CPU path"
    dev = torch.device("cuda")
    cases = CASES if a.cases is None else [tuple(int(v) for v in c.split("x")) for c in a.cases.split(",")]
    model = RefinerV5(**vdn.MODEL_CONFIGS[a.encoder])
    sd = model.state_dict()
    sd.update(synth.fast_state_dict([(k, tuple(v.shape)) for k, v in model.named_parameters()], 1234))
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    rt = model._engines()["rt"]
    rows, tails = [], []
    for (n, H, W) in cases:
        x = make_clip(n, H, W, dev)
        table = util.window_table(n)

        def driver():
            return model.refine_video_depth(x)[0]

        def baseline():
            st = DeviceStitcher(rt, len(table), H, W)
            for idxs in table:
                st.push(model.forward(x[torch.tensor(idxs, device=dev)][None])[0])
            res = st.result(n)
            util.check_finite(res, "baseline")
            return util.to_host(res)

        got, want = driver().copy(), baseline().copy()
        e = float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want.astype(np.float64)))
        worst = float(np.abs(got - want).max() / np.abs(want).max())
        (d_med, d_best), (b_med, b_best) = clock_fps([driver, baseline], n, 1, a.iters)
        slots_n, distinct = sum(len(w) for w in table), len({f for w in table for f in w})
        rows.append((n, H, W, len(table), slots_n, distinct, d_med, d_best, b_med, b_best, e, worst))
        print(rows[-1], flush=True)

        # the tail of one window (the last: repeats and padding) against the launches it fuses
        scaled = model._scaled(x)
        slots = torch.from_numpy(util.window_slots(n)).to(dev)[-1].contiguous()
        NH, NW = model.NET_HW
        net = torch.rand((util.INFER_LEN, NH, NW), device=dev)
        kind, residual, coef = model._tail()
        fused, d0, unfused = (torch.empty((util.INFER_LEN, H, W), device=dev) for _ in range(3))

        def tail():
            rt.refine_window_tail(net, scaled, slots, kind, residual, coef, fused)

        def launches():
            g = scaled.index_select(0, slots.long())
            rt.upsample_f32(net, d0, util.INFER_LEN, NH, NW, H, W, relu=True)
            rt.refine_finish(g, d0, coef[0], coef[1], coef[2], residual, unfused)

        tail()
        launches()
        assert torch.equal(fused, unfused), "the fused tail and the launches it replaces differ"
        t_med, t_best = event_us(tail, 5, a.tail_iters)
        u_med, u_best = event_us(launches, 5, a.tail_iters)
        px = util.INFER_LEN * H * W
        tails.append((H, W, t_med, t_best, u_med, u_best, 8 * px / (t_med * 1e-6) / 1e9))
        print(tails[-1], flush=True)
        del x, scaled, fused, d0, unfused
        util.release_host_buffers()
        torch.cuda.empty_cache()

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = ["# refine_video_depth: the depth refiners' windowed clip driver", "",
             f"`python tools/refine_clip_bench.py` on {torch.cuda.get_device_name(0)} (torch {torch.__version__}), "
             f"{'on top of commit ' + commit if commit else 'working tree without git metadata'}; v5 {a.encoder} (the network runs at "
             f"224 x 224), synthetic weights, one GPU. Frames/s by a host clock around a call that ends in the blocking pinned "
             f"device-to-host copy: median (best) of {a.iters} clips per variant after one warm-up clip, driver and baseline "
             "alternating in one process.", "",
             "Driver = `refine_video_depth`: median / scale / resize / normals / encoder once per DISTINCT frame into the clip-level "
             "tap cache, the temporal head per window, `vdn_refine_window_tail`, `DeviceStitcher`. Baseline = per-window `forward` "
             "of the 32 gathered frames (every slot through the whole front and the encoder again) pushed through `DeviceStitcher`, "
             "the same range check and copy: what the code before this driver offers. `agreement` is the driver's clip against the "
             "baseline's, rel-L2 / worst pixel of max.", "",
             "| frames | H x W | windows | slots | distinct | driver frames/s | baseline frames/s | driver / baseline | agreement |",
             "|---|---|---|---|---|---|---|---|---|"]
    for n, H, W, nw, slots_n, distinct, d_med, d_best, b_med, b_best, e, worst in rows:
        lines.append(f"| {n} | {H} x {W} | {nw} | {slots_n} | {distinct} | {d_med:.1f} ({d_best:.1f}) | {b_med:.1f} ({b_best:.1f}) | "
                     f"{d_med / b_med:.2f} x | {e:.1e} / {worst:.1e} |")
    lines += ["", "The window tail on one 32-slot window (the clip's last: keyframe copies and padding), HIP events, median (best) of "
              f"{a.tail_iters}: `vdn_refine_window_tail` against `index_select` by slots + `vdn_upsample_bilinear_f32(relu)` + "
              "`vdn_refine_finish`, `torch.equal` first. GB/s over the tail's compulsory 8 B per output pixel (scaled read, result "
              "written; the 224 x 224 map is small beside them).", "",
              "| H x W | fused tail us | unfused launches us | unfused / fused | fused GB/s |", "|---|---|---|---|---|"]
    for H, W, t_med, t_best, u_med, u_best, gbs in tails:
        lines.append(f"| {H} x {W} | {t_med:.1f} ({t_best:.1f}) | {u_med:.1f} ({u_best:.1f}) | {u_med / t_med:.2f} x | {gbs:.0f} |")
    text = "\n".join(lines) + "\n"
    if a.append:
        text += "\n" + open(a.append).read()
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
