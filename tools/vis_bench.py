#!/usr/bin/env python3
"""Time the colourised depth output (vdn.vis) on one MI355X against the host stage it replaces, and write a markdown
table (profiles/vis.md is a run of this tool):

    python tools/vis_bench.py --out profiles/vis.md

Per shape (518 x 518, 720p, 1080p; 1 and 32 frames), on the same seeded depth data resident on the GPU:
  * device: vdn_minmax_f32 + vdn_colorize (per-frame range, Spectral_r BGR: the run.py / run_video.py form), HIP events around
    the two launches, warm-up, median of --iters; effective GB/s over the compulsory traffic, 4 B (min/max) + 4 B (colourise)
    read and 3 B written per pixel; then the same plus the uint8 copy to the host, by a host clock that ends in the copy;
  * host: the fp32 copy to the host that the scripts start from, plus tests/vis_ref.py (numpy fancy indexing into the
    truncated table) per frame, by a host clock; and, when matplotlib is importable, the reference's own expression with
    cmap() on the same host array.
The device result is compared byte for byte with the host one before anything is timed. Reports, not gates."""
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

SHAPES = [(518, 518), (720, 1280), (1080, 1920)]
FRAMES = [1, 32]


def event_ms(fn, warmup, iters):
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
        times.append(s.elapsed_time(e))
    return statistics.median(times), min(times)


def clock_ms(fn, warmup, iters):
    """Host clock around work that ends in a blocking copy (or is host work altogether)."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frame-ms", type=float, default=3.7, help="model time per frame the cost is set against")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import vis_ref as R
    from vdn import synth, util, vis
    try:
        import matplotlib
        cmap = matplotlib.colormaps.get_cmap("Spectral_r")
        host_kind = f"matplotlib {matplotlib.__version__} cmap() also timed"
    except ImportError:
        cmap = None
        host_kind = "matplotlib not importable: tests/vis_ref.py only"
    table = R.tables()["Spectral_r"]
    rt = vis._runtime(torch.device("cuda"))
    lut = vis.lut("Spectral_r", "bgr", False, 3, rt.device)
    rows = []
    for (H, W) in SHAPES:
        for N in FRAMES:
            depth = torch.from_numpy(synth.depth_clip(1234, N, H, W, max_depth=80.0).astype(np.float32)).to(rt.device)
            mm = torch.empty((N, 2), dtype=torch.float32, device=rt.device)
            out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=rt.device)

            def device():
                rt.minmax(depth, N, mm)
                rt.colorize(depth, mm, lut, out)

            def device_to_host():
                device()
                return util.to_host(out) if N > 1 else out.cpu().numpy()

            def host():
                d = util.to_host(depth) if N > 1 else depth.cpu().numpy()
                return np.stack([R.run_frame(d[f], None, True, False, table) for f in range(N)])

            def host_mpl():
                d = util.to_host(depth) if N > 1 else depth.cpu().numpy()
                res = []
                for f in range(N):
                    x = (d[f] - d[f].min()) / (d[f].max() - d[f].min()) * 255.0
                    res.append((cmap(x.astype(np.uint8))[:, :, :3] * 255)[:, :, ::-1].astype(np.uint8))
                return np.stack(res)

            got, want = np.array(device_to_host()), host()
            assert np.array_equal(got, want), f"{N}x{H}x{W}: device and host pictures differ in {(got != want).sum()} bytes"
            px = N * H * W
            dev_ms, dev_min = event_ms(device, a.warmup, a.iters)
            d2h_ms, _ = clock_ms(device_to_host, 2, a.iters)
            host_ms, _ = clock_ms(host, 1, a.host_iters)
            mpl_ms = clock_ms(host_mpl, 1, a.host_iters)[0] if cmap is not None else None
            if cmap is not None:
                assert np.array_equal(host_mpl(), want), "cmap() and the table lookup differ"
            rows.append((N, H, W, dev_ms, dev_min, 11 * px / (dev_ms * 1e-3) / 1e9, d2h_ms, host_ms, mpl_ms,
                         100.0 * dev_ms / (N * a.frame_ms), 100.0 * d2h_ms / (N * a.frame_ms)))
            print(rows[-1], flush=True)

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = ["# vdn.vis: the colourised depth output on the device against the host stage it replaces", "",
             f"`python tools/vis_bench.py` on {torch.cuda.get_device_name(0)} (torch {torch.__version__}), "
             f"{'on top of commit ' + commit if commit else 'working tree without git metadata'}; median of {a.iters} "
             f"(device) / {a.host_iters} (host) calls after warm-up. {host_kind}.", "",
             "Device = `vdn_minmax_f32` + `vdn_colorize` (per-frame range, Spectral_r, BGR), HIP events; GB/s over 11 B per pixel "
             "(4 + 4 read, 3 written). `+ D2H` adds the uint8 copy to the host (host clock). Host = fp32 copy to the host + "
             "`tests/vis_ref.py` per frame; `cmap()` = the same with matplotlib's call as the scripts make it. The last two "
             f"columns set the device cost against a model step of {a.frame_ms} ms per frame. Every device picture was compared "
             "byte for byte with the host one first.", "",
             "| frames | H x W | device ms (min) | GB/s | device + D2H ms | host ms | host cmap() ms | device / step | device + D2H / step |",
             "|---|---|---|---|---|---|---|---|---|"]
    for N, H, W, dev_ms, dev_min, gbs, d2h_ms, host_ms, mpl_ms, f1, f2 in rows:
        lines.append(f"| {N} | {H} x {W} | {dev_ms:.4f} ({dev_min:.4f}) | {gbs:.0f} | {d2h_ms:.3f} | {host_ms:.2f} | "
                     f"{'n/a' if mpl_ms is None else f'{mpl_ms:.2f}'} | {f1:.2f} % | {f2:.1f} % |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
