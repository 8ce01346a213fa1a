#!/usr/bin/env python3
"""Time vdn.normal_metrics.angular_error (explicit target and from_depth) and vdn.vis.colorize_normals on one MI355X against
the same statements written as float32 torch ops on the device, and against their byte floors; write a markdown table
(profiles/normal_angles.md is a run of this tool):

    python tools/normal_metrics_bench.py --out profiles/normal_angles.md [--bench-parent "<json line>" --bench-this "<json line>"]

Per shape ([2, 32, 518, 518] and [1, 16, 224, 224]), on seeded data resident on the GPU, HIP events, warm-up, median of --iters:
  * vdn: one call of angular_error (the sweep, the fold, the three selects, the rows) or colorize_normals;
  * torch: normalise, cross, atan2, the 3 x 3 erosion as a max-pool, NaN-masked mean / median (torch.nanmedian per frame,
    item and batch) / comparisons, all float32, no synchronisation; for from_depth the target is first made by a reflect pad
    and shifted differences; the picture as normalise, scale, floor, cast, permute.
  * the floor: bytes that must cross HBM over 6.3 TB/s. Statistics: 12 (pred) + 12 (target) or 4 (depth) + 1 (mask) read, plus this
    design's float32 angle plane, written once and read by each of the select's three passes at each of three levels:
    4 + 9 * 4 = 40. Picture: 12 or 4 read, 3 written.
Before timing, the kept counts of the two are compared and the largest difference of the other columns (float32 against
fp64) is recorded, so that the table shows both time the same thing. Reports, not gates. --bench-parent / --bench-this take bench.py's result lines of the parent commit and of this tree, measured on the
same machine, for the profile's last section."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [(2, 32, 518, 518), (1, 16, 224, 224)]
THRESHOLDS = (5.0, 7.5, 11.25, 22.5, 30.0)
HBM_BYTES_PER_S = 6.3e12    # what a float4 copy reaches on this part (8 TB/s on paper)


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


def torch_depth_normal(depth):
    """depth [B, T, H, W] -> (-Ix, -Iy, 1) [B, T, 3, H, W], float32."""
    p = F.pad(depth, (1, 1, 1, 1), mode="reflect")
    H, W = depth.shape[-2:]
    w = lambda r, c: p[..., r:r + H, c:c + W]
    ix = ((w(0, 0) - w(0, 2)) + 2.0 * (w(1, 0) - w(1, 2)) + (w(2, 0) - w(2, 2))) * 0.125
    iy = ((w(0, 0) - w(2, 0)) + 2.0 * (w(0, 1) - w(2, 1)) + (w(0, 2) - w(2, 2))) * 0.125
    return torch.stack([-ix, -iy, torch.ones_like(ix)], dim=2)


def torch_stats(pred, target, mask, from_depth):
    """The nine columns of the batch, the items and the frames as float32 torch ops -> [1 + B + B T, 9]."""
    if from_depth:
        target = torch_depth_normal(target)
    a, b = F.normalize(pred, dim=2), F.normalize(target, dim=2)
    ang = torch.atan2(torch.cross(a, b, dim=2).norm(dim=2), (a * b).sum(2)) * (180.0 / math.pi)
    keep = 1.0 - F.max_pool2d(1.0 - mask.float(), 3, 1, 1)             # the erosion; outside the image erodes nothing
    v = torch.where(keep > 0, ang, torch.full_like(ang, float("nan")))
    B, T = v.shape[:2]
    out = []
    for x in (v.reshape(1, -1), v.reshape(B, -1), v.reshape(B * T, -1)):
        n = (~torch.isnan(x)).sum(1).float()
        cols = [n, torch.nanmean(x, 1), torch.nanmedian(x, 1).values, torch.nanmean(x * x, 1).sqrt()]
        cols += [(x < t).sum(1).float() / n for t in THRESHOLDS]
        out.append(torch.stack(cols, 1))
    return torch.cat(out)


def torch_picture(x, from_depth):
    if from_depth:
        x = torch_depth_normal(x[None])[0]
    v = torch.floor((F.normalize(x, dim=1) * 0.5 + 0.5) * 255.0 + 0.5)
    return v.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit this tree stands on, where the run has no git metadata")
    ap.add_argument("--bench-parent", default=None, help="bench.py's JSON line on the parent commit")
    ap.add_argument("--bench-this", default=None, help="bench.py's JSON line on this tree")
    a = ap.parse_args()

    import normal_angle_ref as A
    from vdn import normal_metrics as M, vis
    dev = torch.device("cuda")
    rows = []
    for shape in SHAPES:
        B, T, H, W = shape
        c = A.make_case(41, (1, 2, H, W), 0.97)                          # two seeded frames, tiled over the clip
        tile = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev).repeat((B, T // 2) + (1,) * (x.ndim - 2)).contiguous()
        pred, target, depth, mask = tile(c["pred"]), tile(c["target"]), tile(c["depth"]), tile(c["mask"])
        px = B * T * H * W
        for from_depth in (False, True):
            t = depth if from_depth else target
            got = M.angular_error(pred, t, mask, from_depth=from_depth)
            got = torch.cat([got["batch"][None], got["items"], got["frames"].reshape(B * T, 9)]).cpu().numpy()
            want = torch_stats(pred, t, mask, from_depth).double().cpu().numpy()
            assert np.array_equal(got[:, 0], want[:, 0]), "kept pixels differ"
            # torch.nanmedian takes the lower middle value, float32 throughout: float32 agreement only
            worst = float(np.abs(got[:, 1:] - want[:, 1:]).max())
            vdn_ms, vdn_min = event_ms(lambda: M.angular_error(pred, t, mask, from_depth=from_depth), a.warmup, a.iters)
            torch_ms, _ = event_ms(lambda: torch_stats(pred, t, mask, from_depth), a.warmup, a.iters)
            inputs, reread = (17 if from_depth else 25), 40
            rows.append(("angular_error" + (" from_depth" if from_depth else ""), shape, vdn_ms, vdn_min, torch_ms, inputs, reread,
                         (inputs + reread) * px / HBM_BYTES_PER_S * 1e3, worst))
            print(rows[-1], flush=True)
        for from_depth in (False, True):
            x = (depth if from_depth else pred).reshape((B * T,) + ((H, W) if from_depth else (3, H, W)))
            got, want = vis.colorize_normals(x, from_depth=from_depth), torch_picture(x, from_depth)
            vdn_ms, vdn_min = event_ms(lambda: vis.colorize_normals(x, from_depth=from_depth), a.warmup, a.iters)
            torch_ms, _ = event_ms(lambda: torch_picture(x, from_depth), a.warmup, a.iters)
            inputs = 4 if from_depth else 12
            rows.append(("colorize_normals" + (" from_depth" if from_depth else ""), shape, vdn_ms, vdn_min, torch_ms, inputs + 3, 0,
                         (inputs + 3) * px / HBM_BYTES_PER_S * 1e3, float((got != want).float().mean())))
            print(rows[-1], flush=True)

    try:
        commit = a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = ["# vdn.normal_metrics and colorize_normals: device time against torch compositions and the byte floor", "",
             f"`python tools/normal_metrics_bench.py` on {torch.cuda.get_device_name(0)} (torch {torch.__version__}), "
             f"{'on top of commit ' + commit if commit else 'working tree without git metadata'}; HIP events, median (minimum) of "
             f"{a.iters} calls after {a.warmup} warm-up calls. Nothing here was measured before; no ratio is a target.", "",
             "`vdn` is one call of the public function: for the statistics the sweep (angles in fp64, block rows, the float32 angle "
             "plane written to the workspace), the one-block fold, the select's three passes at each of the three levels (frames, "
             "items, batch: 18 launches that read the plane nine times) and the rows kernel. The plane was chosen over recomputing "
             "the angle in every pass: a pass then reads 4 B per pixel in place of 25 (or the depth stencil) and runs no fp64 "
             "atan2; it costs 4 B written and 36 B read per pixel, the `re-read` column. `torch` is the same statements as float32 "
             "torch ops on the device (normalise, cross, atan2, max-pool erosion, nanmean, nanmedian per frame / item / batch, "
             "comparisons; reflect pad and shifted differences for from_depth), which are less exact (float32, lower-middle "
             f"median); the last column has their largest difference from the vdn rows. `floor` is (inputs + re-read) bytes per "
             f"pixel over {HBM_BYTES_PER_S / 1e12:.1f} TB/s.", "",
             "| call | B, T, H, W | vdn ms (min) | torch ms | torch / vdn | input B/px | re-read B/px | floor ms | vdn / floor | "
             "vdn against torch |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name, shape, vdn_ms, vdn_min, torch_ms, inputs, reread, floor_ms, diff in rows:
        note = f"{diff:.1e} of bytes differ" if name.startswith("colorize") else f"max column difference {diff:.1e}"
        lines.append(f"| {name} | {', '.join(map(str, shape))} | {vdn_ms:.3f} ({vdn_min:.3f}) | {torch_ms:.3f} | {torch_ms / vdn_ms:.1f}x | "
                     f"{inputs} | {reread} | {floor_ms:.4f} | {vdn_ms / floor_ms:.1f}x | {note} |")
    if a.bench_parent and a.bench_this:
        p, t = json.loads(a.bench_parent), json.loads(a.bench_this)
        lines += ["", "## bench.py, parent commit against this tree", "",
                  "The new file shares no kernel with the timed path; select.hpp's launches are unchanged. Both lines were measured "
                  "on the same machine, one after the other (`bench.py --gpus 1`).", "",
                  "| tree | value | ms per step |", "|---|---|---|",
                  f"| parent | {p.get('value')} | {p.get('ms_per_step')} |", f"| this tree | {t.get('value')} | {t.get('ms_per_step')} |"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
