#!/usr/bin/env python3
"""Time the normal criterion with its gradient (vdn.normals) on one MI355X and write profiles/normal_loss_grad.md.

For the 32-frame 518 x 518 clip of tools/normal_bench.py (prediction, stored target, gt depth and a bool mask resident on the
GPU; seeded by tests/normal_ref.make_case, nothing is read from the reference):
  * the backward launch alone (Runtime.normal_loss_backward on a saved count) for a stored target and for a depth target, beside
    the forward launch (Runtime.normal_eval: partial sums and finalise) on the same inputs, each with the bytes it must move and
    the share of the measured HBM rate that is, as profiles/normal_eval.md reports them;
  * the whole criterion(p, t, m)["normal_loss"].backward() on a leaf that requires a gradient, for both target kinds, beside a
    float32 torch restatement written here (erode by conv2d as the reference does, F.cosine_similarity, masked mean, autograd) on
    the same device, and how far that restatement's float32 gradient is from the device's;
  * a device-to-device copy, for the rate a pass over the inputs can reach.
Each timed call works on the next of `sets` copies of the inputs, enough of them that together they exceed the 256 MiB Infinity
Cache twice over, so a call reads from HBM. A sample is the time of `--batch` calls between two device events, divided by the
batch; the figure is the median (min .. max) of `--iters` samples after `--warmup` calls. The event figures of a single launch
include its launch overhead; the kernels' own times come from a kernel trace, which slows the host and therefore runs on its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/normal_grad_bench.py --trace
and its kernel_stats.csv is handed to the timing run as --kernel-stats CSV. Without it the profile says so.

Correctness at size: the device against tests/normal_grad_ref.py at [1, 2, 518, 518] (H * W a multiple of 4, W not: quads that
cross a row's end), by the per-element bound of tests/test_gpu_normal_grad.py. A report, not a gate."""
import argparse
import csv
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from normal_bench import HBM_MEASURED, sample_us  # noqa: E402

#        what                           bytes per pixel: pred 12, stored target 12 or depth 4, mask 1, gradient 12
BYTES = {"fwd_stored": 25, "fwd_depth": 17, "bwd_stored": 37, "bwd_depth": 29}


def torch_target(depth):
    """normal_vector(depth) with its defaults in torch float32 ops, depth [F, H, W] -> [F, 3, H, W]; no gradient."""
    with torch.no_grad():
        Fr, H, W = depth.shape
        p = F.pad(depth[:, None], (1, 1, 1, 1), mode="reflect")[:, 0]
        w = lambda r, c: p[:, r:r + H, c:c + W]
        ix = ((w(0, 0) - w(0, 2)) + 2.0 * (w(1, 0) - w(1, 2)) + (w(2, 0) - w(2, 2))) * 0.125
        iy = ((w(0, 0) - w(2, 0)) + 2.0 * (w(0, 1) - w(2, 1)) + (w(0, 2) - w(2, 2))) * 0.125
        n = torch.stack([-ix, -iy, torch.ones_like(ix)], 1)
        return n / torch.sqrt((n * n).sum(1, keepdim=True) + 1e-8)


def torch_restatement(pred, target, mask):
    """VideoNormalLoss in torch float32 ops under autograd: pred, target [F, 3, H, W], mask bool [F, H, W] -> 0-dim loss."""
    kernel = torch.ones(1, 1, 3, 3, device=pred.device)
    keep = ~(F.conv2d((~mask)[:, None].float(), kernel, padding=1)[:, 0] > 0)
    cos = F.cosine_similarity(pred, target, dim=1)
    return 1.0 - torch.where(keep, cos, 0.0).sum() / keep.sum()


def make_pool(T, H, W, dev):
    import normal_ref as R
    c = R.make_case(9, (1, T, H, W), "bool", "unit")
    px = T * H * W
    sets = max(2, math.ceil(2 * 256 * 2 ** 20 / (BYTES["fwd_depth"] * px)))
    base = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
    pool = [{k: v.clone() for k, v in base.items()} for _ in range(sets)]
    for s in pool:
        s["m8"] = s["mask"].view(torch.uint8).view(T, H, W)
        s["p4"], s["t4"], s["d3"] = s["pred"].view(T, 3, H, W), s["target"].view(T, 3, H, W), s["depth"].view(T, H, W)
        s["grad"] = torch.empty_like(s["p4"])
    return pool, px


def saved_counts(rt, pool, dev):
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    counts = []
    for s in pool:
        rt.normal_eval(s["p4"], s["t4"], s["m8"], out)
        counts.append(out[1:2].clone())
    return counts


def trace(a, dev):
    from vdn import normals as N
    rt = N._runtime_for(dev)
    pool, _ = make_pool(a.frames, a.size, a.size, dev)
    counts, one = saved_counts(rt, pool, dev), torch.ones(1, dtype=torch.float64, device=dev)
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    for i in range(a.trace_calls):
        s = pool[i % len(pool)]
        for tgt in (s["t4"], s["d3"]):
            rt.normal_eval(s["p4"], tgt, s["m8"], out)
            rt.normal_loss_backward(s["p4"], tgt, s["m8"], counts[i % len(pool)], one, s["grad"])
    torch.cuda.synchronize()
    print(f"traced {a.trace_calls} forward and backward launches per target kind, shape [1, {a.frames}, {a.size}, {a.size}]")


def kernel_rows(path):
    """-> {kernel name: (calls, average us, min us, max us)} for the normal kernels of a kernel_stats.csv."""
    rows = {}
    for r in csv.DictReader(open(path)):
        if "normal_" in r["Name"]:
            name = re.sub(r"\(anonymous namespace\)::", "", r["Name"]).split("(")[0].replace("void ", "")
            rows[name] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3)
    return rows


def bound_ratio(dev, H, W):
    import normal_grad_ref as G
    import normal_ref as R
    from vdn import normals as N
    c = R.make_case(9, (1, 2, H, W), "bool", "unit")
    rows = []
    for from_depth in (False, True):
        tgt = c["depth"] if from_depth else c["target"]
        want, mag = G.normal_loss_grad_ref(c["pred"], tgt, c["mask"], from_depth)
        got = N.normal_loss_grad(*(torch.from_numpy(x).to(dev) for x in (c["pred"], tgt, c["mask"])), from_depth=from_depth)
        bound = 2.0 ** -23 * np.abs(want) + 2.0 ** -40 * mag + 1e-30
        rows.append(("depth target" if from_depth else "stored target", float((np.abs(got.cpu().numpy().astype(np.float64) - want) / bound).max())))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--trace", action="store_true", help="run only the forward and backward launches, for a kernel trace")
    ap.add_argument("--trace-calls", type=int, default=30)
    ap.add_argument("--kernel-stats", metavar="CSV", help="kernel_stats.csv of the --trace run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_loss_grad.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("normal_grad_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    if a.trace:
        return trace(a, dev)
    from vdn import normals as N
    rt = N._runtime_for(dev)
    T, H, W = a.frames, a.size, a.size
    pool, px = make_pool(T, H, W, dev)
    sets = len(pool)
    at = lambda i: pool[i % sets]
    counts, one = saved_counts(rt, pool, dev), torch.ones(1, dtype=torch.float64, device=dev)
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    crit = N.VideoNormalLoss()
    leaves = [s["pred"].clone().requires_grad_() for s in pool]
    leaves4 = [s["p4"].clone().requires_grad_() for s in pool]

    def both(i, from_depth):
        q = leaves[i % sets]
        q.grad = None
        fn = crit.forward_from_depth if from_depth else crit
        fn(q, at(i)["depth" if from_depth else "target"], at(i)["mask"])["normal_loss"].backward()

    def torch_both(i, from_depth):
        q = leaves4[i % sets]
        q.grad = None
        tgt = torch_target(at(i)["d3"]) if from_depth else at(i)["t4"]
        torch_restatement(q, tgt, at(i)["mask"][0]).backward()

    S = lambda fn: sample_us(fn, a.warmup, a.iters, a.batch)
    t = dict(
        fwd_stored=S(lambda i: rt.normal_eval(at(i)["p4"], at(i)["t4"], at(i)["m8"], out)),
        fwd_depth=S(lambda i: rt.normal_eval(at(i)["p4"], at(i)["d3"], at(i)["m8"], out)),
        bwd_stored=S(lambda i: rt.normal_loss_backward(at(i)["p4"], at(i)["t4"], at(i)["m8"], counts[i % sets], one, at(i)["grad"])),
        bwd_depth=S(lambda i: rt.normal_loss_backward(at(i)["p4"], at(i)["d3"], at(i)["m8"], counts[i % sets], one, at(i)["grad"])),
        both_stored=S(lambda i: both(i, False)),
        both_depth=S(lambda i: both(i, True)),
        torch_stored=sample_us(lambda i: torch_both(i, False), 3, max(5, a.iters // 2), 3),
        torch_depth=sample_us(lambda i: torch_both(i, True), 3, max(5, a.iters // 2), 3),
    )
    src = [torch.empty(BYTES["fwd_depth"] * px, dtype=torch.uint8, device=dev).random_(0, 255) for _ in range(sets)]
    dst = torch.empty_like(src[0])
    t["copy"] = S(lambda i: dst.copy_(src[i % sets]))
    copy_rate = 2 * BYTES["fwd_depth"] * px / t["copy"][0] / 1e6          # TB/s

    # the float32 restatement's gradient against the device's, on the first set
    rel = {}
    for from_depth in (False, True):
        both(0, from_depth)
        ours = leaves[0].grad.view(T, 3, H, W).double()
        torch_both(0, from_depth)
        ref = leaves4[0].grad.double()
        rel[from_depth] = float(((ours - ref).norm() / ours.norm()).item())
    ratios = bound_ratio(dev, H, W)
    kern = kernel_rows(a.kernel_stats) if a.kernel_stats else {}

    f3 = lambda v: f"{v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})"
    tbs = lambda us, b: b * px / us / 1e6
    row = lambda what, key: (f"| {what}, {BYTES[key]} B/pixel = {BYTES[key] * px / 1e6:.0f} MB | {f3(t[key])} | {tbs(t[key][0], BYTES[key]):.2f} | "
                             f"{tbs(t[key][0], BYTES[key]) * 1e12 / HBM_MEASURED:.0%} |")
    lines = [
        "# vdn.normals: VideoNormalLoss with its gradient on the device",
        "",
        f"Written by `tools/normal_grad_bench.py` on {torch.cuda.get_device_name(0)}. Device events around {a.batch} calls, "
        f"{a.warmup} warm-up calls,",
        f"median (min .. max) of {a.iters} samples, in microseconds per call. Every call works on the next of {sets} copies of the",
        "inputs, which together exceed the Infinity Cache twice over, so the inputs come from HBM. Bandwidth is the compulsory",
        f"traffic over the time; the share is of {HBM_MEASURED / 1e12:.2f} TB/s (a float4 copy measured on this part; the copy below reached "
        f"{copy_rate:.2f} TB/s in this run).",
        "",
        f"## [1, {T}, {H}, {W}]: {px / 1e6:.2f} M pixels",
        "",
        "### One launch, by device events (launch overhead included)",
        "",
        "| What | us per call | TB/s | of measured HBM rate |",
        "|---|---|---|---|",
        row("`vdn_normal_eval` (partials + finalise), stored target", "fwd_stored"),
        row("`vdn_normal_loss_backward`, stored target", "bwd_stored"),
        row("`vdn_normal_eval` (partials + finalise), target from depth", "fwd_depth"),
        row("`vdn_normal_loss_backward`, target from depth", "bwd_depth"),
        f"| device-to-device copy of {BYTES['fwd_depth'] * px / 1e6:.0f} MB (reads + writes = 2 x) | {f3(t['copy'])} | {copy_rate:.2f} | "
        f"{copy_rate * 1e12 / HBM_MEASURED:.0%} |",
        "",
        f"Backward over forward: {t['bwd_stored'][0] / t['fwd_stored'][0]:.2f} x with a stored target, "
        f"{t['bwd_depth'][0] / t['fwd_depth'][0]:.2f} x with a depth target.",
        "",
        "### The kernels alone",
        "",
    ]
    if kern:
        lines += [f"`rocprofv3 --kernel-trace --stats` of `tools/normal_grad_bench.py --trace` (a run of its own; warm-up launches included):", "",
                  "| kernel | calls | avg us | min us | max us |", "|---|---:|---:|---:|---:|"]
        lines += [f"| `{n[:90]}` | {c} | {av:.1f} | {mn:.1f} | {mx:.1f} |" for n, (c, av, mn, mx) in sorted(kern.items())] + [""]
    else:
        lines += ["Not measured: no kernel trace was handed to this run (`--kernel-stats`).", ""]
    lines += [
        "### forward + backward() through autograd",
        "",
        "| What | us per call |",
        "|---|---|",
        f"| `VideoNormalLoss()(p, target, mask)['normal_loss'].backward()` | {f3(t['both_stored'])} |",
        f"| float32 torch restatement of the same (conv2d erosion, `F.cosine_similarity`, autograd) | {f3(t['torch_stored'])} |",
        f"| `VideoNormalLoss().forward_from_depth(p, depth, mask)['normal_loss'].backward()` | {f3(t['both_depth'])} |",
        f"| float32 torch restatement, the target made from depth by torch ops first | {f3(t['torch_depth'])} |",
        "",
        f"Against the restatement: {t['torch_stored'][0] / t['both_stored'][0]:.1f} x with a stored target, "
        f"{t['torch_depth'][0] / t['both_depth'][0]:.1f} x from depth. The restatement's float32 gradient differs from the device's by "
        f"{rel[False]:.1e} (rel-L2, stored target) and {rel[True]:.1e} (from depth); it is a yardstick for time, the oracle is "
        "`tests/normal_grad_ref.py`.",
        "",
        "## The device against the restatement at size",
        "",
        f"Largest `|got - want| / (2^-23 |want| + 2^-40 mag + 1e-30)` at [1, 2, {H}, {W}], the bar of `tests/test_gpu_normal_grad.py` (1 is the",
        "bar; 0.5 is one float32 rounding):",
        "",
        "| case | largest ratio to the bound |",
        "|---|---|",
    ] + [f"| {n} | {v:.3f} |" for n, v in ratios]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
