#!/usr/bin/env python3
"""Time the depth criterion with its gradient (vdn.loss) on one MI355X and write profiles/depth_loss_grad.md.

For [1, 32, 518, 518] and [4, 16, 224, 224] (prediction, target and a bool mask resident on the GPU):
  * VideoDepthLoss.forward without a gradient, forward + backward through autograd (criterion(p, t, k)["total_loss"]
    .backward() on a leaf that requires a gradient), and the backward launch alone on saved state;
  * the torch-ops composition of tools/loss_bench.py (imported) under autograd on the same device, forward + backward, and how
    far its float32 gradient is from the device's, over all pixels and with the pixels that hold a frame's median left out
    (torch.median passes a frame's whole g_m to one pixel, so one frame whose float32 median lands elsewhere moves the norm);
  * a device-to-device copy, for the rate a read of the inputs can reach.
Each timed call works on the next of `sets` copies of the inputs, enough of them that together they exceed the 256 MiB
Infinity Cache twice over, so a call reads from HBM. A sample is the time of `--batch` calls between two device events,
divided by the batch; the figure is the median (min .. max) of `--iters` samples after `--warmup` calls.

The split by pass comes from a kernel trace, which slows the host and therefore runs on its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/loss_grad_bench.py --trace
(the backward launch alone, at the first shape), and its kernel_stats.csv is handed to the timing run as --kernel-stats CSV.
Without it the profile says that the split was not measured.

Correctness at size: the device against the restatement tests/loss_grad_ref.py at [1, 2, 518, 518], the benchmark's frame
(H * W a multiple of 4, W not: quads that span a row's end), by the per-element bound of tests/test_gpu_loss_grad.py, and the
same on that file's 14 recorded cases and its oracle-only ones. Reports, not gates. This tool writes the whole file, the
section on the dropped recompute form included: those figures were measured by this tool while the library still held both
forms and are kept here as constants."""
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

from loss_bench import torch_composition  # noqa: E402
from normal_bench import HBM_MEASURED, sample_us  # noqa: E402

# The recompute form (every pass evaluates the stencil again; workspace a function of B and T alone), measured by this tool,
# alternately with the plane form in one process, before it was dropped: shape -> us (forward + backward, backward alone,
# the same two for the plane form in that run), and the kernels of one launch at the first shape.
RECOMPUTE = {(1, 32, 518, 518): (939.1, 678.5, 628.1, 379.8), (4, 16, 224, 224): (502.7, 303.3, 373.4, 179.9)}
RECOMPUTE_KERNELS = (("grad_stats_kernel", 186.8, 217.5), ("grad_solve1_kernel", 14.9, 15.0), ("grad_fit_partial_kernel", 225.6, 98.9),
                     ("grad_solve2_kernel", 21.4, 21.7), ("grad_write_kernel", 235.1, 29.6))


def make_pool(shape, dev):
    import loss_ref as R
    c = R.make_case(9, shape, 0.8)
    once = 9 * int(np.prod(shape))
    sets = max(2, math.ceil(2 * 256 * 2 ** 20 / once))
    base = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
    return [{k: v.clone() for k, v in base.items()} for _ in range(sets)], once


def saved_state(pool):
    """Per set, what the autograd function saves: the forward's launch with its per-frame outputs, and copies of the state."""
    from vdn import loss as L
    out = []
    for s in pool:
        rt, res, ss, p, t, m = L._launch(s["pred"], s["target"], s["mask"], 0.5, 4, 10.0, "cuda", True, state=True)
        out.append((rt, p, t, m, ss, res.clone()))
    return out


def backward_alone(state, coeff):
    from vdn import loss as L
    rt, p, t, m, ss, res = state
    return L._backward(rt, p, t, m, 0.5, 4, 10.0, ss, res, coeff)


def trace(shape, dev, calls):
    pool, _ = make_pool(shape, dev)
    states = saved_state(pool)
    coeff = torch.tensor([1.0, 10.0, 0.0], device=dev)
    for i in range(calls):
        backward_alone(states[i % len(states)], coeff)
    torch.cuda.synchronize()
    print(f"traced {calls} backward launches, shape {list(shape)}")


def time_shape(shape, a, dev):
    from vdn import loss as L
    pool, once = make_pool(shape, dev)
    sets = len(pool)
    crit = L.VideoDepthLoss()
    leaves = [s["pred"].clone().requires_grad_() for s in pool]
    coeff = torch.tensor([1.0, 10.0, 0.0], device=dev)
    at = lambda i: pool[i % sets]

    def fwd_bwd(i):
        q = leaves[i % sets]
        q.grad = None
        crit(q, at(i)["target"], at(i)["mask"])["total_loss"].backward()

    def torch_fwd_bwd(i):
        q = leaves[i % sets]
        q.grad = None
        torch_composition(q, at(i)["target"], at(i)["mask"])[4].backward()

    states = saved_state(pool)
    t = dict(forward=sample_us(lambda i: crit(at(i)["pred"], at(i)["target"], at(i)["mask"]), a.warmup, a.iters, a.batch),
             both=sample_us(fwd_bwd, a.warmup, a.iters, a.batch),
             bwd=sample_us(lambda i: backward_alone(states[i % sets], coeff), a.warmup, a.iters, a.batch),
             torch_ops=sample_us(torch_fwd_bwd, 2, max(3, a.iters // 4), 2))
    got = backward_alone(states[0], coeff).double()
    q = leaves[0]
    q.grad = None
    torch_composition(q, pool[0]["target"], pool[0]["mask"])[4].backward()
    ref = q.grad.double()
    # the pixels that hold a frame's median on the device's side: kept, and a == m (the forward's float32 fit and medians)
    rt, p, tt, m, ss, res = states[0]
    B, T = shape[:2]
    aligned = ss[:, 0].view(B, 1, 1, 1) * p + ss[:, 1].view(B, 1, 1, 1)
    med = res[L.OUT_SLOTS:L.OUT_SLOTS + 4 * B * T].view(B, T, 4)[..., 0].float().view(B, T, 1, 1)
    holders = (aligned == med) & (m != 0)
    rel = float(((got - ref).norm() / ref.norm()).item())
    rest = ~holders
    rel_rest = float((((got - ref) * rest).norm() / (ref * rest).norm()).item())
    at_holders = float(((got - ref) * holders).abs().max().item())
    src = [torch.empty(once, dtype=torch.uint8, device=dev).random_(0, 255) for _ in range(sets)]
    dst = torch.empty_like(src[0])
    t["copy"] = sample_us(lambda i: dst.copy_(src[i % sets]), a.warmup, a.iters, a.batch)
    return dict(shape=shape, px=int(np.prod(shape)), sets=sets, once=once, t=t, torch_rel=rel, torch_rel_rest=rel_rest,
                holders=int(holders.sum().item()), at_holders=at_holders, gmax=float(got.abs().max().item()))


def bound_ratios(dev):
    """-> rows (case, largest |device - restatement| / bound) for the cases of tests/test_gpu_loss_grad.py."""
    import test_gpu_loss_grad as TG
    from test_loss_grad_host import oracle
    from test_loss_host import CASES, case_id
    from vdn import loss as L
    rows = []
    todo = [(case_id(c), oracle(i), dict(alpha=c["alpha"], stable_scale=c["stable_scale"])) for i, c in enumerate(CASES)]
    todo += [(n, TG.extra(n), {}) for n in TG.EXTRA]
    import loss_grad_ref as G
    import loss_ref as R
    big = R.make_case(9, (1, 2, 518, 518), 0.8)
    todo.append(("[1, 2, 518, 518] (the benchmark's frame, seed 9)", (big, G.depth_loss_grad_ref(big["pred"], big["target"], big["mask"])), {}))
    for name, (case, r), kw in todo:
        got = L.depth_loss_grad(*(torch.from_numpy(np.array(case[k])).to(dev) for k in ("pred", "target", "mask")), **kw)
        rows.append((name, TG.ratio_to_bound(got.cpu().numpy(), r)))
    return rows


def kernel_table(path):
    rows = [r for r in csv.DictReader(open(path)) if "grad_" in r["Name"]]
    tot = sum(float(r["TotalDurationNs"]) / int(r["Calls"]) for r in rows)
    lines = ["| kernel | calls | avg us | min us | max us | share of the launch |", "|---|---:|---:|---:|---:|---:|"]
    for r in sorted(rows, key=lambda r: r["Name"]):
        name = re.sub(r"\(.*", "", re.sub(r"\(anonymous namespace\)::", "", r["Name"]))[:80]
        lines.append(f"| `{name}` | {r['Calls']} | {float(r['AverageNs']) / 1e3:.1f} | {float(r['MinNs']) / 1e3:.1f} | "
                     f"{float(r['MaxNs']) / 1e3:.1f} | {float(r['AverageNs']) / tot:.0%} |")
    lines.append(f"| the five kernels of one launch | | {tot / 1e3:.1f} | | | |")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 32, 518, 518, 4, 16, 224, 224])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--trace", action="store_true", help="run only the backward launch, for a kernel trace")
    ap.add_argument("--trace-calls", type=int, default=30)
    ap.add_argument("--kernel-stats", metavar="CSV", help="kernel_stats.csv of the --trace run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_loss_grad.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_grad_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    shapes = [tuple(a.shapes[i:i + 4]) for i in range(0, len(a.shapes), 4)]
    if a.trace:
        return trace(shapes[0], dev, a.trace_calls)
    results = [time_shape(s, a, dev) for s in shapes]
    ratios = bound_ratios(dev)

    f3 = lambda t: f"{t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f})"
    lines = [
        "# vdn.loss: VideoDepthLoss with its gradient on the device",
        "",
        f"Written by `tools/loss_grad_bench.py` on {torch.cuda.get_device_name(0)}. Device events around {a.batch} calls, "
        f"{a.warmup} warm-up calls,",
        f"median (min .. max) of {a.iters} samples, in microseconds per call. Every call works on the next of several copies of",
        "the inputs (column `sets`), which together exceed the Infinity Cache twice over, so the inputs come from HBM.",
        f"A read of the inputs is 9 B per pixel (prediction, target, mask); measured float4 copy {HBM_MEASURED / 1e12:.2f} TB/s.",
        "",
    ]
    for r in results:
        t = r["t"]
        read = t["copy"][0] / 2
        lines += [
            f"## {list(r['shape'])}: {r['px'] / 1e6:.2f} M pixels, {r['sets']} sets",
            "",
            "| What | us per call | reads of the inputs at the copy's rate |",
            "|---|---|---|",
            f"| `VideoDepthLoss.forward`, no gradient recorded | {f3(t['forward'])} | {t['forward'][0] / read:.1f} |",
            f"| forward + backward through autograd | {f3(t['both'])} | {t['both'][0] / read:.1f} |",
            f"| the backward launch alone (5 kernels) | {f3(t['bwd'])} | {t['bwd'][0] / read:.1f} |",
            f"| torch-ops composition of the same steps under autograd, float32, forward + backward | {f3(t['torch_ops'])} | {t['torch_ops'][0] / read:.1f} |",
            f"| device-to-device copy of {r['once'] / 1e6:.0f} MB (reads + writes = 2 x) | {f3(t['copy'])} | 2.0 |",
            "",
            f"Forward + backward against the torch-ops composition: {t['torch_ops'][0] / t['both'][0]:.1f} x. One read of the inputs at the "
            f"copy's rate takes {read:.1f} us. The composition's float32 gradient differs from the device's by {r['torch_rel']:.1e} "
            f"(rel-L2) over all pixels and by {r['torch_rel_rest']:.1e} with the {r['holders']} pixels that hold a frame's median left out; at "
            f"those pixels the largest difference is {r['at_holders']:.2e}, the largest component of the gradient {r['gmax']:.2e}. The "
            "composition sums every pixel in float32 and is a yardstick for time; the oracle is `tests/loss_grad_ref.py`, below.",
            "",
        ]
    lines += ["## The backward launch by pass", ""]
    if a.kernel_stats:
        lines += [f"`rocprofv3 --kernel-trace --stats` of `tools/loss_grad_bench.py --trace` at {list(shapes[0])} (a run of its own; "
                  "warm-up launches included):", ""] + kernel_table(a.kernel_stats) + [""]
    else:
        lines += ["Not measured: no kernel trace was handed to this run (`--kernel-stats`).", ""]
    lines += [
        "## Recompute or plane: the measurement behind the choice",
        "",
        "Passes 3 and 5 need g_x again. `plane` (what the library does): pass 1 leaves g_x in an fp64 plane of the workspace, 8 B per",
        "pixel. `recompute`: every pass evaluates the stencil again from the inputs and the workspace depends on B and T alone.",
        "Both were in the library, selected per call, when this tool timed them alternately in one process (same method as above;",
        "their gradients were bit-equal); the recompute form was then dropped. Those figures, kept as constants in the tool, in",
        "microseconds:",
        "",
        "| shape | forward + backward, recompute | plane | the backward alone, recompute | plane |",
        "|---|---|---|---|---|",
    ] + [f"| {list(k)} | {v[0]:.1f} | {v[2]:.1f} | {v[1]:.1f} | {v[3]:.1f} |" for k, v in RECOMPUTE.items()] + [
        "",
        f"By kernel at {list(next(iter(RECOMPUTE)))}, average of 30 traced launches:",
        "",
        "| kernel | recompute | plane |",
        "|---|---|---|",
    ] + [f"| `{n}` | {x:.1f} | {y:.1f} |" for n, x, y in RECOMPUTE_KERNELS] + [""]
    worst = max(v for _, v in ratios)
    lines += [
        "## The device against the restatement",
        "",
        "Largest `|got - want| / (4 * 2^-24 * (|sc * g_a| + |fit correction|) + 1e-30)` per case, the bar of",
        f"`tests/test_gpu_loss_grad.py` (1 is the bar; 0.25 is one float32 rounding); the largest over all cases is {worst:.3f}.",
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
