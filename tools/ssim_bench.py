#!/usr/bin/env python3
"""Time the SSIM term of the depth criterion (vdn.loss, csrc/ssim.hip) on one MI355X and write profiles/ssim_loss.md.

For [1, 32, 518, 518] and [2, 32, 518, 518] (prediction, target and a bool mask resident on the GPU):
  * DepthShallowSSIMLoss and SSIMVideoDepthLoss(ssim_loss_scale=0.1): forward without a gradient, and forward + backward
    through autograd (total_loss.backward() on a leaf that requires a gradient); the term's backward launch alone on saved
    state;
  * VideoDepthLoss at the same shape, forward and forward + backward: what the composite costs without the term;
  * the same statements in torch float32 ops on the same device (level 0 of the restated MS_SSIM; the four pooled levels,
    which are factors of exactly 1, are left out in its favour), autograd for the gradient, and how far its value and
    gradient are from the device's;
  * the byte floor: two float32 planes read once and one written, at the rate a float4 copy reaches on this part.
Each timed call works on the next of `sets` copies of the inputs, enough of them that together they exceed the 256 MiB
Infinity Cache twice over. A sample is the time of `--batch` calls between two device events, divided by the batch; the figure
is the median (min .. max) of `--iters` samples after `--warmup` calls.

The split by kernel comes from a kernel trace, which runs on its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ssim_bench.py --trace
(forward and backward of the term alone, at the first shape); its kernel_stats.csv is handed to the timing run as
--kernel-stats CSV. Without it the profile says that the split was not measured.

Also written: the fp64 floor of the gradient (tests/ssim_ref.fp64_floor: the two summation orders against each other) on the
cases of tests/test_gpu_ssim.py and of the fixture, the float32-against-float64 yardstick the fixture records, and the device
against the restatement on those cases. Reports, not gates."""
import argparse
import csv
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

from normal_bench import HBM_MEASURED, sample_us  # noqa: E402

SHAPES = ((1, 32, 518, 518), (2, 32, 518, 518))
# The first form of the folds, measured by this tool before it was replaced: one lane per frame (forward) or per item (the two
# solves of the backward) walked every tile's row in turn. shape -> us (forward, backward alone), and the kernels of one
# forward and one backward launch at the first shape.
# What was checked once when the fit's correction moved into loss_px.hpp; kept as text, this tool does not measure it.
LIFTED = "## The fit's correction, written once\n\nThe per-pixel correction through the fit is `FitGrad` of csrc/loss_px.hpp, used by loss_grad.hip's write pass and by ssim.hip's. `tools/criteria_dump.py` on the parent's build and on this one, same machine: all 253 files of the existing criteria (loss, its fit alone, trimmed, their two backward passes, normals, eval, metric, silog) are byte-identical; the 40 new files are the SSIM term's. Compiled for the device alone, loss_grad.hip's assembly has the parent's instructions but for the order of five scalar loads and two conversions in `grad_write_kernel`'s prologue.\n"
ONE_LANE = {(1, 32, 518, 518): (424.8, 3494.2), (2, 32, 518, 518): (594.5, 4408.2)}
ONE_LANE_KERNELS = (("fit_solve_kernel", 1594.8), ("hold_solve_kernel", 1436.4), ("adjoint_kernel", 243.4), ("max_solve_kernel", 196.9),
                    ("tile_kernel<true>", 183.5), ("tile_kernel<false>", 167.8), ("finish_kernel", 54.3), ("write_kernel<4, true, false>", 33.0),
                    ("max_partial_kernel<4, true>", 20.2))


def torch_ssim(pred, target, mask):
    """loss/loss.py:296-323 on level 0 of the restated MS_SSIM, in float32 torch ops."""
    from vdn.loss import SSIM_WINDOW
    B, S, H, W = pred.shape
    pm = (pred * mask).view(B, -1).max(dim=1, keepdim=True)[0]
    tm = (target * mask).view(B, -1).max(dim=1, keepdim=True)[0]
    mv = torch.clamp(torch.max(pm, tm), min=1e-8).view(B, 1, 1, 1)
    x, y = (pred / mv).view(B * S, 1, H, W), (target / mv).view(B * S, 1, H, W)
    win = torch.tensor(SSIM_WINDOW, dtype=torch.float32, device=pred.device)
    f = lambda z: Fn.conv2d(Fn.conv2d(z, win.view(1, 1, 11, 1)), win.view(1, 1, 1, 11))
    mu1, mu2 = f(x), f(y)
    s1, s2, s12 = f(x * x) - mu1 * mu1, f(y * y) - mu2 * mu2, f(x * y) - mu1 * mu2
    cs = ((2 * s12 + 0.03 ** 2) / (s1 + s2 + 0.03 ** 2)).flatten(2).mean(-1)
    return 1.0 - torch.relu(cs).mean()


def make_pool(shape, dev):
    import ssim_ref as S
    c = S.make_case(7, (1, 2) + shape[2:], 0.875, gain=1.5)        # two frames, tiled over the clip: the time does not depend on the data
    reps = (shape[0], shape[1] // 2, 1, 1)
    base = {k: torch.from_numpy(v).to(dev).repeat(*reps).contiguous() for k, v in c.items()}
    once = 9 * int(np.prod(shape))
    sets = max(2, math.ceil(2 * 256 * 2 ** 20 / once))
    return [{k: v.clone() for k, v in base.items()} for _ in range(sets)], once


def saved_state(pool):
    from vdn import loss as L
    out = []
    for s in pool:
        rt, p, t, m, _ = L._ssim_stage(s["pred"], s["target"], s["mask"], "cuda", False)
        out.append((rt, p, t, m, L._ssim_launch(rt, p, t, m, None)))
    return out


def term_backward(state, coeff, grad):
    from vdn import loss as L
    rt, p, t, m, st = state
    return L._ssim_backward(rt, p, t, m, None, st, coeff, grad, False)


def trace(shape, dev, calls):
    from vdn import loss as L
    pool, _ = make_pool(shape, dev)
    states = saved_state(pool)
    coeff, grad = torch.ones(1, device=dev), torch.empty_like(pool[0]["pred"])
    for i in range(calls):
        rt, p, t, m, _ = states[i % len(pool)]
        L._ssim_launch(rt, p, t, m, None)
        term_backward(states[i % len(pool)], coeff, grad)
    torch.cuda.synchronize()
    print(f"traced {calls} forward and backward launches, shape {list(shape)}")


def time_shape(shape, a, dev):
    from vdn import _abi, loss as L
    pool, once = make_pool(shape, dev)
    sets = len(pool)
    at = lambda i: pool[i % sets]
    leaves = [s["pred"].clone().requires_grad_() for s in pool]
    fmask = [s["mask"].float() for s in pool]
    term, whole, rest = L.DepthShallowSSIMLoss(), L.SSIMVideoDepthLoss(ssim_loss_scale=0.1), L.VideoDepthLoss()
    states = saved_state(pool)
    coeff, grad = torch.ones(1, device=dev), torch.empty_like(pool[0]["pred"])

    def both(value):
        def run(i):
            q = leaves[i % sets]
            q.grad = None
            value(q, i).backward()
        return run

    run = lambda fn, slow=False: sample_us(fn, 2 if slow else a.warmup, max(3, a.iters // 4) if slow else a.iters, 2 if slow else a.batch)
    with torch.no_grad():
        t = dict(term_fwd=run(lambda i: term(at(i)["pred"], at(i)["target"], at(i)["mask"])),
                 whole_fwd=run(lambda i: whole(at(i)["pred"], at(i)["target"], at(i)["mask"])),
                 rest_fwd=run(lambda i: rest(at(i)["pred"], at(i)["target"], at(i)["mask"])),
                 torch_fwd=run(lambda i: torch_ssim(at(i)["pred"], at(i)["target"], fmask[i % sets]), True))
    t.update(term_both=run(both(lambda q, i: term(q, at(i)["target"], at(i)["mask"]))),
             whole_both=run(both(lambda q, i: whole(q, at(i)["target"], at(i)["mask"])["total_loss"])),
             rest_both=run(both(lambda q, i: rest(q, at(i)["target"], at(i)["mask"])["total_loss"])),
             term_bwd=run(lambda i: term_backward(states[i % sets], coeff, grad)),
             torch_both=run(both(lambda q, i: torch_ssim(q, at(i)["target"], fmask[i % sets])), True))
    # the device against the float32 torch composition, at size
    q = leaves[0]
    q.grad = None
    v_t = torch_ssim(q, pool[0]["target"], fmask[0])
    v_t.backward()
    g_t = q.grad.double()
    g_d = L.ssim_loss_grad(pool[0]["pred"], pool[0]["target"], pool[0]["mask"]).double()
    v_d = L.ssim_loss(pool[0]["pred"], pool[0]["target"], pool[0]["mask"])["ssim_loss"]
    agree = (abs(v_d - float(v_t.detach())), float(((g_d - g_t) ** 2).sum().sqrt() / (g_d ** 2).sum().sqrt()))
    B, T, H, W = shape
    ws = (int(_abi.lib.vdn_ssim_loss_workspace_bytes(*shape)), int(_abi.lib.vdn_ssim_loss_backward_workspace_bytes(*shape)))
    return dict(shape=shape, t=t, sets=sets, once=once, floor_us=12.0 * B * T * H * W / HBM_MEASURED * 1e6, agree=agree, ws=ws)


def kernel_split(path):
    """-> (kernel, calls, average us) of a --trace run's kernel_stats.csv: every kernel of it is one of csrc/ssim.hip's."""
    import re
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = re.sub(r"\(.*", "", re.sub(r"\(anonymous namespace\)::", "", r["Name"]))[:60]
            rows.append((name, int(r["Calls"]), float(r["AverageNs"]) / 1e3))
    return sorted(rows, key=lambda r: -r[2])


def floors():
    """-> rows (case, floor, device-vs-restatement ratio to the bound) for the test's cases, and the fixture's rows."""
    import ssim_ref as S
    import test_gpu_ssim as T
    import test_ssim_host as Hs
    from vdn import loss as L
    rows = []
    for name, (_, aligned, _, _) in T.CASES.items():
        c, fit, r, floor = T.oracle(name)
        g = L.ssim_loss_grad(*(T.dev(c[n]) for n in ("pred", "target", "mask")), aligned=aligned).cpu().numpy()
        v = L.ssim_loss(*(T.dev(c[n]) for n in ("pred", "target", "mask")), aligned=aligned)
        raw = S.fp64_floor(c["pred"], c["target"], c["mask"], fit)
        rows.append((name, "x".join(map(str, c["pred"].shape)), raw, abs(v["ssim_loss"] - r["fwd"]["loss"]), T.ratio_to_bound(g, r, floor)))
    fix = []
    for name in Hs.NAMES:
        c = Hs.case(name)
        fix.append((name, "x".join(map(str, c["pred"].shape)), S.fp64_floor(c["pred"], c["target"], c["mask"]),
                    S.fp64_floor(c["pred"], c["target"], c["mask"], Hs.whole(name)["fit"], float(Hs.Z["ssim_scale"])),
                    tuple(float(x) for x in Hs.Z[f"{name}_alone_yardstick"]), tuple(float(x) for x in Hs.Z[f"{name}_whole_yardstick"])))
    return rows, fix


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--trace", action="store_true", help="only make launches for a kernel trace")
    ap.add_argument("--kernel-stats", help="kernel_stats.csv of a --trace run under rocprofv3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_loss.md"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from vdn import loss as L
    if a.trace:
        trace(SHAPES[0], dev, 6)
        return
    res = [time_shape(s, a, dev) for s in SHAPES]
    rows, fix = floors()
    us = lambda v: f"{v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})"
    th, tw = L.ssim_tile()
    o = ["# The SSIM term of the depth criterion: time, floor and yardstick", "",
         f"`python tools/ssim_bench.py --iters {a.iters} --warmup {a.warmup} --batch {a.batch}` on one MI355X; microseconds per call, median "
         "(min .. max) of the samples, a sample being the mean of a batch of calls between two device events; inputs cycled through "
         "sets that exceed the Infinity Cache twice over. Tile of the kernels: "
         f"{th} x {tw} outputs. The torch rows are level 0 of the restated MS_SSIM in float32 torch ops on the same device, "
         "autograd for the gradient.", ""]
    for r in res:
        t, B = r["t"], r["shape"][0]
        o += [f"## {list(r['shape'])}  ({r['sets']} sets of {r['once'] / 2 ** 20:.0f} MiB)", "",
              "| what | us | against torch | against the byte floor |", "|---|---|---|---|"]
        for key, label, ref in (("term_fwd", "DepthShallowSSIMLoss forward", "torch_fwd"), ("term_both", "DepthShallowSSIMLoss forward + backward", "torch_both"),
                                ("term_bwd", "vdn_ssim_loss_backward alone", None), ("whole_fwd", "SSIMVideoDepthLoss forward", None),
                                ("whole_both", "SSIMVideoDepthLoss forward + backward", None), ("rest_fwd", "VideoDepthLoss forward", None),
                                ("rest_both", "VideoDepthLoss forward + backward", None), ("torch_fwd", "torch composition forward", None),
                                ("torch_both", "torch composition forward + backward", None)):
            o.append(f"| {label} | {us(t[key])} | {(f'{t[ref][0] / t[key][0]:.2f}x faster' if ref else '')} | {t[key][0] / r['floor_us']:.1f}x |")
        o += ["", f"Byte floor (two float32 planes read, one written, at {HBM_MEASURED / 1e12:.2f} TB/s): {r['floor_us']:.1f} us. "
              f"The term adds {t['whole_fwd'][0] - t['rest_fwd'][0]:.1f} us to the criterion's forward and "
              f"{t['whole_both'][0] - t['rest_both'][0]:.1f} us to forward + backward. Workspace: forward {r['ws'][0] / 2 ** 20:.1f} MiB, "
              f"backward {r['ws'][1] / 2 ** 20:.1f} MiB.",
              f"Device against the float32 torch composition at this size: value {r['agree'][0]:.2e}, gradient rel-L2 {r['agree'][1]:.2e}.", ""]
    o += ["## The backward's form", "",
          "The backward keeps fp64 planes: the forward's tile kernel runs again and leaves P, Q and N over the outputs (3 planes), the "
          "adjoint reads them with a halo of 10 and leaves g_a (1 plane) for the write pass, which needs the item-wide sums G0 and G1 "
          "first. The other form, an adjoint that recomputes the output maps from the inputs with a halo of 20 and no planes, was NOT "
          "built, so there is no measurement of it here: at a 16 x 32 tile it evaluates the moments on 36 x 52 inputs per 512 pixels, "
          "3.7 times the forward's filtering, against 32 bytes per pixel written and read by the plane form. The per-kernel split "
          "below is what a comparison would start from.", ""]
    if a.kernel_stats:
        o += ["| kernel | calls | average us |", "|---|---|---|"] + [f"| `{n}` | {c} | {v:.1f} |" for n, c, v in kernel_split(a.kernel_stats)] + [""]
    else:
        o += ["The split by kernel was not measured in this run (see the tool's text for the rocprofv3 command).", ""]
    o += ["## The folds", "",
          "A frame's tiles (512 of outputs, 561 of pixels at 518 x 518) are added by one block per frame, a lane taking the tiles "
          "lane, lane + 256, .. and the lanes joined as reduce.hpp states; the one-block solves then walk an item's frames. The "
          "first form had one lane per frame (forward) or per item (the backward's two solves) walk every tile in turn, a chain of "
          "dependent loads: measured then, with this tool,", "",
          "| shape | forward then | forward now | backward alone then | backward alone now |", "|---|---|---|---|---|"]
    o += [f"| {list(r['shape'])} | {ONE_LANE[r['shape']][0]:.1f} | {r['t']['term_fwd'][0]:.1f} | {ONE_LANE[r['shape']][1]:.1f} | {r['t']['term_bwd'][0]:.1f} |"
          for r in res if r["shape"] in ONE_LANE]
    o += ["", "and per kernel at the first shape then: " + ", ".join(f"`{n}` {v:.1f}" for n, v in ONE_LANE_KERNELS) + " us.", ""]
    o += ["## The gradient's fp64 floor", "",
          "tests/ssim_ref.fp64_floor: the restatement's gradient with the window applied along H then W against W then H, largest "
          "difference relative to the sum of the magnitudes of the adjoint's parts. tests/test_gpu_ssim.py allows 8 times the case's "
          "own figure on top of the float32 roundings; the last column is the device's largest error over that whole bound.", "",
          "| case | shape | floor | value: device - restatement | gradient: device error / bound |", "|---|---|---|---|---|"]
    o += [f"| {n} | {s} | {f:.2e} | {v:.1e} | {w:.3f} |" for n, s, f, v, w in rows]
    o += ["", "## The yardstick: the reference's float32 run against its float64 run", "",
          "tools/make_golden_ssim.py, recorded in tests/golden/ssim_cases.npz; tests/test_ssim_host.py holds the restatement to four "
          "times each figure. pytorch_msssim itself is restated there (it is not installed): parity with the library's own file is "
          "not pinned.", "",
          "| case | shape | floor alone | floor whole | alone: value, gradient rel-L2 | whole (ssim_loss_scale 0.3): value, gradient rel-L2 |", "|---|---|---|---|---|---|"]
    o += [f"| {n} | {s} | {fa:.2e} | {fw:.2e} | {ya[0]:.2e}, {ya[1]:.2e} | {yw[0]:.2e}, {yw[1]:.2e} |" for n, s, fa, fw, ya, yw in fix]
    o += ["", LIFTED]
    with open(a.out, "w") as f:
        f.write("\n".join(o) + "\n")
    print("\n".join(o))


if __name__ == "__main__":
    main()
