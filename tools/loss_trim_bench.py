#!/usr/bin/env python3
"""Time the trimmed depth criterion (vdn.loss.TrimmedVideoDepthLoss, vdn_depth_loss_trimmed and its backward) on one MI355X and
write profiles/depth_loss_trim.md.

For [2, 32, 518, 518] and [4, 16, 224, 224] (prediction, target and a bool mask resident on the GPU), trim = 0.2:
  * the trimmed forward launch (vdn_depth_loss_trimmed) against the untrimmed vdn_depth_loss of the same build and shape;
  * the trimmed backward launch alone on saved state against the untrimmed one;
  * a torch-ops composition of the trimmed criterion on the same device (tools/loss_bench.py's composition with the
    reference's sort-and-slice per term, len() and its host synchronisation included), forward, and forward + backward under
    autograd; and how far its float32 values are from the device's;
  * a device-to-device copy, for the rate a read of the inputs can reach.
Each timed call works on the next of `sets` copies of the inputs, enough of them that together they exceed the 256 MiB
Infinity Cache twice over, so a call reads from HBM. A sample is the time of `--batch` calls between two device events,
divided by the batch; the figure is the median (min .. max) of `--iters` samples after `--warmup` calls. No time target:
the profile states what the selections add over the untrimmed criterion.

This tool writes the whole file, the section on the selection schemes included. Four schemes were in the library behind one
entry point, selected per call, when this tool timed them in turn, twice over, in one process (same method as above; their
outputs were bit-identical): the keys recomputed by every pass of the select or read from float32 key planes that one sweep
wrote, and one select of three slots or three selects of one slot. The three that lost were then dropped; their figures are
kept here as constants."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from normal_bench import HBM_MEASURED, sample_us  # noqa: E402

TRIM = 0.2
# shape -> the untrimmed launch, then per scheme (first round, second round): medians in us, measured by this tool while the
# library held all four
SCHEMES = ("keys recomputed by every pass, one select of three slots (kept)", "float32 key planes, one select of three slots",
           "keys recomputed by every pass, three selects of one slot", "float32 key planes, three selects of one slot")
MEASURED = {(2, 32, 518, 518): (438.3, ((824.3, 826.7), (882.6, 884.1), (1208.7, 1208.3), (1244.0, 1245.7))),
            (4, 16, 224, 224): (179.7, ((355.4, 354.5), (362.0, 362.1), (522.6, 521.9), (518.7, 518.3)))}


def torch_trimmed(p, t, keep, trim=TRIM, alpha=0.5, scales=4, stable_scale=10.0):
    """tests/loss_trim_ref.depth_loss_trim_ref in torch float32 ops, the selection as the reference does it: sort the counted
    residuals, keep the first int(len * (1 - trim)), divide by the count. -> the five values."""
    B, T, H, W = p.shape
    k = keep.float()
    flat = lambda x: x.flatten(1)
    a00, a01, a11 = flat(k * p * p).sum(1), flat(k * p).sum(1), flat(k).sum(1)
    b0, b1 = flat(k * p * t).sum(1), flat(k * t).sum(1)
    det = a00 * a11 - a01 * a01
    ok = det != 0
    scale = torch.where(ok, (a11 * b0 - a01 * b1) / (det + 1e-6), torch.zeros_like(det))
    shift = torch.where(ok, (-a01 * b0 + a00 * b1) / (det + 1e-6), torch.zeros_like(det))
    a = scale.view(B, 1, 1, 1) * p + shift.view(B, 1, 1, 1)
    n_f = k.sum((2, 3))

    def robust(x):
        m = torch.median((k * x).flatten(2), dim=2).values
        m = torch.where(n_f > 0, m, torch.zeros_like(m))
        x0 = x - m[..., None, None]
        s = torch.where(n_f > 0, ((k * x0.abs()).sum((2, 3)) / n_f.clamp_min(1)).clamp_min(1e-6), torch.ones_like(m))
        return x0 / s[..., None, None]

    def trimmed(res, counted):
        r = res[counted].abs()
        kept = int(len(r) * (1.0 - trim))
        if kept <= 0:
            return p.sum() * 0.0
        return torch.sort(r).values[:kept].sum() / len(r)

    d = k * (robust(a) - robust(t))
    spatial = trimmed(d, keep)
    if alpha > 0:
        for s in range(scales):
            step = 2 ** s
            ds, ks = d[..., ::step, ::step], k[..., ::step, ::step]
            gx = ((ds[..., :, 1:] - ds[..., :, :-1]).abs() * ks[..., :, 1:] * ks[..., :, :-1]).sum()
            gy = ((ds[..., 1:, :] - ds[..., :-1, :]).abs() * ks[..., 1:, :] * ks[..., :-1, :]).sum()
            M = ks.sum()
            spatial = spatial + alpha * torch.where(M > 0, (gx + gy) / M.clamp_min(1), torch.zeros_like(M))
    tmin = torch.where(keep, t, torch.inf).amin((2, 3))
    tmax = torch.where(keep, t, -torch.inf).amax((2, 3))
    th = (tmax - tmin) * 0.05
    pg, tg = a[:, 1:] - a[:, :-1], t[:, 1:] - t[:, :-1]
    k2 = keep[:, 1:] & keep[:, :-1] & (tg.abs() < th[:, 1:, None, None])
    stable = trimmed(pg - tg, k2)
    k3 = keep & (t > 1e-3) & (t < 70)
    absrel = trimmed((a - t) / t, k3)
    n = k.sum()
    hits = (keep & (torch.maximum(a / t, t / a) < 1.25)).sum()
    d1 = torch.where(n > 0, hits / n.clamp_min(1), torch.zeros_like(n))
    return spatial, stable, absrel, d1, spatial + stable_scale * stable


def make_pool(shape, dev):
    import loss_ref as R
    c = R.make_case(9, shape, 0.8)
    once = 9 * int(np.prod(shape))
    sets = max(2, math.ceil(2 * 256 * 2 ** 20 / once))
    base = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
    return [{k: v.clone() for k, v in base.items()} for _ in range(sets)], once


def time_shape(shape, a, dev):
    from vdn import loss as L
    pool, once = make_pool(shape, dev)
    sets = len(pool)
    at = lambda i: pool[i % sets]
    keep = 1.0 - TRIM
    launch = lambda i, **kw: L._launch(at(i)["pred"], at(i)["target"], at(i)["mask"], 0.5, 4, 10.0, "cuda", True, **kw)
    t = {"untrimmed": sample_us(lambda i: launch(i), a.warmup, a.iters, a.batch)}
    t["trimmed"] = sample_us(lambda i: launch(i, keep=keep), a.warmup, a.iters, a.batch)
    coeff = torch.tensor([1.0, 10.0, 0.0], device=dev)
    states = {}
    for name, kw in (("untrimmed", {}), ("trimmed", dict(keep=keep))):
        states[name] = []
        for s in pool:
            rt, res, ss, p, tt, m = L._launch(s["pred"], s["target"], s["mask"], 0.5, 4, 10.0, "cuda", True, state=True, **kw)
            states[name].append((rt, p, tt, m, ss, res.clone()))
    bwd = lambda name, i, k: L._backward(*states[name][i % sets][:4], 0.5, 4, 10.0, *states[name][i % sets][4:], coeff, k)
    t["bwd_untrimmed"] = sample_us(lambda i: bwd("untrimmed", i, 1.0), a.warmup, a.iters, a.batch)
    t["bwd_trimmed"] = sample_us(lambda i: bwd("trimmed", i, keep), a.warmup, a.iters, a.batch)
    crit = L.TrimmedVideoDepthLoss(trim=TRIM)
    leaves = [s["pred"].clone().requires_grad_() for s in pool]

    def both(i):
        q = leaves[i % sets]
        q.grad = None
        crit(q, at(i)["target"], at(i)["mask"])["total_loss"].backward()

    def torch_both(i):
        q = leaves[i % sets]
        q.grad = None
        torch_trimmed(q, at(i)["target"], at(i)["mask"])[4].backward()

    t["both"] = sample_us(both, a.warmup, a.iters, a.batch)
    with torch.no_grad():
        t["torch_fwd"] = sample_us(lambda i: torch_trimmed(at(i)["pred"], at(i)["target"], at(i)["mask"]), 2, max(3, a.iters // 3), 2)
        ref = [float(v) for v in torch_trimmed(pool[0]["pred"], pool[0]["target"], pool[0]["mask"])]
    t["torch_both"] = sample_us(torch_both, 2, max(3, a.iters // 3), 2)
    got = L.depth_loss(pool[0]["pred"], pool[0]["target"], pool[0]["mask"], trim=TRIM)
    keys = ("spatial_loss", "stable_loss", "absRel_loss", "d1", "total_loss")
    src = [torch.empty(once, dtype=torch.uint8, device=dev).random_(0, 255) for _ in range(sets)]
    dst = torch.empty_like(src[0])
    t["copy"] = sample_us(lambda i: dst.copy_(src[i % sets]), a.warmup, a.iters, a.batch)
    return dict(shape=shape, px=int(np.prod(shape)), sets=sets, once=once, t=t, got={k: got[k] for k in keys},
                torch={k: v for k, v in zip(keys, ref)}, sel={k: got[k].tolist() for k in ("trim_k", "trim_less", "trim_tied")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[2, 32, 518, 518, 4, 16, 224, 224])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_loss_trim.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_trim_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    shapes = [tuple(a.shapes[i:i + 4]) for i in range(0, len(a.shapes), 4)]
    results = [time_shape(s, a, dev) for s in shapes]
    f3 = lambda t: f"{t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f})"
    lines = [
        "# vdn.loss: the trimmed depth criterion on the device",
        "",
        f"Written by `tools/loss_trim_bench.py` on {torch.cuda.get_device_name(0)}, trim = {TRIM}. Device events around {a.batch} calls, "
        f"{a.warmup} warm-up calls,",
        f"median (min .. max) of {a.iters} samples, in microseconds per call. Every call works on the next of several copies of",
        "the inputs (column `sets`), which together exceed the Infinity Cache twice over, so the inputs come from HBM.",
        f"A read of the inputs is 9 B per pixel (prediction, target, mask); measured float4 copy {HBM_MEASURED / 1e12:.2f} TB/s.",
        "The forward launches include the per-frame outputs that the backward needs (frame_stats, frame_counts).",
        "",
    ]
    for r in results:
        t = r["t"]
        read = t["copy"][0] / 2
        base = t["untrimmed"][0]
        lines += [f"## {list(r['shape'])}: {r['px'] / 1e6:.2f} M pixels, {r['sets']} sets", "",
                  f"Selection at this shape: k = {r['sel']['trim_k']}, below the threshold {r['sel']['trim_less']}, at it {r['sel']['trim_tied']} "
                  "(data, stable, absRel).", "",
                  "| What | us per call | reads of the inputs at the copy's rate |", "|---|---|---|",
                  f"| `vdn_depth_loss` (untrimmed forward launch) | {f3(t['untrimmed'])} | {t['untrimmed'][0] / read:.1f} |",
                  f"| `vdn_depth_loss_trimmed` (forward launch) | {f3(t['trimmed'])} | {t['trimmed'][0] / read:.1f} |",
                  f"| the untrimmed backward launch alone | {f3(t['bwd_untrimmed'])} | {t['bwd_untrimmed'][0] / read:.1f} |",
                  f"| the trimmed backward launch alone | {f3(t['bwd_trimmed'])} | {t['bwd_trimmed'][0] / read:.1f} |",
                  f"| `TrimmedVideoDepthLoss`, forward + backward through autograd | {f3(t['both'])} | {t['both'][0] / read:.1f} |",
                  f"| torch-ops composition of the trimmed criterion, float32, forward | {f3(t['torch_fwd'])} | {t['torch_fwd'][0] / read:.1f} |",
                  f"| the same under autograd, forward + backward | {f3(t['torch_both'])} | {t['torch_both'][0] / read:.1f} |",
                  f"| device-to-device copy of {r['once'] / 1e6:.0f} MB (reads + writes = 2 x) | {f3(t['copy'])} | 2.0 |", "",
                  f"The trimmed forward against the untrimmed: +{t['trimmed'][0] - base:.1f} us ({t['trimmed'][0] / base:.2f} x). "
                  f"The trimmed backward against the untrimmed: +{t['bwd_trimmed'][0] - t['bwd_untrimmed'][0]:.1f} us. Forward + backward against "
                  f"the torch-ops composition: {t['torch_both'][0] / t['both'][0]:.1f} x. Values, device (fp64 sums) against the composition (float32):",
                  "", "| key | device | torch-ops composition | difference |", "|---|---|---|---|"]
        lines += [f"| {k} | {r['got'][k]:.9g} | {r['torch'][k]:.9g} | {r['got'][k] - r['torch'][k]:+.1e} |" for k in r["got"]]
        lines.append("")
    lines += ["## Key planes or recomputed keys, one sweep or three: the measurement behind the choice", "",
              "The select's three passes need each counted residual's float32 key. `recompute`: every pass evaluates the residuals again",
              "from the inputs (two fp64 divisions and the normalisation per pixel) and the workspace depends on B and T alone. `planes`:",
              "one sweep writes three float32 key planes (12 B per pixel of workspace) that the passes read. `one select`: the three",
              "terms are three slots of one select, so a pass sweeps once; `three selects`: one slot each, three sweeps per pass. All",
              "four were in the library, selected per call, when this tool timed them in turn, twice over, in one process (same method",
              "as above; their outputs, out[40] with the per-frame state, were bit-identical). The first was kept and the others",
              "dropped. Those figures, kept as constants in the tool, forward launch in microseconds (median, first round / second round):",
              "", "| shape | untrimmed | " + " | ".join(SCHEMES) + " |", "|---|---|" + "---|" * len(SCHEMES)]
    lines += [f"| {list(k)} | {v[0]:.1f} | " + " | ".join(f"{x:.1f} / {y:.1f}" for x, y in v[1]) + " |" for k, v in MEASURED.items()]
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
