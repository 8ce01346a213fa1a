#!/usr/bin/env python3
"""Time the depth criterion (vdn.loss) on one MI355X and write profiles/depth_loss.md.

For [1, 32, 518, 518] and [4, 16, 224, 224] (prediction, target and a bool mask resident on the GPU):
  * VideoDepthLoss.forward (no synchronisation: timed by device events around the launches) and depth_loss (the same
    launches plus the per-frame outputs and one synchronising copy);
  * the fit pass alone (compute_scale_and_shift on the clip flattened to [B, T * H, W]) and the select alone
    (Runtime.frame_median on the target: the same seven launches on one key per pixel);
  * a composition of torch ops on the same device that follows tests/loss_ref.py step by step in float32 (masked sums, the
    2 x 2 solve, torch.median of the masked maps, the four strided gradient grids, the thresholded frame differences, absRel
    and d1), written for this tool;
  * a device-to-device copy, for the achievable bandwidth beside the achieved one.
Each timed call works on the next of `sets` copies of the inputs, enough of them that together they exceed the 256 MiB
Infinity Cache twice over, so a call reads from HBM, not from what the call before it left in the cache. A sample is the
time of `--batch` calls between two device events, divided by the batch; the figure is the median of `--iters` samples.
Bytes. Compulsory: prediction (4 B) + target (4 B) + mask (1 B) per pixel, read once. The kernels read them six times (fit,
three histogram passes, the deviation pass, the fused pass) and the fused pass reads the next frame's 9 B as well: 63 B per
pixel, the traffic the bandwidth column uses; the 2.7 grid neighbours per pixel of the fused pass are re-reads that the
caches are expected to serve and are not counted.

Also lists what the tests assert: per recorded case of tests/golden/loss_cases.npz the reference's value and the restatement's
deviation from it, the largest deviation per key as tools/make_golden_loss.py stored it (the bars of tests/test_loss_host.py
are four times those), and the device against the restatement on the recorded cases (the 1e-9 bar of
tests/test_gpu_loss.py). Reports, not gates. This tool writes the whole file."""
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

from normal_bench import HBM_MEASURED, HBM_SPEC, sample_us  # noqa: E402

PASSES, LAUNCHES = 7, 13   # reads of the 9 B per pixel (six of the frame, one of the next frame); kernels of one vdn_depth_loss


def torch_composition(p, t, keep, alpha=0.5, scales=4, stable_scale=10.0):
    """tests/loss_ref.depth_loss_ref in torch float32 ops. p, t float32 [B, T, H, W], keep bool. -> the five values."""
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

    d = k * (robust(a) - robust(t))
    n = k.sum()
    spatial = torch.where(n > 0, d.abs().sum() / n.clamp_min(1), torch.zeros_like(n))
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
    c2 = k2.sum()
    stable = torch.where(c2 > 0, torch.where(k2, (pg - tg).abs(), 0.0).sum() / c2.clamp_min(1), torch.zeros_like(spatial))
    k3 = keep & (t > 1e-3) & (t < 70)
    c3 = k3.sum()
    absrel = torch.where(c3 > 0, torch.where(k3, ((a - t) / t).abs(), 0.0).sum() / c3.clamp_min(1), torch.zeros_like(spatial))
    hits = (keep & (torch.maximum(a / t, t / a) < 1.25)).sum()
    d1 = torch.where(n > 0, hits / n.clamp_min(1), torch.zeros_like(n))
    return spatial, stable, absrel, d1, spatial + stable_scale * stable


def time_shape(shape, a, dev):
    import loss_ref as R
    from vdn import loss as L
    B, T, H, W = shape
    c = R.make_case(9, shape, 0.8)
    px = B * T * H * W
    once = 9 * px
    sets = max(2, math.ceil(2 * 256 * 2 ** 20 / once))
    base = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
    pool = [{k: v.clone() for k, v in base.items()} for _ in range(sets)]
    for s in pool:
        s["fit"] = tuple(s[k].view(B, T * H, W) for k in ("pred", "target", "mask"))
    crit = L.VideoDepthLoss()
    rt = L.runtime_for(dev, base["pred"])
    med = torch.empty(B * T, dtype=torch.float32, device=dev)
    at = lambda i: pool[i % sets]
    t = dict(
        forward=sample_us(lambda i: crit(at(i)["pred"], at(i)["target"], at(i)["mask"]), a.warmup, a.iters, a.batch),
        call=sample_us(lambda i: L.depth_loss(at(i)["pred"], at(i)["target"], at(i)["mask"]), a.warmup, a.iters, a.batch),
        fit=sample_us(lambda i: L.compute_scale_and_shift(*at(i)["fit"]), a.warmup, a.iters, a.batch),
        select=sample_us(lambda i: rt.frame_median(at(i)["target"].view(B * T, H * W), med), a.warmup, a.iters, a.batch),
        torch_ops=sample_us(lambda i: torch_composition(at(i)["pred"], at(i)["target"], at(i)["mask"]), a.warmup, max(3, a.iters // 4), 2),
    )
    src = [torch.empty(once, dtype=torch.uint8, device=dev).random_(0, 255) for _ in range(sets)]
    dst = torch.empty_like(src[0])
    t["copy"] = sample_us(lambda i: dst.copy_(src[i % sets]), a.warmup, a.iters, a.batch)
    got = L.depth_loss(base["pred"], base["target"], base["mask"])
    comp = [float(v) for v in torch_composition(base["pred"], base["target"], base["mask"])]
    keys = ("spatial_loss", "stable_loss", "absRel_loss", "d1", "total_loss")
    return dict(shape=shape, px=px, sets=sets, once=once, t=t, values={k: got[k] for k in keys},
                comp_diff={k: abs(comp[i] - got[k]) for i, k in enumerate(keys)})


def differences(dev):
    """-> (per-case table lines, rows of (what, measured))."""
    import loss_ref as R
    import test_loss_host as Hs
    from vdn import loss as L
    bar, rows = Hs.bars(), []
    table = ["| seed | shape | kind | keep | mask | alpha | stable_scale | " + " | ".join(f"`{k}`" for k in Hs.KEYS) + " |",
             "|" + "---|" * (7 + len(Hs.KEYS))]
    for c in Hs.CASES:
        case = Hs.case_inputs(c)
        got = R.depth_loss_ref(case["pred"], case["target"], case["mask"], alpha=c["alpha"], stable_scale=c["stable_scale"])
        cells = [f"{c['expected'][k]:.7g} ({got[k] - c['expected'][k]:+.1e})" if k in got else "absent" for k in Hs.KEYS]
        table.append(f"| {c['seed']} | {'x'.join(map(str, c['shape']))} | {c['kind']} | {c['keep_rate']:g} | {c['mask_dtype']} | "
                     f"{c['alpha']:g} | {c['stable_scale']:g} | " + " | ".join(cells) + " |")
    for k in Hs.KEYS:
        rows.append((f"restatement vs the reference's recorded `{k}`, largest over {len(Hs.CASES)} cases (bar 4 x)", f"{bar[k] / 4:.2e}"))
    worst = {}
    for c in Hs.CASES:
        case = Hs.case_inputs(c)
        want = R.depth_loss_ref(case["pred"], case["target"], case["mask"], alpha=c["alpha"], stable_scale=c["stable_scale"])
        got = L.depth_loss(*(torch.from_numpy(np.array(case[k])).to(dev) for k in ("pred", "target", "mask")), alpha=c["alpha"],
                           stable_scale=c["stable_scale"])
        for k in Hs.KEYS + ("data",):
            if k in want:
                worst[k] = max(worst.get(k, 0.0), abs(got[k] - want[k]))
        worst["g_k"] = max(worst.get("g_k", 0.0), float(np.abs(got["g"].numpy() - want["g"]).max()))
        for k in ("s_pred", "s_target"):
            worst["s"] = max(worst.get("s", 0.0), float(np.abs(got[k].numpy() - want[k]).max()))
    for k, v in worst.items():
        rows.append((f"device vs restatement, `{k}`, largest over the recorded cases (bar 1e-9"
                     + (", times 1 + stable_scale)" if k == "total_loss" else ")"), f"{v:.2e}"))
    return table, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 32, 518, 518, 4, 16, 224, 224])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_loss.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    shapes = [tuple(a.shapes[i:i + 4]) for i in range(0, len(a.shapes), 4)]
    results = [time_shape(s, a, dev) for s in shapes]
    table, rows = differences(dev)

    f3 = lambda t: f"{t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f})"
    tbs = lambda us, b: b / us / 1e6
    lines = [
        "# vdn.loss: VideoDepthLoss on the device",
        "",
        f"Written by `tools/loss_bench.py` on {torch.cuda.get_device_name(0)}. Device events around {a.batch} calls, "
        f"{a.warmup} warm-up calls,",
        f"median (min .. max) of {a.iters} samples, in microseconds per call. Every call works on the next of several copies of",
        "the inputs (column `sets`), which together exceed the Infinity Cache twice over, so the inputs come from HBM.",
        f"The kernels read the 9 B per pixel (prediction, target, mask) {PASSES} times: fit, three histogram passes of the select, the",
        f"deviation pass, and the fused pass for the frame and for the next frame. Bandwidth is that traffic over the time; HBM peak {HBM_SPEC / 1e12:.1f} TB/s (data sheet), "
        f"{HBM_MEASURED / 1e12:.2f} TB/s (measured float4 copy).",
        "",
    ]
    for r in results:
        t = r["t"]
        fw = tbs(t["forward"][0], PASSES * r["once"])
        lines += [
            f"## {list(r['shape'])}: {r['px'] / 1e6:.2f} M pixels, {r['sets']} sets",
            "",
            "| What | us per call | TB/s | of measured HBM peak |",
            "|---|---|---|---|",
            f"| `VideoDepthLoss.forward` ({LAUNCHES} kernels + the float32 cast, no synchronisation), {PASSES} x 9 B/pixel = {PASSES * r['once'] / 1e6:.0f} MB | {f3(t['forward'])} | {fw:.2f} | {fw * 1e12 / HBM_MEASURED:.0%} |",
            f"| `depth_loss` (the same + per-frame outputs + synchronising copy) | {f3(t['call'])} | - | - |",
            f"| `compute_scale_and_shift` (the fit pass + solve), 9 B/pixel | {f3(t['fit'])} | {tbs(t['fit'][0], r['once']):.2f} | {tbs(t['fit'][0], r['once']) * 1e12 / HBM_MEASURED:.0%} |",
            f"| the select alone: `vdn_frame_median` of the target (7 kernels, one key per pixel), 3 x 4 B/pixel | {f3(t['select'])} | {tbs(t['select'][0], 12 * r['px']):.2f} | {tbs(t['select'][0], 12 * r['px']) * 1e12 / HBM_MEASURED:.0%} |",
            f"| torch-ops composition of the same steps, float32, same device | {f3(t['torch_ops'])} | - | - |",
            f"| device-to-device copy of {r['once'] / 1e6:.0f} MB (reads + writes = 2 x) | {f3(t['copy'])} | {tbs(t['copy'][0], 2 * r['once']):.2f} | {tbs(t['copy'][0], 2 * r['once']) * 1e12 / HBM_MEASURED:.0%} |",
            "",
            f"`forward` vs the torch-ops composition: {t['torch_ops'][0] / t['forward'][0]:.1f} x. Fit and select alone take "
            f"{(t['fit'][0] + t['select'][0]) / t['forward'][0]:.0%} of `forward`, which leaves {t['forward'][0] - t['fit'][0] - t['select'][0]:.0f} us for the "
            f"deviation pass, the fused pass and the two one-block kernels. One read of the inputs at the copy's rate "
            f"would take {t['copy'][0] / 2:.1f} us: `forward` is {t['forward'][0] / (t['copy'][0] / 2):.1f} reads long. Values: "
            + ", ".join(f"`{k}` {v:.6f}" for k, v in r["values"].items()) + "; the float32 composition differs by "
            + ", ".join(f"{v:.1e}" for v in r["comp_diff"].values()) + ".",
            "",
        ]
    big = results[0]["t"]
    lines += [
        "## What the times say, and the next measurement",
        "",
        "* The inputs are read seven times where once would do, and `forward` takes several times those seven reads at the copy's",
        "  rate: the criterion is bound by its pass structure and by latency, not by bytes.",
        f"* The select on one key per pixel takes {big['select'][0]:.0f} us of `forward`'s {big['forward'][0]:.0f} us at {list(results[0]['shape'])}"
        f" ({big['select'][0] / big['forward'][0]:.0%}), and {results[-1]['t']['select'][0]:.0f} of {results[-1]['t']['forward'][0]:.0f} us at {list(results[-1]['shape'])};",
        "  inside `forward` it handles two keys per pixel. Its three histogram passes count in LDS with integer atomics, and the",
        "  keys here collide: every dropped pixel is the key of 0.0, and depths within a factor of two share their top 11 bits.",
        "  Its three scans are one block per (frame, slot): 256 lanes sum 8 bins each and the lane whose run holds the rank walks",
        "  it. Next: a per-wave private",
        "  histogram, or counting the zeros of dropped pixels from the kept count instead of through the atomics.",
        "* The fused pass keeps four consecutive pixels per lane, as `vdn_normal_eval` does, although `profiles/normal_eval.md` found",
        "  the strided neighbour loads, not the bytes, to set that kernel's time. Here the pattern is lighter: the pixel's own nine",
        "  bytes and the next frame's are 16-byte and 4-byte quad loads, the right-hand neighbour of the finest grid comes from",
        "  the quad, and what remains scalar is the lower neighbour of the finest grid (a row away: coalesced across lanes only at",
        "  a stride of four pixels) and the neighbours of the coarser grids, which a quarter, a sixteenth and a sixty-fourth of",
        "  the pixels have. The fp64 divisions (two per normalised difference) are the other cost. The table above bounds the",
        "  fused and deviation passes together; it does not separate them. Next: a kernel trace of one call for the per-kernel",
        "  split, then one pixel per lane in the fused pass (every load coalesced, the lower neighbour included) against the quad",
        "  form, and the three histogram passes on quad loads (`LossKey` reads a byte and two floats per pixel, coalesced across",
        "  lanes but one pixel per lane).",
        f"* Fusing fit, deviation and fused pass further is not possible: each needs the result of the one before for the whole",
        f"  frame (scale and shift, then the medians, then the scales). At {list(results[0]['shape'])} the fit alone takes {big['fit'][0]:.0f} us.",
        "",
        "## The restatement against the reference, per recorded case",
        "",
        "`tests/loss_ref.py` fits and sums in float64; the imported reference computes in float32. The reference's value, and in",
        "brackets the restatement minus it. Both sides decide the same pixels of d1 in every case (asserted by",
        "`tools/make_golden_loss.py`). The `[1, 2, 1, 1]` case draws its two frames 3.0 apart instead of 0.2: two pixels determine the",
        "fit, so the residual is the fit's own rounding, and with pixels 0.2 apart the reference's float32 determinant cancels to",
        "four digits. The `straddle` case keeps one pixel each at 0, 5e-4, 1.5e-3, 69.5 and 71 per frame; `|a - t| / t` reaches 100",
        "at 1.5e-3, which is why `absRel_loss` carries the largest float32 deviation.",
        "",
    ] + table + [""]
    lines += ["## Differences the tests assert", "", "| Case | measured |", "|---|---|"] + [f"| {w} | {d} |" for w, d in rows]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
