#!/usr/bin/env python3
"""Time the normal evaluation (vdn.normals) on one MI355X and write profiles/normal_eval.md.

For [1, 32, 224, 224] and [1, 32, 518, 518] (pred, gt depth, stored target and a bool mask resident on the GPU):
  * vdn.normals.normal_loss_from_depth (the fused path, with its one synchronising copy) and VideoNormalLoss.forward on a
    stored target (no synchronisation: timed by device events around the launches);
  * the kernels alone, Runtime.normal_eval in both modes;
  * a composition of torch ops on the same device that follows tests/normal_ref.py step by step in float32 (reflect pad,
    shifted differences, normalise, erode by max-pooling the inverted mask, cosine, masked mean);
  * a device-to-device copy, for the achievable bandwidth beside the achieved one.
Each timed call works on the next of `sets` copies of the inputs, enough of them that together they exceed the 256 MiB
Infinity Cache twice over, so a call reads from HBM, not from what the call before it left in the cache. A sample is the
time of `--batch` calls between two device events, divided by the batch; the figure is the median of `--iters` samples.
Bytes of the fused kernel = pred (12 B) + depth (4 B) + mask (1 B) per pixel: the compulsory traffic; neighbours of the
stencil and the erosion are re-reads that the caches are expected to serve.

Also measures what the tests assert (tests/test_gpu_normals.py): kernel vs tests/normal_ref.py on the test shapes, kernel vs
the reference's recorded values, the share of normal_vector values that equal the rounded restatement, and forward vs the
fused path. Reports, not gates."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12   # B/s: a float4 copy on this part, and the data sheet


def sample_us(fn, warmup, iters, batch):
    """fn(i) is called with a running index; returns (median, min, max) microseconds per call."""
    k = 0
    for _ in range(warmup):
        fn(k)
        k += 1
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(batch):
            fn(k)
            k += 1
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) * 1e3 / batch)
    return statistics.median(times), min(times), max(times)


def torch_composition(pred, depth, mask):
    """tests/normal_ref.normal_loss_ref(target_is_depth=True) in torch float32 ops. pred [F,3,H,W], depth [F,H,W], mask bool."""
    Fr, H, W = depth.shape
    p = F.pad(depth[:, None], (1, 1, 1, 1), mode="reflect")[:, 0]
    w = lambda r, c: p[:, r:r + H, c:c + W]
    ix = ((w(0, 0) - w(0, 2)) + 2.0 * (w(1, 0) - w(1, 2)) + (w(2, 0) - w(2, 2))) * 0.125
    iy = ((w(0, 0) - w(2, 0)) + 2.0 * (w(0, 1) - w(2, 1)) + (w(0, 2) - w(2, 2))) * 0.125
    n = torch.stack([-ix, -iy, torch.ones_like(ix)], 1)
    n = n / torch.sqrt((n * n).sum(1, keepdim=True) + 1e-8)
    keep = F.max_pool2d((~mask)[:, None].float(), 3, 1, 1)[:, 0] == 0     # the pool pads with -inf: outside erodes nothing
    na = pred.norm(dim=1, keepdim=True).clamp_min(1e-8)
    nb = n.norm(dim=1, keepdim=True).clamp_min(1e-8)
    cos = ((pred / na) * (n / nb)).sum(1)
    total, count = torch.where(keep, cos, 0.0).sum(), keep.sum()
    return torch.where(count > 0, 1.0 - total / count, torch.ones_like(total))


def time_shape(T, H, W, a, dev):
    import normal_ref as R
    from vdn import normals as N
    rt = N._runtime_for(dev)
    c = R.make_case(9, (1, T, H, W), "bool", "unit")
    px = T * H * W
    fused_bytes, stored_bytes = 17 * px, 25 * px
    sets = max(2, math.ceil(2 * 256 * 2 ** 20 / fused_bytes))
    base = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
    pool = [{k: v.clone() for k, v in base.items()} for _ in range(sets)]
    for s in pool:
        s["m8"] = s["mask"].view(torch.uint8).view(T, H, W)
        s["p4"], s["t4"], s["d3"] = s["pred"].view(T, 3, H, W), s["target"].view(T, 3, H, W), s["depth"].view(T, H, W)
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    loss = N.VideoNormalLoss()
    at = lambda i: pool[i % sets]
    t = dict(
        fused_call=sample_us(lambda i: N.normal_loss_from_depth(at(i)["pred"], at(i)["depth"], at(i)["mask"]), a.warmup, a.iters, a.batch),
        forward=sample_us(lambda i: loss(at(i)["pred"], at(i)["target"], at(i)["mask"]), a.warmup, a.iters, a.batch),
        fused_kernel=sample_us(lambda i: rt.normal_eval(at(i)["p4"], at(i)["d3"], at(i)["m8"], out), a.warmup, a.iters, a.batch),
        stored_kernel=sample_us(lambda i: rt.normal_eval(at(i)["p4"], at(i)["t4"], at(i)["m8"], out), a.warmup, a.iters, a.batch),
        nomask_kernel=sample_us(lambda i: rt.normal_eval(at(i)["p4"], at(i)["d3"], None, out), a.warmup, a.iters, a.batch),
        torch_ops=sample_us(lambda i: torch_composition(at(i)["p4"], at(i)["d3"], at(i)["mask"][0]), a.warmup, a.iters, a.batch),
    )
    src = [torch.empty(fused_bytes, dtype=torch.uint8, device=dev).random_(0, 255) for _ in range(sets)]
    dst = torch.empty_like(src[0])
    t["copy"] = sample_us(lambda i: dst.copy_(src[i % sets]), a.warmup, a.iters, a.batch)
    got = N.normal_loss_from_depth(base["pred"], base["depth"], base["mask"])
    want = R.normal_loss_ref(c["pred"], c["depth"], c["mask"], True)[0]
    comp = float(torch_composition(pool[0]["p4"], pool[0]["d3"], base["mask"][0]))
    return dict(shape=(1, T, H, W), px=px, sets=sets, fused_bytes=fused_bytes, stored_bytes=stored_bytes, t=t,
                diff=abs(got - want), comp_diff=abs(comp - want))


def differences(dev):
    import normal_ref as R
    import test_normals_host as Hs
    import test_gpu_normals as G
    from vdn import normals as N
    rows = []
    for c in Hs.CASES:
        case = Hs.case_inputs(c)
        pred, target, depth, mask = (G.dev(case[k]) for k in ("pred", "target", "depth", "mask"))
        stored = float(N.VideoNormalLoss()(pred, target, mask)["normal_loss"])
        fused = N.normal_loss_from_depth(pred, depth, mask)
        rows.append((f"reference fixture seed {c['seed']} {c['shape']} mask {c['mask_kind']}, target {c['target_kind']} (bar 2e-6)",
                     f"forward {abs(stored - c['expected']):.2e}, from depth {abs(fused - c['expected_depth']):.2e}"))
    for shape in G.SHAPES:
        worst_loss = worst_mean = 0.0
        for from_depth in (False, True):
            for masked in (False, True):
                got, want = G.run(G.inputs(shape, masked), from_depth, masked, per_frame=True), G.reference(shape, masked, from_depth)
                ok = ~np.isnan(want[1])
                worst_loss = max(worst_loss, abs(got[0] - want[0]))
                worst_mean = max(worst_mean, float(np.abs(got[1].numpy()[ok] - want[1][ok]).max()) if ok.any() else 0.0)
        rows.append((f"normal_ref {shape}, both target kinds, with and without mask (bar 1e-9)",
                     f"loss {worst_loss:.2e}, per-frame mean {worst_mean:.2e}"))
    for shape in G.SHAPES:
        d = G.inputs(shape, False)["depth"]
        got = N.normal_vector(G.dev(d)[:, :, None]).cpu().numpy()
        want = R.normal_vector_ref(d).astype(np.float32)
        ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want)).astype(np.float64)
        rows.append((f"normal_vector {shape} vs the restatement rounded to float32 (bar 1 ulp)",
                     f"{float((got == want).mean()):.4%} equal, max {float(ulps.max()):.0f} ulp"))
    for depth, args, want in Hs.recorded_normals():
        got = N.normal_vector(G.dev(depth)[:, :, None], **args).cpu().numpy()
        rows.append((f"recorded reference normals {depth.shape} (bar {Hs.normals_bar(depth):.2e})", f"{float(np.abs(got - want).max()):.2e}"))
    for shape in ((3, 64, 257), (1, 224, 224)):
        c = G.inputs(shape, True)
        pred, depth, mask = G.dev(c["pred"]), G.dev(c["depth"]), G.dev(c["mask"])
        fused = N.normal_loss_from_depth(pred, depth, mask)
        stored = N.normal_loss(pred, N.normal_vector(depth[:, :, None]), mask)
        rows.append((f"stored normal_vector target vs fused path {shape} (bar 1e-9)", f"{abs(fused - stored):.2e}"))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[224, 518])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_eval.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("normal_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    results = [time_shape(a.frames, s, s, a, dev) for s in a.sizes]
    rows = differences(dev)

    f3 = lambda t: f"{t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f})"
    tbs = lambda us, b: b / us / 1e6
    lines = [
        "# vdn.normals: VideoNormalLoss and normal_vector on the device",
        "",
        f"Written by `tools/normal_bench.py` on {torch.cuda.get_device_name(0)}. Device events around {a.batch} calls, "
        f"{a.warmup} warm-up calls,",
        f"median (min .. max) of {a.iters} samples, in microseconds per call. Every call works on the next of several copies of",
        "the inputs (column `sets`), which together exceed the Infinity Cache twice over, so the inputs come from HBM.",
        f"Bandwidth is the compulsory traffic over the time; HBM peak {HBM_SPEC / 1e12:.1f} TB/s (data sheet), "
        f"{HBM_MEASURED / 1e12:.2f} TB/s (measured float4 copy).",
        "",
    ]
    for r in results:
        t = r["t"]
        fk, sk = tbs(t["fused_kernel"][0], r["fused_bytes"]), tbs(t["stored_kernel"][0], r["stored_bytes"])
        lines += [
            f"## {list(r['shape'])}: {r['px'] / 1e6:.2f} M pixels, {r['sets']} sets",
            "",
            "| What | us per call | TB/s | of measured HBM peak |",
            "|---|---|---|---|",
            f"| `normal_loss_from_depth` (fused kernel + finalise + synchronising copy) | {f3(t['fused_call'])} | - | - |",
            f"| `VideoNormalLoss.forward`, stored target (no synchronisation) | {f3(t['forward'])} | - | - |",
            f"| `vdn_normal_eval`, target from depth, 17 B/pixel = {r['fused_bytes'] / 1e6:.0f} MB | {f3(t['fused_kernel'])} | {fk:.2f} | {fk * 1e12 / HBM_MEASURED:.0%} |",
            f"| `vdn_normal_eval`, target from depth, no mask, 16 B/pixel | {f3(t['nomask_kernel'])} | {tbs(t['nomask_kernel'][0], 16 * r['px']):.2f} | {tbs(t['nomask_kernel'][0], 16 * r['px']) * 1e12 / HBM_MEASURED:.0%} |",
            f"| `vdn_normal_eval`, stored target, 25 B/pixel = {r['stored_bytes'] / 1e6:.0f} MB | {f3(t['stored_kernel'])} | {sk:.2f} | {sk * 1e12 / HBM_MEASURED:.0%} |",
            f"| torch-ops composition of the same steps, float32, same device | {f3(t['torch_ops'])} | - | - |",
            f"| device-to-device copy of {r['fused_bytes'] / 1e6:.0f} MB (reads + writes = 2 x) | {f3(t['copy'])} | {tbs(t['copy'][0], 2 * r['fused_bytes']):.2f} | {tbs(t['copy'][0], 2 * r['fused_bytes']) * 1e12 / HBM_MEASURED:.0%} |",
            "",
            f"Fused call vs the torch-ops composition: {t['torch_ops'][0] / t['fused_call'][0]:.1f} x; fused kernel vs stored-target kernel: "
            f"{t['stored_kernel'][0] / t['fused_kernel'][0]:.2f} x. On these inputs the fused path and `tests/normal_ref.py` differ by "
            f"{r['diff']:.2e}; the float32 composition differs from it by {r['comp_diff']:.2e}.",
            "",
        ]
    lines += ["## Differences the tests assert", "", "| Case | measured |", "|---|---|"] + [f"| {w} | {d} |" for w, d in rows]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
