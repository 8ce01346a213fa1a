#!/usr/bin/env python3
"""Time the clip evaluation (vdn.eval) on one MI355X and write profiles/eval_metrics.md.

On a 98 x 518 x 518 clip (pred, gt, mask resident on the GPU):
  * the device path, vdn.eval.eval_single_by_data including its one synchronising copy of the seven values, and the two
    kernel passes alone (Runtime.eval_fit, Runtime.eval_metrics): HIP events, warm-up, median of `--iters` calls;
  * tests/eval_ref.py on the host (numpy float64), one call;
  * a plain device-to-device copy of the bytes the two passes read, for the achievable bandwidth beside the achieved one.
Bytes per pass = pred + gt (4 B each) + mask (1 B) per pixel; the gradient neighbour of the metrics pass is counted once
more for gt and pred only where the TGM mask asks for it, so the figure given is the compulsory traffic.

Also measures what the tests assert: the largest relative difference of the four fp64 metrics and whether the three delta
accuracies are equal as float32, kernel vs tests/eval_ref.py on the test shapes and kernel vs the reference's recorded
values (tests/golden/eval_cases.npz). Reports, not gates."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def median_ms(fn, warmup, iters):
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
    return statistics.median(times), min(times), max(times)


def differences():
    import eval_ref as R
    import test_eval_host as H
    import test_gpu_eval as G
    from vdn.eval import eval_single_by_data

    def diff(got, want):
        rel = [abs(got[i] - want[i]) / abs(want[i]) for i in R.F64_IDX if not (np.isnan(got[i]) and np.isnan(want[i]))]
        same = all(np.float32(got[i]) == np.float32(want[i]) or (np.isnan(got[i]) and np.isnan(want[i])) for i in R.DELTA_IDX)
        return max(rel, default=0.0), same

    rows = []
    for c in H.CASES:
        pred, gt, mask = H.case_inputs(c)
        got = eval_single_by_data(pred, gt, domain=c["domain"], dataset_min_depth=c["dmin"], dataset_max_depth=c["dmax"], mask=mask)
        rows.append((f"reference fixture seed {c['seed']} {c['shape']} {c['domain']}", *diff(got, c["expected"])))
    for shape in G.SHAPES:
        worst, same = 0.0, True
        for domain in ("depth", "disp"):
            for with_mask in (False, True):
                for over_time in (False, True):
                    pred, gt, mask = G.clip(shape, domain, with_mask)
                    got = eval_single_by_data(pred, gt, domain=domain, mask=mask, tgm_over_time=over_time)
                    d, s = diff(got, G.reference(shape, domain, with_mask, tgm_over_time=over_time))
                    worst, same = max(worst, d), same and s
        rows.append((f"eval_ref {shape}, both domains, with and without mask, both TGM strides", worst, same))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=98)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_bench.py measures on the GPU; none is visible")
    import eval_ref as R
    from vdn import _abi
    from vdn.eval import _runtime, eval_single_by_data
    T, H, W = a.frames, a.size, a.size
    pred, gt, mask = R.make_case(7, (T, H, W), "depth", True, (T // 2,))
    dev = torch.device("cuda:0")
    p, g, m = (torch.from_numpy(x).to(dev) for x in (pred, gt, mask))
    m = m.view(torch.uint8)
    rt = _runtime(dev)
    coef = torch.zeros(2, dtype=torch.float64, device=dev)
    out = torch.zeros(7, dtype=torch.float64, device=dev)
    px = T * H * W
    nbytes = 9 * px
    t_all = median_ms(lambda: eval_single_by_data(p, g, mask=m), a.warmup, a.iters)
    t_fit = median_ms(lambda: rt.eval_fit(p, g, m, 1e-3, 70.0, _abi.EVAL_DEPTH, coef), a.warmup, a.iters)
    t_met = median_ms(lambda: rt.eval_metrics(p, g, m, 1e-3, 70.0, _abi.EVAL_DEPTH, _abi.EVAL_TGM_ROWS, coef, out), a.warmup, a.iters)
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    t_copy = median_ms(lambda: dst.copy_(src), a.warmup, a.iters)
    got = eval_single_by_data(p, g, mask=m)
    t0 = time.perf_counter()
    want = R.eval_ref(pred, gt, 98, "depth", mask=mask)
    t_host = (time.perf_counter() - t0) * 1e3
    big_rel = max(abs(got[i] - want[i]) / abs(want[i]) for i in R.F64_IDX)
    big_same = all(np.float32(got[i]) == np.float32(want[i]) for i in R.DELTA_IDX)
    rows = differences()

    gbs = lambda ms, b: b / ms / 1e6
    lines = [
        "# vdn.eval: clip evaluation metrics on the device",
        "",
        f"Written by `tools/eval_bench.py` on {torch.cuda.get_device_name(0)}; clip {T} x {H} x {W}, domain depth, with a mask,",
        f"one frame without a valid pixel. HIP events, {a.warmup} warm-up calls, median (min .. max) of {a.iters} calls.",
        "",
        "| What | ms | GB/s |",
        "|---|---|---|",
        f"| `eval_single_by_data` on resident tensors (fit + metrics + copy of 7 values) | {t_all[0]:.3f} ({t_all[1]:.3f} .. {t_all[2]:.3f}) | {gbs(t_all[0], 2 * nbytes):.0f} (2 passes x {nbytes / 1e6:.0f} MB) |",
        f"| `vdn_eval_fit` (masked sums + solve) | {t_fit[0]:.3f} ({t_fit[1]:.3f} .. {t_fit[2]:.3f}) | {gbs(t_fit[0], nbytes):.0f} |",
        f"| `vdn_eval_metrics` (fused metrics + finalise) | {t_met[0]:.3f} ({t_met[1]:.3f} .. {t_met[2]:.3f}) | {gbs(t_met[0], nbytes):.0f} |",
        f"| device-to-device copy of {nbytes / 1e6:.0f} MB (reads + writes = 2 x) | {t_copy[0]:.3f} ({t_copy[1]:.3f} .. {t_copy[2]:.3f}) | {gbs(t_copy[0], 2 * nbytes):.0f} |",
        f"| `tests/eval_ref.py` on the host (numpy float64, one call) | {t_host:.0f} | - |",
        "",
        f"Speed-up of the device path over the host restatement: {t_host / t_all[0]:.0f} x. The host figure is this project's",
        "restatement, which solves the normal equations; the reference's SVD `lstsq` over every valid pixel is slower still and",
        "was not timed here.",
        "",
        f"On this clip the kernels and `eval_ref` differ by {big_rel:.2e} relative at most on the four fp64 metrics; delta1..3",
        f"equal as float32: {big_same} ({T - 1} kept frames, both sum the float32 mean in frame order).",
        "",
        "## Differences the tests assert (bar: 1e-9 relative on AbsRel, TGM, AbsDiff, RMSE; delta1..3 equal as float32)",
        "",
        "| Case | max relative difference, fp64 metrics | delta1..3 equal as float32 |",
        "|---|---|---|",
    ] + [f"| {w} | {d:.2e} | {s} |" for w, d, s in rows]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
