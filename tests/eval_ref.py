"""CPU restatement of the reference's clip evaluation (eval_depthcrafter/eval.py:55-151, metric.py) for the tests of
vdn.eval: float64 throughout, the closed-form normal equations in place of the SVD lstsq, and the reference's float32
corners kept where they decide a result:

  * valid = gt > min and gt < max is a float32 comparison (numpy compares a float32 array with a Python float in float32);
  * the TGM gradient of gt is a float32 subtraction compared with float32(0.05); the gradient of the aligned
    prediction is float64;
  * the three delta accuracies are float32: count / n per frame and the mean over the kept frames. The mean is summed
    serially in frame order, which is what the device does. torch's CPU sum keeps four interleaved accumulators, so it
    agrees with a serial sum for up to four kept frames and can differ by one float32 ulp beyond that.

Also the seeded case generator shared by tools/make_golden_eval.py and the tests (tests/golden/eval_cases.npz stores
seeds and arguments, not arrays)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

eval_metrics = ["abs_relative_difference", "delta1_acc", "temporal_gradient_matching_error", "abs_difference",
                "rmse_linear", "delta2_acc", "delta3_acc"]
DELTA_IDX = (1, 5, 6)
F64_IDX = (0, 2, 3, 4)
TGM_THRESHOLD = 0.05


def resize_hp(x: np.ndarray, size) -> np.ndarray:
    """Half-pixel bilinear resize of f32 [T, IH, IW] (cv2.resize's default geometry; no antialiasing)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))[:, None]
    return F.interpolate(t, size=tuple(int(s) for s in size), mode="bilinear", align_corners=False)[:, 0].numpy()


def fit_ref(p: np.ndarray, t: np.ndarray):
    """(scale, shift) minimising |scale * p + shift - t|^2 over the given float64 samples; the minimum-norm solution
    when all p are equal (what lstsq returns for the rank-1 system); (nan, nan) without a sample."""
    n = p.size
    if n == 0:
        return float("nan"), float("nan")
    if p.min() == p.max():
        c, mt = float(p.flat[0]), t.sum() / n
        return c * mt / (c * c + 1.0), mt / (c * c + 1.0)
    spp, sp, spt, st = (p * p).sum(), p.sum(), (p * t).sum(), t.sum()
    det = spp * n - sp * sp
    return (n * spt - sp * st) / det, (spp * st - sp * spt) / det


def _mean_f32_serial(q) -> float:
    s = np.float32(0)
    for v in q:
        s = np.float32(s + np.float32(v))
    return float(np.float32(s / np.float32(len(q)))) if len(q) else float("nan")


def eval_ref(pred, gt, seq_len=98, domain="depth", dataset_min_depth=1e-3, dataset_max_depth=70, mask=None,
             tgm_over_time=False, return_parts=False):
    if domain not in ("depth", "disp"):
        raise ValueError(domain)
    pred, gt = np.asarray(pred, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    seq_len = min(seq_len, pred.shape[0])
    if pred.shape[-2:] != gt.shape[-2:]:
        pred = resize_hp(pred, gt.shape[-2:])
    pred, gt = pred[:seq_len], gt[:seq_len]
    lo, hi = float(dataset_min_depth), float(dataset_max_depth)
    valid = (gt > np.float32(lo)) & (gt < np.float32(hi))
    if mask is not None:
        valid &= np.asarray(mask)[:seq_len].astype(bool)
    p = np.maximum(pred.astype(np.float64), lo)
    g = gt.astype(np.float64)
    t = g[valid] if domain == "disp" else 1.0 / (g[valid] + 1e-8)
    scale, shift = fit_ref(p[valid], t)

    a = np.maximum(scale * p + shift, lo)
    if domain == "depth":
        pos = a > 0
        a = np.where(pos, 1.0 / np.where(pos, a, 1.0), 0.0)
    a = np.minimum(np.maximum(a, lo), hi)

    keep = [f for f in range(gt.shape[0]) if valid[f].any()]
    with np.errstate(all="ignore"):
        absrel, absdiff, rmse, deltas = [], [], [], [[], [], []]
        for f in keep:
            v, n = valid[f], int(valid[f].sum())
            d = a[f][v] - g[f][v]
            absdiff.append(np.abs(d).sum() / n)
            absrel.append((np.abs(d) / g[f][v]).sum() / n)
            rmse.append(np.sqrt((d * d).sum() / n))
            r = np.maximum(a[f][v] / g[f][v], g[f][v] / a[f][v])
            for k, thr in enumerate((1.25, 1.25 ** 2, 1.25 ** 3)):
                deltas[k].append(np.float32(np.float32((r < thr).sum()) / np.float32(n)))
        thr32 = np.float32(TGM_THRESHOLD)
        tgm = []
        if tgm_over_time:      # metric.py:3-33 on [1, kept frames, H, W]: pairs of consecutive kept frames
            for f0, f1 in zip(keep[:-1], keep[1:]):
                m = valid[f0] & ((gt[f1] - gt[f0]) < thr32)
                dd = np.abs((a[f1] - a[f0]) - (gt[f1] - gt[f0]).astype(np.float64))
                tgm.append(np.float64(dd[m].sum()) / np.float64(m.sum()))
        else:                  # what the reference computes on [T, H, W]: the gradient along H, per kept frame
            for f in keep:
                dg = gt[f, 1:] - gt[f, :-1]
                m = valid[f, :-1] & (dg < thr32)
                dd = np.abs((a[f, 1:] - a[f, :-1]) - dg.astype(np.float64))
                tgm.append(np.float64(dd[m].sum()) / np.float64(m.sum()))
        mean = lambda q: float(np.mean(q)) if len(q) else float("nan")
        out = [mean(absrel), _mean_f32_serial(deltas[0]), mean(tgm), mean(absdiff), mean(rmse),
               _mean_f32_serial(deltas[1]), _mean_f32_serial(deltas[2])]
    if return_parts:
        return out, dict(scale=scale, shift=shift, valid=valid, aligned=a, keep=keep)
    return out


# ------------------------------------------------------------------------------------------------ seeded cases
def make_case(seed: int, shape, domain: str, with_mask: bool, empty_frames=(), dmin=1e-3, dmax=70.0):
    """A clip that exercises every branch of the evaluation: gt depth in and out of (dmin, dmax), whole frames without a
    valid pixel, predictions below dmin, aligned values beyond dmax, and gt gradients on both sides of the TGM threshold.
    Returns (pred f32 [T,H,W], gt f32 [T,H,W], mask bool [T,H,W] or None)."""
    T, H, W = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    gt = np.empty((T, H, W), np.float64)
    for f in range(T):
        gt[f] = 2.0 + 6.0 * yy + 3.0 * np.sin(3.0 * xx + 0.7 * f) ** 2 + 0.15 * rng.standard_normal((H, W))
    u = rng.random((T, H, W))
    gt = np.where(u < 0.15, 0.0, np.where(u < 0.30, 75.0 + 10.0 * rng.random((T, H, W)), gt))
    for f in empty_frames:
        gt[f] = 0.0 if f % 2 == 0 else 80.0
    # outliers sit mostly on pixels outside the fit (invalid gt), so the fit stays near the true scale and shift
    invalid = (gt <= dmin) | (gt >= dmax)
    rate = np.where(invalid, 0.25, 0.01)
    if domain == "depth":      # the prediction is an affine-invariant disparity
        pred = 3.0 / np.maximum(gt, 0.5) + 0.2 + 0.08 * rng.standard_normal((T, H, W))
        small = rng.random((T, H, W)) < rate
        pred = np.where(small, -0.05 + 0.25 * rng.random((T, H, W)), pred)   # below dmin, or aligned past dmax
    else:
        pred = 0.5 * gt + 1.0 + 0.3 * rng.standard_normal((T, H, W))
        big = (rng.random((T, H, W)) < 0.1) & invalid
        pred = np.where(big, 200.0 + 30.0 * rng.random((T, H, W)), pred)     # aligned past dmax
        pred = np.where(rng.random((T, H, W)) < rate, -1.0, pred)            # below dmin
    mask = (rng.random((T, H, W)) < 0.8) if with_mask else None
    return pred.astype(np.float32), gt.astype(np.float32), mask
