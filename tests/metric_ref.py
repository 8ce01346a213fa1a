"""The arithmetic contract of csrc/metric.hip (include/vdn.h: vdn_metric_eval, vdn_silog_loss, vdn_silog_loss_backward) restated
in numpy, and the seeded cases of tests/golden/metric_cases.npz. tests/test_metric_host.py holds this file to what the
reference's own eval_depth and SiLogLoss recorded there; tests/test_gpu_metric.py holds the device to this file.

float32, one rounding per operation: the mask's bounds, the align-corners resampling of the prediction, thresh and the three
quotients d1 d2 d3. float64 from the float32 inputs on: everything else. numpy rounds each float32 operation of a float32
array on its own, which is what the kernels' contract(off) arithmetic does."""
from __future__ import annotations

import numpy as np

KEYS = ("d1", "d2", "d3", "abs_rel", "sq_rel", "rmse", "rmse_log", "log10", "silog")
F32 = np.float32
MIN_DEPTH, MAX_DEPTH = 0.001, 20.0

#         seed  (B, H, W)     mask     special          lambd
CASES = [(31, (2, 37, 53), "bool", "plain", 0.5),
         (32, (2, 37, 53), "uint8", "bounds", 0.5),
         (33, (2, 37, 53), "float", "mask_values", 0.5),
         (34, (1, 23, 67), "bool", "ratio", 0.85),
         (35, (2, 16, 16), "bool", "nine_ten", 0.5),
         (36, (2, 23, 67), "uint8", "empty_item", 0.5),
         (37, (1, 16, 16), "bool", "empty_all", 0.5),
         (38, (2, 16, 16), "bool", "equal", 0.5),
         (39, (1, 37, 53), "bool", "negative_radicand", 2.0),
         (40, (1, 64, 64), "float", "plain", 0.15)]
GRAD_SAMPLES = 16


def case_dict(seed, shape, mask, special, lambd) -> dict:
    return dict(seed=int(seed), shape=tuple(int(s) for s in shape), mask=str(mask), special=str(special), lambd=float(lambd))


def sample_idx(numel: int, n: int = GRAD_SAMPLES) -> np.ndarray:
    return (np.arange(n, dtype=np.int64) * 2654435761 + 12345) % numel


def make_case(c: dict, pshape=None) -> dict:
    """-> pred f32 [B, h, w] ((h, w) = pshape, or the depth's), depth f32 [B, H, W], mask [B, H, W] in the case's dtype."""
    B, H, W = c["shape"]
    rng = np.random.default_rng(c["seed"])
    depth = rng.uniform(0.05, 25.0, (B, H, W)).astype(F32)          # a fifth of it lies past MAX_DEPTH
    noise = np.exp(rng.normal(0.0, 0.35, (B, H, W))).astype(F32)
    keep = rng.random((B, H, W)) < 0.7
    sp = c["special"]
    values = keep.astype(np.int64)
    if sp == "bounds":     # the two bounds themselves (kept) and their outer neighbours (dropped), all under a mask of 1
        lo, hi = F32(MIN_DEPTH), F32(MAX_DEPTH)
        depth[:, 0, :4] = (lo, np.nextafter(lo, F32(0)), hi, np.nextafter(hi, F32(np.inf)))
        values[:, 0, :4] = 1
    if sp == "mask_values":  # values other than 0 and 1: none of them keeps
        other = rng.random((B, H, W))
        values = np.where(other < 0.1, 2, values)
    if sp == "nine_ten":
        values[:] = 0
        flat = values.reshape(B, -1)
        flat[0, rng.permutation(H * W)[:9]] = 1
        flat[1, rng.permutation(H * W)[:10]] = 1
        depth = np.clip(depth, 0.05, 19.0).astype(F32)
    if sp == "empty_item":
        values[B - 1] = 0
    if sp == "empty_all":
        values[:] = 0
    pred = (depth * noise).astype(F32)
    if sp == "ratio":      # thresh exactly 1.25, 1.5625 and 1.953125, from either side: none of them is below its threshold
        depth[0, 0, :6] = (1.0, 2.0, 4.0, 2.5, 1.5625, 1.953125)
        pred[0, 0, :6] = (1.25, 3.125, 7.8125, 2.0, 1.0, 1.0)
        values[0, 0, :6] = 1
    if sp == "equal":      # pred == target at every kept pixel: the radicand is exactly 0
        pred = np.where(values == 1, depth, pred).astype(F32)
    if sp == "negative_radicand":  # dl nearly constant and lambd = 2: mean(dl^2) - 2 mean(dl)^2 < 0
        pred = (depth * F32(2.0) * np.exp(rng.normal(0.0, 0.01, (B, H, W)))).astype(F32)
    if c["mask"] == "bool":
        mask = values == 1
    elif c["mask"] == "uint8":
        mask = values.astype(np.uint8)
    else:
        mask = values.astype(F32)
        if sp == "mask_values":
            mask = np.where((values == 0) & (rng.random((B, H, W)) < 0.1), F32(0.5), mask).astype(F32)
    if pshape is not None:
        small = rng.uniform(0.05, 25.0, (B,) + tuple(pshape)).astype(F32)
        pred = small
    return dict(pred=pred, depth=depth, mask=mask)


def checksum(case: dict) -> np.ndarray:
    return np.array([case["pred"].astype(np.float64).sum(), case["depth"].astype(np.float64).sum(),
                     case["mask"].astype(np.float64).sum()])


def keep_mask(mask, depth, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH) -> np.ndarray:
    """(valid_mask == 1) & (depth >= min_depth) & (depth <= max_depth), the bounds in float32; None bounds: the mask alone."""
    keep = np.asarray(mask) == 1
    if min_depth is not None:
        keep = keep & (depth >= F32(min_depth)) & (depth <= F32(max_depth))
    return keep


def ac_coords(n_in: int, n_out: int):
    """align_corners=True source pixels and the weight of the second, in float32 (csrc/resample.hpp: ac_scale, ac_coord rounded)."""
    scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    src = scale * np.arange(n_out, dtype=F32)
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    i1 = np.where(i0 < n_in - 1, i0 + 1, i0)
    return i0, i1, (src - i0.astype(F32)).astype(F32)


def resample_ac(pred: np.ndarray, H: int, W: int) -> np.ndarray:
    """pred f32 [..., h, w] -> f32 [..., H, W]: top = fl(fl(fl(1 - lx) a00) + fl(lx a01)), bot alike, v = fl(fl(fl(1 - ly) top) +
    fl(ly bot))."""
    pred = np.asarray(pred, F32)
    y0, y1, ly = ac_coords(pred.shape[-2], H)
    x0, x1, lx = ac_coords(pred.shape[-1], W)
    ly = ly[:, None]
    wx0, wy0 = F32(1) - lx, F32(1) - ly
    r0, r1 = pred[..., y0, :], pred[..., y1, :]
    top = wx0 * r0[..., x0] + lx * r0[..., x1]
    bot = wx0 * r1[..., x0] + lx * r1[..., x1]
    out = wy0 * top + ly * bot
    assert out.dtype == F32
    return out


def eval_depth_ref(p: np.ndarray, t: np.ndarray) -> np.ndarray:
    """1-D float32 p, t -> float64 [9] in KEYS' order."""
    p, t = np.asarray(p, F32).reshape(-1), np.asarray(t, F32).reshape(-1)
    n = p.size
    with np.errstate(all="ignore"):
        a, b = t / p, p / t
        q = np.where((b > a) | np.isnan(b), b, a)                      # torch.max: a NaN wins
        nf = F32(n)
        d = [float(F32(np.count_nonzero(q < F32(thr))) / nf) for thr in (1.25, 1.5625, 1.953125)]
        p, t = p.astype(np.float64), t.astype(np.float64)
        diff, dl = p - t, np.log(p) - np.log(t)
        nn = np.float64(n)
        m2, m1 = (dl * dl).sum() / nn, dl.sum() / nn
        rest = [(np.abs(diff) / t).sum() / nn, (diff * diff / t).sum() / nn, np.sqrt((diff * diff).sum() / nn), np.sqrt(m2),
                np.abs(np.log10(p) - np.log10(t)).sum() / nn, np.sqrt(m2 - 0.5 * (m1 * m1))]
    return np.array(d + [float(v) for v in rest], np.float64)


def eval_rows(pred, depth, mask, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH) -> np.ndarray:
    """pred [B, h, w], depth [B, H, W], mask [B, H, W] -> float64 [B, 10]: n, then the nine."""
    depth = np.asarray(depth, F32)
    B, H, W = depth.shape
    if tuple(pred.shape[1:]) != (H, W):
        pred = resample_ac(pred, H, W)
    keep = keep_mask(mask, depth, min_depth, max_depth)
    rows = np.empty((B, 10), np.float64)
    for b in range(B):
        rows[b, 0] = keep[b].sum()
        rows[b, 1:] = eval_depth_ref(pred[b][keep[b]], depth[b][keep[b]])
    return rows


def silog_ref(pred, target, keep, lambd) -> np.ndarray:
    """-> float64 [4] = loss | n | sum dl | sum dl^2 over the kept pixels, dl = log(target) - log(pred)."""
    with np.errstate(all="ignore"):
        dl = np.log(np.asarray(target, F32)[keep].astype(np.float64)) - np.log(np.asarray(pred, F32)[keep].astype(np.float64))
        n = np.float64(dl.size)
        s1, s2 = dl.sum(), (dl * dl).sum()
        m1 = s1 / n
        return np.array([np.sqrt(s2 / n - lambd * (m1 * m1)), n, s1, s2], np.float64)


def silog_grad_ref(pred, target, keep, lambd, coeff=1.0) -> np.ndarray:
    """-> float64 of pred's shape: coeff * -(dl - lambd * mean) / (n * loss * pred) at kept pixels, 0 at dropped ones; coeff
    as float32. The device rounds this once to float32."""
    loss, n, s1, _ = silog_ref(pred, target, keep, lambd)
    pred = np.asarray(pred, F32)
    out = np.zeros(pred.shape, np.float64)
    with np.errstate(all="ignore"):
        p = pred[keep].astype(np.float64)
        dl = np.log(np.asarray(target, F32)[keep].astype(np.float64)) - np.log(p)
        out[keep] = np.float64(F32(coeff)) * (-(dl - lambd * (s1 / n)) / ((n * loss) * p))
    return out
