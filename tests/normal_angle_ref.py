"""CPU restatement of vdn.normal_metrics and vdn.vis.colorize_normals (include/vdn.h, vdn_normal_angle_*): float64 numpy from
the float32 samples.

  * angle = arctan2(|a x b|, a . b) * 180 / pi, every product and sum rounded on its own in the order the header states. NaN
    when any component is NaN or inf, otherwise 90 when either vector is zero.
  * from_depth: b = (-Ix, -Iy, 1) of normal_ref.sobel_ref (Sobel / 8 on the reflect-padded float32 depth), not normalised.
  * kept pixels: the mask (None = all ones), through normal_ref.erode_ref when erode. Dropped pixels are selected away.
  * rows [1 + B + B T, 9] = n, mean, median, rmse, a5, a7_5, a11_25, a22_5, a30 of the batch, the items and the frames; the
    median is numpy.median of the angles rounded to float32, taken in float64; the shares compare the float64 angle, strictly.
  * the picture: byte = floor(((a_c / |a|) * 0.5 + 0.5) * 255 + 0.5), 128 for a zero or non-finite vector.

Also the seeded input maker of the tests: exactly rounded operations alone (integer hashes, dyadic weights, + - * / sqrt), so
every machine regenerates the same bits."""
from __future__ import annotations

import numpy as np

import normal_ref as R
from ssim_ref import _hash01, _smooth

NAMES = ["n", "mean", "median", "rmse", "a5", "a7_5", "a11_25", "a22_5", "a30"]
THRESHOLDS = (5.0, 7.5, 11.25, 22.5, 30.0)
DEG = 180.0 / np.pi


def angle_ref(a, b):
    """a, b [..., 3, H, W] (float32 values, any float dtype) -> the angle in degrees, float64 [..., H, W]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a0, a1, a2 = a[..., 0, :, :], a[..., 1, :, :], a[..., 2, :, :]
    b0, b1, b2 = b[..., 0, :, :], b[..., 1, :, :], b[..., 2, :, :]
    with np.errstate(all="ignore"):
        finite = np.isfinite(a).all(-3) & np.isfinite(b).all(-3)
        aa, bb = (a0 * a0 + a1 * a1) + a2 * a2, (b0 * b0 + b1 * b1) + b2 * b2
        cx, cy, cz = a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0
        d = (a0 * b0 + a1 * b1) + a2 * b2
        ang = np.arctan2(np.sqrt((cx * cx + cy * cy) + cz * cz), d) * DEG
    ang = np.where((aa == 0.0) | (bb == 0.0), 90.0, ang)
    return np.where(finite, ang, np.nan)


def depth_normal_ref(depth):
    """depth float32 [..., H, W] -> (-Ix, -Iy, 1) float64 [..., 3, H, W], not normalised."""
    ix, iy = R.sobel_ref(depth)
    return np.stack([-ix, -iy, np.ones_like(ix)], axis=-3)


def kept_ref(shape, mask, erode=True):
    m = np.ones(shape, bool) if mask is None else np.asarray(mask) != 0
    return R.erode_ref(m) if erode else m


def angle_map_ref(pred, target, mask=None, from_depth=False, erode=True):
    """pred float32 [B, T, 3, H, W]; target normals [B, T, 3, H, W] or depth [B, T, H, W] -> (the float64 angles [B, T, H, W]
    with NaN at a dropped pixel, the kept pixels as bool)."""
    a = np.asarray(pred, np.float32).astype(np.float64)
    b = depth_normal_ref(target) if from_depth else np.asarray(target, np.float32).astype(np.float64)
    keep = kept_ref(a.shape[:2] + a.shape[3:], mask, erode)
    return np.where(keep, angle_ref(a, b), np.nan), keep


def row_ref(ang, keep):
    """The nine numbers of one set: ang float64 and keep bool of the same shape."""
    v = ang[keep]
    n = v.size
    if n == 0 or np.isnan(v).any():
        return [float(n)] + [np.nan] * 8
    med = float(np.median(v.astype(np.float32).astype(np.float64)))
    return [float(n), float(v.mean()), med, float(np.sqrt((v * v).mean()))] + [float((v < t).sum()) / n for t in THRESHOLDS]


def stats_ref(ang, keep):
    """ang, keep [B, T, H, W] -> rows float64 [1 + B + B T, 9]."""
    B, T = ang.shape[:2]
    rows = [row_ref(ang, keep)] + [row_ref(ang[i], keep[i]) for i in range(B)]
    rows += [row_ref(ang[i, t], keep[i, t]) for i in range(B) for t in range(T)]
    return np.array(rows, np.float64)


def colorize_ref(x, from_depth=False, bgr=False):
    """x normals float32 [N, 3, H, W] or depth [N, H, W] -> (bytes uint8 [N, H, W, 3], the float64 v_c [N, H, W, 3] before the
    rounding, NaN where the vector is zero or not finite)."""
    a = depth_normal_ref(x) if from_depth else np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        aa = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        ok = np.isfinite(a).all(1) & (aa != 0.0)
        v = ((a / np.sqrt(aa)[:, None]) * 0.5 + 0.5) * 255.0
    v = np.where(ok[:, None], v, np.nan)
    with np.errstate(all="ignore"):
        byte = np.where(ok[:, None], np.floor(np.where(ok[:, None], v, 0.0) + 0.5), 128.0).astype(np.uint8)
    byte, v = np.moveaxis(byte, 1, -1), np.moveaxis(v, 1, -1)
    return (byte[..., ::-1], v[..., ::-1]) if bgr else (byte, v)


# ------------------------------------------------------------------------------------------------ seeded cases
MAX_TAN = 0.5625   # tan of half the largest rotation: 2 atan(0.5625) = 58.7 degrees


def make_depth(seed, shape):
    """A smooth positive depth with a little noise, float32 [B, T, H, W]."""
    B, T, H, W = shape
    d = np.empty(shape, np.float64)
    for f in range(B * T):
        s = seed * 1000 + f * 10
        d.reshape(B * T, H, W)[f] = (2.0 + 3.0 * _smooth(s, H, W) + 0.0625 * _hash01(s + 1, H * W).reshape(H, W)) * (min(H, W) * 0.25)
    return d.astype(np.float32)


def rotate(unit, tau):
    """unit [..., 3, H, W] of length one with uz > 0, tau [..., H, W] = tan(theta / 2) -> (1 + tau^2) times `unit` turned by
    theta towards w = (0, uz, -uy) / |.|, which is orthogonal to it: (1 - tau^2) unit + 2 tau w. + - * / sqrt alone."""
    uy, uz = unit[..., 1, :, :], unit[..., 2, :, :]
    w = np.stack([np.zeros_like(uy), uz, -uy], axis=-3) / np.sqrt(uz * uz + uy * uy)[..., None, :, :]
    t = tau[..., None, :, :]
    return (1.0 - t * t) * unit + (2.0 * t) * w


def make_case(seed, shape, keep_rate=0.7, mask_kind="bool"):
    """Seeded inputs: a depth, its unit normals times a hashed length as the stored target, and a prediction that is the
    unit normal turned by 0 .. 58.7 degrees (a smooth field times a hashed factor per pixel) times
    another hashed length, so that every threshold has pixels on both sides.
    -> dict(pred f32 [B,T,3,H,W], target f32 [B,T,3,H,W], depth f32 [B,T,H,W], mask bool or float32 [B,T,H,W])."""
    B, T, H, W = shape
    depth = make_depth(seed, shape)
    unit = R.normal_vector_ref(depth)
    tau, lt, lp = np.empty(shape), np.empty(shape), np.empty(shape)
    mask = np.empty(shape, bool)
    for f in range(B * T):
        s = seed * 1000 + f * 10
        sm = _smooth(s + 2, H, W) * _hash01(s + 3, H * W).reshape(H, W)
        tau.reshape(B * T, H, W)[f] = MAX_TAN * sm
        lt.reshape(B * T, H, W)[f] = 0.25 + 3.0 * _hash01(s + 4, H * W).reshape(H, W)
        lp.reshape(B * T, H, W)[f] = 0.5 + _hash01(s + 5, H * W).reshape(H, W)
        mask.reshape(B * T, H, W)[f] = _hash01(s + 6, H * W).reshape(H, W) < keep_rate
    pred = rotate(unit, tau) * lp[:, :, None]
    target = unit * lt[:, :, None]
    if mask_kind == "float":
        mask = mask.astype(np.float32)
    return dict(pred=pred.astype(np.float32), target=target.astype(np.float32), depth=depth, mask=mask)
