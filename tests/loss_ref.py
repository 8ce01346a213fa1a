"""CPU restatement of the reference's VideoDepthLoss (loss/loss.py:326-367, with trim = 0, batch-based reduction and no
SSIM term) for the tests of vdn.loss, in numpy. This is the arithmetic contract of csrc/loss.hip (include/vdn.h,
vdn_depth_loss): the fit and every sum in float64 from the float32 samples, and in np.float32 exactly the operations the
reference's float32 tensors decide something with:

  * scale and shift of the fit, rounded once;
  * the aligned prediction a = fl32(fl32(scale * p) + shift);
  * the lower median m (an input sample or 0, so exact);
  * the temporal threshold fl32(fl32(max - min) * 0.05f) and the frame differences fl32(a_t - a_{t-1}), fl32(t_t - t_{t-1});
  * the bounds 1e-3f, 70f on the target and the two float32 quotients and the bound 1.25f of d1.

Dropped pixels are selected away (np.where) before anything is summed, so NaN or inf under them reaches nothing; the
reference multiplies them by 0 and would carry the NaN into its sums.

Also the seeded input maker shared by tools/make_golden_loss.py and the tests (tests/golden/loss_cases.npz stores seeds and
arguments, not the inputs)."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def fit_ref(prediction, target, mask):
    """[B, ...] each -> float32 (scale [B], shift [B]): compute_scale_and_shift over each item's pixels, sums in float64."""
    B = prediction.shape[0]
    p = np.asarray(prediction, F32).astype(np.float64).reshape(B, -1)
    t = np.asarray(target, F32).astype(np.float64).reshape(B, -1)
    k = (np.asarray(mask) != 0).reshape(B, -1)
    with np.errstate(all="ignore"):
        a00 = np.where(k, p * p, 0.0).sum(1)
        a01 = np.where(k, p, 0.0).sum(1)
        a11 = k.sum(1).astype(np.float64)
        b0 = np.where(k, p * t, 0.0).sum(1)
        b1 = np.where(k, t, 0.0).sum(1)
        det = a00 * a11 - a01 * a01
        scale = np.where(det != 0, (a11 * b0 - a01 * b1) / (det + 1e-6), 0.0)
        shift = np.where(det != 0, (-a01 * b0 + a00 * b1) / (det + 1e-6), 0.0)
    return scale.astype(F32), shift.astype(F32)


def align_ref(prediction, scale, shift):
    """float32 [B, T, H, W]: two separately rounded float32 operations."""
    with np.errstate(all="ignore"):
        return (scale.reshape(-1, 1, 1, 1) * np.asarray(prediction, F32)).astype(F32) + shift.reshape(-1, 1, 1, 1)


def robust_ref(x, keep):
    """x float32 [F, H, W], keep bool -> (m float32 [F], s float64 [F], xn float64 [F, H, W])."""
    F = x.shape[0]
    n = keep.reshape(F, -1).sum(1)
    v = np.where(keep, x, F32(0)).reshape(F, -1)
    m = np.sort(v, axis=1)[:, (v.shape[1] - 1) // 2] + F32(0)      # the lower median; + 0 turns -0.0 into +0.0
    m = np.where(n > 0, m, F32(0)).astype(F32)
    x64, m64 = x.astype(np.float64), m.astype(np.float64).reshape(F, 1, 1)
    with np.errstate(all="ignore"):
        sq = np.where(keep, np.abs(x64 - m64), 0.0).reshape(F, -1).sum(1)
        s = np.where(n > 0, np.maximum(sq / np.maximum(n, 1), 1e-6), 1.0)
        return m, s, (x64 - m64) / s.reshape(F, 1, 1)


def gradient_ref(d, keep, scales):
    """d float64 [F, H, W] (an - tn), keep bool -> (g_k [scales], M_k [scales])."""
    g, M = np.zeros(scales), np.zeros(scales, np.int64)
    for k in range(scales):
        step = 2 ** k
        dk, kk = d[:, ::step, ::step], keep[:, ::step, ::step]
        with np.errstate(all="ignore"):
            gx = np.where(kk[:, :, 1:] & kk[:, :, :-1], np.abs(dk[:, :, 1:] - dk[:, :, :-1]), 0.0)
            gy = np.where(kk[:, 1:, :] & kk[:, :-1, :], np.abs(dk[:, 1:, :] - dk[:, :-1, :]), 0.0)
        M[k] = kk.sum()
        g[k] = (gx.sum() + gy.sum()) / M[k] if M[k] else 0.0
    return g, M


def depth_loss_ref(prediction, target, mask, alpha=0.5, scales=4, stable_scale=10):
    """prediction, target float32 [B, T, H, W]; mask [B, T, H, W], non-zero = keep. Returns a dict of float64 values:
    spatial_loss, stable_loss (when stable_scale > 0), absRel_loss, d1, total_loss, data, g [scales], M [scales] int64,
    m_pred, m_target float32 [B, T], s_pred, s_target float64 [B, T], count int64 [B, T], scale, shift float32 [B],
    d1_hits, absrel_count, stable_count (integers)."""
    p, t = np.asarray(prediction, F32), np.asarray(target, F32)
    B, T, H, W = p.shape
    keep = np.asarray(mask) != 0
    scale, shift = fit_ref(p, t, keep)
    a = align_ref(p, scale, shift)
    fl = lambda x: x.reshape(B * T, H, W)
    m_p, s_p, an = robust_ref(fl(a), fl(keep))
    m_t, s_t, tn = robust_ref(fl(t), fl(keep))
    n = int(keep.sum())
    with np.errstate(all="ignore"):
        d = an - tn
        data = float(np.where(fl(keep), np.abs(d), 0.0).sum()) / n if n else 0.0
    g, M = gradient_ref(d, fl(keep), scales) if alpha > 0 else (np.zeros(scales), np.zeros(scales, np.int64))
    out = dict(data=data, g=g, M=M, m_pred=m_p.reshape(B, T), m_target=m_t.reshape(B, T), s_pred=s_p.reshape(B, T),
               s_target=s_t.reshape(B, T), count=keep.sum((2, 3)).astype(np.int64), scale=scale, shift=shift)
    out["spatial_loss"] = data + (alpha * float(g.sum()) if alpha > 0 else 0.0)
    out["total_loss"] = out["spatial_loss"]
    if stable_scale > 0:
        if T < 2:
            raise ValueError("the temporal term needs T >= 2")
        with np.errstate(all="ignore"):
            tmin = np.where(keep, t, F32(np.inf)).min((2, 3))
            tmax = np.where(keep, t, F32(-np.inf)).max((2, 3))
            th = ((tmax - tmin).astype(F32) * F32(0.05)).astype(F32)
            pg = (a[:, 1:] - a[:, :-1]).astype(F32)
            tg = (t[:, 1:] - t[:, :-1]).astype(F32)
            k2 = keep[:, 1:] & keep[:, :-1] & (np.abs(tg) < th[:, 1:, None, None])
            c = int(k2.sum())
            out["stable_loss"] = float(np.where(k2, np.abs(pg.astype(np.float64) - tg.astype(np.float64)), 0.0).sum()) / c if c else 0.0
        out["stable_count"] = c
        out["total_loss"] = out["spatial_loss"] + stable_scale * out["stable_loss"]
    with np.errstate(all="ignore"):
        k3 = keep & (t > F32(1e-3)) & (t < F32(70))
        c3 = int(k3.sum())
        a64, t64 = a.astype(np.float64), t.astype(np.float64)
        out["absRel_loss"] = float(np.where(k3, np.abs((a64 - t64) / t64), 0.0).sum()) / c3 if c3 else 0.0
        hit = keep & (np.maximum((a / t).astype(F32), (t / a).astype(F32)) < F32(1.25))   # np.maximum keeps a NaN: false
        out["d1"] = float(hit.sum()) / n if n else 0.0
    out["absrel_count"], out["d1_hits"] = c3, int(hit.sum())
    return out


# ------------------------------------------------------------------------------------------------ seeded cases
def make_case(seed: int, shape, keep_rate=0.8, kind="plain", mask_dtype="bool", empty_frames=(), empty_items=(), frame_noise=0.2):
    """Seeded inputs of one case, shape = (B, T, H, W): dict(pred, target float32, mask bool | uint8 | float32).
    The target is a static scene per item plus frame noise of standard deviation frame_noise (at 0.2 the temporal threshold
    keeps most pixels and drops some); the prediction is an affine map of it, different per item, plus noise.
    kind: 'plain' | 'anti' (negative slope; the target straddles 0, so the zeros of dropped pixels sort into the middle)
          | 'straddle' (W >= 5: the first five pixels of every frame are kept targets 0, 5e-4, 1.5e-3, 69.5 and 71)."""
    B, T, H, W = shape
    rng = np.random.default_rng(seed)
    base = rng.uniform(1.0, 10.0, (B, 1, H, W))
    target = base + frame_noise * rng.standard_normal(shape)
    slope = rng.uniform(0.5, 2.0, (B, 1, 1, 1)) * (-1.0 if kind == "anti" else 1.0)
    offset = rng.uniform(-1.0, 1.0, (B, 1, 1, 1))
    u = rng.random(shape)
    mask = np.ones(shape, bool) if keep_rate >= 1.0 else u < keep_rate
    if kind == "anti":
        target = target - 5.5
    elif kind == "straddle":
        target[:, :, 0, :5] = (0.0, 5e-4, 1.5e-3, 69.5, 71.0)
        mask[:, :, 0, :5] = True
    elif kind != "plain":
        raise ValueError(kind)
    pred = (target - offset) / slope + 0.15 * rng.standard_normal(shape) * np.abs(1.0 / slope)
    for f in empty_frames:
        mask.reshape(B * T, H, W)[f] = False
    for b in empty_items:
        mask[b] = False
    mask = {"bool": mask, "uint8": mask.astype(np.uint8), "float": mask.astype(np.float32)}[mask_dtype]
    return dict(pred=pred.astype(F32), target=target.astype(F32), mask=mask)


def checksum(case) -> list:
    return [float(case[k].astype(np.float64).sum()) for k in ("pred", "target", "mask")]
