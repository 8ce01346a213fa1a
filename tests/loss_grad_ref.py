"""CPU restatement of the gradient of the reference's VideoDepthLoss with respect to its prediction, in numpy float64 on top
of the forward pieces of tests/loss_ref.py. This is the arithmetic contract of csrc/loss_grad.hip (include/vdn.h,
vdn_depth_loss_backward): what torch's autograd computes for

    L = w_total * total_loss + w_spatial * spatial_loss + w_stable * stable_loss + w_absRel * absRel_loss

(d1 is piecewise constant), with the two float32 roundings of the aligned prediction a = fl32(fl32(sc * p) + sh) given the
derivative 1. With c_sp = w_total + w_spatial, c_st = stable_scale * w_total + w_stable (the temporal term exists when
stable_scale > 0) and c_ar = w_absRel:

  g_x   at a kept pixel, d = x - y the difference of the normalised maps, M the kept pixels, M_k the kept points of grid k:
            c_sp * (sign(d) / M + alpha * (n_0 / M_0 + n_1 / M_1 + ...)),   n_k = sum over the pixel's kept neighbours at
        stride 2^k on grid k of sign(d_self - d_nb): an integer, since every pair |d_nb - d_self| of the forward has the
        derivative -sign(d_nb - d_self) at d_self whichever side the pixel is on. sign(0) = 0, as torch.abs' backward.
  per frame, x = (a - m) / s, s = max(s_raw, 1e-6), s_raw = sum_keep |a - m| / cnt:
        g_s = -sum g_x x / s   when cnt > 0 and s_raw >= 1e-6 (the clamp passes nothing below its bound), else 0
        g_m = -sum g_x / s - g_s * sigma / cnt,   sigma = sum_keep sign(a - m)     (d s / d m = -sigma / cnt)
  g_a = g_x / s + g_s * sign(a - m) / cnt
        + g_m at the median's holder: the kept pixel of lowest index with a == m; nobody when m == 0 and the frame has a
          dropped pixel (the median is then taken to be a dropped pixel's 0, where mask * a has the derivative 0), or when
          the frame keeps nothing
        + c_st * (sign(pg - tg) at the later frame's side of a counted pair - the same at the earlier frame's) / M_t
        + c_ar * sign(a - t) / (t * M_ar) where the forward counts the pixel
  through the fit, per item: G0 = sum g_a p, G1 = sum g_a, D = det + 1e-6,
        g_p = sc * g_a + keep * (G0 * (dN0 - sc * dD) + G1 * (dN1 - sh * dD)) / D
        dN0 = a11 t - b1, dN1 = -b0 - a01 t + 2 p b1, dD = 2 (p a11 - a01); 0 for an item with det == 0.

A dropped pixel's gradient is +0.0 and NaN or inf under it reaches nothing."""
from __future__ import annotations

import numpy as np

import loss_ref as R

F32 = np.float32
MAY_BE_ZERO = ("a-m", "x-y")   # signs whose argument is exactly 0 at the pixel that holds a frame's median, at most once a frame


def _sign_min(arg, where, mins, key):
    """sign(arg) where `where`, 0 elsewhere; records the smallest non-zero |arg| and the number of exact zeros under `key`."""
    with np.errstate(all="ignore"):
        s = np.where(where, np.sign(np.where(where, arg, 0.0)), 0.0)
        mag = np.abs(np.where(where, arg, np.inf))
    nz = mag[mag > 0]
    lo, zeros = mins.get(key, (np.inf, 0))
    mins[key] = (min(lo, float(nz.min()) if nz.size else np.inf), zeros + int((mag == 0).sum()))
    return s


def depth_loss_grad_ref(prediction, target, mask, alpha=0.5, scales=4, stable_scale=10, weights=(1.0, 0.0, 0.0, 0.0)):
    """prediction, target float32 [B, T, H, W]; mask non-zero = keep; weights = (total, spatial, stable, absRel).
    Returns dict(grad float64 [B, T, H, W], mag_a = |sc * g_a|, mag_fit = |fit correction| (both float64 [B, T, H, W], for
    the float32 bound of the device test), g_a, holder int64 [B, T] (flat index in the frame, -1 nobody), g_s, g_m float64
    [B, T], min_abs = {'x-y' | 'nb' | 'temporal' | 'a-t' | 'a-m': (smallest non-zero |argument| of a sign taken, number of
    arguments that are exactly 0)}, fwd = loss_ref.depth_loss_ref's dictionary)."""
    p32, t32 = np.asarray(prediction, F32), np.asarray(target, F32)
    B, T, H, W = p32.shape
    F = B * T
    keep = np.asarray(mask) != 0
    fwd = R.depth_loss_ref(p32, t32, keep, alpha=alpha, scales=scales, stable_scale=stable_scale)
    w_total, w_sp, w_st, w_ar = (float(w) for w in weights)
    temporal = stable_scale > 0
    c_sp, c_st, c_ar = w_total + w_sp, (stable_scale * w_total + w_st) if temporal else 0.0, w_ar
    sc32, sh32 = fwd["scale"], fwd["shift"]
    a32 = R.align_ref(p32, sc32, sh32)
    fl = lambda v: v.reshape(F, H, W)
    kf = fl(keep)
    a, t, p = a32.astype(np.float64), t32.astype(np.float64), p32.astype(np.float64)
    m, s = fwd["m_pred"].astype(np.float64).reshape(F, 1, 1), fwd["s_pred"].reshape(F, 1, 1)
    mt, st = fwd["m_target"].astype(np.float64).reshape(F, 1, 1), fwd["s_target"].reshape(F, 1, 1)
    cnt = fwd["count"].reshape(F).astype(np.float64)
    mins = {}
    with np.errstate(all="ignore"):
        x = np.where(kf, (fl(a) - m) / s, 0.0)
        d = np.where(kf, (fl(a) - m) / s - (fl(t) - mt) / st, 0.0)
    # ---- (i) g_x
    Mtot = float(keep.sum())
    sd = _sign_min(d, kf, mins, "x-y")
    reg = np.zeros((F, H, W))
    for k in range(scales if alpha > 0 else 0):
        step = 2 ** k
        dk, kk = d[:, ::step, ::step], kf[:, ::step, ::step]
        n = np.zeros(dk.shape)
        sx = _sign_min(dk[:, :, 1:] - dk[:, :, :-1], kk[:, :, 1:] & kk[:, :, :-1], mins, "nb")
        n[:, :, 1:] += sx
        n[:, :, :-1] -= sx
        sy = _sign_min(dk[:, 1:, :] - dk[:, :-1, :], kk[:, 1:, :] & kk[:, :-1, :], mins, "nb")
        n[:, 1:, :] += sy
        n[:, :-1, :] -= sy
        if fwd["M"][k] > 0:
            reg[:, ::step, ::step] += n / float(fwd["M"][k])         # k ascending: the device adds the grids in this order
    gx = np.where(kf, c_sp * ((sd / Mtot if Mtot else 0.0) + alpha * reg), 0.0) if Mtot else np.zeros((F, H, W))
    # ---- (ii) per frame
    sam = _sign_min(fl(a) - m, kf, mins, "a-m")
    with np.errstate(all="ignore"):
        s_raw = np.where(cnt > 0, np.where(kf, np.abs(fl(a) - m), 0.0).reshape(F, -1).sum(1) / np.maximum(cnt, 1), 0.0)
    live = (cnt > 0) & (s_raw >= 1e-6)
    s1, c1 = s.reshape(F), np.maximum(cnt, 1)
    g_s = np.where(live, -(gx * x).reshape(F, -1).sum(1) / s1, 0.0)
    sigma = sam.reshape(F, -1).sum(1)
    g_m = np.where(cnt > 0, -gx.reshape(F, -1).sum(1) / s1 - g_s * sigma / c1, 0.0)
    holder = np.full(F, -1, np.int64)
    for f in range(F):
        if cnt[f] > 0 and not (m[f, 0, 0] == 0 and cnt[f] < H * W):
            hit = np.flatnonzero(kf[f].ravel() & (fl(a32)[f].ravel() == F32(m[f, 0, 0])))
            holder[f] = hit[0] if hit.size else -1
    # ---- (iii) g_a
    g_a = np.where(kf, gx / s + g_s.reshape(F, 1, 1) * sam / c1.reshape(F, 1, 1), 0.0)
    for f in range(F):
        if holder[f] >= 0:
            g_a[f].reshape(-1)[holder[f]] += g_m[f]
    g_a = g_a.reshape(B, T, H, W)
    if temporal and fwd["stable_count"] > 0 and c_st != 0:
        with np.errstate(all="ignore"):
            tmin = np.where(keep, t32, F32(np.inf)).min((2, 3))
            tmax = np.where(keep, t32, F32(-np.inf)).max((2, 3))
            th = ((tmax - tmin).astype(F32) * F32(0.05)).astype(F32)
            pg = (a32[:, 1:] - a32[:, :-1]).astype(F32)
            tg = (t32[:, 1:] - t32[:, :-1]).astype(F32)
            k2 = keep[:, 1:] & keep[:, :-1] & (np.abs(tg) < th[:, 1:, None, None])
        assert int(k2.sum()) == fwd["stable_count"]
        sg = _sign_min(pg.astype(np.float64) - tg.astype(np.float64), k2, mins, "temporal")
        later, earlier = np.zeros((B, T, H, W)), np.zeros((B, T, H, W))
        later[:, 1:], earlier[:, :-1] = sg, sg
        g_a = g_a + np.where(keep, c_st * (later - earlier) / float(fwd["stable_count"]), 0.0)
    with np.errstate(all="ignore"):
        k3 = keep & (t32 > F32(1e-3)) & (t32 < F32(70))
    if fwd["absrel_count"] > 0 and c_ar != 0:
        sa = _sign_min(a - t, k3, mins, "a-t")
        with np.errstate(all="ignore"):
            g_a = g_a + np.where(k3, c_ar * sa / (t * float(fwd["absrel_count"])), 0.0)
    # ---- (iv) through the fit
    sc, sh = sc32.astype(np.float64).reshape(B, 1, 1, 1), sh32.astype(np.float64).reshape(B, 1, 1, 1)
    sums = lambda v: np.where(keep, v, 0.0).reshape(B, -1).sum(1).reshape(B, 1, 1, 1)
    with np.errstate(all="ignore"):
        a00, a01, a11, b0, b1 = sums(p * p), sums(p), sums(np.ones_like(p)), sums(p * t), sums(t)
        det = a00 * a11 - a01 * a01
        D = det + 1e-6
        G0, G1 = sums(g_a * p), sums(g_a)
        dN0 = a11 * t - b1
        dN1 = -b0 - a01 * t + 2.0 * p * b1
        dD = 2.0 * (p * a11 - a01)
        fit = np.where(keep & (det != 0), (G0 * (dN0 - sc * dD) + G1 * (dN1 - sh * dD)) / D, 0.0)
        direct = np.where(keep & (det != 0), sc * g_a, 0.0)
    grad = direct + fit + 0.0
    return dict(grad=grad, mag_a=np.abs(direct), mag_fit=np.abs(fit), g_a=g_a, holder=holder.reshape(B, T),
                g_s=g_s.reshape(B, T), g_m=g_m.reshape(B, T), min_abs=mins, fwd=fwd)
