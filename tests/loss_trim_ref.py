"""CPU restatement of the reference's VideoDepthLoss with trim > 0 (loss/loss.py:164-219 and 326-367, batch-based reduction, no
SSIM term) and of its gradient with respect to the prediction, in numpy, on top of tests/loss_ref.py and tests/loss_grad_ref.py.
This is the arithmetic contract of vdn_depth_loss_trimmed and vdn_depth_loss_trimmed_backward (include/vdn.h). Only the
selection and the weights u are new; the fit, the alignment, the robust normalisation, the grids g_k, d1 and every count are
loss_ref's.

For each of three sets of counted residuals |r| (fp64, as loss_ref sums them)
    data    |an - tn| over the kept pixels                         n = kept pixels
    stable  |pg - tg| over the counted temporal pairs              n = stable_count
    absRel  |(a - t) / t| over the pixels absRel counts            n = absrel_count
the reference sorts, keeps the first k = int(n * (1.0 - trim)) and divides their sum by n. Here:
    rank    keep = 1.0 - trim (a Python float), k = int(n * keep);
    key     the float32 rounding of |r|, compared by its bit pattern (non-negative, so ordered); every NaN is the one key
            0x7FC00000, above +inf's, as torch.sort puts it; uncounted elements have no key;
    thr     the key of rank k - 1; n_less = #{key < thr}, n_tied = #{key == thr}, w = (k - n_less) / n_tied;
    term    (sum_{key < thr} |r| + w * sum_{key == thr} |r|) / n, 0 when k == 0;
    u       per counted element: 1 where key < thr, w where key == thr, 0 otherwise (all 0 when k == 0).
The reference keeps an arbitrary k - n_less of the tied elements (its sort is not stable); they are equal to float32, so w
gives its value to float32 rounding, and the same bits on every run.

Gradient: u multiplies the three terms of loss_grad_ref's chain,
    g_x data part      c_sp * u * sign(d) / M
    stable part of g_a c_st * (u e at the later frame's pixel - u e at the earlier frame's) / stable_count, e = sign(pg - tg)
    absRel part of g_a c_ar * u * sign(a - t) / (t * absrel_count)
and the regulariser, the frame chain and the fit chain follow unchanged. With every u = 1 this is loss_grad_ref."""
from __future__ import annotations

import numpy as np

import loss_grad_ref as G
import loss_ref as R

F32 = np.float32
TERMS = ("data", "stable", "absRel")
NAN_KEY = np.uint32(0x7FC00000)


def keys_of(r):
    """float64 |r| -> uint32 keys."""
    with np.errstate(all="ignore"):
        v = np.asarray(r, np.float64).astype(F32)
    k = v.view(np.uint32).copy()
    k[np.isnan(v)] = NAN_KEY
    return k


def select_ref(r, counted, keep):
    """r float64 (any shape), counted bool of that shape, keep = 1.0 - trim -> dict(k, n_less, n_tied, thr (float64 value of the
    float32 threshold), w, term, u float64 of r's shape)."""
    n = int(counted.sum())
    k = int(n * keep)
    u = np.zeros(r.shape)
    if k <= 0:
        return dict(k=0, n_less=0, n_tied=0, thr=0.0, w=0.0, term=0.0, u=u, n=n)
    rc = r[counted]
    kb = keys_of(rc)
    thr = np.sort(kb)[k - 1]
    less, tied = kb < thr, kb == thr
    n_less, n_tied = int(less.sum()), int(tied.sum())
    w = (k - n_less) / n_tied
    with np.errstate(all="ignore"):
        term = (float(rc[less].sum()) + w * float(rc[tied].sum())) / n
    u[counted] = np.where(less, 1.0, np.where(tied, w, 0.0))
    return dict(k=k, n_less=n_less, n_tied=n_tied, thr=float(np.array([thr], np.uint32).view(F32)[0]), w=w, term=term, u=u, n=n)


def residuals_ref(p, t, keep, fwd, stable_scale):
    """The three residual sets from loss_ref's state -> {term: (r float64, counted bool)}; data and absRel [B, T, H, W], stable
    [B, T - 1, H, W] (pair (t, t + 1) at index t)."""
    B, T, H, W = p.shape
    a = R.align_ref(p, fwd["scale"], fwd["shift"])
    a64, t64 = a.astype(np.float64), t.astype(np.float64)
    sh = lambda v: np.asarray(v, np.float64).reshape(B, T, 1, 1)
    with np.errstate(all="ignore"):
        d = (a64 - sh(fwd["m_pred"])) / sh(fwd["s_pred"]) - (t64 - sh(fwd["m_target"])) / sh(fwd["s_target"])
        out = {"data": (np.abs(d), keep)}
        k3 = keep & (t > F32(1e-3)) & (t < F32(70))
        out["absRel"] = (np.abs((a64 - t64) / t64), k3)
        if stable_scale > 0:
            tmin = np.where(keep, t, F32(np.inf)).min((2, 3))
            tmax = np.where(keep, t, F32(-np.inf)).max((2, 3))
            th = ((tmax - tmin).astype(F32) * F32(0.05)).astype(F32)
            pg = (a[:, 1:] - a[:, :-1]).astype(F32)
            tg = (t[:, 1:] - t[:, :-1]).astype(F32)
            k2 = keep[:, 1:] & keep[:, :-1] & (np.abs(tg) < th[:, 1:, None, None])
            out["stable"] = (np.abs(pg.astype(np.float64) - tg.astype(np.float64)), k2)
        else:
            out["stable"] = (np.zeros((B, max(T - 1, 0), H, W)), np.zeros((B, max(T - 1, 0), H, W), bool))
    return out


def depth_loss_trim_ref(prediction, target, mask, alpha=0.5, scales=4, stable_scale=10, trim=0.2):
    """loss_ref.depth_loss_ref's dictionary with the trimmed spatial_loss, stable_loss, absRel_loss, total_loss and data, plus
    trim_k, trim_less, trim_tied (int64 [3]), trim_threshold, trim_weight (float64 [3]) in the order of TERMS and 'sel' =
    {term: select_ref's dictionary} (the weights u for the gradient)."""
    if not 0 <= trim < 1:
        raise ValueError(trim)
    keep_frac = 1.0 - trim
    p, t = np.asarray(prediction, F32), np.asarray(target, F32)
    keep = np.asarray(mask) != 0
    out = R.depth_loss_ref(p, t, keep, alpha=alpha, scales=scales, stable_scale=stable_scale)
    res = residuals_ref(p, t, keep, out, stable_scale)
    sel = {k: select_ref(res[k][0], res[k][1], keep_frac) for k in TERMS}
    assert sel["data"]["n"] == int(keep.sum()) and sel["absRel"]["n"] == out["absrel_count"]
    assert stable_scale <= 0 or sel["stable"]["n"] == out["stable_count"]
    out["data"] = sel["data"]["term"]
    out["spatial_loss"] = out["data"] + (alpha * float(out["g"].sum()) if alpha > 0 else 0.0)
    out["absRel_loss"] = sel["absRel"]["term"]
    out["total_loss"] = out["spatial_loss"]
    if stable_scale > 0:
        out["stable_loss"] = sel["stable"]["term"]
        out["total_loss"] = out["spatial_loss"] + stable_scale * out["stable_loss"]
    out.update(trim_k=np.array([sel[k]["k"] for k in TERMS], np.int64), trim_less=np.array([sel[k]["n_less"] for k in TERMS], np.int64),
               trim_tied=np.array([sel[k]["n_tied"] for k in TERMS], np.int64), trim_threshold=np.array([sel[k]["thr"] for k in TERMS]),
               trim_weight=np.array([sel[k]["w"] for k in TERMS]), sel=sel)
    return out


def depth_loss_trim_grad_ref(prediction, target, mask, alpha=0.5, scales=4, stable_scale=10, weights=(1.0, 0.0, 0.0, 0.0), trim=0.2):
    """As loss_grad_ref.depth_loss_grad_ref (the same dictionary, without min_abs) for the trimmed criterion; fwd is
    depth_loss_trim_ref's dictionary."""
    p32, t32 = np.asarray(prediction, F32), np.asarray(target, F32)
    B, T, H, W = p32.shape
    F = B * T
    keep = np.asarray(mask) != 0
    fwd = depth_loss_trim_ref(p32, t32, keep, alpha=alpha, scales=scales, stable_scale=stable_scale, trim=trim)
    sel = fwd["sel"]
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
    # ---- (i) g_x: the data part weighted by u, the regulariser as it was
    Mtot = float(keep.sum())
    sd = G._sign_min(d, kf, mins, "x-y") * fl(sel["data"]["u"])
    reg = np.zeros((F, H, W))
    for k in range(scales if alpha > 0 else 0):
        step = 2 ** k
        dk, kk = d[:, ::step, ::step], kf[:, ::step, ::step]
        n = np.zeros(dk.shape)
        sx = G._sign_min(dk[:, :, 1:] - dk[:, :, :-1], kk[:, :, 1:] & kk[:, :, :-1], mins, "nb")
        n[:, :, 1:] += sx
        n[:, :, :-1] -= sx
        sy = G._sign_min(dk[:, 1:, :] - dk[:, :-1, :], kk[:, 1:, :] & kk[:, :-1, :], mins, "nb")
        n[:, 1:, :] += sy
        n[:, :-1, :] -= sy
        if fwd["M"][k] > 0:
            reg[:, ::step, ::step] += n / float(fwd["M"][k])
    gx = np.where(kf, c_sp * (sd / Mtot + alpha * reg), 0.0) if Mtot else np.zeros((F, H, W))
    # ---- (ii) per frame
    sam = G._sign_min(fl(a) - m, kf, mins, "a-m")
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
        res = residuals_ref(p32, t32, keep, fwd, stable_scale)
        k2 = res["stable"][1]
        with np.errstate(all="ignore"):
            pg = (a32[:, 1:] - a32[:, :-1]).astype(F32)
            tg = (t32[:, 1:] - t32[:, :-1]).astype(F32)
        sg = G._sign_min(pg.astype(np.float64) - tg.astype(np.float64), k2, mins, "temporal") * sel["stable"]["u"]
        later, earlier = np.zeros((B, T, H, W)), np.zeros((B, T, H, W))
        later[:, 1:], earlier[:, :-1] = sg, sg
        g_a = g_a + np.where(keep, c_st * (later - earlier) / float(fwd["stable_count"]), 0.0)
    with np.errstate(all="ignore"):
        k3 = keep & (t32 > F32(1e-3)) & (t32 < F32(70))
    if fwd["absrel_count"] > 0 and c_ar != 0:
        sa = G._sign_min(a - t, k3, mins, "a-t") * sel["absRel"]["u"]
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
                g_s=g_s.reshape(B, T), g_m=g_m.reshape(B, T), fwd=fwd)


# ------------------------------------------------------------------------------------------------ constructed cases
def data_selection_is_stable(prediction, target, mask, alpha=0.5, scales=4, stable_scale=10, trim=0.2, ulps=4):
    """True when moving every per-frame scale s of the robust normalisation by +-ulps fp64 ulps (both maps, all four sign
    combinations) changes none of thr, n_less, n_tied of the data term: the device sums s in another order than numpy, and a
    case used for an exact comparison of the selection must not hang on that. The stable and absRel residuals are exact
    functions of float32 values and need no such guard."""
    p, t = np.asarray(prediction, F32), np.asarray(target, F32)
    keep = np.asarray(mask) != 0
    fwd = R.depth_loss_ref(p, t, keep, alpha=alpha, scales=scales, stable_scale=stable_scale)
    base = None
    for dp in (0, ulps, -ulps):
        for dt in (0, ulps, -ulps):
            moved = dict(fwd)
            for key, d in (("s_pred", dp), ("s_target", dt)):
                s = fwd[key].copy()
                for _ in range(abs(d)):
                    s = np.nextafter(s, np.inf if d > 0 else -np.inf)
                moved[key] = s
            r, counted = residuals_ref(p, t, keep, moved, stable_scale)["data"]
            sel = select_ref(r, counted, 1.0 - trim)
            got = (sel["thr"], sel["n_less"], sel["n_tied"])
            base = got if base is None else base
            if got != base:
                return False
    return True


def make_tie_case():
    """[1, 2, 8, 8], values on multiples of 1/8, many residuals on every threshold. The left half of each frame is kept, so both
    medians are exactly 0 (the 32 zeros of the dropped pixels sort first). The target is 1, 2 or 4 at a kept pixel (powers of
    two, so every absRel ratio is the difference times an exact power of two) and the same in both frames; the prediction is
    the target plus e, e in {0, +-1/2, +-1}, with every prediction value shared by a pixel with +e and one with -e: e is
    orthogonal to 1 and to the prediction, so the fit is exactly scale 1 and shift 0 (both round to that in float32), and the
    kept means of both maps are 2 in each frame, so both normalisation scales are 2. The roles rotate between the frames,
    which spreads |pg - tg| = |e_1 - e_0| over {0, 1/2, 1, 3/2}. (A target that is one constant over a frame's kept pixels
    would make the temporal threshold 0.05 * (max - min) = 0 and the stable term empty, and a fit of scale 1 impossible; three
    powers of two, static in time, keep the ratios exact and all three terms tied.)"""
    roles = {1.0: [(+0.5)] * 4 + [0.0] * 8, 2.0: [(-0.5)] * 4 + [(+1.0)] * 4 + [0.0] * 6, 4.0: [(-1.0)] * 4 + [0.0] * 2}
    tk = np.array([1.0] * 12 + [2.0] * 14 + [4.0] * 6)
    order = np.random.default_rng(7).permutation(32)           # where the 32 kept pixels of a frame sit; the same in both
    target, pred = np.full((1, 2, 8, 8), 3.0), np.full((1, 2, 8, 8), 5.0)
    mask = np.zeros((1, 2, 8, 8), bool)
    mask[..., :4] = True
    for f in range(2):
        e = np.zeros(32)
        for tv, r in roles.items():
            idx = np.flatnonzero(tk == tv)
            e[idx] = np.roll(r, 3 * f)
        tt, pp = np.empty(32), np.empty(32)
        tt[order], pp[order] = tk, tk + e
        target[0, f, :, :4], pred[0, f, :, :4] = tt.reshape(8, 4), pp.reshape(8, 4)
    return dict(pred=pred.astype(F32), target=target.astype(F32), mask=mask)


def make_last_pass_case():
    """[1, 2, 16, 16], everything kept: the absRel residuals are 1 + j * 2^-22 = 1 + i * 2^-23, i = 2 j < 256, so all their keys
    share the top 22 bits and the select's last pass alone tells them apart. Per frame 64 pixels have the target 64 and the
    prediction 128 + j * 2^-16 (the ratio (p - 64) / 64 is exact); each has a partner with the same prediction and the target
    2 p - 64 > 70, which absRel does not count, so that e = p - t is orthogonal to 1 and to p and the fit is scale 1, shift 0
    to float32 (a = p bit for bit). 64 more pairs at the prediction 100 with targets 72 and 128 give the fit its conditioning."""
    pred, target = np.empty((1, 2, 256)), np.empty((1, 2, 256))
    for f in range(2):
        fine = 128.0 + (64 * f + np.arange(64)) * 2.0 ** -16
        pred[0, f] = np.concatenate([fine, fine, np.full(128, 100.0)])
        target[0, f] = np.concatenate([np.full(64, 64.0), 2.0 * fine - 64.0, np.full(64, 72.0), np.full(64, 128.0)])
    shape = (1, 2, 16, 16)
    return dict(pred=pred.reshape(shape).astype(F32), target=target.reshape(shape).astype(F32), mask=np.ones(shape, bool))
