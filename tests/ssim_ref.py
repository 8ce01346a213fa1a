"""CPU restatement of the SSIM term of the reference's depth criterion (loss/loss.py:296-323, DepthShallowSSIMLoss with the
weights [1, 0, 0, 0, 0] its VideoDepthLoss constructs it with) and of its gradient with respect to the prediction, in numpy.
This is the arithmetic contract of csrc/ssim.hip (include/vdn.h, vdn_ssim_loss and vdn_ssim_loss_backward).

Forward. In float32, as the reference's tensors: the aligned prediction a = fl32(fl32(scale * p) + shift) when a fit is given
(a = p otherwise); per item the maximum over the kept a and the kept targets, 0 taking part when the item drops a pixel (the
reference multiplies by the mask), then max(., 1e-8f); x = fl32(a / max_val), y = fl32(t / max_val). From there float64: the
eleven taps of WINDOW (float32 values widened) filter x, y, x^2, y^2, x y without padding, along H and then W (order="HW";
"WH" is the other order, for the floor of the device test), cs = (2 (e12 - mu1 mu2) + C2) / ((e11 - mu1^2) + (e22 - mu2^2) +
C2), cs_f the mean over the (H - 10)(W - 10) outputs of a frame, loss = 1 - mean_f relu(cs_f). The four pooled levels of
MS_SSIM enter its product as value ** 0 == 1 with a zero gradient and are not computed.

Gradient of coeff * loss. With P = 1 / D, Q = A / D^2 (A, D the numerator and denominator of cs) and T(.) the transpose of the
valid filter (zero outside the outputs), for a frame with cs_f > 0 and w = -coeff / (F (H - 10)(W - 10)):
    g_x = 2 w (y T(P) - T(mu2 P) - x T(Q) + T(mu1 Q)),      g_y its mirror image,
and exactly nothing for a frame that relu gates. Through the maximum: dL/dmax_val = -sum_j (g_x x + g_y y)_j / max_val over
the item, which the filter's adjoint turns into the closed form the device evaluates,
    sum_j (g_x x + g_y y)_j = 2 C2 w sum_o (A - D) / D^2                                   (both are computed here),
given with weight 1 to the lowest-index kept prediction pixel that holds the maximum, 1/2 when the target's maximum equals
it (torch.max's rule), 0 when the target, a dropped pixel's zero or the clamp holds it. g_a = g_x / max_val + that term.
Through the fit (when given): g_p = sc g_a + keep (G0 (dN0 - sc dD) + G1 (dN1 - sh dD)) / D_fit with G0 = sum g_a p and G1 =
sum g_a over ALL the item's pixels, the sums of the fit over the kept ones; 0 for an item with det == 0."""
from __future__ import annotations

import numpy as np

import loss_ref as R

F32 = np.float32
C2 = 0.03 ** 2
HALO = 10
# torch.exp(-(k - 5)^2 / (2 * 1.5^2)) / sum in float32, k = 0 .. 10: the library's _fspecial_gauss_1d(11, 1.5)
WINDOW = np.array([float.fromhex(h) for h in (
    "0x1.0d9570p-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.106560p-2", "0x1.b43c3ep-3",
    "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8", "0x1.0d9570p-10")], np.float64)
HOLDERS = ("prediction", "target", "dropped", "clamp", "tie")   # the codes 0 .. 4 of the state's second slot


def _valid(z, axis):
    """The eleven taps along `axis` without padding, taps in ascending order."""
    axis %= z.ndim
    n = z.shape[axis] - HALO
    out = np.zeros(z.shape[:axis] + (n,) + z.shape[axis + 1:])
    for k in range(11):
        out = out + WINDOW[k] * np.take(z, range(k, k + n), axis=axis)
    return out


def _full(z, axis):
    """The transpose of _valid along `axis`: out[i] = sum_k g_k z[i - k], zero outside."""
    axis %= z.ndim
    n = z.shape[axis]
    pad = [(0, 0)] * z.ndim
    pad[axis] = (HALO, HALO)
    zp = np.pad(z, pad)
    out = np.zeros(z.shape[:axis] + (n + HALO,) + z.shape[axis + 1:])
    for k in range(11):
        out = out + WINDOW[k] * np.take(zp, range(HALO - k, HALO - k + n + HALO), axis=axis)
    return out


def filt(z, order="HW", full=False):
    f = _full if full else _valid
    a, b = (-2, -1) if order == "HW" else (-1, -2)
    return f(f(z, a), b)


def item_max(a32, t32, keep):
    """Per item of float32 [B, ...]: (max_val float32 after the clamp, holder code, weight of the prediction's path, flat index
    in the item of the kept prediction pixel that holds the prediction's maximum or -1)."""
    B = a32.shape[0]
    mv, code, weight, index = np.zeros(B, F32), np.zeros(B, np.int64), np.zeros(B), np.full(B, -1, np.int64)
    for b in range(B):
        a, t, k = a32[b].ravel(), t32[b].ravel(), keep[b].ravel()
        dropped = not k.all()
        pm = a[k].max() if k.any() else F32(-np.inf)
        tm = t[k].max() if k.any() else F32(-np.inf)
        kept_holds = k.any()
        if dropped:
            first_drop = int(np.flatnonzero(~k)[0])
            if pm < 0 or not k.any():
                kept_holds = False
            elif pm == 0:
                kept_holds = int(np.flatnonzero(k & (a == pm))[0]) < first_drop
            pm, tm = max(pm, F32(0)), max(tm, F32(0))
        m = max(pm, tm)
        mv[b] = max(m, F32(1e-8))
        if tm > pm:
            code[b] = 3 if m < F32(1e-8) else 1
        elif not kept_holds:
            code[b] = 2            # a maximum of 0, which the clamp then raises: no gradient either way
        elif m < F32(1e-8):
            code[b] = 3
        else:
            code[b], weight[b] = (4, 0.5) if tm == pm else (0, 1.0)
        if kept_holds:
            index[b] = int(np.flatnonzero(k & (a == a[k].max()))[0])
    return mv, code, weight, index


def _prepare(prediction, target, mask, fit):
    p32, t32 = np.asarray(prediction, F32), np.asarray(target, F32)
    keep = np.asarray(mask) != 0
    B = p32.shape[0]
    if fit is None:
        a32 = p32
    else:
        a32 = R.align_ref(p32, np.asarray(fit[0], F32), np.asarray(fit[1], F32)).astype(F32)
    mv, code, weight, index = item_max(a32, t32, keep)
    with np.errstate(all="ignore"):
        x = (a32 / mv.reshape(B, 1, 1, 1)).astype(F32).astype(np.float64)
        y = (t32 / mv.reshape(B, 1, 1, 1)).astype(F32).astype(np.float64)
    return p32, t32, keep, a32, mv, code, weight, index, x, y


def _maps(x, y, order):
    mu1, mu2, e11, e22, e12 = (filt(z, order) for z in (x, y, x * x, y * y, x * y))
    A = 2.0 * (e12 - mu1 * mu2) + C2
    D = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + C2
    return mu1, mu2, A, D


def ssim_ref(prediction, target, mask, fit=None, order="HW"):
    """prediction, target float32 [B, T, H, W], mask non-zero = keep, fit None or (scale [B], shift [B]) float32.
    -> dict(loss, mean_cs, gated (frames with cs_f <= 0 or NaN), cs float64 [B, T], max_val float32 [B], holder int64 [B]
    (index into HOLDERS), weight float64 [B], index int64 [B])."""
    p32, t32, keep, a32, mv, code, weight, index, x, y = _prepare(prediction, target, mask, fit)
    B, T, H, W = p32.shape
    _, _, A, D = _maps(x, y, order)
    cs = (A / D).reshape(B, T, -1).sum(2) / float((H - HALO) * (W - HALO))
    live = cs > 0
    mean_cs = float(np.where(live, cs, 0.0).sum() / (B * T))
    return dict(loss=1.0 - mean_cs, mean_cs=mean_cs, gated=int((~live).sum()), cs=cs, max_val=mv, holder=code, weight=weight,
                index=index)


def ssim_grad_ref(prediction, target, mask, fit=None, coeff=1.0, order="HW", prior=None):
    """The gradient of coeff * loss with respect to the prediction (added to `prior`, float32, when given) -> dict(grad float64
    [B, T, H, W]; mag: |sc g_x / max_val| + |sc max-path term| + |fit correction| (+ |prior|), for the float32 bound; parts:
    the sum of the magnitudes of the four adjoint parts of sc g_x / max_val and of the maximum's term (plus, through the fit, of what the item-wide sums
    G0 and G1 carry of them into the pixel's correction), for the fp64 floor; g_x, g_a; hold [B] the term
    given to each item's holder; dmax_direct, dmax_closed [B]: dL/dmax_val by the sum over pixels and by the closed form; fwd)."""
    p32, t32, keep, a32, mv, code, weight, index, x, y = _prepare(prediction, target, mask, fit)
    B, T, H, W = p32.shape
    n_out = float((H - HALO) * (W - HALO))
    mu1, mu2, A, D = _maps(x, y, order)
    cs = (A / D).reshape(B, T, -1).sum(2) / n_out
    w = np.where(cs > 0, -float(coeff) / (B * T * n_out), 0.0).reshape(B, T, 1, 1)
    P, Q = 1.0 / D, A / (D * D)
    FP, FQ = filt(P, order, True), filt(Q, order, True)
    parts_x = [y * FP, -filt(mu2 * P, order, True), -x * FQ, filt(mu1 * Q, order, True)]
    parts_y = [x * FP, -filt(mu1 * P, order, True), -y * FQ, filt(mu2 * Q, order, True)]
    g_x = 2.0 * w * (parts_x[0] + parts_x[1] + parts_x[2] + parts_x[3])
    g_y = 2.0 * w * (parts_y[0] + parts_y[1] + parts_y[2] + parts_y[3])
    mvd = mv.astype(np.float64)
    dmax_direct = -(g_x * x + g_y * y).reshape(B, -1).sum(1) / mvd
    S = ((A - D) / (D * D)).reshape(B, T, -1).sum(2)
    dmax_closed = -(2.0 * C2 * (w.reshape(B, T) * S).sum(1)) / mvd
    hold = weight * dmax_closed
    g_a = g_x / mvd.reshape(B, 1, 1, 1)
    holder_term = np.zeros((B, T * H * W))
    for b in range(B):
        if weight[b] != 0:
            holder_term[b, index[b]] = hold[b]
    holder_term = holder_term.reshape(B, T, H, W)
    parts = 2.0 * np.abs(w) * sum(np.abs(q) for q in parts_x) / mvd.reshape(B, 1, 1, 1) + np.abs(holder_term)
    if fit is None:
        grad, mag = g_a + holder_term, np.abs(g_a) + np.abs(holder_term)
    else:
        g_a = g_a + holder_term
        sc = np.asarray(fit[0], F32).astype(np.float64).reshape(B, 1, 1, 1)
        sh = np.asarray(fit[1], F32).astype(np.float64).reshape(B, 1, 1, 1)
        p, t = p32.astype(np.float64), t32.astype(np.float64)
        sums = lambda v: np.where(keep, v, 0.0).reshape(B, -1).sum(1).reshape(B, 1, 1, 1)
        total = lambda v: v.reshape(B, -1).sum(1).reshape(B, 1, 1, 1)
        with np.errstate(all="ignore"):
            a00, a01, a11, b0, b1 = sums(p * p), sums(p), sums(np.ones_like(p)), sums(p * t), sums(t)
            det = a00 * a11 - a01 * a01
            Dfit = det + 1e-6
            G0, G1 = total(g_a * p), total(g_a)
            dN0 = a11 * t - b1
            dN1 = -b0 - a01 * t + 2.0 * p * b1
            dD = 2.0 * (p * a11 - a01)
            corr = np.where(keep & (det != 0), (G0 * (dN0 - sc * dD) + G1 * (dN1 - sh * dD)) / Dfit, 0.0)
            # what the two item-wide sums carry into every kept pixel's correction: the parts' magnitudes, summed as G0 and G1 are
            parts_fit = np.where(keep & (det != 0), (total(parts * np.abs(p)) * np.abs(dN0 - sc * dD)
                                                    + total(parts) * np.abs(dN1 - sh * dD)) / np.abs(Dfit), 0.0)
        ok = det != 0
        grad = np.where(ok, sc * g_a, 0.0) + corr
        mag = np.where(ok, np.abs(sc * (g_a - holder_term)) + np.abs(sc * holder_term), 0.0) + np.abs(corr)
        parts = np.where(ok, np.abs(sc) * parts, 0.0) + parts_fit
        g_a = g_a - holder_term
    if prior is not None:
        grad = grad + np.asarray(prior, F32).astype(np.float64)
        mag = mag + np.abs(np.asarray(prior, F32).astype(np.float64))
    return dict(grad=grad + 0.0, mag=mag, parts=parts, g_x=g_x, g_a=g_a, hold=hold, dmax_direct=dmax_direct, dmax_closed=dmax_closed,
                fwd=dict(cs=cs, max_val=mv, holder=code, weight=weight, index=index, gated=int((~(cs > 0)).sum()),
                         loss=1.0 - float(np.where(cs > 0, cs, 0.0).sum() / (B * T))))


def fp64_floor(prediction, target, mask, fit=None, coeff=1.0):
    """The largest difference between the two summation orders of the gradient, relative to the sum of the adjoint parts'
    magnitudes (where that sum is not zero): what fp64 leaves of the cancelling parts. The device test allows 8 times it."""
    a = ssim_grad_ref(prediction, target, mask, fit, coeff, "HW")
    b = ssim_grad_ref(prediction, target, mask, fit, coeff, "WH")
    live = a["parts"] > 0
    return float((np.abs(a["grad"] - b["grad"])[live] / a["parts"][live]).max()) if live.any() else 0.0


def _hash01(seed, n):
    """n reproducible values k / 2^24 in [0, 1): splitmix64 of the index, in integer arithmetic alone."""
    h = np.arange(n, dtype=np.uint64) + np.uint64(seed * 0x9E3779B97F4A7C15 % (1 << 64))
    h = (h ^ (h >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    h = (h ^ (h >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    h = h ^ (h >> np.uint64(31))
    return (h >> np.uint64(40)).astype(np.float64) / float(1 << 24)


def _smooth(seed, H, W, cell=8):
    """A field in [0, 1) with structure at the window's scale: hashed values on a grid of `cell` pixels, blended bilinearly
    with the dyadic weights k / cell. Every product and sum is exact in float64."""
    gh, gw = H // cell + 2, W // cell + 2
    g = _hash01(seed, gh * gw).reshape(gh, gw)
    yi, xi = np.arange(H) // cell, np.arange(W) // cell
    fy, fx = ((np.arange(H) % cell) / float(cell))[:, None], ((np.arange(W) % cell) / float(cell))[None, :]
    g00, g01, g10, g11 = g[yi][:, xi], g[yi][:, xi + 1], g[yi + 1][:, xi], g[yi + 1][:, xi + 1]
    return (g00 * (1 - fx) + g01 * fx) * (1 - fy) + (g10 * (1 - fx) + g11 * fx) * fy


def make_case(seed, shape, keep_rate=0.875, inverse=(), gain=1.0):
    """Seeded inputs made of exactly rounded operations alone (integer hashes, dyadic weights), so every machine regenerates
    the same bits: a smooth positive target with noise, a prediction that is an affine map of it plus its own smooth field and
    noise, times `gain` (1.5 puts the item's maximum in the prediction), a hashed mask. inverse: the (item, frame) pairs whose prediction is the contrast inverse of the target and whose pixels are all dropped, so
    that the fit does not see them and the SSIM term, which ignores the mask, does.
    -> dict(pred, target float32 [B, T, H, W], mask bool)."""
    B, T, H, W = shape
    pred, target, mask = np.empty(shape, F32), np.empty(shape, F32), np.empty(shape, bool)
    for b in range(B):
        for t in range(T):
            s = seed * 1000 + (b * T + t) * 10
            tt = 1.0 + 2.0 * _smooth(s, H, W) + 0.25 * _hash01(s + 1, H * W).reshape(H, W)
            pp = gain * (0.5 * tt + 0.5 + 0.375 * _smooth(s + 2, H, W) + 0.125 * _hash01(s + 3, H * W).reshape(H, W))
            if (b, t) in inverse:
                pp = (tt.max() + tt.min()) - tt
            pred[b, t], target[b, t] = pp.astype(F32), tt.astype(F32)
            mask[b, t] = (_hash01(s + 4, H * W).reshape(H, W) < keep_rate) & ((b, t) not in inverse)
    return dict(pred=pred, target=target, mask=mask)


def checksum(case) -> list:
    return [float(case[k].astype(np.float64).sum()) for k in ("pred", "target", "mask")]
