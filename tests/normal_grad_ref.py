"""CPU restatement of the gradient of the reference's VideoNormalLoss with respect to its prediction, in numpy float64 on top
of the forward pieces of tests/normal_ref.py (imported, not copied). This is the arithmetic contract of csrc/normals_grad.hip
(include/vdn.h, vdn_normal_loss_backward): what torch's autograd computes for coeff * normal_loss.

F.cosine_similarity clamps the two norms to eps = 1e-8 in place and outside the graph, so autograd differentiates
sum_c (p_c / n) * (t_c / n_t) with n = max(|p|, 1e-8) and n_t = max(|t|, 1e-8) as if dn/dp = p / |p| on both sides of the clamp,
and 0 at |p| = 0 (torch's norm backward at the origin). With that = t / n_t and N the pixels the erosion keeps over the batch:

    kept pixel:     dL/dp_c = -(coeff / N) * (that_c - ((p . that) / n) * (p_c / |p|)) / n       (p_c / |p| := 0 where |p| = 0)
    dropped pixel:  +0.0 in all three channels (skipped: NaN or inf under it reaches nothing)
    N = 0:          +0.0 everywhere

For |p| >= 1e-8 that is (that - cos * phat) / |p|; for 0 < |p| < 1e-8 it is neither that nor that / n: p = (3e-9, 0, 0) gives
0.7 of that_x / 1e-8 in x. The steps are the device's: 1 / n and 1 / n_t formed once and multiplied in. coeff enters as its
float32 value, the dtype in which autograd hands a float32 loss its gradient.

Also the seeded maker of the one case with pixels on and under the clamp, shared by tools/make_golden_normal_grad.py and the
tests (tests/golden/normal_grad_cases.npz stores seeds and arguments, not the inputs)."""
from __future__ import annotations

import numpy as np

import normal_ref as R

# what make_special writes at its chosen kept pixels: predictions under the clamp (0 < |p| < 1e-8)
TINY = np.array([(3e-9, 0.0, 0.0), (0.0, -4e-9, 0.0), (1e-9, 2e-9, -2e-9), (-5e-9, 5e-9, 5e-9), (0.0, 0.0, 9e-9), (6e-9, -1e-9, 0.0)],
                np.float32)
N_ZERO_PRED = N_ZERO_TARGET = 5


def norm_ref(a):
    """a float64 [..., 3, H, W] -> |a| [..., H, W], summed in cosine_ref's order."""
    with np.errstate(all="ignore"):
        return np.sqrt((a[..., 0, :, :] ** 2 + a[..., 1, :, :] ** 2) + a[..., 2, :, :] ** 2)


def normal_loss_grad_ref(pred, target, mask, target_is_depth=False, coeff=1.0):
    """pred float32 [B, T, 3, H, W]; target normals [B, T, 3, H, W] or depth [B, T, H, W]; mask [B, T, H, W] or None.
    Returns (grad, mag), both float64 [B, T, 3, H, W]: the gradient of coeff * normal_loss and, per element, the magnitude
    |coeff| / (N * n) * (|that_c| + |p . that| / n * |p_c| / |p|) of the two terms whose difference it is (0 where grad is
    +0.0 by definition)."""
    a = np.asarray(pred, np.float32).astype(np.float64)
    b = R.normal_vector_ref(target) if target_is_depth else np.asarray(target, np.float32).astype(np.float64)
    keep = R.erode_ref(np.ones(a.shape[:2] + a.shape[3:], bool) if mask is None else mask)
    n_kept = int(keep.sum())
    grad, mag = np.zeros_like(a), np.zeros_like(a)
    if n_kept == 0:
        return grad, mag
    g = float(np.float32(coeff))
    with np.errstate(all="ignore"):
        na, nb = norm_ref(a), norm_ref(b)
        inv_n, inv_nt = 1.0 / np.where(na < 1e-8, 1e-8, na), 1.0 / np.where(nb < 1e-8, 1e-8, nb)
        inv_na = np.where(na >= 1e-8, inv_n, np.where(na > 0.0, 1.0 / np.where(na > 0.0, na, 1.0), 0.0))
        inv_n, inv_nt, inv_na = (v[..., None, :, :] for v in (inv_n, inv_nt, inv_na))
        th = b * inv_nt
        d = (((a[..., 0, :, :] * th[..., 0, :, :] + a[..., 1, :, :] * th[..., 1, :, :]) + a[..., 2, :, :] * th[..., 2, :, :])[..., None, :, :]
             * inv_n)
        k = -(g / float(n_kept))
        full = k * ((th - d * (a * inv_na)) * inv_n)
        full_mag = abs(k) * inv_n * (np.abs(th) + np.abs(d) * np.abs(a * inv_na))
    sel = np.broadcast_to(keep[..., None, :, :], a.shape)
    grad[sel] = full[sel]            # selected, not multiplied: NaN under a dropped pixel is gone
    mag[sel] = full_mag[sel]
    return grad, mag


def make_special(seed: int, shape):
    """normal_ref.make_case(seed, shape, 'bool') with, at kept pixels drawn from the same seed: N_ZERO_PRED predictions set to
    exactly zero, len(TINY) predictions set to the rows of TINY (under the clamp), and N_ZERO_TARGET stored targets set to zero
    (at pixels whose prediction stays ordinary). Returns the case and dict(zero_pred, tiny, zero_target): flat indices into
    [B * T, H * W] in the order written."""
    case = R.make_case(seed, shape, "bool")
    B, T, H, W = shape
    keep = R.erode_ref(case["mask"]).reshape(B * T, H * W)
    rng = np.random.default_rng(seed + 1000)
    fr, px = np.nonzero(keep)
    pick = rng.choice(fr.size, N_ZERO_PRED + len(TINY) + N_ZERO_TARGET, replace=False)
    where = list(zip(fr[pick], px[pick]))
    pred, target = case["pred"].reshape(B * T, 3, H * W), case["target"].reshape(B * T, 3, H * W)
    idx = dict(zero_pred=where[:N_ZERO_PRED], tiny=where[N_ZERO_PRED:N_ZERO_PRED + len(TINY)], zero_target=where[N_ZERO_PRED + len(TINY):])
    for f, p in idx["zero_pred"]:
        pred[f, :, p] = 0.0
    for (f, p), v in zip(idx["tiny"], TINY):
        pred[f, :, p] = v
    for f, p in idx["zero_target"]:
        target[f, :, p] = 0.0
    return case, {k: np.array([f * H * W + p for f, p in v], np.int64) for k, v in idx.items()}
