"""CPU restatement of the reference's normal evaluation for the tests of vdn.normals: normal_vector / sobel_ix_iy
(utils/normal_utils.py:4-52) and VideoNormalLoss (loss/loss.py:370-409), in float64 numpy from the float32 samples.

  * The stencil is the cross-correlation of the reflect-padded map (no edge repeat) with kx = [[1,0,-1],[2,0,-2],[1,0,-1]]
    and ky = [[1,2,1],[0,0,0],[-1,-2,-1]], divided by 8 when normalize_kernel.
  * scale_xy, scale_z and eps enter as their float32 values: the reference multiplies float32 tensors by them.
  * Erosion: a pixel is kept when it and all of its 3 x 3 neighbours inside the image are non-zero (the reference
    zero-pads the inverted mask, so positions outside the image erode nothing).
  * cos = sum_c (a_c / max(|a|, 1e-8)) * (b_c / max(|b|, 1e-8)): F.cosine_similarity of torch 2.x. Dropped pixels are
    selected away before anything is summed. loss = 1 - sum / count, and 1.0 when count is 0.

Also the seeded input maker shared by tools/make_golden_normals.py and the tests (tests/golden/normal_cases.npz stores
seeds and arguments, not the inputs)."""
from __future__ import annotations

import numpy as np


def sobel_ref(depth, normalize_kernel=True):
    """depth [..., H, W] float32 -> Ix, Iy float64 of the same shape."""
    d = np.asarray(depth, np.float32).astype(np.float64)
    H, W = d.shape[-2:]
    if H < 2 or W < 2:
        raise ValueError("reflect pad needs H, W >= 2")
    p = np.pad(d, [(0, 0)] * (d.ndim - 2) + [(1, 1), (1, 1)], mode="reflect")
    w = lambda r, c: p[..., r:r + H, c:c + W]
    k = 0.125 if normalize_kernel else 1.0
    with np.errstate(all="ignore"):
        ix = ((w(0, 0) - w(0, 2)) + 2.0 * (w(1, 0) - w(1, 2)) + (w(2, 0) - w(2, 2))) * k
        iy = ((w(0, 0) - w(2, 0)) + 2.0 * (w(0, 1) - w(2, 1)) + (w(0, 2) - w(2, 2))) * k
    return ix, iy


def normal_vector_ref(depth, normalize_kernel=True, scale_xy=1.0, scale_z=1.0, eps=1e-8):
    """depth [..., H, W] float32 -> normals float64 [..., 3, H, W]."""
    ix, iy = sobel_ref(depth, normalize_kernel)
    sxy, sz, e = float(np.float32(scale_xy)), float(np.float32(scale_z)), float(np.float32(eps))
    nx, ny = -sxy * ix, -sxy * iy
    with np.errstate(all="ignore"):
        norm = np.sqrt(((nx * nx + ny * ny) + sz * sz) + e)
        return np.stack([nx / norm, ny / norm, np.broadcast_to(sz, nx.shape) / norm], axis=-3)


def erode_ref(mask):
    """mask [..., H, W], non-zero = use -> bool of the same shape."""
    m = np.asarray(mask) != 0
    H, W = m.shape[-2:]
    p = np.pad(m, [(0, 0)] * (m.ndim - 2) + [(1, 1), (1, 1)], mode="constant", constant_values=True)
    out = np.ones_like(m)
    for r in range(3):
        for c in range(3):
            out &= p[..., r:r + H, c:c + W]
    return out


def cosine_ref(a, b):
    """a, b float64 [..., 3, H, W] -> cosine [..., H, W]."""
    with np.errstate(all="ignore"):
        na = np.sqrt((a[..., 0, :, :] ** 2 + a[..., 1, :, :] ** 2) + a[..., 2, :, :] ** 2)
        nb = np.sqrt((b[..., 0, :, :] ** 2 + b[..., 1, :, :] ** 2) + b[..., 2, :, :] ** 2)
        na = np.where(na < 1e-8, 1e-8, na)[..., None, :, :]
        nb = np.where(nb < 1e-8, 1e-8, nb)[..., None, :, :]
        return ((a / na) * (b / nb)).sum(-3)


def normal_loss_ref(pred, target, mask=None, target_is_depth=False):
    """pred float32 [B, T, 3, H, W]; target normals [B, T, 3, H, W] or depth [B, T, H, W]; mask [B, T, H, W] or None.
    Returns (loss, per-frame mean cosine [B, T] (NaN without a kept pixel), per-frame count [B, T] int64)."""
    a = np.asarray(pred, np.float32).astype(np.float64)
    b = normal_vector_ref(target) if target_is_depth else np.asarray(target, np.float32).astype(np.float64)
    keep = erode_ref(np.ones(a.shape[:2] + a.shape[3:], bool) if mask is None else mask)
    cos = np.where(keep, cosine_ref(a, b), 0.0)          # selected, not multiplied: NaN under a dropped pixel is gone
    sums, counts = cos.sum((-1, -2)), keep.sum((-1, -2)).astype(np.int64)
    n = int(counts.sum())
    with np.errstate(all="ignore"):
        loss = 1.0 - float(sums.sum()) / n if n else 1.0
        return loss, sums / counts, counts


# ------------------------------------------------------------------------------------------------ seeded cases
def make_depth(rng, shape):
    """A smooth depth map with a step edge and noise, float32 [B, T, H, W]: slopes on both sides of 1, so normals tilt."""
    B, T, H, W = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    d = np.empty(shape, np.float64)
    for b in range(B):
        for t in range(T):
            d[b, t] = (2.0 + 3.0 * yy + 1.5 * np.sin(5.0 * xx + 0.6 * t + b) ** 2 + 4.0 * (xx + 0.3 * yy > 0.7 + 0.02 * t)
                       + 0.05 * rng.standard_normal((H, W))) * min(H, W) * 0.25
    return d.astype(np.float32)


def make_case(seed: int, shape, mask_kind: str = "none", target_kind: str = "unit", empty_frames=(), false_rate=0.05):
    """Seeded inputs of one loss case. shape = (B, T, H, W).
    mask_kind: 'none' (realised as all-true) | 'bool' | 'float' (0/1 float32) | 'allfalse'; empty_frames are set all-false.
    target_kind: 'unit' (normal_vector of the depth, float32) | 'scaled' (the same times a positive random length).
    Returns dict(pred f32 [B,T,3,H,W], depth f32 [B,T,H,W], target f32 [B,T,3,H,W], mask)."""
    B, T, H, W = shape
    rng = np.random.default_rng(seed)
    depth = make_depth(rng, shape)
    unit = normal_vector_ref(depth)
    pred = unit + 0.3 * rng.standard_normal(unit.shape)           # a noisy estimate, not unit length
    pred *= 0.5 + rng.random((B, T, 1, H, W))
    target = unit.copy()
    if target_kind == "scaled":
        target *= 0.25 + 3.0 * rng.random((B, T, 1, H, W))
    elif target_kind != "unit":
        raise ValueError(target_kind)
    if mask_kind == "none":
        mask = np.ones((B, T, H, W), bool)
    elif mask_kind in ("bool", "float"):
        mask = rng.random((B, T, H, W)) >= false_rate
    elif mask_kind == "allfalse":
        mask = np.zeros((B, T, H, W), bool)
    else:
        raise ValueError(mask_kind)
    for f in empty_frames:
        mask.reshape(B * T, H, W)[f] = False
    if mask_kind == "float":
        mask = mask.astype(np.float32)
    return dict(pred=pred.astype(np.float32), depth=depth, target=target.astype(np.float32), mask=mask)


def checksum(case) -> list:
    return [float(case[k].astype(np.float64).sum()) for k in ("pred", "depth", "target", "mask")]
