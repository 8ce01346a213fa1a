"""The numpy float32 restatement of the batch preparation (include/vdn.h: vdn_prep_rgb, vdn_prep_depth) and the seeded maker
of the cases recorded in tests/golden/prep_cases.npz (written by tools/make_golden_prep.py from the reference's own functions).

Every step is one float32 numpy operation per reference operation: numpy's float32 subtract and divide are IEEE, as torch's
are, and np.min / np.max / np.where(x < m, m, x) keep a NaN the way torch.min / torch.max / torch.clamp do. The generator
refuses to write the fixture unless this restatement equals the reference under np.array_equal(..., equal_nan=True)."""
from __future__ import annotations

import numpy as np

F = np.float32
EPS = F(1e-8)
MEAN = np.array([0.485, 0.456, 0.406], F)   # timm.data.constants.IMAGENET_DEFAULT_MEAN
STD = np.array([0.229, 0.224, 0.225], F)    # timm.data.constants.IMAGENET_DEFAULT_STD

# op: which composition of the scripts a case runs
#   pre     preprocess_depth_sequences(depth, masks, norm)                      clamp0 [+ normalize]
#   bwn     the nested batch_wise_min_max_norm(x, masks) alone                  normalize
#   inv     1. / torch.clamp(gt, min=1e-8)                                      reciprocal
#   invpre  preprocess_depth_sequences(1. / torch.clamp(gt, min=1e-8), masks, norm)   reciprocal, clamp0 [+ normalize]
#   rgb     preprocess_rgb_sequences        viz     preprocess_rgb_viz_sequences
FLAGS = {"pre": (False, True), "bwn": (False, False), "inv": (True, False), "invpre": (True, True)}

CASES = [
    dict(op="pre", seed=101, shape=(2, 3, 1, 13, 13), mask="bool", special="plain", norm=True),
    dict(op="pre", seed=102, shape=(1, 2, 1, 16, 16), mask="uint8", special="plain", norm=True),
    dict(op="pre", seed=103, shape=(2, 2, 1, 1, 1), mask="bool", special="all_kept", norm=True),
    dict(op="pre", seed=104, shape=(2, 3, 1, 13, 13), mask="bool", special="empty_item", norm=True),
    dict(op="pre", seed=105, shape=(2, 3, 1, 13, 13), mask="uint8", special="constant_item", norm=True),
    dict(op="bwn", seed=106, shape=(2, 3, 1, 13, 13), mask="none", special="negative", norm=True),
    dict(op="bwn", seed=107, shape=(1, 2, 1, 16, 16), mask="bool", special="plain", norm=True),
    dict(op="pre", seed=108, shape=(2, 3, 1, 13, 13), mask="bool", special="negative", norm=False),
    dict(op="pre", seed=109, shape=(1, 2, 1, 16, 16), mask="bool", special="negative", norm=True),
    dict(op="inv", seed=110, shape=(2, 3, 1, 13, 13), mask="none", special="gt_small", norm=False),
    dict(op="invpre", seed=111, shape=(2, 3, 1, 13, 13), mask="bool", special="gt_small", norm=True),
    dict(op="invpre", seed=112, shape=(2, 2, 1, 1, 1), mask="bool", special="all_kept", norm=True),
    dict(op="pre", seed=113, shape=(2, 3, 1, 13, 13), mask="bool", special="nan_kept", norm=True),
    dict(op="pre", seed=114, shape=(2, 3, 1, 13, 13), mask="bool", special="dropped_nan", norm=True),
    dict(op="rgb", seed=115, shape=(2, 2, 3, 5, 5), mask="none", special="outside", norm=True),
    dict(op="viz", seed=115, shape=(2, 2, 3, 5, 5), mask="none", special="outside", norm=False),
    dict(op="rgb", seed=116, shape=(1, 2, 3, 4, 4), mask="none", special="outside", norm=True),
    dict(op="viz", seed=116, shape=(1, 2, 3, 4, 4), mask="none", special="outside", norm=False),
]


def clamp_min(x, m):
    return np.where(x < m, F(m), x).astype(F)


def clamp_max(x, m):
    return np.where(x > m, F(m), x).astype(F)


def prep_rgb_ref(x: np.ndarray, normalize: bool) -> np.ndarray:
    """x float32 [..., 3, H, W] -> the same shape."""
    x = np.asarray(x, F)
    c = clamp_max(clamp_min(x, 0), 1)
    if not normalize:
        return c
    return ((c - MEAN[:, None, None]).astype(F) / STD[:, None, None]).astype(F)


def prep_depth_ref(x: np.ndarray, mask, reciprocal: bool, clamp0: bool, normalize: bool):
    """x float32 [B, ...], mask [B, ...] (non-zero = keep) or None -> (out float32 of x's shape, minmax float32 [B, 2] or None)."""
    x = np.asarray(x, F)
    B = x.shape[0]
    v = x.reshape(B, -1)
    with np.errstate(all="ignore"):
        if reciprocal:
            v = (F(1) / clamp_min(v, EPS)).astype(F)
        if clamp0:
            v = clamp_min(v, 0)
        if not normalize:
            return v.reshape(x.shape), None
        keep = np.ones(v.shape, bool) if mask is None else (np.asarray(mask).reshape(B, -1) != 0)
        out = np.zeros_like(v)
        mm = np.empty((B, 2), F)
        for b in range(B):
            kept = v[b][keep[b]]
            if kept.size == 0:
                mm[b] = (np.inf, -np.inf)
                continue                                   # +0.0 everywhere
            lo, hi = F(kept.min()), F(kept.max())         # np.min / np.max: a NaN makes the result NaN
            mm[b] = (lo, hi)
            d = clamp_min(np.asarray(F(hi - lo)), EPS)
            out[b] = clamp_max(clamp_min(((v[b] - lo).astype(F) / d).astype(F), 0), 1)
    return out.reshape(x.shape), mm


def make_case(c: dict) -> dict:
    """The inputs of a case: x float32 of c['shape'], mask of the case's kind (or None), drawn from the seed alone."""
    rng = np.random.default_rng(c["seed"])
    shape = tuple(c["shape"])
    sp = c["special"]
    if c["op"] in ("rgb", "viz"):
        x = rng.uniform(-0.5, 1.5, shape).astype(F)
        flat = x.reshape(-1)
        flat[:4] = (-0.0, 0.0, 1.0, 2.0)
        return dict(x=x, mask=None)
    lo = -5.0 if sp == "negative" else 0.1
    x = rng.uniform(lo, 20.0, shape).astype(F)
    keep = rng.random(shape) < 0.7
    B = shape[0]
    xf, kf = x.reshape(B, -1), keep.reshape(B, -1)      # views
    if sp == "all_kept":
        kf[:] = True
    else:
        kf[:, 0] = True                                  # every item keeps something unless a special empties it
    if sp == "empty_item":
        kf[B - 1] = False
    if sp == "constant_item":
        xf[0] = F(0.7)
    if sp == "gt_small":
        xf[0, :3] = (0.0, 1e-9, 5e-8)
        kf[0, :3] = True
    if sp == "nan_kept":
        xf[0, 7] = np.nan
        kf[0, 7] = True
    if sp == "dropped_nan":
        for b in range(B):
            idx = np.flatnonzero(~kf[b])[:3]
            assert idx.size == 3
            xf[b, idx] = (np.nan, np.inf, -np.inf)
    mask = {"bool": keep, "uint8": keep.astype(np.uint8) * 255, "none": None}[c["mask"]]
    return dict(x=x, mask=mask)


def checksum(case: dict) -> np.ndarray:
    x = case["x"].astype(np.float64)
    return np.array([x[np.isfinite(x)].sum(), 0 if case["mask"] is None else int((case["mask"] != 0).sum())], np.float64)


def restate(c: dict, case: dict) -> np.ndarray:
    """What the device must give for a case, in the shape the scripts' function returns."""
    if c["op"] in ("rgb", "viz"):
        return prep_rgb_ref(case["x"], c["op"] == "rgb")
    reciprocal, clamp0 = FLAGS[c["op"]]
    out, _ = prep_depth_ref(case["x"], case["mask"], reciprocal, clamp0, c["norm"] and c["op"] != "inv")
    return out if c["op"] == "inv" else out.squeeze(2)
