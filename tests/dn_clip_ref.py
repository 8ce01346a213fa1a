"""Restatements for the depth + normal model's clip driver (VideoDepthEstimationModel.infer_video): the
window table by brute force, the whole stitch in float64, vdn_dn_stitch_apply as the float32 numpy expression with one
rounding per operation, and the launch grid include/vdn.h documents. Held to vdn.util by tests/test_dn_clip_host.py."""
import math

import numpy as np

F32 = np.float32


def window_table(N, S, overlap):
    """Windows of S slots every S - overlap frames over the clip padded with copies of its last frame. A window after the
    first is kept when some slot behind its overlap shows a frame of the clip itself, found by looking at every slot."""
    step = S - overlap
    padded = list(range(N)) + [N - 1] * (S + step)
    real = [True] * N + [False] * (S + step)
    table = []
    for start in range(0, N + step, step):
        if start + S > len(padded):
            break
        new = [i for i in range(overlap, S) if real[start + i]]
        if start == 0 or (start < N and new):
            table.append([padded[start + i] for i in range(S)])
    return table


def fit64(pred, target):
    """(scale, shift, det, s0, s2) of compute_scale_and_shift_full with an all-ones mask, float64 from exactly rounded
    sums; (1, 0) when det == 0."""
    p, t = np.asarray(pred, np.float64).reshape(-1), np.asarray(target, np.float64).reshape(-1)
    s0, s1, s2, s3, s4 = math.fsum(p * p), math.fsum(p), float(p.size), math.fsum(p * t), math.fsum(t)
    det = s0 * s2 - s1 * s1
    if det == 0.0:
        return 1.0, 0.0, det, s0, s2
    return (s2 * s3 - s1 * s4) / det, (-s1 * s3 + s0 * s4) / det, det, s0, s2


def stitch64(depths, normals, N, overlap, align=True, clamp0=False):
    """The stitch of the issue in float64: depths [S, H, W] and normals [S, 3, H, W] per window of window_table(N, S,
    overlap) -> (depth [N, H, W], normal [N, 3, H, W], coefs [windows, 2], fits [(det, s0, s2) per fitted window])."""
    S = len(depths[0])
    step = S - overlap
    shape = tuple(np.asarray(depths[0]).shape[1:])
    out_d, out_n = np.full((N,) + shape, np.nan), np.full((N, 3) + shape, np.nan)
    coefs, fits = [], []
    for k, (d, n) in enumerate(zip(depths, normals)):
        d, n = np.asarray(d, np.float64), np.asarray(n, np.float64)
        start = k * step
        keep = min(S, N - start)
        ov = overlap if k else 0
        scale, shift = 1.0, 0.0
        if ov and align:
            scale, shift, det, s0, s2 = fit64(d[:ov], out_d[start:start + ov])
            fits.append((det, s0, s2))
        coefs.append((scale, shift))
        nd = d * scale + shift
        if clamp0:
            nd = np.maximum(nd, 0.0)
        nn = n.copy()
        nn[:, :2] *= scale          # gradient of scale * d + shift; the clamp does not alter it
        nn[:, 2] = 1.0
        for i in range(keep):
            w = 1.0 if i >= ov else i / (ov - 1)
            if w == 1.0:
                out_d[start + i], out_n[start + i] = nd[i], nn[i]
            else:
                out_d[start + i] = out_d[start + i] * (1.0 - w) + nd[i] * w
                out_n[start + i, :2] = out_n[start + i, :2] * (1.0 - w) + nn[i, :2] * w
                out_n[start + i, 2] = 1.0
    return out_d, out_n, np.asarray(coefs, np.float64), fits


def stitch_apply32(depth, normal, scale, shift, out_depth, out_normal, overlap, keep, clamp0):
    """vdn_dn_stitch_apply in float32, every operation rounded on its own (include/vdn.h): depth [T, hw], normal [T, 3, hw],
    out_depth [>= T, hw] and out_normal [>= T, 3, hw] as they are before the call -> (out_depth, out_normal) after it."""
    d, n = np.asarray(depth, F32), np.asarray(normal, F32)
    scale, shift = F32(scale), F32(shift)
    od, on = np.array(out_depth, F32), np.array(out_normal, F32)
    nd = (d * scale + shift).astype(F32)
    if clamp0:
        nd = np.where(nd < 0, F32(0), nd)
    nx, ny = (n[:, 0] * scale).astype(F32), (n[:, 1] * scale).astype(F32)
    step = F32(1) / F32(overlap - 1) if overlap > 1 else F32(0)
    for t in range(keep):
        if t < overlap:
            w = F32(0) if t == 0 else (F32(1) if t == overlap - 1 else F32(t) * step)
            od[t] = od[t] * (F32(1) - w) + nd[t] * w
            on[t, 0] = on[t, 0] * (F32(1) - w) + nx[t] * w
            on[t, 1] = on[t, 1] * (F32(1) - w) + ny[t] * w
        else:
            od[t], on[t, 0], on[t, 1] = nd[t], nx[t], ny[t]
        on[t, 2] = F32(1)
    return od, on


def launch_grid(hw, keep, vec):
    """(blocks in x, lanes of one grid trip over a plane, pixel groups of a plane) of vdn_dn_stitch_apply as include/vdn.h
    states its launch: 256-lane blocks, min(ceil(groups / 256), max(1, 2048 / (4 keep))) of them per (frame, plane)."""
    groups = hw // 4 if vec else hw
    gx = min(-(-groups // 256), max(1, 2048 // (4 * keep)))
    return gx, gx * 256, groups
