"""Plain CPU restatements of the video path's small kernels (csrc/stitch.hip, refine.hip with the median on select.hpp,
hiera.hip, dn_head.hip's prologue and tail, points.hip), for tests/test_gpu_video_kernel_edges.py. Where the kernel's bar is
a tolerance the restatement is float64; where it is "the same bits" it is float32 numpy / torch with one rounding per
operation, in the order the kernel's comment spells out. tests/test_video_kernels_ref_host.py holds each of them to what it
restates (torch.quantile, vdn.util, the oracle's Sobel normals, hiera_ref, F.conv2d + F.interpolate, the point-cloud script's
expression)."""
import math

import numpy as np
import torch

F32 = np.float32


# ------------------------------------------------------------------------------------------------ median (select.hpp)
NAN = float("nan")
INF = float("inf")
NEG_NAN = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
FMAX = float(np.finfo(np.float32).max)
SUB = float(np.float32(1e-45))   # the smallest subnormal
# frames of special values: signed zeros, subnormals, the largest finite values, infinities with odd and even counts, and a
# NaN of either sign alone, next to infinities and in the majority
MEDIAN_ROWS = [
    [1, 2, 4, 5], [3], [1, 2], [-0.0, 0.0], [0.0, -0.0], [-7.5, 7.5], [2, 2, 2, 2, 2],
    [SUB, 2 * SUB, 3 * SUB], [-SUB, SUB], [SUB, 3 * SUB],
    [FMAX, FMAX], [-FMAX, FMAX], [-FMAX, 1, FMAX], [FMAX, FMAX, 1, 0],
    [INF, 1, 2], [1, INF, INF], [-INF, 1, INF], [-INF, INF], [1, INF], [-INF, -INF, 1, 2], [INF, INF, INF, INF], [1, 2, INF, INF],
    [1, 2, NAN, 4, 5], [1, 2, NEG_NAN, 4, 5], [NAN, NAN, NAN, 1, 2], [NEG_NAN, NAN, 1], [NAN], [1, NAN], [NEG_NAN, -INF, INF, 3],
]


def ordered_keys(x):
    """select.hpp ordered_key: the uint32 whose unsigned order is the float order (-0 below +0, a NaN by its sign bit)."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def key_values(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & 0x80000000, k & 0x7FFFFFFF, ~k).astype(np.uint32).view(F32)


def select_lerp(x):
    """The select and the blend alone, without the NaN rule: ranks floor and ceil of (n - 1) / 2 in key order, then at::lerp's
    two-sided form in float32. x [F, n] -> [F]."""
    x = np.ascontiguousarray(x, dtype=F32)
    n = x.shape[1]
    k = np.sort(ordered_keys(x), axis=1)
    a, b = key_values(k[:, (n - 1) // 2]), key_values(k[:, n // 2])
    with np.errstate(invalid="ignore", over="ignore"):
        if n & 1:                                   # w = 0: a + 0 * (b - a)
            return (a + F32(0) * (b - a)).astype(F32)
        return (b - (b - a) * (F32(1) - F32(0.5))).astype(F32)


def frame_median(x):
    """vdn_frame_median: torch.quantile(x[f], 0.5); a frame that holds a NaN of either sign gets a NaN."""
    x = np.ascontiguousarray(x, dtype=F32)
    out = select_lerp(x)
    out[np.isnan(x).any(axis=1)] = np.nan
    return out


def pass_bins(v):
    """The bins a float falls in on the three passes of the radix select: top 11, next 11, last 10 key bits."""
    k = int(ordered_keys(np.array([v], dtype=F32))[0])
    return k >> 21, (k >> 10) & 2047, k & 1023


# ------------------------------------------------------------------------------------------------ stitch (stitch.hip)
def stitch_fit(pred, target):
    """The 2 x 2 closed form of utils/util.py:49-60 in float64 from exactly rounded sums (math.fsum of exact float64
    products of float32 values). Returns (scale, shift, det, s0, s2); (1, 0) when det == 0."""
    p, t = np.asarray(pred, dtype=F32).reshape(-1).astype(np.float64), np.asarray(target, dtype=F32).reshape(-1).astype(np.float64)
    s0, s1, s2, s3, s4 = math.fsum(p * p), math.fsum(p), float(p.size), math.fsum(p * t), math.fsum(t)
    det = s0 * s2 - s1 * s1
    if det == 0.0:
        return 1.0, 0.0, det, s0, s2
    return (s2 * s3 - s1 * s4) / det, (-s1 * s3 + s0 * s4) / det, det, s0, s2


def stitch_apply(window, scale, shift, out_tail, align_len, overlap, ref_frame):
    """vdn_stitch_apply in float32, every operation rounded on its own: fit(d) = max(d * scale + shift, 0); frames
    align_len .. overlap - 1 blend into out_tail as o * (1 - w) + fit * w with w = 0, k * (1 / (interp - 1)), 1; frames
    overlap .. T - 1 are fit alone; ref1 = fit(frame ref_frame). window [T, hw], out_tail [interp, hw]. Returns
    (out_tail, out_new, ref1)."""
    win = np.asarray(window, dtype=F32)
    scale, shift = F32(scale), F32(shift)
    fit = np.maximum(win * scale + shift, F32(0)).astype(F32)
    interp = overlap - align_len
    step = F32(1) / F32(interp - 1)
    tail = np.empty_like(np.asarray(out_tail, dtype=F32))
    for k in range(interp):
        w = F32(0) if k == 0 else (F32(1) if k == interp - 1 else F32(k) * step)
        tail[k] = np.asarray(out_tail[k], dtype=F32) * (F32(1) - w) + fit[align_len + k] * w
    return tail, fit[overlap:].copy(), fit[ref_frame].copy()


# ------------------------------------------------------------------------------------------------ refiner (refine.hip)
def refine_scale(x, median, w, b, max_log_scale, max_depth):
    """x [F, n] / max_depth * s_f with s_f = exp(tanh(w * median_f / max_depth + b) * max_log_scale), float64."""
    s = np.exp(np.tanh(np.asarray(median, dtype=np.float64) / max_depth * w + b) * max_log_scale)
    return np.asarray(x, dtype=np.float64) / max_depth * s[:, None], s


def sobel_pack(d, eps=1e-8):
    """vdn_refine_pack with normals: [F, 3, H, W] = (d, nx, ny), n = (-Ix, -Iy, 1) / sqrt(Ix^2 + Iy^2 + 1 + eps), Sobel / 8
    as a cross-correlation on the reflect-padded map (H, W >= 2), float64."""
    d = np.asarray(d, dtype=np.float64)
    p = np.pad(d, ((0, 0), (1, 1), (1, 1)), mode="reflect")
    H, W = d.shape[1:]

    def at(dy, dx):
        return p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]

    ix = ((at(-1, -1) - at(-1, 1)) + 2.0 * (at(0, -1) - at(0, 1)) + (at(1, -1) - at(1, 1))) / 8.0
    iy = ((at(-1, -1) - at(1, -1)) + 2.0 * (at(-1, 0) - at(1, 0)) + (at(-1, 1) - at(1, 1))) / 8.0
    inv = 1.0 / np.sqrt(ix * ix + iy * iy + 1.0 + eps)
    return np.stack([d, -ix * inv, -iy * inv], axis=1)


def refine_finish(scaled, depth, w, b, max_depth, residual):
    depth = np.asarray(depth, dtype=np.float64)
    if not residual:
        return depth * max_depth
    return (np.asarray(scaled, dtype=np.float64) + (depth * w + b)) * max_depth


# ------------------------------------------------------------------------------------------------ Hiera (hiera.hip)
def unrolled_of_yx(y, x, n):
    """hiera.hip: token index of grid position (y, x) on a (7 << n)-sided grid with n stride-2 levels left, level 1 (the
    lowest bit) the most significant digit."""
    y, x = np.asarray(y), np.asarray(x)
    d = np.zeros_like(y)
    for k in range(1, n + 1):
        d = d * 4 + (((y >> (k - 1)) & 1) * 2 + ((x >> (k - 1)) & 1))
    return d * 49 + (y >> n) * 7 + (x >> n)


def _unrolled_grid(n):
    side = 7 << n
    yy, xx = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    return unrolled_of_yx(yy, xx, n)                                       # [side, side] -> u


def hiera_embed_rows(img):
    """vdn_hiera_embed's first 147 columns: rows[f * 3136 + u, (c * 7 + ky) * 7 + kx] = img[f, c, 4y - 3 + ky, 4x - 3 + kx]
    (0 outside) with (y, x) the position of unrolled token u. img f32 [F, 3, 224, 224] -> f32 [F * 3136, 147]."""
    img = np.asarray(img, dtype=F32)
    Fr = img.shape[0]
    p = np.pad(img, ((0, 0), (0, 0), (3, 3), (3, 3)))
    win = np.lib.stride_tricks.sliding_window_view(p, (7, 7), axis=(2, 3))[:, :, ::4, ::4]   # [F, 3, 56, 56, 7, 7]
    rows = win.transpose(0, 2, 3, 1, 4, 5).reshape(Fr, 3136, 147)
    out = np.empty_like(rows)
    out[:, _unrolled_grid(3).reshape(-1)] = rows
    return out.reshape(Fr * 3136, 147)


def hiera_pool(x, n):
    """y[f, j, :] = fmaxf over g < 4 of x[f, g * n + j, :]: a NaN loses against a number (C's fmaxf), where torch.max keeps it."""
    x = np.asarray(x, dtype=F32)
    g = x.reshape(x.shape[0], 4, n, x.shape[-1])
    return np.fmax(np.fmax(g[:, 0], g[:, 1]), np.fmax(g[:, 2], g[:, 3]))


def hiera_reroll(tokens, stage):
    """map[f, y, x, :] = tokens[f, u(y, x), :] on the (56 >> stage)-sided grid."""
    tokens = np.asarray(tokens)
    return tokens[:, _unrolled_grid(3 - stage)]


# ------------------------------------------------------------------------------------------------ head (dn_head.hip)
def dn_prologue(a, b, frames, C, hw, ape=None, S=1):
    """token[f * hw + p, c] = a[f][c * hw + p] (+ b) (+ ape[f % S][c]) as float32 torch additions in that order."""
    v = a.reshape(frames, C, hw)
    if b is not None:
        v = v + b.reshape(frames, C, hw)
    if ape is not None:
        v = v + ape[torch.arange(frames) % S][:, :, None]
    return v.permute(0, 2, 1).reshape(frames * hw, C).contiguous()


def _ac_axis(I, O):
    """align_corners=True source rows of an axis: (i0, i1, w) with src = o * (I - 1) / (O - 1), 0 when O == 1."""
    o = np.arange(O, dtype=np.float64)
    src = o * ((I - 1) / (O - 1)) if O > 1 else np.zeros(O)
    i0 = np.minimum(np.floor(src).astype(np.int64), I - 1)
    return i0, np.minimum(i0 + 1, I - 1), src - i0


def dn_tail(x, w, bias, OH, OW, depth_in=None, relu=False):
    """vdn_dn_tail in float64: conv3x3 (Cin -> 3, pad 1) + bias of the NHWC map x [F, IH, IW, Cin] with w [3, Cin, 3, 3], then
    the bilinear align_corners resize to (OH, OW) when that differs. Returns (raw [F, 3, OH, OW], depth [F, OH, OW] = relu?(ch0 +
    depth_in?), normal [F, 3, OH, OW] = (-ch1, -ch2, 1))."""
    x, w, bias = (np.asarray(t, dtype=np.float64) for t in (x, w, bias))
    Fr, IH, IW, _ = x.shape
    p = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    y = np.zeros((Fr, 3, IH, IW))
    for ky in range(3):
        for kx in range(3):
            y += np.einsum("fyxc,oc->foyx", p[:, ky:ky + IH, kx:kx + IW], w[:, :, ky, kx])
    y += bias[None, :, None, None]
    if (OH, OW) != (IH, IW):
        y0, y1, wy = _ac_axis(IH, OH)
        x0, x1, wx = _ac_axis(IW, OW)
        rows = y[:, :, y0] * (1 - wy)[None, None, :, None] + y[:, :, y1] * wy[None, None, :, None]
        y = rows[:, :, :, x0] * (1 - wx) + rows[:, :, :, x1] * wx
    d = y[:, 0] + (np.asarray(depth_in, dtype=np.float64) if depth_in is not None else 0.0)
    if relu:
        d = np.maximum(d, 0.0)
    return y, d, np.stack([-y[:, 1], -y[:, 2], np.ones_like(d)], axis=1)


# ------------------------------------------------------------------------------------------------ points (points.hip)
def depth_to_points(depth, rgb, fx, fy):
    """points.hip, pixel by pixel in float64: x = (col - w / 2) / fx, y = (row - h / 2) / fy, point = (x z, y z, z),
    colour = rgb / 255."""
    depth = np.asarray(depth, dtype=F32)
    h, w = depth.shape
    i = np.arange(h * w)
    row, col = i // w, i - (i // w) * w
    x, y, z = (col.astype(np.float64) - w / 2.0) / fx, (row.astype(np.float64) - h / 2.0) / fy, depth.reshape(-1).astype(np.float64)
    return np.stack([x * z, y * z, z], axis=1), np.asarray(rgb).reshape(-1, 3).astype(np.float64) / 255.0
