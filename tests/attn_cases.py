"""Adversarial score patterns for the attention kernels, their plain references and the conditioned bars.

The rest of the suite draws q, k and v from randn: scaled logits stay below ~45, where exp2 can neither overflow nor underflow
in fp32, so a softmax without any max subtraction passes it. `make` prescribes the scaled logits instead:

    logit[i, j] = g0[i] * p0[j] + g1[i] * p1[j] + N(0, 1)

Channel 0 of q / k carries g0 (0 or 1) and the per-key profile p0 (up to +-120), channel 1 the per-row gain g1 (0, +-1, +-8,
+-40) and the per-key profile p1 (in [-3, -1]), the other channels the noise. The row factors are small multiples of powers of
two, exact in fp16, so a pattern is the same after rounding to the operand planes (the key factors round like any value; the
tests compute their references on the values the planes hold).

Bars (`bars`): max(B, 4 * e32) with B the bar the kernel's own test uses on randn inputs and e32 the error of plain fp32
torch.softmax attention against fp64 on the same inputs — an fp32 logit of 120 has an ulp of 7.6e-6, so no fp32 kernel can hold
1e-5 there; the 4 covers another accumulation order. The worst-pixel bar is max(ratio * B, 4 * worst-pixel error of the fp32
reference): the fp32 reference's own worst pixel, not its rel-L2 times the ratio."""
import math

import torch

from common import rel_l2, worst_px

CASES = ("offset_pos", "offset_neg", "ramp_up_fast", "ramp_up_slow", "ramp_down", "one_hot_last", "one_hot_first", "flat",
         "mixed_rows")
LN2 = math.log(2.0)
OFFSET = 120.0                     # offset_pos / offset_neg: every logit
FAST, SLOW, DOWN = 9.0, 4.0, 32.0  # ramps: bits (log2 domain) per key tile
HOT = 80.0                         # one_hot_*: the hot key's lead; mixed_rows: the spike
GAINS = (0.0, 1.0, 8.0, 40.0)      # mixed_rows: |g1| cycles through these, the sign flips every four rows
SPIKE_ROW = 6                      # mixed_rows: row SPIKE_ROW of every 64-row query tile has the spike at the last key


def pattern(case, nq, nk, tile=64):
    """(g0 [nq], p0 [nk], g1 [nq], p1 [nk]) in fp64, scaled-logit units. `tile`: keys over which a ramp gains its bits (the
    kernels' key tile; the single-tile temporal kernels pass a smaller one to get the same range over their few frames)."""
    i, j = torch.arange(nq, dtype=torch.float64), torch.arange(nk, dtype=torch.float64)
    g0, p0, g1, p1 = torch.ones(nq, dtype=torch.float64), torch.zeros(nk, dtype=torch.float64), torch.zeros(nq, dtype=torch.float64), torch.zeros(nk, dtype=torch.float64)
    if case == "offset_pos":
        p0 += OFFSET
    elif case == "offset_neg":
        p0 -= OFFSET
    elif case == "ramp_up_fast":
        p0 = j * (FAST * LN2 / tile)
    elif case == "ramp_up_slow":
        p0 = j * (SLOW * LN2 / tile)
    elif case == "ramp_down":
        p0 = -j * (DOWN * LN2 / tile)
    elif case == "one_hot_last":
        p0[nk - 1] = HOT
    elif case == "one_hot_first":
        p0[0] = HOT
    elif case == "flat":
        g0 = torch.zeros(nq, dtype=torch.float64)
    elif case == "mixed_rows":
        g0 = (i % 64 == SPIKE_ROW).double()
        p0[nk - 1] = HOT
        g1 = torch.tensor(GAINS, dtype=torch.float64)[(i % 4).long()] * (1 - 2 * ((i // 4) % 2))
        # +1 at key 0, -1 at key 1, fading out over half a tile: rows of either sign have their maximum in tile 0. The -2 under
        # it shifts a whole row by -2 g1: next to a +40 row, whose maximum is -40, sits a -40 row whose maximum is +120, so a
        # reference point shared between rows underflows the small ones even in fp32
        p1 = (1 - 2 * (j % 2)) * (1 - j / (tile / 2)).clamp_min(0) - 2
    else:
        raise ValueError(case)
    return g0, p0, g1, p1


def _pow2_near(x):
    return 2.0 ** round(math.log2(x))


def make(case, nq, nk, dh, scale, seed, tile=64):
    """-> (q [nq, dh], k [nk, dh], v [nk, dh]) fp32 whose scaled logits scale * q k^T follow `case`."""
    assert dh >= 4 and nq >= 1 and nk >= 1
    g0, p0, g1, p1 = pattern(case, nq, nk, tile)
    g = torch.Generator().manual_seed(1000003 * CASES.index(case) + seed)
    sigma = (scale * math.sqrt(dh - 2)) ** -0.5          # scale * sum of dh - 2 products of N(0, sigma^2) pairs: N(0, 1)
    q = torch.randn(nq, dh, generator=g, dtype=torch.float64) * sigma
    k = torch.randn(nk, dh, generator=g, dtype=torch.float64) * sigma
    v = torch.randn(nk, dh, generator=g, dtype=torch.float64)
    a0 = _pow2_near(math.sqrt(OFFSET / scale))           # |q| ~ |k| at the largest logit
    a1 = _pow2_near((3 / (GAINS[-1] * scale)) ** 0.5)
    q[:, 0], k[:, 0] = g0 * a0, p0 / (scale * a0)
    q[:, 1], k[:, 1] = g1 * a1, p1 / (scale * a1)
    if case == "flat":
        q.zero_()
    return q.float(), k.float(), v.float()


def make_batch(case, n, nq, nk, dh, scale, seed, tile=64):
    """n independent problems stacked: (q [n, nq, dh], k [n, nk, dh], v [n, nk, dh])."""
    qkv = [make(case, nq, nk, dh, scale, seed * 131 + b, tile) for b in range(n)]
    return tuple(torch.stack(t) for t in zip(*qkv))


def attend64(s, v):
    """softmax over the last axis of already scaled logits, times v, in fp64."""
    return torch.softmax(s.double(), dim=-1) @ v.double()


def ref64(q, k, v, scale):
    return attend64(q.double() @ k.double().transpose(-1, -2) * scale, v)


def ref32(q, k, v, scale):
    q, k, v = q.float().cpu(), k.float().cpu(), v.float().cpu()
    return torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1) @ v


def _e5m2(x):
    return x.float().to(torch.float8_e5m2).double()


def qk8_movement(qh, ql, kh, kl, v, scale):
    """How far the fp64 attention moves when the score cross terms K_hi Q_lo^T + K_lo Q_hi^T are computed from the 8-bit planes
    (e5m2 of the hi plane, e5m2 of lo * 2^10) instead of exactly: (rel-L2, worst pixel). The planes come as float tensors."""
    qh, ql, kh, kl = (t.double() for t in (qh, ql, kh, kl))
    hh = qh @ kh.transpose(-1, -2)
    exact = ql @ kh.transpose(-1, -2) + qh @ kl.transpose(-1, -2)
    q8, k8 = _e5m2(qh), _e5m2(kh)
    ql8, kl8 = _e5m2(ql * 1024.0) / 1024.0, _e5m2(kl * 1024.0) / 1024.0
    rounded = ql8 @ k8.transpose(-1, -2) + q8 @ kl8.transpose(-1, -2)
    a, b = attend64((hh + exact) * scale, v), attend64((hh + rounded) * scale, v)
    return rel_l2(b, a), worst_px(b, a)


def bars(q, k, v, scale, B, ratio, extra=(0.0, 0.0)):
    """-> (ref64, e32, rel-L2 bar, worst-pixel bar) for a kernel whose own test holds B (rel-L2) and ratio * B (worst pixel).
    `extra`: 4x of it is added (the qk8 rows' qk8_movement)."""
    r64 = ref64(q, k, v, scale)
    r32 = ref32(q, k, v, scale)
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all())
    e32, e32px = rel_l2(r32, r64), worst_px(r32, r64)
    return r64, e32, max(B, 4 * e32) + 4 * extra[0], max(ratio * B, 4 * e32px) + 4 * extra[1]


def check(kernel, case, shape, mode, got, ref, e32, bar, bar_px):
    """Prints the table row of one run, then asserts it: finite, rel-L2 and worst pixel under their bars."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    finite = bool(torch.isfinite(got).all())
    err, px = (rel_l2(got, ref), worst_px(got, ref)) if finite else (float("nan"), float("nan"))
    print(f"\n| {kernel} | {case} | {shape} | {mode} | {err:.2e} | {px:.2e} | {e32:.2e} | {bar:.1e} | {bar_px:.1e} |")
    assert finite, (kernel, case, shape, mode, "non-finite output")
    assert err < bar and px < bar_px, (kernel, case, shape, mode, err, px, bar, bar_px)
    return err, px
