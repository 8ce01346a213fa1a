"""Inputs, float64 references and bars of the tests that hold each kernel's align_corners weight flavour in place
(csrc/resample.hpp: "rounded" = fl(fl(scale * dst) - i0), "fused" = fl(scale * dst - i0)); no kernels.

The input is a one-pixel checkerboard along W (neighbours 2 apart), constant along H and over the channels: the blend along W
is then a + 2 l (or a + 2 - 2 l), so a weight that moves by d moves the output by 2 d. The two flavours' weights differ by up to
half an ulp of the source coordinate, 2^-18 = 64 U at coordinates in [64, 128) (U = 2^-24).

Every bar is arithmetic only, in units of U max|x|, and none of it is taken from what the kernels return:
  BLEND  7.5  an fp32 evaluation of (1 - ly) ((1 - lx) a + lx b) + ly (...) against the exactly evaluated lerp of the SAME fp32
              weights: U/2 on each 1 - l (two levels) and 3 roundings per level (2 products, 1 sum; fewer where products are
              fused) of values below max|x|: 3.5 U + 4 U. This is half of test_gpu_geometry.py's UPSAMPLE BAR, which stands
              between two such evaluations.
  SPLIT  8.5  a value stored as fp16 planes hi = toward-zero fp16, lo = nearest fp16 of the rest: the rest is below 2^-10 |v|
              and its rounding below 2^-11 of that, 2^-21 |v| = 8 U |v|; where the rest is subnormal its rounding is 2^-25 =
              U/2 absolute, and max|x| >= 1 here.
  HALF   2^-11 = 8192 U  a value stored as ONE fp16 plane, rounded to nearest.
  CORNER 4.5  vdn_oc1_combine's four corner weights fl(fl(1 - ly) fl(1 - lx)) etc.: 1.5 U relative on each weight (their
              absolute values sum to 1), U/2 on each of the four products (together 0.5 U max|x|), U/2 max|x| on each of the
              four sums (three inside the tap, one onto the accumulator): 1.5 + 0.5 + 2 = 4 U, and 0.5 U for the second order.
A test asserts, on the CPU and before it touches the GPU, that the OTHER flavour's reference is at least 4 bars away from the
documented one's (`discriminates`): the device within one bar of the one is then at least three bars from the other."""
import functools

import torch

from oc1_ref import upsample_nhwc

U = 2.0 ** -24
BLEND, SPLIT, HALF, CORNER = 7.5, 8.5, 2.0 ** 13, 4.5
SHAPES = [(76, 133), (148, 259), (296, 518)]        # W -> OW candidates, smallest first (the DPT head's x1.75 resize)
SHAPES_2X = [(74, 148), (148, 296), (296, 592)]     # for the 2x combine
OTHER = {"rounded": "fused", "fused": "rounded"}


def board(B, H, W, C, lo, hi):
    """f32 [B, H, W, C]: lo at even columns, hi at odd ones."""
    row = torch.where(torch.arange(W) % 2 == 0, torch.tensor(float(lo)), torch.tensor(float(hi)))
    return row[None, None, :, None].expand(B, H, W, C).contiguous()


@functools.lru_cache(maxsize=None)
def refs(H, W, OH, OW, lo, hi):
    """{flavour: float64 [OH, OW]} blend of the board under fp32 coordinates of each flavour; computed once, never written to."""
    x = board(1, H, W, 1, lo, hi).double()
    return {f: upsample_nhwc(x, OH, OW, torch.float32, f)[0, :, :, 0] for f in ("rounded", "fused")}


def gap(H, W, OH, OW, lo, hi):
    """max |rounded - fused| of the two references, in units of U max|x|."""
    r = refs(H, W, OH, OW, lo, hi)
    return float((r["rounded"] - r["fused"]).abs().max()) / (U * max(abs(lo), abs(hi)))


def discriminates(H, W, OH, OW, lo, hi, bar):
    return gap(H, W, OH, OW, lo, hi) >= 4 * bar


def smallest(shapes, H, OH, lo, hi, bar):
    """The first (W, OW) of `shapes` at which the two flavours' references are 4 bars apart."""
    for W, OW in shapes:
        if discriminates(H, W, OH, OW, lo, hi, bar):
            return W, OW
    raise AssertionError("no listed shape tells the flavours apart at this bar")
