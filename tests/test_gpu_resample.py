"""Holds each kernel's align_corners weight flavour (csrc/resample.hpp) in place on the MI355X: the device output against the
float64 blend of a one-pixel checkerboard under the flavour documented for that kernel, at a bar derived from the arithmetic
(resample_ref.py), after asserting on the CPU that the OTHER flavour's reference misses that bar by 4 x or more.

  rounded  upsample_kernel (vdn_upsample_bilinear), oc1_combine_kernel (vdn_oc1_combine), dn_tail_kernel (vdn_dn_tail);
           upsample_f32_kernel is pinned to torch's fp32 by test_gpu_geometry.py
  fused    depth_tail_kernel (vdn_depth_tail)
The resize that tells the flavours apart runs along W; H is a handful of rows (8 -> 14, 8 -> 16 for the 2x combine)."""
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, OH = 8, 14


def runtime(split):
    from vdn import _abi
    from vdn.runtime import Runtime
    assert torch.cuda.is_available() and _abi.lib.vdn_arch_ok() == 1
    return Runtime(DEV, torch.float16, split)


def check(name, got, flavour, bar, shape, lo, hi):
    """got f32/f64 [B, OH, OW] on the CPU against the `flavour` reference of the {lo, hi} board, bar in U max|x|."""
    h, W, oh, OW = shape
    ref = R.refs(h, W, oh, OW, lo, hi)
    m = max(abs(lo), abs(hi))
    err = float((got.double() - ref[flavour]).abs().max()) / (R.U * m)
    other = float((got.double() - ref[R.OTHER[flavour]]).abs().max()) / (R.U * m)
    print(f"[resample] {name} {W} -> {OW}: max |device - fp64 blend, {flavour} weights| {err:.1f} U max|x|, bar {bar} U; "
          f"to the {R.OTHER[flavour]} weights {other:.1f} U (the references are {R.gap(h, W, oh, OW, lo, hi):.1f} U apart)")
    assert torch.isfinite(got).all() and err <= bar, (name, err, bar)


@pytest.mark.parametrize("split", [False, True])
def test_upsample_planes_rounded(split):
    """16-bit planes, C = 8, 76 -> 133. One fp16 plane rounds by 2^-11 and can only agree; the split planes discriminate."""
    W, OW = 76, 133
    bar = R.BLEND + (R.SPLIT if split else R.HALF)
    assert R.discriminates(H, W, OH, OW, -1, 1, bar) == split
    rt, B, C = runtime(split), 2, 8
    x = rt.to_half(R.board(B, H, W, C, -1, 1).reshape(-1, C).to(DEV))
    y = rt.hbuf(f"t_resample_up{int(split)}", (B * OH * OW, C))
    rt.upsample(x, y, B, H, W, OH, OW, C)
    got = y.float().cpu().reshape(B, OH, OW, C)
    for c in (0, C - 1):
        check(f"upsample split={int(split)} c={c}", got[..., c], "rounded", bar, (H, W, OH, OW), -1, 1)


def test_oc1_combine_rounded():
    """The centre tap image holds the board, the other eight zeros, the bias is zero: the output is the board sampled at the
    pixel's own position with the four-corner-weight form."""
    h, oh, Co, B = 8, 16, 16, 1
    W, OW = R.smallest(R.SHAPES_2X, h, oh, -1, 1, R.CORNER)
    assert (W, OW) == (74, 148)
    rt = runtime(True)
    z = torch.zeros(B, h, W, 9, Co)
    z[:, :, :, 4, :] = R.board(B, h, W, Co, -1, 1)
    out = torch.empty(B * oh * OW, Co, device=DEV)
    rt.oc1_combine(z.reshape(B * h * W, 9 * Co).to(DEV), torch.zeros(Co, device=DEV), out, B, h, W, oh, OW, Co)
    got = out.cpu().reshape(B, oh, OW, Co)
    for c in (0, Co - 1):
        check(f"oc1_combine c={c}", got[..., c], "rounded", R.CORNER, (h, W, oh, OW), -1, 1)


def test_dn_tail_rounded():
    """Weight 1 at the centre tap from input channel 0 to output channel 0, everything else and the bias zero: the fmaf chain
    reproduces the source value exactly and raw[:, 0] is the blend.

    The kernel's weight has been the rounded one since it was written: hipcc packs its two axes into one v_pk_mul_f32 and one
    v_pk_add_f32, which cannot be fused (profiles/resample_refactor.md)."""
    W, OW = 76, 133
    assert R.discriminates(H, W, OH, OW, -1, 1, R.BLEND)
    rt, F, Cin = runtime(True), 2, 8
    x = torch.zeros(F, H, W, Cin)
    x[..., 0] = R.board(F, H, W, 1, -1, 1)[..., 0]
    w = torch.zeros(3, Cin, 3, 3)
    w[0, 0, 1, 1] = 1.0
    raw = torch.empty(F, 3, OH, OW, device=DEV)
    rt.dn_tail(x.to(DEV), F, H, W, Cin, w.to(DEV), torch.zeros(3, device=DEV), OH, OW, raw=raw)
    got = raw.cpu()
    assert float(got[:, 1:].abs().max()) == 0.0
    check("dn_tail", got[:, 0], "rounded", R.BLEND, (H, W, OH, OW), -1, 1)


def test_depth_tail_fused():
    """C = 32; the 3 x 3 weight is 1 at the centre tap from channel 0 to channel 0, bias2 = 0, w1 = e0, b1 = 0, relu=False:
    the output is the blend of the {1, 3} board (positive: the ReLU after the 3 x 3 conv passes it) split into fp16 planes,
    whose sum the MFMAs and the 32 -> 1 dot product carry exactly."""
    from vdn import pack
    C, B = 32, 2
    bar = R.BLEND + R.SPLIT
    W, OW = R.smallest(R.SHAPES, H, OH, 1, 3, bar)
    assert (W, OW) == (148, 259)
    for I, O in ((H, OH), (W, OW)):   # vdn_depth_tail's own guard: the 13 x 13 source patch covers a tile's halo
        assert int(17.0 * ((I - 1) / (O - 1))) + 3 <= 13
    rt = runtime(True)
    x = torch.zeros(B, H, W, C)
    x[..., 0] = R.board(B, H, W, 1, 1, 3)[..., 0]
    w2 = torch.zeros(32, C, 3, 3)
    w2[0, 0, 1, 1] = 1.0
    w1 = torch.zeros(32)
    w1[0] = 1.0
    d = torch.empty(B, OH, OW, device=DEV)
    rt.depth_tail(x.reshape(-1, C).to(DEV), pack.conv3x3_taps(w2.to(DEV), rt.prec), torch.zeros(32, device=DEV), w1.to(DEV), 0.0,
                  d, B, H, W, C, OH, OW, relu=False)
    check("depth_tail", d.cpu(), "fused", bar, (H, W, OH, OW), 1, 3)
