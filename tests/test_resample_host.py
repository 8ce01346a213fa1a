"""The CPU side of tests/test_gpu_resample.py: the numpy-exact emulation of the two align_corners weight flavours, and that
the shapes the GPU tests use tell them apart at each test's bar (resample_ref.py derives the bars)."""
import numpy as np
import torch

import resample_ref as R
from oc1_ref import ac_coords


def test_fused_weight_is_the_once_rounded_one_and_rounded_is_torchs():
    for I, O in R.SHAPES + R.SHAPES_2X + [(518, 1080)]:
        i0, i1, lr = ac_coords(O, I, torch.float32)
        j0, j1, lf = ac_coords(O, I, torch.float32, weight="fused")
        assert torch.equal(i0, j0) and torch.equal(i1, j1)
        s = np.float32(I - 1) / np.float32(O - 1)
        o = np.arange(O, dtype=np.float32)
        src = s * o
        assert src.dtype == np.float32 and np.array_equal(lr.numpy(), src - i0.numpy().astype(np.float32))
        exact = np.float64(s) * o.astype(np.float64)            # 24 x 24 bits: exact in float64
        assert np.array_equal(exact.astype(np.float32), src)    # the rounded flavour's product is its one rounding
        assert np.array_equal(lf.numpy(), (exact - i0.numpy()).astype(np.float32))
        assert float((lr - lf).abs().max()) <= float(np.spacing(np.float32(I - 1))) / 2
        assert int((lr != lf).sum()) > O // 2     # the flavours differ at most destination indices


def test_chosen_shapes_tell_the_flavours_apart():
    # (H, OH, board, bar, candidate shapes, the shape the GPU test must end up with)
    for H, OH, lo, hi, bar, shapes, want in [
        (8, 14, -1, 1, R.BLEND + R.SPLIT, R.SHAPES, (76, 133)),       # upsample, split planes
        (8, 14, -1, 1, R.BLEND, R.SHAPES, (76, 133)),                 # dn_tail
        (8, 14, 1, 3, R.BLEND + R.SPLIT, R.SHAPES, (148, 259)),       # depth_tail
        (8, 16, -1, 1, R.CORNER, R.SHAPES_2X, (74, 148)),             # oc1_combine
    ]:
        got = R.smallest(shapes, H, OH, lo, hi, bar)
        print(f"[resample] board {{{lo}, {hi}}} bar {bar} U: " + ", ".join(
            f"{W}->{OW} gap {R.gap(H, W, OH, OW, lo, hi):.1f} U" for W, OW in shapes) + f"; chosen {got}")
        assert got == want, (got, want)
    # one fp16 plane cannot tell them apart: its rounding alone is 8192 U
    assert not any(R.discriminates(8, W, 14, OW, -1, 1, R.BLEND + R.HALF) for W, OW in R.SHAPES)
