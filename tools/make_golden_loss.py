#!/usr/bin/env python3
"""Generate tests/golden/loss_cases.npz: the values of the IMPORTED reference's loss.loss.VideoDepthLoss (run on the CPU in
float32) for seeded inputs from tests/loss_ref.make_case. The file stores seeds, shapes, arguments, input checksums, the
reference's values per key and, per key, the largest deviation of the restatement tests/loss_ref.py from them as measured
here (tests/test_loss_host.py allows four times that).

loss/loss.py imports pytorch_msssim at module level (for the SSIM term, which this project does not compute): the in-memory
stand-in of tools/make_golden_normals.py lets the module import. VideoDepthLoss also constructs the SSIM term it never calls
at ssim_loss_scale = 0, so the stand-in's empty class gets a constructor that takes the arguments and keeps nothing.

Condition on the cases. The reference fits in float32 and the restatement in float64, so close to the 1.25 bound of d1 the
two can decide a pixel differently. Every recorded case must give the same integer round(d1 * count) on both sides; a seed
that does not is to be replaced (none of the shapes below did). A deviation bar above 1e-4 means the restatement is wrong.

Usage: python tools/make_golden_loss.py   (tools/loss_bench.py lists the recorded values and deviations in profiles/depth_loss.md)
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import GOLD, REF, ROOT  # noqa: E402
from make_golden_normals import install_msssim_stand_in  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))

KEYS = ("spatial_loss", "stable_loss", "absRel_loss", "d1", "total_loss")
# Two pixels fix the two unknowns of the fit, so at [1, 2, 1, 1] the residual is the fit's own rounding: with pixels 0.2 apart
# the float32 determinant of the reference cancels to 4 digits (its absRel_loss is 2e-4 where float64 gives 1e-8). That case
# therefore draws its frames 3.0 apart (FRAME_NOISE), where the float32 fit is good to 1e-6.
FRAME_NOISE = {45: 3.0}
#        seed (B, T, H, W)     keep kind        mask     empty frames  empty items  alpha stable_scale
CASES = [(41, (2, 3, 17, 13), 0.8, "plain", "bool", (), (), 0.5, 10),       # odd sizes, ragged grids, two fits
         (42, (1, 2, 9, 11), 0.8, "plain", "uint8", (), (), 0.5, 10),
         (43, (1, 4, 16, 16), 0.8, "plain", "bool", (), (), 0.5, 10),       # whole quads
         (44, (1, 2, 2, 3), 0.8, "plain", "bool", (), (), 0.5, 10),         # grids that collapse to a point
         (45, (1, 2, 1, 1), 1.0, "plain", "bool", (), (), 0.5, 10),
         (46, (1, 3, 64, 48), 0.8, "plain", "bool", (), (), 0.5, 10),
         (47, (1, 3, 17, 13), 0.3, "plain", "bool", (), (), 0.5, 10),       # both medians are exactly 0
         (48, (1, 2, 16, 16), 1.0, "plain", "uint8", (), (), 0.5, 10),      # even H * W: the lower of the two middle values
         (49, (1, 4, 17, 13), 0.8, "plain", "bool", (2,), (), 0.5, 10),     # an empty frame
         (50, (2, 3, 17, 13), 0.8, "plain", "bool", (), (1,), 0.5, 10),     # an empty item: det == 0, alignment 0
         (51, (1, 3, 17, 13), 0.6, "anti", "bool", (), (), 0.5, 10),        # negative scale, zeros sort into the middle
         (52, (1, 3, 17, 13), 0.8, "straddle", "bool", (), (), 0.5, 10),    # targets around 1e-3 and 70, a kept 0
         (53, (2, 3, 17, 13), 0.8, "plain", "bool", (), (), 0.0, 10),       # no regulariser
         (54, (1, 3, 9, 11), 0.8, "plain", "uint8", (), (), 0.5, 0)]        # no temporal term: the key is absent


def main():
    argparse.ArgumentParser(description=__doc__.splitlines()[0]).parse_args()
    sys.path.insert(0, REF)
    install_msssim_stand_in()
    # VideoDepthLoss constructs the SSIM term it never calls at ssim_loss_scale = 0: the stand-in's class must take arguments
    sys.modules["pytorch_msssim"].MS_SSIM = type("MS_SSIM", (), {"__init__": lambda self, *args, **kw: None})
    from loss.loss import VideoDepthLoss
    import loss_ref as R

    dev = {k: 0.0 for k in KEYS}
    expected = {k: [] for k in KEYS}
    sums, hits = [], []
    for seed, shape, keep, kind, mdt, ef, ei, alpha, ss in CASES:
        c = R.make_case(seed, shape, keep, kind, mdt, ef, ei, FRAME_NOISE.get(seed, 0.2))
        with torch.no_grad():
            want = VideoDepthLoss(alpha=alpha, stable_scale=ss)(torch.from_numpy(c["pred"].copy()), torch.from_numpy(c["target"].copy()),
                                                               torch.from_numpy(c["mask"].copy()))
        got = R.depth_loss_ref(c["pred"], c["target"], c["mask"], alpha=alpha, stable_scale=ss)
        assert set(want) == set(KEYS) - (set() if ss > 0 else {"stable_loss"}), sorted(want)
        n = int((c["mask"] != 0).sum())
        ref_hits = int(round(float(want["d1"]) * n))
        assert ref_hits == got["d1_hits"], f"seed {seed}: d1 decides {ref_hits} vs {got['d1_hits']} pixels: replace the seed"
        line = [f"{seed}", "x".join(map(str, shape)), kind, f"{keep}", mdt]
        for k in KEYS:
            if k not in want:
                expected[k].append(np.nan)
                line.append("absent")
                assert k not in got
                continue
            w = float(want[k])
            expected[k].append(w)
            dev[k] = max(dev[k], abs(got[k] - w))
            line.append(f"{w:.7g} ({got[k] - w:+.1e})")
        print(" | ".join(line))
        sums.append(R.checksum(c))
        hits.append(ref_hits)
    print("largest deviation of the restatement per key:", {k: f"{v:.2e}" for k, v in dev.items()})
    assert all(4 * v <= 1e-4 for v in dev.values()), "the restatement is wrong"
    np.savez(os.path.join(GOLD, "loss_cases.npz"), seed=np.array([c[0] for c in CASES]), shape=np.array([c[1] for c in CASES]),
             keep_rate=np.array([c[2] for c in CASES], np.float64), kind=np.array([c[3] for c in CASES]),
             mask_dtype=np.array([c[4] for c in CASES]), empty_frames=np.array([list(c[5]) + [-1] * (4 - len(c[5])) for c in CASES]),
             empty_items=np.array([list(c[6]) + [-1] * (4 - len(c[6])) for c in CASES]),
             frame_noise=np.array([FRAME_NOISE.get(c[0], 0.2) for c in CASES], np.float64),
             alpha=np.array([c[7] for c in CASES], np.float64), stable_scale=np.array([c[8] for c in CASES], np.float64),
             checksum=np.array(sums, np.float64), d1_hits=np.array(hits, np.int64),
             **{f"expected_{k}": np.array(expected[k], np.float64) for k in KEYS},
             **{f"deviation_{k}": np.float64(dev[k]) for k in KEYS})
    print("wrote", os.path.join(GOLD, "loss_cases.npz"))


if __name__ == "__main__":
    main()
