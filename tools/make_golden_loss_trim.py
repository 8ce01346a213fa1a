#!/usr/bin/env python3
"""Generate tests/golden/loss_trim_cases.npz: the values of the IMPORTED reference's loss.loss.VideoDepthLoss(trim=...) (run on
the CPU in float32) for seeded inputs from tests/loss_ref.make_case, and for the small cases prediction.grad of its total_loss
(autograd). The file stores seeds, shapes, arguments, input checksums, the reference's five values, the gradients, and the
largest deviations of the restatement tests/loss_trim_ref.py from them as measured here (tests/test_loss_trim_host.py allows
four times each). The file holds data only. The pytorch_msssim stand-in is that of tools/make_golden_loss.py.

Conditions on the cases, asserted here; a seed that breaks one is to be replaced, not excused:
  * d1 decides the same pixels on both sides (as tools/make_golden_loss.py);
  * the data term's selection (thr, n_less, n_tied) does not change when every per-frame scale of the restatement moves by
    +-4 fp64 ulps: the device sums the scales in another order, and tests/test_gpu_loss_trim.py compares the selection exactly;
  * a case whose gradient is recorded has n_tied == 1 at all three thresholds (or k == 0): without ties the kept set of the
    reference's unstable sort is unambiguous;
  * no value deviates by more than 1e-4 / 4 and no gradient by more than 1e-4: more means a wrong restatement, not rounding.
The tie case of tests/loss_trim_ref.make_tie_case is run through the reference too: with many residuals on each threshold the
reference keeps an arbitrary subset of equal values, so its values must agree with the restatement's weighted ones, and the
ratio of its absRel_loss to the all-kept value (trim = 0) is recorded: the recipe's absRel ratios are bit-identical across
the tied pixels where the reference can run.

Usage: python tools/make_golden_loss_trim.py
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
GRAD_PIXELS = 2000   # gradients are recorded for cases up to this size
#        seed (B, T, H, W)     keep kind     mask     empty frames  empty items  alpha stable_scale trim
CASES = [(141, (2, 3, 17, 13), 0.8, "plain", "bool", (), (), 0.5, 10, 0.05),     # odd sizes, ragged grids, two fits
         (141, (2, 3, 17, 13), 0.8, "plain", "bool", (), (), 0.5, 10, 0.2),
         (141, (2, 3, 17, 13), 0.8, "plain", "bool", (), (), 0.5, 10, 0.5),
         (143, (1, 4, 16, 16), 0.8, "plain", "bool", (), (), 0.5, 10, 0.05),     # whole quads
         (143, (1, 4, 16, 16), 0.8, "plain", "uint8", (), (), 0.5, 10, 0.2),
         (143, (1, 4, 16, 16), 0.8, "plain", "bool", (), (), 0.5, 10, 0.5),
         (144, (1, 2, 2, 3), 1.0, "plain", "bool", (), (), 0.5, 10, 0.05),       # k = int(6 * 0.95) = 5
         (144, (1, 2, 2, 3), 1.0, "plain", "bool", (), (), 0.5, 10, 0.2),
         (144, (1, 2, 2, 3), 1.0, "plain", "bool", (), (), 0.5, 10, 0.5),
         (142, (1, 2, 9, 11), 0.8, "plain", "uint8", (), (), 0.5, 10, 0.999),    # k == 0 in every term
         (149, (1, 4, 17, 13), 0.8, "plain", "bool", (2,), (), 0.5, 10, 0.2),    # an empty frame
         (150, (2, 3, 17, 13), 0.8, "plain", "bool", (), (1,), 0.5, 10, 0.2),    # an empty item
         (151, (1, 3, 17, 13), 0.6, "anti", "bool", (), (), 0.5, 10, 0.2),       # negative scale
         (153, (2, 3, 17, 13), 0.8, "plain", "bool", (), (), 0.0, 10, 0.2),      # no regulariser
         (154, (1, 3, 9, 11), 0.8, "plain", "uint8", (), (), 0.5, 0, 0.2),       # no temporal term: the key is absent
         (146, (1, 3, 64, 48), 0.8, "plain", "bool", (), (), 0.5, 10, 0.2)]      # values only (above GRAD_PIXELS)


def main():
    argparse.ArgumentParser(description=__doc__.splitlines()[0]).parse_args()
    sys.path.insert(0, REF)
    install_msssim_stand_in()
    sys.modules["pytorch_msssim"].MS_SSIM = type("MS_SSIM", (), {"__init__": lambda self, *args, **kw: None})
    from loss.loss import VideoDepthLoss
    import loss_ref as R
    import loss_trim_ref as TR

    def reference(c, alpha, ss, trim, grad):
        p = torch.from_numpy(c["pred"].copy()).requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            want = VideoDepthLoss(alpha=alpha, trim=trim, stable_scale=ss)(p, torch.from_numpy(c["target"].copy()),
                                                                          torch.from_numpy(c["mask"].copy()))
        g = None
        if grad:
            want["total_loss"].backward()
            g = p.grad.numpy().copy()
        return {k: float(v) for k, v in want.items()}, g

    dev = {k: 0.0 for k in KEYS}
    gdev = [0.0, 0.0]
    expected = {k: [] for k in KEYS}
    sums, hits, out = [], [], {}
    for i, (seed, shape, keep, kind, mdt, ef, ei, alpha, ss, trim) in enumerate(CASES):
        c = R.make_case(seed, shape, keep, kind, mdt, ef, ei)
        with_grad = int(np.prod(shape)) <= GRAD_PIXELS
        want, g = reference(c, alpha, ss, trim, with_grad)
        got = TR.depth_loss_trim_ref(c["pred"], c["target"], c["mask"], alpha=alpha, stable_scale=ss, trim=trim)
        assert set(want) == set(KEYS) - (set() if ss > 0 else {"stable_loss"}), sorted(want)
        n = int((c["mask"] != 0).sum())
        ref_hits = int(round(want["d1"] * n))
        assert ref_hits == got["d1_hits"], f"seed {seed}: d1 decides {ref_hits} vs {got['d1_hits']} pixels: replace the seed"
        assert TR.data_selection_is_stable(c["pred"], c["target"], c["mask"], alpha=alpha, stable_scale=ss, trim=trim), \
            f"seed {seed} trim {trim}: the data term's selection hangs on the last bits of a frame's scale: replace the seed"
        line = [f"{seed}", "x".join(map(str, shape)), f"trim {trim}", "k " + "/".join(map(str, got["trim_k"])),
                "tied " + "/".join(map(str, got["trim_tied"]))]
        for k in KEYS:
            if k not in want:
                expected[k].append(np.nan)
                line.append("absent")
                assert k not in got
                continue
            expected[k].append(want[k])
            dev[k] = max(dev[k], abs(got[k] - want[k]))
            line.append(f"{want[k]:.7g} ({got[k] - want[k]:+.1e})")
        if with_grad:
            assert all(t == 1 or k == 0 for t, k in zip(got["trim_tied"], got["trim_k"])), f"seed {seed} trim {trim}: a tie at a threshold"
            r = TR.depth_loss_trim_grad_ref(c["pred"], c["target"], c["mask"], alpha=alpha, stable_scale=ss, trim=trim)
            diff, scale = r["grad"] - g.astype(np.float64), float(np.abs(g).max())
            rel = float(np.sqrt((diff ** 2).sum() / max(float((g.astype(np.float64) ** 2).sum()), 1e-300))) if scale else float(np.abs(diff).max())
            mx = float(np.abs(diff).max()) / scale if scale else float(np.abs(diff).max())
            gdev = [max(gdev[0], rel), max(gdev[1], mx)]
            line.append(f"grad max|g| {scale:.3g} rel-L2 {rel:.1e} max/max {mx:.1e}")
            out[f"grad_{i}"] = g.ravel()
        print(" | ".join(line))
        sums.append(R.checksum(c))
        hits.append(ref_hits)
    print("largest deviation of the restatement per key:", {k: f"{v:.2e}" for k, v in dev.items()}, "gradient (rel-L2, max/max):",
          [f"{v:.2e}" for v in gdev])
    assert all(4 * v <= 1e-4 for v in dev.values()) and max(gdev) <= 1e-4, "the restatement is wrong"

    # the tie case: the reference's arbitrary choice among equal values against the weights w
    c = TR.make_tie_case()
    want, _ = reference(c, 0.5, 10, 0.2, False)
    full, _ = reference(c, 0.5, 10, 0.0, False)
    got = TR.depth_loss_trim_ref(c["pred"], c["target"], c["mask"], trim=0.2)
    assert all(1 < t and 0 < w < 1 for t, w in zip(got["trim_tied"], got["trim_weight"])), (got["trim_tied"], got["trim_weight"])
    tie_dev = max(abs(got[k] - want[k]) for k in KEYS)
    ratio = want["absRel_loss"] / full["absRel_loss"]
    ours = got["absRel_loss"] / R.depth_loss_ref(c["pred"], c["target"], c["mask"])["absRel_loss"]
    print(f"tie case: largest deviation {tie_dev:.2e}; absRel trimmed / all kept: reference {ratio!r}, restatement {ours!r}")
    assert tie_dev <= 1e-5 and abs(ratio - ours) <= 1e-6
    np.savez(os.path.join(GOLD, "loss_trim_cases.npz"), seed=np.array([c[0] for c in CASES]), shape=np.array([c[1] for c in CASES]),
             keep_rate=np.array([c[2] for c in CASES], np.float64), kind=np.array([c[3] for c in CASES]),
             mask_dtype=np.array([c[4] for c in CASES]), empty_frames=np.array([list(c[5]) + [-1] * (4 - len(c[5])) for c in CASES]),
             empty_items=np.array([list(c[6]) + [-1] * (4 - len(c[6])) for c in CASES]),
             alpha=np.array([c[7] for c in CASES], np.float64), stable_scale=np.array([c[8] for c in CASES], np.float64),
             trim=np.array([c[9] for c in CASES], np.float64), checksum=np.array(sums, np.float64), d1_hits=np.array(hits, np.int64),
             **{f"expected_{k}": np.array(expected[k], np.float64) for k in KEYS},
             **{f"deviation_{k}": np.float64(dev[k]) for k in KEYS}, grad_deviation=np.array(gdev, np.float64),
             tie_expected=np.array([want[k] for k in KEYS], np.float64), tie_absrel_ratio=np.float64(ratio), **out)
    path = os.path.join(GOLD, "loss_trim_cases.npz")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
