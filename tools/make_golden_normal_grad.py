#!/usr/bin/env python3
"""Generate tests/golden/normal_grad_cases.npz: prediction.grad of the IMPORTED reference's loss.loss.VideoNormalLoss (autograd
on the CPU in float32) for seeded inputs from tests/normal_ref.make_case, both against the stored target and against
utils.normal_utils.normal_vector(depth), flattened; the seeds and arguments of the cases; and per recorded gradient the
deviation of the restatement tests/normal_grad_ref.py from it as measured here: rel-L2, and max-abs divided by the reference's
max-abs (tests/test_normal_grad_host.py allows four times each). The file holds data only.

The cases are small and new (none is the 224 x 224 case of tools/make_golden_normals.py). The last one, SPECIAL, is
normal_grad_ref.make_special: a handful of kept predictions exactly zero, a handful under the clamp of F.cosine_similarity
(0 < |p| < 1e-8) and a handful of kept stored targets zero. Its gradient has entries of the size 1e8 / N, so it is recorded
and measured on its own, where they cannot swamp the other cases' rel-L2.

The pytorch_msssim stand-in is that of tools/make_golden_normals.py.

Conditions on the cases, asserted here before anything is written; a case that breaks one is to be replaced, not excused:
  * every random-mask case keeps between 25 % and 90 % of its pixels after the reference's own erosion (empty frames aside),
    which is also the restatement's erosion;
  * outside SPECIAL no kept prediction is shorter than 1e-3;
  * together the cases cover no mask, a bool and a float mask, an all-false mask, a frame without a kept pixel, B > 1 and a
    scaled target;
  * no deviation exceeds 1e-4: more than that means the restatement is wrong.

Usage: python tools/make_golden_normal_grad.py
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

#        seed  (B, T, H, W)      mask        target    frames without a kept pixel
CASES = [(61, (1, 2, 19, 23), "none", "unit", ()),
         (62, (1, 3, 21, 26), "bool", "unit", ()),
         (63, (1, 2, 24, 18), "float", "scaled", ()),
         (64, (1, 2, 11, 13), "allfalse", "unit", ()),
         (65, (2, 2, 17, 22), "bool", "scaled", (1,))]
SPECIAL = (66, (1, 2, 16, 20))
MIN_LENGTH = 1e-3


def main():
    argparse.ArgumentParser(description=__doc__.splitlines()[0]).parse_args()
    sys.path.insert(0, REF)
    install_msssim_stand_in()
    from loss.loss import VideoNormalLoss
    from utils.normal_utils import normal_vector
    import normal_grad_ref as G
    import normal_ref as R

    crit = VideoNormalLoss()

    def reference(case, from_depth):
        p = torch.from_numpy(case["pred"].copy()).requires_grad_()
        t = normal_vector(torch.from_numpy(case["depth"].copy())[:, :, None]) if from_depth else torch.from_numpy(case["target"].copy())
        crit(p, t, torch.from_numpy(case["mask"].copy()))["normal_loss"].backward()
        assert p.grad.dtype == torch.float32
        return p.grad.numpy()

    def deviation(case, from_depth, what):
        want = reference(case, from_depth)
        got, _ = G.normal_loss_grad_ref(case["pred"], case["depth"] if from_depth else case["target"], case["mask"], from_depth)
        keep = R.erode_ref(case["mask"])
        assert np.isfinite(want).all() and np.isfinite(got).all(), what
        diff, scale = got - want.astype(np.float64), float(np.abs(want).max())
        if scale == 0:
            assert not keep.any() and not got.any(), what
            rel = mx = 0.0
        else:
            rel = float(np.sqrt((diff ** 2).sum() / (want.astype(np.float64) ** 2).sum()))
            mx = float(np.abs(diff).max()) / scale
        print(f"{what}: kept {keep.mean():.3f} max|g| {scale:.3g} rel-L2 {rel:.2e} max-abs/max {mx:.2e}")
        assert rel <= 1e-4 and mx <= 1e-4, "the restatement is wrong"
        return want.ravel(), np.array([rel, mx], np.float64)

    out = {}
    for seed, shape, mask_kind, target_kind, empty in CASES:
        case = R.make_case(seed, shape, mask_kind, target_kind, empty)
        assert int(np.prod(shape)) <= 4000
        keep = R.erode_ref(case["mask"])
        assert np.array_equal(crit.eroded_mask(torch.from_numpy(case["mask"].copy())).numpy(), keep)
        if mask_kind in ("bool", "float"):
            full = [f for f in range(shape[0] * shape[1]) if f not in empty]
            share = float(keep.reshape(-1, shape[2] * shape[3])[full].mean())
            assert 0.25 <= share <= 0.90, (seed, share)
            assert all(not keep.reshape(-1, shape[2] * shape[3])[f].any() for f in empty)
        length = np.sqrt((case["pred"].astype(np.float64) ** 2).sum(2))
        assert not keep.any() or length[keep].min() >= MIN_LENGTH, (seed, length[keep].min())
        for from_depth in (False, True):
            key = f"{seed}_{'depth' if from_depth else 'stored'}"
            out[f"grad_{key}"], out[f"deviation_{key}"] = deviation(case, from_depth, f"seed {seed} {shape} {mask_kind} {target_kind} {key}")
    kinds = {c[2] for c in CASES}
    assert kinds == {"none", "bool", "float", "allfalse"} and any(c[3] == "scaled" for c in CASES)
    assert any(c[1][0] > 1 for c in CASES) and any(c[4] for c in CASES)

    seed, shape = SPECIAL
    case, idx = G.make_special(seed, shape)
    keep = R.erode_ref(case["mask"]).reshape(-1)
    assert 0.25 <= keep.mean() <= 0.90
    length = np.sqrt((case["pred"].astype(np.float64) ** 2).sum(2)).reshape(-1)
    tlen = np.sqrt((case["target"].astype(np.float64) ** 2).sum(2)).reshape(-1)
    assert all(keep[v].all() for v in idx.values())
    assert (length[idx["zero_pred"]] == 0).all() and ((length[idx["tiny"]] > 0) & (length[idx["tiny"]] < 1e-8)).all()
    assert (tlen[idx["zero_target"]] == 0).all() and (length[idx["zero_target"]] >= MIN_LENGTH).all()
    rest = keep.copy()
    rest[np.concatenate([idx["zero_pred"], idx["tiny"]])] = False
    assert length[rest].min() >= MIN_LENGTH
    for from_depth in (False, True):
        key = f"{seed}_{'depth' if from_depth else 'stored'}"
        out[f"grad_{key}"], out[f"deviation_{key}"] = deviation(case, from_depth, f"special seed {seed} {shape} {key}")

    path = os.path.join(GOLD, "normal_grad_cases.npz")
    np.savez(path, seed=np.array([c[0] for c in CASES]), shape=np.array([c[1] for c in CASES]), mask_kind=np.array([c[2] for c in CASES]),
             target_kind=np.array([c[3] for c in CASES]), empty=np.array([list(c[4]) + [-1] * (4 - len(c[4])) for c in CASES]),
             checksum=np.array([R.checksum(R.make_case(*c)) for c in CASES], np.float64), special_seed=np.array(seed),
             special_shape=np.array(shape), special_checksum=np.array(R.checksum(case), np.float64),
             **{f"special_{k}": v for k, v in idx.items()}, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
