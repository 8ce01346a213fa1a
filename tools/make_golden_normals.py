#!/usr/bin/env python3
"""Generate tests/golden/normal_cases.npz: the normal loss of the IMPORTED reference (loss.loss.VideoNormalLoss against
utils.normal_utils.normal_vector, run on the CPU in float32) for seeded inputs from tests/normal_ref.make_case.
The file stores seeds, shapes, arguments, input checksums and the expected values; the only arrays are the reference's
normal_vector output for two small shapes.

loss/loss.py imports pytorch_msssim at module level (for a loss this project does not use): an in-memory stand-in with an
empty MS_SSIM class lets the module import.

Every random-mask case must keep between 25 % and 90 % of its pixels after the reference's own erosion, and the cases
together must cover every mask and target kind; both are asserted here before tests/normal_ref.py is compared with the
reference.

Usage: python tools/make_golden_normals.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import GOLD, REF, ROOT  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))

#        seed  (B, T, H, W)       mask        target    frames without a kept pixel
CASES = [(21, (1, 4, 37, 53), "none", "unit", ()),
         (22, (1, 4, 37, 53), "bool", "unit", ()),
         (23, (1, 3, 41, 30), "float", "unit", ()),
         (24, (1, 4, 37, 53), "bool", "unit", (2,)),
         (25, (1, 2, 23, 31), "allfalse", "unit", ()),
         (26, (2, 3, 37, 53), "bool", "scaled", ()),
         (27, (2, 2, 64, 257), "float", "scaled", (1,)),
         (28, (1, 1, 224, 224), "bool", "unit", ())]
# Recorded with normal_vector's default arguments: the bar of the comparison (4 * 2^-24 * max(1, max|d|): float32 rounding in a
# six-term stencil whose weights sum to 1 in magnitude per side, through a map whose derivative is at most 1) is derived
# for the kernel / 8 and scale_z = 1. Other arguments are tested on the device against tests/normal_ref.py.
#           seed (B, S, Y, X)  normalize_kernel scale_xy scale_z eps
NV_CASES = [(31, (1, 1, 5, 7), True, 1.0, 1.0, 1e-8),
            (32, (1, 2, 9, 8), True, 1.0, 1.0, 1e-8)]


def install_msssim_stand_in():
    m = types.ModuleType("pytorch_msssim")
    m.MS_SSIM = type("MS_SSIM", (), {})
    sys.modules["pytorch_msssim"] = m


def main():
    sys.path.insert(0, REF)
    install_msssim_stand_in()
    from loss.loss import VideoNormalLoss
    from utils.normal_utils import normal_vector
    import normal_ref as R

    # the image-based branch of the reference cannot run: record what it does
    c = R.make_case(1, (1, 2, 8, 9), "bool")
    try:
        VideoNormalLoss(reduction="image-based")(torch.from_numpy(c["pred"]), torch.from_numpy(c["target"]),
                                                 torch.from_numpy(c["mask"]))
        raise AssertionError("the reference's image-based reduction ran")
    except (IndexError, RuntimeError) as e:
        print(f"reduction='image-based' raises {type(e).__name__}: {str(e).splitlines()[0][:100]}")

    out = dict(seed=[], shape=[], mask_kind=[], target_kind=[], empty=[], checksum=[], expected=[], expected_depth=[],
               kept_share=[])
    loss = VideoNormalLoss()
    for seed, shape, mask_kind, target_kind, empty in CASES:
        c = R.make_case(seed, shape, mask_kind, target_kind, empty)
        pred, target, depth, mask = (torch.from_numpy(c[k].copy()) for k in ("pred", "target", "depth", "mask"))
        share = float(loss.eroded_mask(mask).float().mean())
        if mask_kind in ("bool", "float"):
            full = [f for f in range(shape[0] * shape[1]) if f not in empty]
            s = float(loss.eroded_mask(mask).flatten(0, 1)[full].float().mean())
            assert 0.25 <= s <= 0.90, s
        assert np.array_equal(loss.eroded_mask(mask).numpy(), R.erode_ref(c["mask"]))
        want = float(loss(pred, target, mask)["normal_loss"])
        want_depth = float(loss(pred, normal_vector(depth[:, :, None]), mask)["normal_loss"])
        got = R.normal_loss_ref(c["pred"], c["target"], c["mask"])[0]
        got_depth = R.normal_loss_ref(c["pred"], c["depth"], c["mask"], target_is_depth=True)[0]
        print(f"seed {seed} {shape} mask={mask_kind:8s} target={target_kind:6s} empty={empty}: kept {share:.3f} "
              f"loss {want:.7f} (restatement {got - want:+.1e}) from depth {want_depth:.7f} ({got_depth - want_depth:+.1e})")
        assert abs(got - want) <= 2e-6 and abs(got_depth - want_depth) <= 2e-6
        out["seed"].append(seed)
        out["shape"].append(shape)
        out["mask_kind"].append(mask_kind)
        out["target_kind"].append(target_kind)
        out["empty"].append(list(empty) + [-1] * (4 - len(empty)))
        out["checksum"].append(R.checksum(c))
        out["expected"].append(want)
        out["expected_depth"].append(want_depth)
        out["kept_share"].append(share)
    kinds = set(out["mask_kind"])
    assert kinds == {"none", "bool", "float", "allfalse"} and "scaled" in out["target_kind"]
    assert any(s[0] > 1 for s in out["shape"]) and any(e[0] >= 0 for e in out["empty"])

    nv = {}
    for i, (seed, shape, nk, sxy, sz, eps) in enumerate(NV_CASES):
        d = R.make_depth(np.random.default_rng(seed), shape)
        want = normal_vector(torch.from_numpy(d.copy())[:, :, None], nk, sxy, sz, eps).numpy()
        got = R.normal_vector_ref(d, nk, sxy, sz, eps)
        bar = 4 * 2.0 ** -24 * max(1.0, float(np.abs(d).max()))
        print(f"normal_vector seed {seed} {shape}: restatement vs reference max abs {np.abs(got - want).max():.2e} (bar {bar:.2e})")
        assert np.abs(got - want).max() <= bar
        nv[f"nv{i}"] = want.astype(np.float32)
        nv[f"nv{i}_depth_checksum"] = np.float64(d.astype(np.float64).sum())
    np.savez(os.path.join(GOLD, "normal_cases.npz"), seed=np.array(out["seed"]), shape=np.array(out["shape"]),
             mask_kind=np.array(out["mask_kind"]), target_kind=np.array(out["target_kind"]), empty=np.array(out["empty"]),
             checksum=np.array(out["checksum"], np.float64), expected=np.array(out["expected"], np.float64),
             expected_depth=np.array(out["expected_depth"], np.float64), kept_share=np.array(out["kept_share"], np.float64),
             nv_seed=np.array([c[0] for c in NV_CASES]), nv_shape=np.array([c[1] for c in NV_CASES]),
             nv_args=np.array([[float(c[2]), c[3], c[4], c[5]] for c in NV_CASES], np.float64), **nv)
    print("wrote", os.path.join(GOLD, "normal_cases.npz"))


if __name__ == "__main__":
    main()
