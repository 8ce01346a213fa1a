#!/usr/bin/env python3
"""Generate tests/golden/loss_grad_cases.npz: prediction.grad of the IMPORTED reference's loss.loss.VideoDepthLoss (autograd on
the CPU in float32, the only dtype it runs in) for the seeded cases of tools/make_golden_loss.py, whose CASES, seeds and
arguments are imported, not retyped. For every case the file stores the float32 gradient of total_loss, flattened; for the
seeds in ALONE also the gradients of spatial_loss, stable_loss and absRel_loss alone, and for those in ABSREL_ALONE that of
absRel_loss alone (a second case behind the absRel chain, since seed 52's cannot be compared: below); and per recorded gradient the deviation
of the restatement tests/loss_grad_ref.py from it as measured here: rel-L2, and max-abs divided by the reference's max-abs
(tests/test_loss_grad_host.py allows four times each). The file holds data only.

The pytorch_msssim stand-in is that of tools/make_golden_loss.py.

Conditions on the cases, asserted here; a seed that breaks one is to be replaced, not excused:
  * every sign the restatement takes has an argument above 1e-9 in magnitude, so float32 and fp64 decide it alike. The one
    exception is structural and exact on both sides: the pixel that holds a frame's median has a - m = 0, and x - y = 0
    where it holds the target's median too, so 'a-m' and 'x-y' may have as many exact zeros as the case has frames; a
    difference of neighbours, a temporal difference and a - t may have none;
  * no two kept pixels of a frame share the median's value;
  * no deviation exceeds 1e-4: more than that means the restatement is wrong.
One recorded gradient cannot be compared: absRel_loss alone on seed 52, which keeps a target of exactly 0. The reference's
(a - t) / t is selected away there after the division, the division's backward multiplies the selection's zero by 1 / 0, and
the NaN spreads through the fit to every pixel. It is recorded as it is (all NaN) with a NaN deviation; total_loss does not
contain absRel_loss, so that case's other gradients are finite and compared.

Usage: python tools/make_golden_loss_grad.py
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import GOLD, REF, ROOT  # noqa: E402
from make_golden_loss import CASES, FRAME_NOISE  # noqa: E402
from make_golden_normals import install_msssim_stand_in  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))

ALONE = (41, 52)
ABSREL_ALONE = (46,)
#          key             weights (total, spatial, stable, absRel)
KEYS = (("total_loss", (1.0, 0.0, 0.0, 0.0)), ("spatial_loss", (0.0, 1.0, 0.0, 0.0)), ("stable_loss", (0.0, 0.0, 1.0, 0.0)),
        ("absRel_loss", (0.0, 0.0, 0.0, 1.0)))
SIGN_FLOOR = 1e-9


def main():
    argparse.ArgumentParser(description=__doc__.splitlines()[0]).parse_args()
    sys.path.insert(0, REF)
    install_msssim_stand_in()
    sys.modules["pytorch_msssim"].MS_SSIM = type("MS_SSIM", (), {"__init__": lambda self, *args, **kw: None})
    from loss.loss import VideoDepthLoss
    import loss_ref as R
    import loss_grad_ref as G

    out, worst, pixels, disagree = {}, 0.0, 0, 0
    for seed, shape, keep, kind, mdt, ef, ei, alpha, ss in CASES:
        c = R.make_case(seed, shape, keep, kind, mdt, ef, ei, FRAME_NOISE.get(seed, 0.2))
        for key, weights in KEYS if seed in ALONE else KEYS[:1] + KEYS[3:] if seed in ABSREL_ALONE else KEYS[:1]:
            p = torch.from_numpy(c["pred"].copy()).requires_grad_()
            VideoDepthLoss(alpha=alpha, stable_scale=ss)(p, torch.from_numpy(c["target"].copy()), torch.from_numpy(c["mask"].copy()))[key].backward()
            want = p.grad.numpy()
            assert want.dtype == np.float32
            got = G.depth_loss_grad_ref(c["pred"], c["target"], c["mask"], alpha=alpha, stable_scale=ss, weights=weights)
            if not np.isfinite(want).all():
                # (a - t) / t at a kept target of exactly 0: the reference selects that pixel away after the division, whose
                # backward multiplies the selection's zero by 1 / 0, and the NaN spreads through the fit to every pixel. The
                # restatement and the device skip the pixels absRel does not count. Recorded as it is, with no deviation.
                assert key == "absRel_loss" and ((c["mask"] != 0) & (c["target"] == 0)).any() and np.isnan(want).all()
                assert np.isfinite(got["grad"]).all()
                print(f"{seed} {'x'.join(map(str, shape))} {key}: the reference's gradient is NaN everywhere (a kept target of 0)")
                out[f"grad_{seed}_{key}"] = want.ravel()
                out[f"deviation_{seed}_{key}"] = np.array([np.nan, np.nan], np.float64)
                continue
            for what, (lo, zeros) in got["min_abs"].items():
                assert lo > SIGN_FLOOR, f"seed {seed} {key}: a sign of {what} is taken at {lo:.1e}: replace the seed"
                assert zeros <= (shape[0] * shape[1] if what in G.MAY_BE_ZERO else 0), f"seed {seed} {key}: {zeros} exact zeros of {what}: replace the seed"
            if key == "total_loss":
                a = R.align_ref(c["pred"], got["fwd"]["scale"], got["fwd"]["shift"]).reshape(-1, shape[2] * shape[3])
                k = (c["mask"] != 0).reshape(a.shape)
                for f, m in enumerate(got["fwd"]["m_pred"].ravel()):
                    assert (k[f] & (a[f] == m)).sum() <= 1, f"seed {seed}: frame {f} has two kept pixels at the median: replace the seed"
            diff = got["grad"] - want.astype(np.float64)
            scale = float(np.abs(want).max())
            rel = float(np.sqrt((diff ** 2).sum() / max(float((want.astype(np.float64) ** 2).sum()), 1e-300))) if scale else float(np.abs(diff).max())
            mx = float(np.abs(diff).max()) / scale if scale else float(np.abs(diff).max())
            pixels += want.size
            disagree += int((np.abs(diff) > 1e-4 * max(scale, 1e-300)).sum()) if scale else int((diff != 0).sum())
            zeros = {w: z for w, (lo, z) in got["min_abs"].items() if z}
            print(f"{seed} {'x'.join(map(str, shape))} {key}: max|g| {scale:.3g} rel-L2 {rel:.2e} max-abs/max {mx:.2e} max-abs {np.abs(diff).max():.2e}"
                  f" smallest sign argument {min(lo for lo, _ in got['min_abs'].values()):.1e} exact zeros {zeros}")
            worst = max(worst, rel, mx)
            out[f"grad_{seed}_{key}"] = want.ravel()
            out[f"deviation_{seed}_{key}"] = np.array([rel, mx], np.float64)
    print(f"{disagree} of {pixels} recorded components differ by more than 1e-4 of the largest; worst deviation {worst:.2e}")
    assert worst <= 1e-4 and disagree == 0, "the restatement is wrong"
    np.savez(os.path.join(GOLD, "loss_grad_cases.npz"), seed=np.array([c[0] for c in CASES]), alone=np.array(ALONE), absrel_alone=np.array(ABSREL_ALONE),
             keys=np.array([k for k, _ in KEYS]), weights=np.array([w for _, w in KEYS], np.float64), **out)
    print("wrote", os.path.join(GOLD, "loss_grad_cases.npz"), os.path.getsize(os.path.join(GOLD, "loss_grad_cases.npz")), "bytes")


if __name__ == "__main__":
    main()
