#!/usr/bin/env python3
"""Generate tests/golden/eval_cases.npz: the seven clip metrics of the IMPORTED reference
(eval_depthcrafter.eval.eval_single_by_data, run on the CPU) for seeded clips from tests/eval_ref.make_case.
The file stores seeds, shapes, arguments, input checksums and the expected values, not arrays.

cv2 is not needed for equal sizes: an in-memory shim returns the image unchanged (dropping a trailing singleton channel, as
cv2.resize does) and raises when a resize is asked for.

Every case must exercise each branch of the evaluation; that is asserted here on the reference's own arithmetic
(numpy, SVD lstsq), before tests/eval_ref.py is compared with the reference.

Usage: python tools/make_golden_eval.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import GOLD, REF, ROOT  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))

#        seed  (T, H, W)      domain   mask   frames without a valid pixel
CASES = [(11, (6, 37, 53), "depth", False, (0, 3)),
         (12, (6, 37, 53), "depth", True, (2, 5)),
         (13, (6, 37, 53), "disp", False, (1, 5)),
         (14, (5, 41, 30), "disp", True, (0,)),
         (15, (4, 23, 67), "depth", True, (3,))]
DMIN, DMAX = 1e-3, 70.0


def install_cv2_shim():
    cv2 = types.ModuleType("cv2")

    def resize(image, dsize, *a, **k):
        if (image.shape[1], image.shape[0]) != tuple(dsize):
            raise NotImplementedError("cv2 shim: only the identity resize")
        return image[..., 0] if image.ndim == 3 and image.shape[2] == 1 else image

    cv2.resize = resize
    sys.modules["cv2"] = cv2
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            m = types.ModuleType("tqdm")
            m.tqdm = lambda it, *a, **k: it
            sys.modules["tqdm"] = m


def conditions(pred, gt, mask, domain):
    """The branch coverage of one case, from the reference's statements (eval.py:81-128, metric.py:3-33, 115-129)."""
    valid = np.logical_and(gt > DMIN, gt < DMAX)
    if mask is not None:
        valid = np.logical_and(valid, mask)
    share = valid.mean()
    assert 0.05 < share < 0.95, share
    n = valid.sum((-1, -2))
    assert (n == 0).any() and (n > 0).any(), n
    p64 = pred.astype(np.float64)
    low = (p64 < DMIN).mean()
    assert low > 0.01, low
    p = np.clip(p64, a_min=DMIN, a_max=None)
    g = gt[valid].reshape(-1, 1).astype(np.float64)
    t = g if domain == "disp" else 1.0 / (g + 1e-8)
    A = np.concatenate([p[valid].reshape(-1, 1), np.ones_like(g)], axis=-1)
    scale, shift = np.linalg.lstsq(A, t, rcond=None)[0]
    a = np.clip(scale * p + shift, a_min=DMIN, a_max=None)
    if domain == "depth":
        a = 1.0 / a
    upper = int((a > DMAX).sum())
    assert upper > 0, upper
    a = np.clip(a, DMIN, DMAX)
    kept = n > 0
    dg = gt[kept][:, 1:] - gt[kept][:, :-1]                      # float32, as the reference's tensors
    m = valid[kept][:, :-1] & (dg < np.float32(0.05))
    tgm_share = m.mean()
    assert 0.05 < tgm_share < 0.95, tgm_share
    assert (m.sum((-1, -2)) > 0).all()
    ulp = np.spacing(np.float32(0.05))
    assert (np.abs(dg.astype(np.float64) - float(np.float32(0.05))) > ulp).all()
    g64 = gt.astype(np.float64)
    with np.errstate(all="ignore"):
        r = np.maximum(a / g64, g64 / a)[valid]
    for thr in (1.25, 1.25 ** 2, 1.25 ** 3):
        assert (np.abs(r - thr) > 1e-9 * thr).all(), thr
    return dict(valid=share, low=low, upper=upper, tgm=tgm_share)


def main():
    sys.path.insert(0, REF)
    install_cv2_shim()
    from eval_depthcrafter.eval import eval_metrics, eval_single_by_data
    import eval_ref as R
    assert list(eval_metrics) == R.eval_metrics
    out = dict(seed=[], shape=[], domain=[], with_mask=[], empty=[], checksum=[], expected=[])
    for seed, shape, domain, with_mask, empty in CASES:
        pred, gt, mask = R.make_case(seed, shape, domain, with_mask, empty, DMIN, DMAX)
        cond = conditions(pred, gt, mask, domain)
        want = eval_single_by_data(pred.copy(), gt.copy(), device="cpu", seq_len=98, domain=domain,
                                   dataset_min_depth=DMIN, dataset_max_depth=DMAX,
                                   mask=None if mask is None else mask.copy())
        got = R.eval_ref(pred, gt, 98, domain, DMIN, DMAX, mask)
        rel = [abs(got[i] - want[i]) / abs(want[i]) for i in R.F64_IDX]
        print(f"seed {seed} {shape} {domain:5s} mask={with_mask}: {cond} eval_ref vs reference max rel {max(rel):.2e}")
        print("   ", want)
        assert max(rel) < 1e-12, rel
        for i in R.DELTA_IDX:
            assert np.float32(got[i]) == np.float32(want[i]), (i, got[i], want[i])
        out["seed"].append(seed)
        out["shape"].append(shape)
        out["domain"].append(domain)
        out["with_mask"].append(with_mask)
        out["empty"].append(list(empty) + [-1] * (4 - len(empty)))
        out["checksum"].append([pred.astype(np.float64).sum(), gt.astype(np.float64).sum(),
                                -1.0 if mask is None else float(mask.sum())])
        out["expected"].append(want)
    np.savez(os.path.join(GOLD, "eval_cases.npz"), seed=np.array(out["seed"]), shape=np.array(out["shape"]),
             domain=np.array(out["domain"]), with_mask=np.array(out["with_mask"]), empty=np.array(out["empty"]),
             checksum=np.array(out["checksum"], np.float64), expected=np.array(out["expected"], np.float64),
             dmin=np.float64(DMIN), dmax=np.float64(DMAX), metrics=np.array(R.eval_metrics))
    print("wrote", os.path.join(GOLD, "eval_cases.npz"))


if __name__ == "__main__":
    main()
