#!/usr/bin/env python3
"""Generate tests/golden/metric_cases.npz: what the IMPORTED reference (metric_depth/util/metric.py:eval_depth and
metric_depth/util/loss.py:SiLogLoss, run on the CPU) gives for the seeded cases of tests/metric_ref.py, with the mask composed
as metric_depth/train.py:133 and :169 compose it, in float32. The file stores seeds, shapes, arguments, input checksums and
expected values, not arrays.

Each case runs twice. In float32, as the scripts run it: the bits of d1 d2 d3 and the values the scripts would print. On
.double() copies of the same float32 inputs (the mask still composed in float32): the six continuous metrics, the loss and
its autograd gradient (a checksum and a few sampled elements), which is what tests/metric_ref.py restates. The largest
relative gap between the two runs is recorded as `f32_gap`: it says how far the scripts' printed values sit from the contract
and is not a tolerance for anything.

Every case must exercise the branch it is named for; that is asserted here before tests/metric_ref.py is compared with the
reference.

Usage: python tools/make_golden_metric.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import GOLD, REF, ROOT  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))


def conditions(c, case, keep):
    """The branch a case is named for, from the inputs and the float32 mask alone."""
    import metric_ref as R
    sp, depth, pred, mask = c["special"], case["depth"], case["pred"], case["mask"]
    n = keep.reshape(keep.shape[0], -1).sum(1)
    assert n.max() <= 4096, n
    if sp in ("plain", "bounds", "mask_values", "ratio", "equal", "negative_radicand"):
        assert (n >= 10).all() and 0.05 < keep.mean() < 0.95
        assert ((np.asarray(mask) == 1) & ~keep).any()            # the bounds drop something the mask keeps
    if sp == "bounds":
        lo, hi = np.float32(R.MIN_DEPTH), np.float32(R.MAX_DEPTH)
        assert (depth[:, 0, :4] == np.array([lo, np.nextafter(lo, np.float32(0)), hi, np.nextafter(hi, np.float32(np.inf))])).all()
        assert (np.asarray(mask)[:, 0, :4] == 1).all() and (keep[:, 0, :4] == np.array([True, False, True, False])).all()
    if sp == "mask_values":
        assert mask.dtype == np.float32 and (mask == 2).any() and (mask == 0.5).any() and not keep[(mask != 1)].any()
    if sp == "ratio":
        with np.errstate(all="ignore"):
            q = np.maximum(depth / pred, pred / depth)[0, 0, :6]
        assert q.tolist() == [1.25, 1.5625, 1.953125, 1.25, 1.5625, 1.953125] and keep[0, 0, :6].all()
    if sp == "nine_ten":
        assert n.tolist() == [9, 10]
    if sp == "empty_item":
        assert n[-1] == 0 and n[0] >= 10
    if sp == "empty_all":
        assert n.sum() == 0
    if sp == "equal":
        assert (pred[keep] == depth[keep]).all() and (pred[~keep] != depth[~keep]).any()
    return n


def main():
    sys.path.insert(0, os.path.join(REF, "metric_depth"))
    from util.loss import SiLogLoss
    from util.metric import eval_depth
    import metric_ref as R
    out = {k: [] for k in ("seed", "shape", "mask", "special", "lambd", "checksum")}
    arrays, gap = {}, 0.0
    for i, spec in enumerate(R.CASES):
        c = R.case_dict(*spec)
        case = R.make_case(c)
        pred, depth, mask = (torch.from_numpy(case[k]) for k in ("pred", "depth", "mask"))
        keep = (mask == 1) & (depth >= R.MIN_DEPTH) & (depth <= R.MAX_DEPTH)      # train.py:133 / :169, float32 tensors
        assert np.array_equal(keep.numpy(), R.keep_mask(case["mask"], case["depth"]))
        n = conditions(c, case, keep.numpy())
        f32, f64 = [], []
        for b in range(pred.shape[0]):
            r32 = eval_depth(pred[b][keep[b]], depth[b][keep[b]])
            r64 = eval_depth(pred[b][keep[b]].double(), depth[b][keep[b]].double())
            assert tuple(r32) == R.KEYS
            f32.append([r32[k] for k in R.KEYS])
            f64.append([r64[k] for k in R.KEYS])
        f32, f64 = np.array(f32, np.float64), np.array(f64, np.float64)
        crit = SiLogLoss(c["lambd"])
        loss32 = float(crit(pred, depth, keep))
        p64 = pred.double().requires_grad_(True)
        loss64 = crit(p64, depth.double(), keep)
        loss64.backward()
        grad = p64.grad.numpy()
        # ---- what the case is named for, on the reference's own results
        sp = c["special"]
        if sp == "empty_item":
            assert np.isnan(f32[-1]).all() and np.isnan(f64[-1]).all() and not np.isnan(f64[0]).any()
        if sp == "empty_all":
            assert np.isnan(f64).all() and np.isnan(loss64.item()) and not grad.any()
        if sp == "equal":
            assert loss64.item() == 0.0 and np.isnan(grad[keep.numpy()]).all() and not grad[~keep.numpy()].any()
        if sp == "negative_radicand":
            assert np.isnan(loss64.item()) and np.isnan(grad[keep.numpy()]).all() and not grad[~keep.numpy()].any()
        if sp == "ratio":
            k = keep.numpy()[0]
            with np.errstate(all="ignore"):
                q = np.maximum(case["depth"][0] / case["pred"][0], case["pred"][0] / case["depth"][0])[k]
            assert f32[0, 0] == float(np.float32((q < np.float32(1.25)).sum()) / np.float32(k.sum()))
        # ---- tests/metric_ref.py against the reference
        rows = R.eval_rows(case["pred"], case["depth"], case["mask"])
        assert np.array_equal(rows[:, 0], n)
        assert np.array_equal(rows[:, 1:4].astype(np.float32), f32[:, :3].astype(np.float32), equal_nan=True), (rows[:, 1:4], f32[:, :3])
        with np.errstate(all="ignore"):
            rel = np.abs(rows[:, 4:] - f64[:, 3:]) / np.abs(f64[:, 3:])
            g32 = np.abs(f32[:, 3:] - f64[:, 3:]) / np.abs(f64[:, 3:])
        assert np.array_equal(np.isnan(rows[:, 4:]), np.isnan(f64[:, 3:]))
        st = R.silog_ref(case["pred"], case["depth"], keep.numpy(), c["lambd"])
        gref = R.silog_grad_ref(case["pred"], case["depth"], keep.numpy(), c["lambd"])
        assert np.isnan(st[0]) == np.isnan(loss64.item()) and np.array_equal(np.isnan(gref), np.isnan(grad))
        finite = np.isfinite(grad)
        gmax = np.abs(grad[finite]).max() if finite.any() and np.abs(grad[finite]).max() > 0 else 1.0
        worst = max(np.nanmax(rel, initial=0.0), 0.0 if np.isnan(st[0]) or loss64.item() == 0 else abs(st[0] - loss64.item()) / abs(loss64.item()),
                    np.abs(gref - grad)[finite].max(initial=0.0) / gmax)
        if not np.isnan(loss64.item()) and loss64.item() != 0:
            g32 = np.append(g32.reshape(-1), abs(loss32 - loss64.item()) / abs(loss64.item()))
        case_gap = float(np.nanmax(g32, initial=0.0))
        gap = max(gap, case_gap)
        print(f"case {i} seed {c['seed']} {c['shape']} {c['mask']:5s} {sp:18s} n {n.tolist()} metric_ref vs reference(f64) max rel {worst:.2e}; "
              f"reference f32 vs f64 {case_gap:.2e}; loss {loss64.item():.6g}")
        assert worst < 1e-11, worst
        for k in ("seed", "mask", "special", "lambd"):
            out[k].append(c[k])
        out["shape"].append(c["shape"])
        out["checksum"].append(R.checksum(case))
        idx = R.sample_idx(grad.size)
        arrays.update({f"n{i}": n.astype(np.int64), f"f32_{i}": f32, f"f64_{i}": f64,
                       f"loss{i}": np.array([loss32, loss64.item()], np.float64),
                       f"grad{i}": np.concatenate(([np.nansum(grad), np.nansum(np.abs(grad)), float(np.isnan(grad).sum())],
                                                   grad.reshape(-1)[idx])).astype(np.float64)})
    path = os.path.join(GOLD, "metric_cases.npz")
    np.savez(path, seed=np.array(out["seed"]), shape=np.array(out["shape"]), mask=np.array(out["mask"]),
             special=np.array(out["special"]), lambd=np.array(out["lambd"], np.float64), checksum=np.array(out["checksum"], np.float64),
             min_depth=np.float64(R.MIN_DEPTH), max_depth=np.float64(R.MAX_DEPTH), keys=np.array(R.KEYS), f32_gap=np.float64(gap),
             **arrays)
    print("wrote", path, os.path.getsize(path), "bytes; f32 gap", gap)
    assert os.path.getsize(path) < 100 * 1000


if __name__ == "__main__":
    main()
