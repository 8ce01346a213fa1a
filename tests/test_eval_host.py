"""Host-side checks of the clip evaluation (vdn.eval, csrc/eval.hip): the CPU restatement against the values the reference
recorded in tests/golden/eval_cases.npz, the wrapper's argument errors and the VDN_EINVAL paths of the new entry points.
Nothing here launches a kernel."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

import eval_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_cases.npz")


def golden_cases():
    z = np.load(GOLD)
    for i in range(len(z["seed"])):
        yield dict(seed=int(z["seed"][i]), shape=tuple(int(s) for s in z["shape"][i]), domain=str(z["domain"][i]),
                   with_mask=bool(z["with_mask"][i]), empty=tuple(int(e) for e in z["empty"][i] if e >= 0),
                   checksum=z["checksum"][i], expected=z["expected"][i], dmin=float(z["dmin"]), dmax=float(z["dmax"]))


def case_inputs(c):
    pred, gt, mask = R.make_case(c["seed"], c["shape"], c["domain"], c["with_mask"], c["empty"], c["dmin"], c["dmax"])
    got = [pred.astype(np.float64).sum(), gt.astype(np.float64).sum(), -1.0 if mask is None else float(mask.sum())]
    assert np.allclose(got, c["checksum"], rtol=1e-13, atol=0), "the seeded generator no longer draws the recorded clip"
    return pred, gt, mask


CASES = list(golden_cases())


def test_fixture_lists_the_reference_metric_names():
    from vdn.eval import eval_metrics
    assert list(np.load(GOLD)["metrics"]) == R.eval_metrics == eval_metrics


@pytest.mark.parametrize("c", CASES, ids=lambda c: f"seed{c['seed']}-{c['domain']}")
def test_eval_ref_reproduces_the_reference(c):
    pred, gt, mask = case_inputs(c)
    got = R.eval_ref(pred, gt, 98, c["domain"], c["dmin"], c["dmax"], mask)
    for i in R.F64_IDX:
        rel = abs(got[i] - c["expected"][i]) / abs(c["expected"][i])
        print(f"{R.eval_metrics[i]}: {got[i]!r} vs {c['expected'][i]!r} rel {rel:.2e}")
        assert rel <= 1e-12
    for i in R.DELTA_IDX:
        assert np.float32(got[i]) == np.float32(c["expected"][i]) and got[i] == float(np.float32(got[i]))


def test_eval_ref_corner_semantics():
    """What the reference was observed to do at the corners the fixture cannot hold."""
    rng = np.random.default_rng(0)
    pred = rng.random((3, 4, 5), dtype=np.float32)
    assert all(np.isnan(v) for v in R.eval_ref(pred, np.zeros((3, 4, 5), np.float32)))        # no valid pixel: 7 NaN
    gt = (1 + 5 * rng.random((3, 1, 5))).astype(np.float32)
    out = R.eval_ref(pred[:, :1], gt)                                                          # H == 1: no gradient row
    assert np.isnan(out[2]) and not any(np.isnan(out[i]) for i in (0, 1, 3, 4, 5, 6))
    # a constant prediction: the minimum-norm solution of the rank-1 system, as numpy's lstsq gives it
    gt = (1 + 5 * rng.random((2, 4, 5))).astype(np.float32)
    p = np.full(40, 0.3)
    t = 1.0 / (gt.astype(np.float64).ravel() + 1e-8)
    want = np.linalg.lstsq(np.stack([p, np.ones(40)], 1), t, rcond=None)[0]
    assert np.allclose(R.fit_ref(p, t), want, rtol=1e-13, atol=0)


def test_wrapper_argument_errors():
    """Every ValueError comes before the device is touched."""
    from vdn.eval import eval_single_by_data
    p, g = np.ones((4, 3, 5), np.float32), np.ones((4, 3, 5), np.float32)
    with pytest.raises(ValueError, match="domain"):
        eval_single_by_data(p, g, domain="log")
    with pytest.raises(ValueError, match="frames"):
        eval_single_by_data(p, g[:3])                      # 4 predicted frames, 3 of gt
    with pytest.raises(ValueError, match="frames"):
        eval_single_by_data(p, g[:2], seq_len=3)
    with pytest.raises(ValueError, match="mask"):
        eval_single_by_data(p, g, mask=np.ones((4, 3, 4), bool))
    with pytest.raises(ValueError, match="mask"):
        eval_single_by_data(torch.from_numpy(p), torch.from_numpy(g), mask=torch.ones(3, 3, 5))
    with pytest.raises(ValueError):
        eval_single_by_data(p[0], g[0])


def test_eval_entry_points_reject_bad_arguments():
    from vdn import _abi
    L, P = _abi.lib, 4096                                   # P: a non-null, aligned stand-in; nothing is launched
    assert L.vdn_eval_workspace_bytes(0) == 0 and L.vdn_eval_workspace_bytes(3) % 8 == 0
    assert L.vdn_eval_workspace_bytes(98) == 98 * L.vdn_eval_workspace_bytes(1)
    fit_ok = [P, P, None, 2, 12, 1e-3, 70.0, _abi.EVAL_DEPTH, P, P, None]
    met_ok = [P, P, None, 2, 3, 4, 1e-3, 70.0, _abi.EVAL_DISP, _abi.EVAL_TGM_ROWS, P, P, P, None]
    rs_ok = [P, P, 2, 3, 4, 5, 6, None]

    def bad(fn, ok, **changes):
        for idx, val in changes.items():
            args = list(ok)
            args[int(idx[1:])] = val
            assert fn(*args) == -1, (fn.__name__, idx, val)

    bad(L.vdn_eval_fit, fit_ok, a0=None, a1=None, a3=0, a4=0, a5=70.0, a6=float("nan"), a7=2, a8=None, a9=None)
    bad(L.vdn_eval_metrics, met_ok, a0=None, a1=None, a3=0, a4=0, a5=-1, a6=71.0, a8=-1, a9=2, a10=None, a11=None, a12=None)
    bad(L.vdn_resize_bilinear_hp, rs_ok, a0=None, a1=None, a2=0, a3=0, a4=0, a5=0, a6=-3)
    assert L.vdn_eval_fit(*[P + 2 if i == 0 else a for i, a in enumerate(fit_ok)]) == -3      # a float pointer off by 2 bytes
    assert L.vdn_eval_metrics(*[P + 4 if i == 12 else a for i, a in enumerate(met_ok)]) == -3  # a double pointer off by 4
