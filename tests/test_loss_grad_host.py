"""Host-side checks of the depth criterion's gradient (vdn.loss, csrc/loss_grad.hip): the CPU restatement
tests/loss_grad_ref.py against prediction.grad of the reference's VideoDepthLoss as recorded in
tests/golden/loss_grad_cases.npz, the zeros the gradient must have, and the rejected-argument paths of the entry point.
Nothing here launches a kernel.

Bars. The reference's autograd runs in float32 and the restatement in float64. tools/make_golden_loss_grad.py measured, per
recorded gradient, the restatement's rel-L2 deviation and its largest absolute deviation over the reference's largest
component (1.4e-6 at most) and stored both; the bar is four times each, to cover float32 summation order across torch builds.
The generator refuses a deviation above 1e-4, which would mean a wrong restatement rather than rounding.

One recorded gradient is not a number: absRel_loss alone on seed 52, which keeps a target of exactly 0. The reference selects
that pixel away after dividing by it, the division's backward multiplies the selection's zero by 1 / 0, and the NaN spreads
through the fit to every pixel. The restatement and the device skip the pixels absRel does not count and stay finite; the
test states that difference."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import loss_grad_ref as G
from test_loss_host import CASES, case_id, case_inputs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_grad_cases.npz")
Z = np.load(GOLD)
KEYS = {str(k): tuple(float(x) for x in w) for k, w in zip(Z["keys"], Z["weights"])}
ALONE = {int(s) for s in Z["alone"]}
ABSREL_ALONE = {int(s) for s in Z["absrel_alone"]}
RECORDED = [(i, k) for i, c in enumerate(CASES)
            for k in (KEYS if c["seed"] in ALONE else ("total_loss", "absRel_loss") if c["seed"] in ABSREL_ALONE else ("total_loss",))]


@functools.lru_cache(maxsize=None)
def oracle(i, key="total_loss"):
    """The restatement on recorded case i for one key of the dictionary, computed once, shared and never written."""
    c = CASES[i]
    case = case_inputs(c)
    r = G.depth_loss_grad_ref(case["pred"], case["target"], case["mask"], alpha=c["alpha"], stable_scale=c["stable_scale"],
                              weights=KEYS[key])
    for k in ("grad", "mag_a", "mag_fit", "g_a"):
        r[k].setflags(write=False)
    return case, r


def test_fixture_matches_the_loss_cases():
    assert [int(s) for s in Z["seed"]] == [c["seed"] for c in CASES] and len(CASES) == 14
    assert ALONE == {41, 52} and ABSREL_ALONE == {46} and list(KEYS) == ["total_loss", "spatial_loss", "stable_loss", "absRel_loss"]
    for i, k in RECORDED:
        g = Z[f"grad_{CASES[i]['seed']}_{k}"]
        assert g.dtype == np.float32 and g.size == int(np.prod(CASES[i]["shape"]))


@pytest.mark.parametrize("i,key", RECORDED, ids=lambda v: v if isinstance(v, str) else case_id(CASES[v]))
def test_restatement_reproduces_the_references_gradient(i, key):
    c = CASES[i]
    want = Z[f"grad_{c['seed']}_{key}"].reshape(c["shape"]).astype(np.float64)
    rel_dev, max_dev = (float(v) for v in Z[f"deviation_{c['seed']}_{key}"])
    _, r = oracle(i, key)
    got = r["grad"]
    assert np.isfinite(got).all()
    if np.isnan(rel_dev):                                   # see the module's text
        case, _ = oracle(i, key)
        assert key == "absRel_loss" and ((case["mask"] != 0) & (case["target"] == 0)).any() and np.isnan(want).all()
        return
    assert 0 <= rel_dev <= 1e-4 and 0 <= max_dev <= 1e-4
    diff, scale = got - want, float(np.abs(want).max())
    if scale == 0:
        assert not got.any()
        return
    rel = float(np.sqrt((diff ** 2).sum() / (want ** 2).sum()))
    mx = float(np.abs(diff).max()) / scale
    print(f"rel-L2 {rel:.2e} (bar {4 * rel_dev:.2e}), max-abs / max {mx:.2e} (bar {4 * max_dev:.2e}), max |g| {scale:.3g}")
    assert rel <= 4 * rel_dev and mx <= 4 * max_dev


def test_signs_are_decided_alike_and_medians_are_unique():
    """The conditions the generator asserts, on the restatement, for every recorded gradient: a sign is taken of more than
    1e-9; exactly 0 only at the pixel that holds a frame's median (a - m = 0, and x - y = 0 where it holds the target's median
    too), so at most once a frame for those two and never for a neighbour's, a temporal or an absRel difference; and no two kept
    pixels of a frame share the median's value."""
    import loss_ref as R
    for i, key in RECORDED:
        c = CASES[i]
        case, r = oracle(i, key)
        B, T, H, W = c["shape"]
        for what, (lo, zeros) in r["min_abs"].items():
            assert lo > 1e-9, (c["seed"], key, what, lo)
            assert zeros <= (B * T if what in G.MAY_BE_ZERO else 0), (c["seed"], key, what, zeros)
        a = R.align_ref(case["pred"], r["fwd"]["scale"], r["fwd"]["shift"]).reshape(B * T, H * W)
        keep = (case["mask"] != 0).reshape(B * T, H * W)
        for f, m in enumerate(r["fwd"]["m_pred"].ravel()):
            assert (keep[f] & (a[f] == m)).sum() <= 1, (c["seed"], f)


def test_zero_on_the_empty_item_and_on_every_dropped_pixel():
    for i, c in enumerate(CASES):
        case, r = oracle(i)
        drop = case["mask"] == 0
        assert not r["grad"][drop].any() and not np.signbit(r["grad"][drop]).any(), c["seed"]
    i = next(i for i, c in enumerate(CASES) if c["seed"] == 50)
    case, r = oracle(i)
    assert not (case["mask"][1] != 0).any() and not r["grad"][1].any() and r["grad"][0].any()


def test_two_pixels_fix_the_fit():
    """[1, 2, 1, 1]: each frame's pixel is its own median, so x = y = 0, and the threshold of a one-pixel frame is 0, so no
    temporal pair counts: the gradient is identically 0, as the reference's."""
    i = next(i for i, c in enumerate(CASES) if c["seed"] == 45)
    assert CASES[i]["shape"] == (1, 2, 1, 1)
    _, r = oracle(i)
    assert not r["grad"].any() and not Z["grad_45_total_loss"].any()


def test_backward_entry_point_rejects_bad_arguments():
    """The codes of vdn_depth_loss, returned before anything is launched: no GPU is needed."""
    from vdn import _abi
    L, P = _abi.lib, 4096                                   # P: a non-null, aligned stand-in; nothing is launched
    assert L.vdn_depth_loss_backward_workspace_bytes(0, 3, 4, 5) == 0 and L.vdn_depth_loss_backward_workspace_bytes(2, 3, 0, 5) == 0
    small, large = L.vdn_depth_loss_backward_workspace_bytes(2, 3, 4, 5), L.vdn_depth_loss_backward_workspace_bytes(2, 3, 400, 500)
    assert small > 8 * 2 * 3 * 4 * 5 and small % 8 == 0
    assert large - small == 8 * 2 * 3 * (400 * 500 - 4 * 5)   # the fp64 plane of g_x is all that depends on H and W
    #     pred target mask B T  H  W  alpha scales stable fit stats counts out coeff ws grad stream
    ok = [P, P, P, 2, 3, 4, 5, 0.5, 4, 10.0, P, P, P, P, P, P, P, None]

    def call(**changes):
        args = list(ok)
        for idx, val in changes.items():
            args[int(idx[1:])] = val
        return L.vdn_depth_loss_backward(*args)

    for idx in (0, 1, 2, 10, 11, 12, 13, 14, 15, 16):       # every pointer is required
        assert call(**{f"a{idx}": None}) == -1, idx
    for idx, val in dict(a3=0, a4=0, a5=0, a6=-1, a8=-1).items():
        assert call(**{idx: val}) == -1, (idx, val)
    assert call(a4=1) == -1                                 # T == 1 with the temporal term
    assert call(a8=5) == -2 and call(a5=65536, a6=65536) == -2 and call(a3=300, a4=300) == -2
    for idx in (0, 1, 10, 14, 16):
        assert call(**{f"a{idx}": P + 2}) == -3, idx
    for idx in (11, 12, 13, 15):
        assert call(**{f"a{idx}": P + 4}) == -3, idx
    assert call(a0=None, a8=5, a1=P + 2) == -1 and call(a8=5, a1=P + 2) == -2   # the order of vdn_depth_loss
