"""Host-side checks of the trimmed depth criterion (vdn.loss.TrimmedVideoDepthLoss, vdn_depth_loss_trimmed and its backward): the
CPU restatement tests/loss_trim_ref.py against the values and gradients that the reference's VideoDepthLoss(trim=...) recorded
in tests/golden/loss_trim_cases.npz, the restatement at trim = 0, the constructed tie and last-pass cases, the class's
constructor and argument errors, and the rejected-argument paths of both entry points. Nothing here launches a kernel.

Bars. The reference computes in float32 and the restatement fits and sums in float64. tools/make_golden_loss_trim.py measured
the largest deviation per key over the recorded cases (1.1e-6 at most, for total_loss = spatial + 10 * stable) and, over the
recorded gradients, the largest rel-L2 deviation and the largest absolute deviation over the reference's largest component
(1e-6 each); the bars are four times those, to cover float32 summation order across torch builds. The generator refuses a
value bar or a gradient deviation above 1e-4, which would mean a wrong restatement rather than rounding. Gradients are
recorded only for cases with a single residual on each threshold, where the reference's kept set is unambiguous."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

import loss_grad_ref as G
import loss_ref as R
import loss_trim_ref as TR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_trim_cases.npz")
KEYS = ("spatial_loss", "stable_loss", "absRel_loss", "d1", "total_loss")
Z = np.load(GOLD)


def golden_cases():
    for i in range(len(Z["seed"])):
        yield dict(index=i, seed=int(Z["seed"][i]), shape=tuple(int(s) for s in Z["shape"][i]), keep_rate=float(Z["keep_rate"][i]),
                   kind=str(Z["kind"][i]), mask_dtype=str(Z["mask_dtype"][i]),
                   empty_frames=tuple(int(e) for e in Z["empty_frames"][i] if e >= 0),
                   empty_items=tuple(int(e) for e in Z["empty_items"][i] if e >= 0), alpha=float(Z["alpha"][i]),
                   stable_scale=float(Z["stable_scale"][i]), trim=float(Z["trim"][i]), checksum=Z["checksum"][i],
                   d1_hits=int(Z["d1_hits"][i]), expected={k: float(Z[f"expected_{k}"][i]) for k in KEYS},
                   has_grad=f"grad_{i}" in Z.files)


CASES = list(golden_cases())


def case_id(c):
    return f"seed{c['seed']}-{'x'.join(map(str, c['shape']))}-trim{c['trim']}"


def bars() -> dict:
    return {k: 4.0 * float(Z[f"deviation_{k}"]) for k in KEYS}


def case_inputs(c):
    case = R.make_case(c["seed"], c["shape"], c["keep_rate"], c["kind"], c["mask_dtype"], c["empty_frames"], c["empty_items"])
    assert np.allclose(R.checksum(case), c["checksum"], rtol=1e-12, atol=0), "the seeded generator no longer draws the recorded case"
    return case


@functools.lru_cache(maxsize=None)
def oracle(i, weights=(1.0, 0.0, 0.0, 0.0)):
    """Recorded case i: inputs and the restatement (values under 'fwd', gradient for `weights`), computed once, shared and never
    written."""
    c = CASES[i]
    case = case_inputs(c)
    r = TR.depth_loss_trim_grad_ref(case["pred"], case["target"], case["mask"], alpha=c["alpha"], stable_scale=c["stable_scale"],
                                    weights=weights, trim=c["trim"])
    for a in list(case.values()) + [r["grad"], r["mag_a"], r["mag_fit"]]:
        a.setflags(write=False)
    return case, r


def test_bars_are_rounding_sized_and_the_fixture_covers_the_issue():
    for k, b in bars().items():
        print(f"{k}: bar {b:.2e}")
        assert 0 < b <= 1e-4
    assert all(0 < float(v) <= 1e-4 for v in Z["grad_deviation"])
    for shape in ((2, 3, 17, 13), (1, 4, 16, 16), (1, 2, 2, 3)):
        assert {c["trim"] for c in CASES if c["shape"] == shape} >= {0.05, 0.2, 0.5}
    assert any(c["trim"] == 0.999 and c["shape"] == (1, 2, 9, 11) for c in CASES)
    assert any(c["empty_frames"] for c in CASES) and any(c["empty_items"] for c in CASES)
    assert any(c["alpha"] == 0 for c in CASES) and any(c["stable_scale"] == 0 for c in CASES)
    assert sum(c["has_grad"] for c in CASES) >= 12 and not all(c["has_grad"] for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_restatement_reproduces_the_references_values(c):
    _, r = oracle(c["index"])
    got, bar = r["fwd"], bars()
    for k in KEYS:
        want = c["expected"][k]
        if np.isnan(want):                                   # the reference's dictionary has no such key
            assert k == "stable_loss" and c["stable_scale"] == 0 and k not in got
            continue
        print(f"{k}: {got[k]!r} vs {want!r} diff {got[k] - want:+.2e} (bar {bar[k]:.2e})")
        assert abs(got[k] - want) <= bar[k]
    assert got["d1_hits"] == c["d1_hits"]
    if c["trim"] == 0.999:                                   # k == 0: the trimmed terms are exactly 0, the regulariser is not
        assert not got["trim_k"].any() and got["data"] == 0 and got["stable_loss"] == 0 and got["absRel_loss"] == 0
        assert got["spatial_loss"] == c["alpha"] * float(got["g"].sum()) > 0
    case = case_inputs(c)
    assert TR.data_selection_is_stable(case["pred"], case["target"], case["mask"], alpha=c["alpha"], stable_scale=c["stable_scale"],
                                       trim=c["trim"])


@pytest.mark.parametrize("c", [c for c in CASES if c["has_grad"]], ids=case_id)
def test_restatement_reproduces_the_references_gradient(c):
    want = Z[f"grad_{c['index']}"].reshape(c["shape"]).astype(np.float64)
    rel_bar, max_bar = (4.0 * float(v) for v in Z["grad_deviation"])
    _, r = oracle(c["index"])
    assert all(t == 1 or k == 0 for t, k in zip(r["fwd"]["trim_tied"], r["fwd"]["trim_k"]))   # the reference's kept set is unambiguous
    got = r["grad"]
    assert np.isfinite(got).all() and np.abs(want).max() > 0
    diff = got - want
    rel = float(np.sqrt((diff ** 2).sum() / (want ** 2).sum()))
    mx = float(np.abs(diff).max() / np.abs(want).max())
    print(f"rel-L2 {rel:.2e} (bar {rel_bar:.2e}), max-abs / max {mx:.2e} (bar {max_bar:.2e})")
    assert rel <= rel_bar and mx <= max_bar
    drop = case_inputs(c)["mask"] == 0
    assert not got[drop].any()


def test_trim_zero_is_the_untrimmed_restatement():
    """At trim = 0 every counted residual is kept with the weight 1: k = n and the values are depth_loss_ref's (the kept
    residuals are summed in two groups, below and at the threshold, hence the few ulps), the gradient is loss_grad_ref's."""
    for seed, shape in ((41, (2, 3, 17, 13)), (49, (1, 4, 17, 13))):
        case = R.make_case(seed, shape, 0.8, empty_frames=(2,) if seed == 49 else ())
        base = R.depth_loss_ref(case["pred"], case["target"], case["mask"])
        got = TR.depth_loss_trim_grad_ref(case["pred"], case["target"], case["mask"], trim=0.0)
        f = got["fwd"]
        assert f["trim_k"].tolist() == [int(base["count"].sum()), base["stable_count"], base["absrel_count"]]
        assert (f["trim_weight"] == 1).all() and (f["trim_less"] + f["trim_tied"] == f["trim_k"]).all()
        for k in KEYS + ("data",):
            assert abs(f[k] - base[k]) <= 8 * np.finfo(np.float64).eps * abs(base[k]), k
        assert np.array_equal(got["grad"], G.depth_loss_grad_ref(case["pred"], case["target"], case["mask"])["grad"])


def test_selection_semantics():
    r = np.array([0.5, np.nan, 0.25, np.inf, 0.25, 3.0, 0.25, 7.0])
    counted = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
    s = TR.select_ref(r, counted, 1.0 - 0.6)                 # n = 7, k = int(7 * 0.4) = 2: two of the three 0.25s
    assert (s["k"], s["n_less"], s["n_tied"], s["thr"], s["w"]) == (2, 0, 3, 0.25, 2 / 3)
    assert s["term"] == (2 / 3 * 0.75) / 7 and s["u"].tolist() == [0, 0, 2 / 3, 0, 2 / 3, 0, 2 / 3, 0]
    s = TR.select_ref(r, counted, 1.0)                       # k = n: NaN sorts after +inf and is the threshold
    assert (s["k"], s["n_less"], s["n_tied"], s["w"]) == (7, 6, 1, 1.0) and np.isnan(s["thr"]) and np.isnan(s["term"])
    s = TR.select_ref(r, counted, 6.5 / 7)                   # k = 6: +inf is the threshold, the NaN is trimmed
    assert (s["k"], s["n_less"], s["n_tied"], s["thr"]) == (6, 5, 1, np.inf) and s["u"][1] == 0
    assert TR.select_ref(r, counted, 0.1)["k"] == 0 and TR.select_ref(r, np.zeros(8, bool), 0.8)["term"] == 0.0
    assert int(10 * (1.0 - 0.7)) == 3 and int(10 * (1.0 - 0.9)) == 0   # Python's rounding of 1.0 - trim is part of the contract


def test_tie_case_has_weights_strictly_inside_zero_and_one():
    """The constructed case of the device tests against what the reference gave for it: many residuals on each threshold."""
    c = TR.make_tie_case()
    assert c["pred"].shape == (1, 2, 8, 8) and not (c["pred"] * 8 % 1).any() and not (c["target"] * 8 % 1).any()
    r = TR.depth_loss_trim_grad_ref(c["pred"], c["target"], c["mask"], trim=0.2)
    f = r["fwd"]
    assert f["scale"].tolist() == [1.0] and f["shift"].tolist() == [0.0] and not f["m_pred"].any() and not f["m_target"].any()
    assert (f["s_pred"] == 2).all() and (f["s_target"] == 2).all()
    assert (f["trim_tied"] > 1).all() and ((0 < f["trim_weight"]) & (f["trim_weight"] < 1)).all()
    assert f["trim_k"].tolist() == [51, 25, 51] and f["trim_threshold"].tolist() == [0.5, 1.0, 0.5]
    for k, want in zip(KEYS, Z["tie_expected"]):
        assert abs(f[k] - float(want)) <= 1e-6, k            # float32 rounding of the reference's values
    full = R.depth_loss_ref(c["pred"], c["target"], c["mask"])
    assert f["absRel_loss"] / full["absRel_loss"] == 11 / 24 and abs(float(Z["tie_absrel_ratio"]) - 11 / 24) <= 1e-6
    for term in TR.TERMS:                                    # the weights over the tied set sum to k - n_less
        s = f["sel"][term]
        tied = (s["u"] > 0) & (s["u"] < 1)
        assert tied.sum() == s["n_tied"] and abs(s["u"][tied].sum() - (s["k"] - s["n_less"])) < 1e-12
    assert TR.data_selection_is_stable(c["pred"], c["target"], c["mask"])


def test_last_pass_case_shares_the_top_22_bits():
    c = TR.make_last_pass_case()
    f = TR.depth_loss_trim_ref(c["pred"], c["target"], c["mask"], trim=0.2)
    assert f["scale"].tolist() == [1.0] and np.array_equal(R.align_ref(c["pred"], f["scale"], f["shift"]), c["pred"])
    r, counted = TR.residuals_ref(c["pred"], c["target"], c["mask"], f, 10)["absRel"]
    keys = TR.keys_of(r[counted])
    assert counted.sum() == 128 and len(np.unique(keys)) == 128 and len(np.unique(keys >> 10)) == 1
    assert np.array_equal(np.sort(r[counted]), 1 + 2 * np.arange(128) * 2.0 ** -23)
    assert f["trim_k"][2] == 102 and f["trim_threshold"][2] == 1 + 202 * 2.0 ** -23 and f["trim_tied"][2] == 1
    assert TR.data_selection_is_stable(c["pred"], c["target"], c["mask"])


def test_constructor_keys_and_argument_errors():
    """Every ValueError comes before the device is touched; VideoDepthLoss keeps refusing trim."""
    import inspect
    from vdn import _abi, loss as L
    sig = inspect.signature(L.TrimmedVideoDepthLoss.__init__)
    assert [(n, q.default, q.kind) for n, q in list(sig.parameters.items())[1:]] == [
        ("alpha", 0.5, inspect.Parameter.POSITIONAL_OR_KEYWORD), ("scales", 4, inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("trim", 0.2, inspect.Parameter.POSITIONAL_OR_KEYWORD), ("stable_scale", 10, inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("device", "cuda", inspect.Parameter.KEYWORD_ONLY)]
    crit = L.TrimmedVideoDepthLoss(0.3, 4, 0.25, 7)
    assert isinstance(crit, torch.nn.Module) and (crit.trim, crit.stable_scale, crit.initial_alpha, crit.scales) == (0.25, 7, 0.3, 4)
    assert crit.keys == ("spatial_loss", "stable_loss", "absRel_loss", "d1", "total_loss")
    assert L.TrimmedVideoDepthLoss(stable_scale=0).keys == ("spatial_loss", "absRel_loss", "d1", "total_loss")
    assert L.TrimmedVideoDepthLoss(trim=0).trim == 0
    for bad in (-0.1, 1.0, 1.5, float("nan"), "0.2", None):
        with pytest.raises(ValueError, match="trim"):
            L.TrimmedVideoDepthLoss(trim=bad)
    with pytest.raises(NotImplementedError, match="scales"):
        L.TrimmedVideoDepthLoss(scales=5)
    with pytest.raises(NotImplementedError, match="trim"):
        L.VideoDepthLoss(trim=0.2)
    p, m = torch.ones(1, 2, 4, 5), torch.ones(1, 2, 4, 5, dtype=torch.bool)
    with pytest.raises(ValueError, match="prediction"):
        crit(p[0], p[0], m[0])
    with pytest.raises(ValueError, match="mask"):
        crit(p, p, m[..., :3])
    with pytest.raises(ValueError, match="T >= 2"):
        crit(p[:, :1], p[:, :1], m[:, :1])
    with pytest.raises(NotImplementedError, match="target"):
        crit(p.clone().requires_grad_(), p.clone().requires_grad_(), m)
    for fn in (L.depth_loss, L.depth_loss_grad):
        assert inspect.signature(fn).parameters["trim"].kind is inspect.Parameter.KEYWORD_ONLY
        assert inspect.signature(fn).parameters["trim"].default == 0.0
        for bad in (-0.1, 1.0):
            with pytest.raises(ValueError, match="trim"):
                fn(p, p, m, trim=bad)
        with pytest.raises(ValueError, match="T >= 2"):
            fn(p[:, :1], p[:, :1], m[:, :1], trim=0.2)
    with pytest.raises(_abi.VdnError):
        L.TrimmedVideoDepthLoss(device="cpu")(p, p, m)


def test_trimmed_entry_point_rejects_bad_arguments():
    """The codes of vdn_depth_loss and the two new ones, returned before anything is launched: no GPU is needed."""
    from vdn import _abi
    L, P = _abi.lib, 4096                                   # P: a non-null, aligned stand-in; nothing is launched
    size = L.vdn_depth_loss_trimmed_workspace_bytes
    assert size(0, 3) == 0 and size(2, 0) == 0
    assert size(2, 3) % 8 == 0 and size(2, 3) > L.vdn_depth_loss_workspace_bytes(2, 3) + 3 * 2048 * 4   # and the three histograms
    #     pred target mask B T  H  W  alpha scales stable keep ws scale_shift stats counts out stream
    ok = [P, P, P, 2, 3, 4, 5, 0.5, 4, 10.0, 0.8, P, None, None, None, P, None]

    def call(**changes):
        args = list(ok)
        for idx, val in changes.items():
            args[int(idx[1:])] = val
        return L.vdn_depth_loss_trimmed(*args)

    for idx, val in dict(a0=None, a1=None, a2=None, a3=0, a4=0, a5=0, a6=-1, a8=-1, a11=None, a15=None).items():
        assert call(**{idx: val}) == -1, (idx, val)
    assert call(a15=None, a12=P) == -1                      # out is required: there is no fit-only form
    assert call(a4=1) == -1                                 # T == 1 with the temporal term
    for keep in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert call(a10=keep) == -1, keep
    assert call(a8=5) == -2 and call(a5=65536, a6=65536) == -2 and call(a3=300, a4=300) == -2
    assert call(a3=64, a4=64, a5=1024, a6=1024) == -2       # 2^32 elements: one more than the select's counters hold
    assert call(a0=P + 2) == -3 and call(a15=P + 4) == -3 and call(a11=P + 4) == -3 and call(a12=P + 1) == -3
    assert call(a10=0.0, a8=5) == -1 and call(a8=5, a0=P + 2) == -2


def test_trimmed_backward_entry_point_rejects_bad_arguments():
    from vdn import _abi
    L, P = _abi.lib, 4096
    size = L.vdn_depth_loss_trimmed_backward_workspace_bytes
    assert size(0, 3, 4, 5) == 0 and size(2, 3, 0, 5) == 0
    assert size(2, 3, 4, 5) == L.vdn_depth_loss_backward_workspace_bytes(2, 3, 4, 5) and size(2, 3, 4, 5) % 8 == 0
    #     pred target mask B T  H  W  alpha scales stable fit stats counts out coeff ws grad stream
    ok = [P, P, P, 2, 3, 4, 5, 0.5, 4, 10.0, P, P, P, P, P, P, P, None]

    def call(**changes):
        args = list(ok)
        for idx, val in changes.items():
            args[int(idx[1:])] = val
        return L.vdn_depth_loss_trimmed_backward(*args)

    for idx in (0, 1, 2, 10, 11, 12, 13, 14, 15, 16):       # every pointer is required
        assert call(**{f"a{idx}": None}) == -1, idx
    for idx, val in dict(a3=0, a4=0, a5=0, a6=-1, a8=-1).items():
        assert call(**{idx: val}) == -1, (idx, val)
    assert call(a4=1) == -1
    assert call(a8=5) == -2 and call(a5=65536, a6=65536) == -2 and call(a3=300, a4=300) == -2
    assert call(a3=64, a4=64, a5=1024, a6=1024) == -2       # no forward can have written out[20..34] for it
    for idx in (0, 1, 10, 14, 16):
        assert call(**{f"a{idx}": P + 2}) == -3, idx
    for idx in (11, 12, 13, 15):
        assert call(**{f"a{idx}": P + 4}) == -3, idx
    assert call(a0=None, a8=5, a1=P + 2) == -1 and call(a8=5, a1=P + 2) == -2
