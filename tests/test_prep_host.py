"""Host-side checks of the batch preparation (vdn.prep, csrc/prep.hip): the numpy restatement tests/prep_ref.py against the
arrays the reference's own functions recorded in tests/golden/prep_cases.npz, the fixture's coverage, the wrappers' signatures
and argument errors and the rejected-argument paths of the entry points. Nothing here launches a kernel.

Bar: np.array_equal(restatement, recorded, equal_nan=True). The restatement is one float32 IEEE operation per reference
operation, so there is no tolerance; the comparison is numeric and does not tell +0.0 from -0.0."""
from __future__ import annotations

import inspect
import os

import numpy as np
import pytest
import torch

import prep_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prep_cases.npz")


def recorded():
    z = np.load(GOLD)
    for i in range(len(z["seed"])):
        yield i, dict(op=str(z["op"][i]), seed=int(z["seed"][i]), shape=tuple(int(s) for s in z["shape"][i]),
                      mask=str(z["mask"][i]), special=str(z["special"][i]), norm=bool(z["norm"][i])), z["checksum"][i], z[f"exp{i}"]


RECORDED = list(recorded())


def case_id(v):
    i, c = v[0], v[1]
    return f"{i}-{c['op']}-{c['special']}-{c['mask']}"


def case_inputs(c, checksum):
    case = R.make_case(c)
    assert np.allclose(R.checksum(case), checksum, rtol=1e-12, atol=0), "the seeded generator no longer draws the recorded case"
    return case


def test_fixture_is_the_case_list():
    assert [c for _, c, _, _ in RECORDED] == [dict(c, shape=tuple(c["shape"])) for c in R.CASES]
    assert os.path.getsize(GOLD) < 200 * 1000


@pytest.mark.parametrize("rec", RECORDED, ids=case_id)
def test_restatement_equals_the_reference(rec):
    _, c, checksum, want = rec
    got = R.restate(c, case_inputs(c, checksum))
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)


def test_fixture_covers_every_case():
    cs = [c for _, c, _, _ in RECORDED]

    def has(**kw):
        return any(all(c[k] == v for k, v in kw.items()) for c in cs)

    assert has(op="pre", special="plain", mask="bool") and has(op="pre", special="plain", mask="uint8")
    assert has(special="empty_item") and has(special="constant_item") and has(mask="none", norm=True)
    assert has(op="pre", norm=False) and has(op="pre", special="negative", norm=True)
    assert has(op="inv", special="gt_small") and has(op="invpre", special="gt_small")
    assert has(op="rgb", special="outside") and has(op="viz", special="outside")
    assert has(special="nan_kept") and has(special="dropped_nan")
    shapes = {c["shape"] for c in cs}
    assert {(2, 3, 1, 13, 13), (1, 2, 1, 16, 16), (2, 2, 1, 1, 1), (2, 2, 3, 5, 5), (1, 2, 3, 4, 4)} <= shapes
    for _, c, checksum, want in RECORDED:      # each special does what its name says
        case = case_inputs(c, checksum)
        x, m = case["x"], case["mask"]
        B = x.shape[0]
        if c["special"] == "empty_item":
            assert not m[B - 1].any() and m[0].any() and not want[B - 1].any() and want[0].any()
        if c["special"] == "constant_item":
            assert np.unique(x[0]).size == 1 and not want[0].any()
        if c["special"] == "negative":
            assert (x < 0).mean() > 0.05
        if c["special"] == "gt_small":
            assert x.reshape(-1)[:3].tolist() == [0.0, float(np.float32(1e-9)), float(np.float32(5e-8))]
            if c["op"] == "inv":
                assert want.reshape(-1)[:3].tolist() == [1e8, 1e8, float(np.float32(1) / np.float32(5e-8))]
        if c["special"] == "outside":
            assert (x < 0).any() and (x > 1).any()
            if c["op"] == "viz":
                assert want.min() == 0.0 and want.max() == 1.0
        if c["special"] == "nan_kept":
            assert B == 2 and np.isnan(x[0]).sum() == 1 and m[0][np.isnan(x[0])].all()
            assert np.isnan(want[0]).all() and not np.isnan(want[1]).any()
        if c["special"] == "dropped_nan":
            bad = ~np.isfinite(x)
            assert bad.sum() == 3 * B and not m[bad].any()
            assert np.isnan(want).sum() == B and want[np.isfinite(x).squeeze(2)].max() == 1.0


def test_restatement_corner_semantics():
    nan = np.float32(np.nan)
    x = np.array([[1.0, nan, 3.0], [2.0, 2.0, 2.0]], np.float32)
    out, mm = R.prep_depth_ref(x, np.array([[1, 0, 1], [0, 0, 0]], np.uint8), False, False, True)
    assert mm[0].tolist() == [1.0, 3.0] and np.isnan(out[0, 1]) and out[0, 0] == 0.0 and out[0, 2] == 1.0
    assert mm[1].tolist() == [np.inf, -np.inf] and not out[1].any() and not np.signbit(out[1]).any()
    out, mm = R.prep_depth_ref(x, None, False, False, True)
    assert np.isnan(mm[0]).all() and np.isnan(out[0]).all() and not out[1].any()       # hi == lo: the clamp at 1e-8, 0 / 1e-8
    assert np.isnan(R.prep_rgb_ref(np.full((3, 1, 1), nan), True)).all()                 # the clamp keeps a NaN
    assert np.isnan(R.prep_depth_ref(x, None, True, True, False)[0][0, 1])


def test_signatures_match_the_scripts():
    from vdn import prep

    def positional(fn):
        ps = inspect.signature(fn).parameters.values()
        return [(p.name, p.default) for p in ps if p.kind == p.POSITIONAL_OR_KEYWORD]

    E = inspect.Parameter.empty
    assert positional(prep.preprocess_rgb_sequences) == [("rgb_batch", E)]
    assert positional(prep.preprocess_rgb_viz_sequences) == [("rgb_batch", E)]
    assert positional(prep.preprocess_depth_sequences) == [("depth_batch", E), ("masks", E), ("norm", True)]
    assert positional(prep.batch_wise_min_max_norm) == [("x", E), ("masks", E)]
    assert positional(prep.inverse_depth) == [("gt_depths", E), ("min", 1e-8)]
    assert positional(prep.preprocess_inverse_depth_sequences) == [("gt_depths", E), ("masks", E), ("norm", True)]


def test_wrapper_argument_errors():
    """Every ValueError comes before the device is touched (this machine has none); a CPU device is a VdnError."""
    from vdn import _abi, prep, steps
    rgb, d, m = torch.ones(1, 2, 3, 4, 5), torch.ones(1, 2, 1, 4, 5), torch.ones(1, 2, 1, 4, 5, dtype=torch.bool)
    for fn in (prep.preprocess_rgb_sequences, prep.preprocess_rgb_viz_sequences):
        with pytest.raises(ValueError, match="rgb_batch"):
            fn(rgb[0])
        with pytest.raises(ValueError, match="rgb_batch"):
            fn(d)
        with pytest.raises(ValueError, match="empty"):
            fn(rgb[:0])
        with pytest.raises(_abi.VdnError):
            fn(rgb, device="cpu")
    for fn in (prep.preprocess_depth_sequences, prep.preprocess_inverse_depth_sequences):
        with pytest.raises(ValueError, match="must be"):
            fn(d[:, :, 0], m)
        with pytest.raises(ValueError, match="must be"):
            fn(rgb, m)
        with pytest.raises(ValueError, match="masks"):
            fn(d, m[:, :, 0])
        with pytest.raises(ValueError, match="masks"):
            fn(d, m[:, :1])
        with pytest.raises(_abi.VdnError):
            fn(d, m, device="cpu")
        with pytest.raises(_abi.VdnError):
            fn(d, None, device="cpu")
    with pytest.raises(ValueError, match="x must be"):
        prep.batch_wise_min_max_norm(d, m)
    with pytest.raises(ValueError, match="masks"):
        prep.batch_wise_min_max_norm(d[:, :, 0], m)
    with pytest.raises(ValueError, match="min must be"):
        prep.inverse_depth(d, 1e-6)
    with pytest.raises(ValueError, match="non-empty"):
        prep.inverse_depth(d[:0])
    with pytest.raises(_abi.VdnError):
        prep.inverse_depth(d, device="cpu")
    batch = {"rgb": rgb, "depth": d, "mask": m, "depth_anything_v2": d}
    with pytest.raises(ValueError, match="mask"):
        steps.prepare_batch(dict(batch, mask=m[:, :, 0]))
    with pytest.raises(ValueError, match="depth"):
        steps.prepare_batch(dict(batch, depth=d[:, :1]))
    with pytest.raises(ValueError, match="with_rgb"):
        steps.validate_step(lambda x: x, batch, object(), object(), with_rgb=False)
    with pytest.raises(ValueError, match=r"\[B, S, H, W\]"):
        from vdn.eval import eval_batch_by_data
        eval_batch_by_data(d, d)
    with pytest.raises(ValueError, match="rows"):
        steps.MetricMeter().add(torch.zeros(7))
    assert steps.LossMeter().averages() == {} and steps.MetricMeter().means() == []


def test_prep_entry_points_reject_bad_arguments():
    from vdn import _abi
    L, P = _abi.lib, 4096                                   # P: a non-null, aligned stand-in; nothing is launched
    assert L.vdn_prep_trip(1) == 4 * L.vdn_prep_trip(0) > 0
    from vdn import prep
    assert prep.trip_elements(True) == L.vdn_prep_trip(1) and prep.trip_elements(False) == L.vdn_prep_trip(0)
    ws = L.vdn_prep_depth_workspace_bytes
    assert ws(0) == 0 and ws(-1) == 0 and ws(1) > 0 and all(ws(b) % 8 == 0 for b in (1, 2, 3, 7))
    assert ws(32) == 32 * ws(1) and ws(65535) == 65535 * ws(1)                 # it depends on B alone
    rgb_ok = [P, P, 2, 3, 4, 1, None]
    dep_ok = [P, P, P, 2, 12, 1, 1, 1, P, P, None]

    def status(fn, ok, **changes):
        args = list(ok)
        for idx, val in changes.items():
            args[int(idx[1:])] = val
        return fn(*args)

    for k, v in (("a0", None), ("a1", None), ("a2", 0), ("a2", -1), ("a3", 0), ("a4", 0), ("a4", -5)):
        assert status(L.vdn_prep_rgb, rgb_ok, **{k: v}) == -1, (k, v)
    for k, v in (("a0", None), ("a2", None), ("a3", 0), ("a3", -2), ("a4", 0), ("a4", -1), ("a8", None)):
        assert status(L.vdn_prep_depth, dep_ok, **{k: v}) == -1, (k, v)
    assert status(L.vdn_prep_rgb, rgb_ok, a3=32768, a4=32768) == -2           # 3 * H * W past INT32_MAX
    assert status(L.vdn_prep_rgb, rgb_ok, a2=65536) == -2
    assert status(L.vdn_prep_depth, dep_ok, a4=2 ** 31) == -2                 # n past INT32_MAX
    assert status(L.vdn_prep_depth, dep_ok, a3=65536) == -2
    for k in ("a0", "a1"):
        assert status(L.vdn_prep_rgb, rgb_ok, **{k: P + 2}) == -3             # a float pointer off 4 bytes
    for k in ("a0", "a2", "a9"):
        assert status(L.vdn_prep_depth, dep_ok, **{k: P + 2}) == -3
    assert status(L.vdn_prep_depth, dep_ok, a8=P + 4) == -3                   # a workspace off 8
