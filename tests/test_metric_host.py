"""Host-side checks of the metric-depth criterion and scores (vdn.metric, csrc/metric.hip): the numpy restatement
tests/metric_ref.py against what the reference's own eval_depth and SiLogLoss recorded in tests/golden/metric_cases.npz, the
restated align-corners blend against F.interpolate on the CPU, the wrappers' argument errors, the rejected-argument paths of
the entry points and DepthMetricMeter's counting rule on CPU tensors. Nothing here launches a kernel.

Bars. d1 d2 d3: equal as float32 bits (both sides take the same float32 operations). The six continuous metrics, the loss and
the gradient against the reference's float64 run: 1e-11 relative, gradient elements relative to max |grad|. Both sides are
fp64; a sum of at most 4096 terms costs at most 4096 * 2^-53 = 4.5e-13, the rest is margin for log, the few sums per metric
and the sqrt. NaN must meet NaN. The fixture's f32_gap (the reference's float32 run against its float64 run) is a record, not
a tolerance."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import metric_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_cases.npz")
BAR = 1e-11
U = 2.0 ** -24   # test_gpu_geometry.py's unit: UPSAMPLE BAR = 16 U max|x|


def recorded():
    z = np.load(GOLD)
    for i in range(len(z["seed"])):
        c = R.case_dict(z["seed"][i], z["shape"][i], z["mask"][i], z["special"][i], z["lambd"][i])
        yield i, c, z["checksum"][i], dict(n=z[f"n{i}"], f32=z[f"f32_{i}"], f64=z[f"f64_{i}"], loss=z[f"loss{i}"], grad=z[f"grad{i}"])


RECORDED = list(recorded())
FIXTURE = np.load(GOLD)
MIN_DEPTH, MAX_DEPTH = float(FIXTURE["min_depth"]), float(FIXTURE["max_depth"])


def case_id(v):
    return f"{v[0]}-{v[1]['special']}-{v[1]['mask']}"


def case_inputs(c, checksum):
    case = R.make_case(c)
    assert np.allclose(R.checksum(case), checksum, rtol=1e-12, atol=0), "the seeded generator no longer draws the recorded case"
    return case


def close(got, want, bar, scale=None):
    """NaN meets NaN; elsewhere |got - want| <= bar * (scale or |want|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    ref = np.abs(want[ok]) if scale is None else scale
    err = np.abs(got[ok] - want[ok])
    assert (err <= bar * ref).all(), (err.max(initial=0.0), got, want)


def same_f32_bits(got, want):
    """Equal as float32 bits; a NaN meets a NaN of any payload."""
    got, want = np.asarray(got).astype(np.float32), np.asarray(want).astype(np.float32)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert got[~np.isnan(got)].tobytes() == want[~np.isnan(want)].tobytes(), (got, want)


def test_fixture_is_the_case_list():
    assert [c for _, c, _, _ in RECORDED] == [R.case_dict(*s) for s in R.CASES]
    assert os.path.getsize(GOLD) < 100 * 1000
    assert tuple(FIXTURE["keys"]) == R.KEYS and (MIN_DEPTH, MAX_DEPTH) == (R.MIN_DEPTH, R.MAX_DEPTH)
    assert 0 < float(FIXTURE["f32_gap"]) < 1e-5      # a record of the scripts' float32 arithmetic; nothing is held to it
    specials = {c["special"] for _, c, _, _ in RECORDED}
    assert {"plain", "bounds", "mask_values", "ratio", "nine_ten", "empty_item", "empty_all", "equal", "negative_radicand"} <= specials
    assert {c["mask"] for _, c, _, _ in RECORDED} == {"bool", "uint8", "float"}


@pytest.mark.parametrize("rec", RECORDED, ids=case_id)
def test_restated_metrics_equal_the_reference(rec):
    _, c, checksum, want = rec
    case = case_inputs(c, checksum)
    rows = R.eval_rows(case["pred"], case["depth"], case["mask"], MIN_DEPTH, MAX_DEPTH)
    assert np.array_equal(rows[:, 0], want["n"]) and want["n"].max() <= 4096
    same_f32_bits(rows[:, 1:4], want["f32"][:, :3])
    close(rows[:, 4:], want["f64"][:, 3:], BAR)
    close(rows[:, 1:4], want["f64"][:, :3], 0.0)      # the float64 run's quotients are the same small fractions
    sp = c["special"]
    if sp in ("empty_item", "empty_all"):
        assert want["n"][-1] == 0 and np.isnan(rows[-1, 1:]).all()
    if sp == "nine_ten":
        assert want["n"].tolist() == [9, 10]


@pytest.mark.parametrize("rec", RECORDED, ids=case_id)
def test_restated_loss_and_gradient_equal_the_reference(rec):
    _, c, checksum, want = rec
    case = case_inputs(c, checksum)
    keep = R.keep_mask(case["mask"], case["depth"], MIN_DEPTH, MAX_DEPTH)
    st = R.silog_ref(case["pred"], case["depth"], keep, c["lambd"])
    assert st[1] == want["n"].sum()
    close(st[:1], want["loss"][1:], BAR)
    g = R.silog_grad_ref(case["pred"], case["depth"], keep, c["lambd"])
    assert not g[~keep].any()
    total, total_abs, nans = want["grad"][:3]
    assert int(nans) == int(np.isnan(g).sum())
    sampled = want["grad"][3:]
    finite = sampled[np.isfinite(sampled)]
    gmax = float(np.nanmax(np.abs(g), initial=0.0)) or 1.0
    close(g.reshape(-1)[R.sample_idx(g.size)], sampled, BAR, scale=gmax)
    assert abs(np.nansum(g) - total) <= BAR * gmax * g.size and abs(np.nansum(np.abs(g)) - total_abs) <= BAR * max(total_abs, gmax)
    sp = c["special"]
    if sp == "empty_all":
        assert np.isnan(st[0]) and st[1] == 0 and not g.any()
    if sp == "equal":
        assert st[0] == 0.0 and np.isnan(g[keep]).all() and keep.any()
    if sp == "negative_radicand":
        assert np.isnan(st[0]) and np.isnan(g[keep]).all()
    assert finite.size or sp in ("empty_all", "equal", "negative_radicand", "nine_ten")


def test_keep_rule_at_the_bounds_and_for_other_mask_values():
    lo, hi = np.float32(MIN_DEPTH), np.float32(MAX_DEPTH)
    depth = np.array([lo, np.nextafter(lo, np.float32(0)), hi, np.nextafter(hi, np.float32(np.inf)), 1.0, 1.0, 1.0, np.nan], np.float32)
    mask = np.array([1, 1, 1, 1, 2, 0.5, 0, 1], np.float32)
    assert R.keep_mask(mask, depth, MIN_DEPTH, MAX_DEPTH).tolist() == [True, False, True, False, False, False, False, False]
    t = torch.from_numpy(depth)
    want = (torch.from_numpy(mask) == 1) & (t >= MIN_DEPTH) & (t <= MAX_DEPTH)      # torch's float32-tensor-against-number rule
    assert want.tolist() == R.keep_mask(mask, depth, MIN_DEPTH, MAX_DEPTH).tolist()


@pytest.mark.parametrize("src,dst", [((4, 6), (5, 7)), ((1, 1), (5, 7)), ((37, 53), (64, 257)), ((5, 7), (4, 6)), ((64, 48), (96, 128))],
                         ids=str)
def test_restated_blend_is_within_the_upsample_bar_of_interpolate(src, dst):
    rng = np.random.default_rng(5)
    x = rng.uniform(0.05, 25.0, (2,) + src).astype(np.float32)
    got = R.resample_ac(x, *dst)
    want = torch.nn.functional.interpolate(torch.from_numpy(x)[:, None], dst, mode="bilinear", align_corners=True)[:, 0].numpy()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print(f"{src} -> {dst}: max |restated - interpolate| = {err / (U * np.abs(x).max()):.2f} U max|x|")
    assert got.shape == want.shape and err <= 16 * U * np.abs(x).max()
    if src == (1, 1):
        assert (got == x[:, :1, :1]).all()


def test_argument_errors_come_before_the_device():
    from vdn import metric
    from vdn._abi import VdnError
    p, d, m = torch.ones(2, 4, 6), torch.ones(2, 5, 7), torch.ones(2, 5, 7, dtype=torch.bool)
    with pytest.raises(ValueError):
        metric.eval_depth_batch(p[0], d, m, min_depth=0.001, max_depth=20)          # rank
    with pytest.raises(ValueError):
        metric.eval_depth_batch(p[:1], d, m, min_depth=0.001, max_depth=20)         # batch
    with pytest.raises(ValueError):
        metric.eval_depth_batch(p, d, m[:, :4], min_depth=0.001, max_depth=20)      # mask shape
    with pytest.raises(ValueError):
        metric.eval_depth_batch(p, d, m, min_depth=float("nan"), max_depth=20)
    with pytest.raises(ValueError):
        metric.eval_depth_batch(p, d, m, min_depth=None, max_depth=None)
    with pytest.raises(ValueError):
        metric.eval_depth(torch.ones(5), torch.ones(6))
    with pytest.raises(ValueError):
        metric.eval_depth(torch.ones(0), torch.ones(0))
    crit = metric.SiLogLoss()
    assert crit.lambd == 0.5 and isinstance(crit, torch.nn.Module)
    with pytest.raises(ValueError):
        crit(d, d[:1], m)
    with pytest.raises(ValueError):
        crit(d, d, m[:1])
    with pytest.raises(ValueError):
        crit.forward_from_valid(d, d, m, None, None)
    with pytest.raises(ValueError):
        metric.SiLogLoss(lambd="half")
    with pytest.raises(NotImplementedError):
        crit(d, d.clone().requires_grad_(True), m)
    with pytest.raises(ValueError):
        metric.silog_loss_grad(d, d[:1], m)
    for call in (lambda: metric.eval_depth_batch(p, d, m, min_depth=0.001, max_depth=20, device="cpu"),
                 lambda: metric.eval_depth(d, d, device="cpu"),
                 lambda: metric.SiLogLoss(device="cpu")(d, d, m)):
        with pytest.raises(VdnError):
            call()


def test_entry_points_reject_arguments_without_a_launch():
    from vdn import _abi
    lib = _abi.lib
    assert lib.vdn_metric_trip(1) == 4 * lib.vdn_metric_trip(0) == 4 * 256 * 256
    assert lib.vdn_metric_workspace_bytes(0) == 0 and lib.vdn_metric_workspace_bytes(3) == 3 * lib.vdn_metric_workspace_bytes(1)
    assert lib.vdn_metric_workspace_bytes(1) % 8 == 0 and lib.vdn_silog_loss_workspace_bytes() % 8 == 0
    P = 4096                                                   # never dereferenced: every call below is refused first
    ev = lambda *a: lib.vdn_metric_eval(*a, None)              # noqa: E731
    assert ev(None, P, None, 1, 2, 2, 2, 2, 0, 0.0, 0.0, P, P) == -1
    assert ev(P, P, None, 0, 2, 2, 2, 2, 0, 0.0, 0.0, P, P) == -1
    assert ev(P, P, None, 1, 2, 2, 2, 0, 0, 0.0, 0.0, P, P) == -1
    assert ev(P, P, None, 1, 2, 2, 2, 2, 1, float("nan"), 1.0, P, P) == -1
    assert ev(P, P, None, 1, 2, 2, 65536, 65536, 0, 0.0, 0.0, P, P) == -2
    assert ev(P, P, None, 65536, 2, 2, 2, 2, 0, 0.0, 0.0, P, P) == -2
    assert ev(P + 2, P, None, 1, 2, 2, 2, 2, 0, 0.0, 0.0, P, P) == -3
    assert ev(P, P, None, 1, 2, 2, 2, 2, 0, 0.0, 0.0, P + 4, P) == -3
    assert lib.vdn_silog_loss(P, None, None, 8, 0.5, 0, 0.0, 0.0, P, P, None) == -1
    assert lib.vdn_silog_loss(P, P, None, 0, 0.5, 0, 0.0, 0.0, P, P, None) == -1
    assert lib.vdn_silog_loss(P, P, None, 2 ** 31, 0.5, 0, 0.0, 0.0, P, P, None) == -2
    assert lib.vdn_silog_loss(P, P, None, 8, 0.5, 0, 0.0, 0.0, P, P + 4, None) == -3
    assert lib.vdn_silog_loss_backward(P, P, None, 8, 0.5, 0, 0.0, 0.0, None, P, P, None) == -1
    assert lib.vdn_silog_loss_backward(P, P, None, 8, 0.5, 1, 0.0, float("nan"), P, P, P, None) == -1
    assert lib.vdn_silog_loss_backward(P, P, None, 2 ** 31, 0.5, 0, 0.0, 0.0, P, P, P, None) == -2
    assert lib.vdn_silog_loss_backward(P, P, None, 8, 0.5, 0, 0.0, 0.0, P, P, P + 2, None) == -3


def test_meter_counts_items_with_ten_pixels_or_more():
    from vdn.steps import DepthMetricMeter
    rng = np.random.default_rng(3)
    rows = torch.from_numpy(rng.uniform(0.1, 1.0, (5, 10)))
    rows[:, 0] = torch.tensor([9.0, 10.0, 0.0, 4096.0, 11.0])
    rows[2, 1:] = float("nan")                                   # an empty item's NaN reaches nothing
    meter = DepthMetricMeter()
    assert meter.means() == {}
    meter.add(rows[:3])
    meter.add(rows[3:])
    state = meter.state()
    assert state.dtype == torch.float64 and tuple(state.shape) == (10,) and state[-1].item() == 3
    want = rows[1, 1:] + rows[3, 1:] + rows[4, 1:]
    assert torch.equal(state[:-1], want)
    means = meter.means()
    assert tuple(means) == R.KEYS and list(means.values()) == (want / 3).tolist()
    other = DepthMetricMeter()
    other.load_state(state * 2)                                  # what a reduce over two equal ranks would give
    assert list(other.means().values()) == list(means.values())
    none = DepthMetricMeter()
    none.add(rows[:1])
    assert none.state()[-1].item() == 0 and all(np.isnan(v) for v in none.means().values())
    with pytest.raises(ValueError):
        meter.add(rows[:, :7])
