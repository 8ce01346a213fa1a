"""Host-side checks of the depth criterion (vdn.loss, csrc/loss.hip): the CPU restatement tests/loss_ref.py against the values
the reference's VideoDepthLoss recorded in tests/golden/loss_cases.npz, the fixture's coverage, the module's constructor,
keys and argument errors, and the rejected-argument paths of the entry point. Nothing here launches a kernel.

Bars. The reference computes in float32 and the restatement fits and sums in float64. tools/make_golden_loss.py measured
the largest deviation per key over the recorded cases and stored it in the fixture (profiles/depth_loss.md lists them:
3e-6 at most, for total_loss = spatial + 10 * stable and for absRel_loss, where |a - t| / t reaches 100 at a target of
1.5e-3); the bar is four times that per key, to cover float32 summation order across torch builds. The generator refuses
a bar above 1e-4, which would mean a wrong restatement rather than rounding."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

import loss_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_cases.npz")
KEYS = ("spatial_loss", "stable_loss", "absRel_loss", "d1", "total_loss")


def golden_cases():
    z = np.load(GOLD)
    for i in range(len(z["seed"])):
        yield dict(seed=int(z["seed"][i]), shape=tuple(int(s) for s in z["shape"][i]), keep_rate=float(z["keep_rate"][i]),
                   kind=str(z["kind"][i]), mask_dtype=str(z["mask_dtype"][i]),
                   empty_frames=tuple(int(e) for e in z["empty_frames"][i] if e >= 0),
                   empty_items=tuple(int(e) for e in z["empty_items"][i] if e >= 0), frame_noise=float(z["frame_noise"][i]),
                   alpha=float(z["alpha"][i]), stable_scale=float(z["stable_scale"][i]), checksum=z["checksum"][i],
                   d1_hits=int(z["d1_hits"][i]), expected={k: float(z[f"expected_{k}"][i]) for k in KEYS})


def bars() -> dict:
    z = np.load(GOLD)
    return {k: 4.0 * float(z[f"deviation_{k}"]) for k in KEYS}


def case_inputs(c):
    case = R.make_case(c["seed"], c["shape"], c["keep_rate"], c["kind"], c["mask_dtype"], c["empty_frames"], c["empty_items"],
                       c["frame_noise"])
    assert np.allclose(R.checksum(case), c["checksum"], rtol=1e-12, atol=0), "the seeded generator no longer draws the recorded case"
    return case


def case_id(c):
    return f"seed{c['seed']}-{'x'.join(map(str, c['shape']))}-{c['kind']}"


CASES = list(golden_cases())

# Constructed cases beside the recorded ones, for tests/test_gpu_loss.py: R.make_case(seed, shape, 0.8), alpha = 0.5,
# stable_scale = 10, four scales; the reference is not consulted for them.
#   quads-cross-rows            H * W is a multiple of 4 and W is not: every second quad of a lane spans a row's end, where the
#                               finest grid's right-hand neighbour must not come from the lane's own quad;
#   two-trips-quads-cross-rows  33 488 pixels a frame with W % 4 == 2: the same past one trip of the four-pixel sweep;
#   two-trips-single            33 123 pixels, odd: the one-pixel sweep, which runs five trips;
#   two-items-two-trips         two fits, and each item's temporal pairs reach into the second trip.
EXTRA = {"quads-cross-rows": (357, (1, 2, 6, 6)), "two-trips-quads-cross-rows": (85, (1, 2, 184, 182)),
         "two-trips-single": (83, (1, 2, 181, 183)), "two-items-two-trips": (86, (2, 2, 184, 182))}
EXTRA_ARGS = dict(alpha=0.5, stable_scale=10)


@functools.lru_cache(maxsize=None)
def extra(name):
    """Inputs and restatement of a constructed case, computed once, shared and never written."""
    seed, shape = EXTRA[name]
    case = R.make_case(seed, shape, 0.8)
    for a in case.values():
        a.setflags(write=False)
    return case, R.depth_loss_ref(case["pred"], case["target"], case["mask"], **EXTRA_ARGS)


@pytest.mark.parametrize("name", list(EXTRA))
def test_constructed_cases_have_pixels_on_both_sides(name):
    """What the device test needs of the seeds, checked where no device is: every grid keeps points, the temporal term counts
    pairs and drops some, d1 has hits and misses, and the shapes are on the sweep they are named for."""
    from vdn import loss as L
    case, r = extra(name)
    B, T, H, W = case["pred"].shape
    kept, both = int(r["count"].sum()), int(((case["mask"][:, 1:] != 0) & (case["mask"][:, :-1] != 0)).sum())
    print(f"[{name}] M {r['M'].tolist()} kept {kept} temporal pairs {r['stable_count']} of {both} d1 hits {r['d1_hits']} absRel {r['absrel_count']}")
    assert (r["M"] > 0).all() and r["M"][0] == kept and 0 < r["stable_count"] < both and 0 < r["d1_hits"] < kept
    assert r["d1_hits"] < r["absrel_count"] <= kept
    wide = H * W % 4 == 0
    assert wide == (name != "two-trips-single") and W % 4 != 0
    assert (H * W > L.trip_pixels(wide)) == (name != "quads-cross-rows")
    if name == "quads-cross-rows":
        assert r["M"].tolist() == [63, 17, 7, 2]
    if B > 1:
        assert r["scale"][0] != r["scale"][1]


def test_trip_query_is_the_sweeps_stride():
    from vdn import _abi, loss as L
    assert _abi.lib.vdn_depth_loss_trip(1) == 4 * _abi.lib.vdn_depth_loss_trip(0) == L.trip_pixels(True) > 0
    assert L.trip_pixels(False) % 256 == 0


def test_bars_are_rounding_sized():
    for k, b in bars().items():
        print(f"{k}: bar {b:.2e}")
        assert 0 < b <= 1e-4


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_loss_ref_reproduces_the_reference(c):
    case = case_inputs(c)
    got = R.depth_loss_ref(case["pred"], case["target"], case["mask"], alpha=c["alpha"], stable_scale=c["stable_scale"])
    bar = bars()
    for k in KEYS:
        want = c["expected"][k]
        if np.isnan(want):                                   # the reference's dictionary has no such key
            assert k == "stable_loss" and c["stable_scale"] == 0 and k not in got
            continue
        print(f"{k}: {got[k]!r} vs {want!r} diff {got[k] - want:+.2e} (bar {bar[k]:.2e})")
        assert abs(got[k] - want) <= bar[k]
    assert got["d1_hits"] == c["d1_hits"]                   # the two sides decide the same pixels


def test_fixture_covers_every_branch():
    shapes = {c["shape"] for c in CASES}
    assert {(2, 3, 17, 13), (1, 2, 9, 11), (1, 4, 16, 16), (1, 2, 2, 3), (1, 2, 1, 1), (1, 3, 64, 48)} <= shapes
    assert {c["mask_dtype"] for c in CASES} == {"bool", "uint8"}
    assert any(c["alpha"] == 0 for c in CASES) and any(c["stable_scale"] == 0 for c in CASES)
    seen = set()
    for c in CASES:
        case = case_inputs(c)
        B, T, H, W = c["shape"]
        r = R.depth_loss_ref(case["pred"], case["target"], case["mask"], alpha=c["alpha"], stable_scale=c["stable_scale"])
        keep = case["mask"] != 0
        if c["keep_rate"] <= 0.3:
            assert not r["m_pred"].any() and not r["m_target"].any()
            seen.add("zero medians")
        if c["keep_rate"] >= 1.0 and (H * W) % 2 == 0 and H * W > 2:
            v = np.sort(case["target"].reshape(B * T, -1), axis=1)
            assert np.array_equal(r["m_target"].ravel(), v[:, H * W // 2 - 1]) and (v[:, H * W // 2 - 1] < v[:, H * W // 2]).all()
            seen.add("lower median")
        if c["empty_frames"]:
            assert all(r["count"].ravel()[f] == 0 and r["s_pred"].ravel()[f] == 1.0 for f in c["empty_frames"])
            assert r["count"].sum() > 0
            seen.add("empty frame")
        if c["empty_items"]:
            assert all(r["scale"][b] == 0 and r["shift"][b] == 0 and not keep[b].any() for b in c["empty_items"])
            seen.add("empty item")
        if c["kind"] == "anti":
            assert (r["scale"] < 0).all() and (case["target"][keep] < 0).any() and (case["target"][keep] > 0).any()
            seen.add("negative scale")
        if c["kind"] == "straddle":
            t = case["target"][keep]
            assert (t == 0).any() and ((t > 0) & (t < 1e-3)).any() and (t > 70).any() and r["absrel_count"] < keep.sum()
            seen.add("straddle")
        if B > 1 and not c["empty_items"]:
            assert r["scale"][0] != r["scale"][1]
            seen.add("two fits")
        if c["stable_scale"] > 0 and H * W > 6:
            both = (keep[:, 1:] & keep[:, :-1]).sum()
            assert 0 < r["stable_count"] <= both
            if r["stable_count"] < both:                     # the threshold drops some pixels, not all
                seen.add("threshold")
    assert seen == {"threshold", "zero medians", "lower median", "empty frame", "empty item", "negative scale", "straddle", "two fits"}


def test_restatement_corner_semantics():
    p = np.array([1.0, 2.0, 4.0, 3.0], np.float32).reshape(1, 2, 1, 2)
    r = R.depth_loss_ref(p, 2 * p + 1, np.ones(p.shape, bool))
    assert abs(float(r["scale"][0]) - 2) < 1e-6 and abs(float(r["shift"][0]) - 1) < 1e-5
    assert np.allclose(r["m_pred"], [[3.0, 7.0]], atol=1e-5) and r["d1"] == 1.0   # the lower of two values
    assert r["M"].tolist() == [4, 2, 2, 2]                                    # [::2], [::4], [::8] keep one point per frame
    nothing = R.depth_loss_ref(p, p, np.zeros(p.shape, bool))
    assert all(nothing[k] == 0.0 for k in KEYS) and nothing["s_target"].tolist() == [[1.0, 1.0]]
    with pytest.raises(ValueError):
        R.depth_loss_ref(p[:, :1], p[:, :1], np.ones((1, 1, 1, 2), bool))
    assert "stable_loss" not in R.depth_loss_ref(p[:, :1], p[:, :1], np.ones((1, 1, 1, 2), bool), stable_scale=0)


def test_constructor_keys_and_argument_errors():
    """The reference's signature and attributes; every ValueError and NotImplementedError comes before the device is touched;
    a CPU device is a VdnError."""
    import inspect
    from vdn import _abi, loss as L
    sig = inspect.signature(L.VideoDepthLoss.__init__)
    assert [(n, q.default) for n, q in list(sig.parameters.items())[1:7]] == [
        ("alpha", 0.5), ("scales", 4), ("trim", 0.0), ("stable_scale", 10), ("ssim_loss_scale", 0.0), ("reduction", "batch-based")]
    crit = L.VideoDepthLoss(alpha=0.3, stable_scale=7, ssim_loss_scale=0.0)
    assert (crit.stable_scale, crit.ssim_loss_scale, crit.initial_alpha, crit.initial_stable_scale) == (7, 0.0, 0.3, 7)
    assert crit.keys == ("spatial_loss", "stable_loss", "absRel_loss", "d1", "total_loss")
    assert L.VideoDepthLoss(stable_scale=0).keys == ("spatial_loss", "absRel_loss", "d1", "total_loss")
    for kw in (dict(trim=0.2), dict(reduction="image-based"), dict(ssim_loss_scale=0.5), dict(scales=5)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            L.VideoDepthLoss(**kw)
    p, m = torch.ones(1, 2, 4, 5), torch.ones(1, 2, 4, 5, dtype=torch.bool)
    with pytest.raises(ValueError, match="prediction"):
        crit(p[0], p[0], m[0])
    with pytest.raises(ValueError, match="target"):
        crit(p, p[:, :1], m)
    with pytest.raises(ValueError, match="mask"):
        crit(p, p, m[..., :3])
    with pytest.raises(ValueError, match="T >= 2"):
        crit(p[:, :1], p[:, :1], m[:, :1])
    with pytest.raises(ValueError, match="T >= 2"):
        L.depth_loss(p[:, :1], p[:, :1], m[:, :1])
    with pytest.raises(ValueError, match="prediction"):
        L.compute_scale_and_shift(p, p, m)
    with pytest.raises(NotImplementedError):
        L.depth_loss(p, p, m, scales=9)
    with pytest.raises(_abi.VdnError):
        L.VideoDepthLoss(device="cpu")(p, p, m)
    with pytest.raises(_abi.VdnError):
        L.compute_scale_and_shift(p[0], p[0], m[0], device="cpu")


def test_depth_loss_entry_point_rejects_bad_arguments():
    from vdn import _abi
    L, P = _abi.lib, 4096                                   # P: a non-null, aligned stand-in; nothing is launched
    assert L.vdn_depth_loss_workspace_bytes(0, 3) == 0 and L.vdn_depth_loss_workspace_bytes(2, 0) == 0
    assert L.vdn_depth_loss_workspace_bytes(2, 3) % 8 == 0
    assert L.vdn_depth_loss_workspace_bytes(1, 6) - L.vdn_depth_loss_workspace_bytes(2, 3) == -8    # one {scale, shift} slot per item
    #     pred target mask B T  H  W  alpha scales stable ws scale_shift stats counts out stream
    ok = [P, P, P, 2, 3, 4, 5, 0.5, 4, 10.0, P, None, None, None, P, None]

    def call(**changes):
        args = list(ok)
        for idx, val in changes.items():
            args[int(idx[1:])] = val
        return L.vdn_depth_loss(*args)

    for idx, val in dict(a0=None, a1=None, a2=None, a3=0, a4=0, a5=0, a6=-1, a8=-1, a10=None, a14=None).items():
        assert call(**{idx: val}) == -1, (idx, val)
    assert call(a4=1) == -1                                 # T == 1 with the temporal term
    assert call(a8=5) == -2 and call(a5=65536, a6=65536) == -2 and call(a3=300, a4=300) == -2
    assert call(a0=P + 2) == -3 and call(a14=P + 4) == -3 and call(a10=P + 4) == -3 and call(a11=P + 1) == -3
