"""Host-side checks of the SSIM term of the depth criterion (vdn.loss, csrc/ssim.hip): the CPU restatement tests/ssim_ref.py
against the reference's DepthShallowSSIMLoss and its VideoDepthLoss(ssim_loss_scale=0.3) as tests/golden/ssim_cases.npz
records them (tools/make_golden_ssim.py: the reference's own file on an in-memory restatement of pytorch_msssim, which is not
installed; the library's own file is therefore not pinned), the restatement's gradient against central differences, the window,
and the signatures, key order and rejected arguments of the new classes. Nothing here launches a kernel.

Bars. The reference runs in float32 as its scripts do, and was also run in float64; the fixture records how far the two runs
are apart, value and gradient (rel-L2). The restatement is the float64 run but for the contract's float32 steps (the
alignment, the maximum, the division), so against the float64 run it is held to the same figure as the float32 run is, and
against the float32 run to four times it: the float32 composition's rounding and no more. The gradient is compared at the
fixture's 1024 hashed samples per case plus every item's maximum, relative to the recorded norm per sample."""
from __future__ import annotations

import functools
import inspect
import os

import numpy as np
import pytest
import torch

import loss_grad_ref as G
import loss_ref as R
import ssim_ref as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_cases.npz")
Z = np.load(GOLD)
NAMES = [str(n) for n in Z["names"]]


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a recorded case, regenerated from its seed, shared and never written."""
    i = NAMES.index(name)
    c = S.make_case(int(Z["seeds"][i]), tuple(int(v) for v in Z["shapes"][i]), float(Z["keep"][i]),
                    tuple((int(b), int(t)) for b, t in Z[f"{name}_inverse"]), float(Z["gain"][i]))
    for a in c.values():
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def alone(name):
    c = case(name)
    r = S.ssim_grad_ref(c["pred"], c["target"], c["mask"])
    r["grad"].setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def whole(name):
    """The restatement of the composite: the other terms' gradient of tests/loss_grad_ref.py plus ssim_loss_scale times the
    term's through the fit; the dictionary's values in the reference's order."""
    i = NAMES.index(name)
    c = case(name)
    alpha, ss, scale = float(Z["alpha"][i]), float(Z["stable_scale"][i]), float(Z["ssim_scale"])
    base = G.depth_loss_grad_ref(c["pred"], c["target"], c["mask"], alpha=alpha, stable_scale=ss)
    fit = (base["fwd"]["scale"], base["fwd"]["shift"])
    term = S.ssim_grad_ref(c["pred"], c["target"], c["mask"], fit, coeff=scale)
    f = base["fwd"]
    values = {"spatial_loss": f["spatial_loss"], "stable_loss": f.get("stable_loss"), "ssim_loss": term["fwd"]["loss"],
              "absRel_loss": f["absRel_loss"], "d1": f["d1"]}
    values["total_loss"] = f["spatial_loss"] + (ss * f["stable_loss"] if ss > 0 else 0.0) + scale * term["fwd"]["loss"]
    grad = base["grad"] + term["grad"]
    grad.setflags(write=False)
    return dict(grad=grad, values=values, term=term, base=base, fit=fit)


def test_the_inputs_are_the_recorded_ones():
    """The cases are regenerated from integer hashes and exactly rounded operations: the same bits on every machine."""
    for name in NAMES:
        assert S.checksum(case(name)) == [float(v) for v in Z[f"{name}_checksum"]]


def test_window_is_the_fixtures_bit_for_bit():
    """Fails without the feature: vdn.loss has no SSIM_WINDOW."""
    from vdn import loss as L
    w = Z["window"]
    assert w.dtype == np.float32 and w.shape == (11,)
    assert np.array(L.SSIM_WINDOW, np.float64).tobytes() == w.astype(np.float64).tobytes()
    assert S.WINDOW.tobytes() == w.astype(np.float64).tobytes()
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "video-depth-normal-v2_amd", "csrc", "ssim.hip")).read()
    literals = [float.fromhex(h) for h in re.findall(r"0x1\.[0-9a-f]+p-?[0-9]+", src)]
    assert np.array(literals[:11], np.float64).tobytes() == w.astype(np.float64).tobytes()   # the kernel's literals


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference_alone(name):
    r = alone(name)
    v32, v64 = (float(v) for v in Z[f"{name}_alone_value"])
    dv, dg = (float(v) for v in Z[f"{name}_alone_yardstick"])
    at = Z[f"{name}_at"]
    n32, n64 = (float(v) for v in Z[f"{name}_alone_norm"])
    got = r["grad"].ravel()[at]
    per = n64 / np.sqrt(r["grad"].size)            # the recorded norm per sample
    rel64 = float(np.sqrt(((got - Z[f"{name}_alone_grad64"]) ** 2).mean())) / per
    rel32 = float(np.sqrt(((got - Z[f"{name}_alone_grad32"].astype(np.float64)) ** 2).mean())) / per
    print(f"[{name}] value: |restatement - f64 run| {abs(r['fwd']['loss'] - v64):.2e}, - f32 run {abs(r['fwd']['loss'] - v32):.2e} (f32 vs f64 {dv:.2e}); "
          f"gradient rel-L2 at the samples: vs f64 {rel64:.2e}, vs f32 {rel32:.2e} (f32 vs f64 {dg:.2e})")
    assert 0 < dv < 1e-6 and 0 < dg < 1e-4                       # the yardstick itself is float32 rounding
    assert abs(r["fwd"]["loss"] - v64) <= max(dv, 1e-9) and abs(r["fwd"]["loss"] - v32) <= 4 * dv
    assert rel64 <= dg and rel32 <= 4 * dg
    # every item's maximum is among the samples, and where the prediction holds it the spike is the reference's
    B = r["grad"].shape[0]
    for b in range(B):
        j = int(r["fwd"]["index"][b]) + b * (r["grad"].size // B)
        k = int(np.flatnonzero(at == j)[0])
        assert abs(got[k] - Z[f"{name}_alone_grad64"][k]) <= 4 * dg * abs(Z[f"{name}_alone_grad64"][k]) + 1e-12
    assert r["fwd"]["gated"] == len(Z[f"{name}_inverse"])


def test_the_fixture_has_a_maximum_in_the_prediction_and_a_gated_frame():
    assert S.HOLDERS[int(alone("plain")["fwd"]["holder"][0])] == "prediction" and alone("plain")["hold"][0] != 0
    g = alone("plain")["grad"].ravel()
    assert abs(g[int(alone("plain")["fwd"]["index"][0])]) > 100 * np.median(np.abs(g))      # the path through max_val is not optional
    r = alone("gated")
    assert r["fwd"]["gated"] == 1 and r["fwd"]["cs"][0, 1] < 0 and not r["g_x"][0, 1].any()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference_whole(name):
    w = whole(name)
    keys = [str(k) for k in Z[f"{name}_whole_keys"]]
    assert keys == [k for k in ("spatial_loss", "stable_loss", "ssim_loss", "absRel_loss", "d1", "total_loss")
                    if k != "stable_loss" or float(Z["stable_scale"][NAMES.index(name)]) > 0]
    d32, d64 = Z[f"{name}_whole_dict"]
    dv, dg = (float(v) for v in Z[f"{name}_whole_yardstick"])
    for k, a, b in zip(keys, d32, d64):
        tol = 4 * max(abs(float(a) - float(b)), 2.0 ** -24 * abs(float(b)))
        print(f"[{name}] {k}: restatement {w['values'][k]:.9f} f32 {float(a):.9f} f64 {float(b):.9f}")
        assert abs(w["values"][k] - float(a)) <= tol, k
    at = Z[f"{name}_at"]
    n64 = float(Z[f"{name}_whole_norm"][1])
    got = w["grad"].ravel()[at]
    per = n64 / np.sqrt(w["grad"].size)
    rel32 = float(np.sqrt(((got - Z[f"{name}_whole_grad32"].astype(np.float64)) ** 2).mean())) / per
    print(f"[{name}] whole gradient rel-L2 at the samples vs the f32 run {rel32:.2e} (f32 vs f64 {dg:.2e})")
    assert 0 < dg < 1e-4 and rel32 <= 4 * dg


def test_closed_form_of_the_maximums_path_is_the_sum_over_pixels():
    """dL/dmax_val = -sum_j (g_x x + g_y y)_j / max_val, and the form the device evaluates: 2 C2 w sum_o (A - D) / D^2."""
    for name in NAMES:
        r = alone(name)
        assert np.allclose(r["dmax_direct"], r["dmax_closed"], rtol=1e-9, atol=1e-15), (r["dmax_direct"], r["dmax_closed"])
        assert (r["dmax_closed"] != 0).all()


def test_gradient_against_central_differences():
    """On a handful of elements of a small case, the holder of the maximum among them, alone and through the fit (which is
    then fitted again for every perturbed prediction). The loss is evaluated with its float32 steps, so the step is large
    (2^-7) and the bar 2e-3 of the largest of the handful."""
    c = S.make_case(21, (2, 2, 24, 27), 0.875, ((1, 0),), 1.5)
    n = c["pred"][0].size
    for through_fit in (False, True):
        fit_of = lambda q: R.fit_ref(q, c["target"], c["mask"]) if through_fit else None
        loss = lambda q: S.ssim_ref(q, c["target"], c["mask"], fit_of(q))["loss"]
        r = S.ssim_grad_ref(c["pred"], c["target"], c["mask"], fit_of(c["pred"]))
        assert r["fwd"]["gated"] == 1
        holders = [int(r["fwd"]["index"][b]) + b * n for b in range(2) if r["fwd"]["weight"][b] != 0]
        assert holders or through_fit, "no item's maximum is in its prediction"
        pairs = []
        for j in [int(v) for v in (S._hash01(5, 6) * c["pred"].size)] + holders:
            hi, lo = c["pred"].copy(), c["pred"].copy()
            hi.reshape(-1)[j] += np.float32(2.0 ** -7)
            lo.reshape(-1)[j] -= np.float32(2.0 ** -7)
            pairs.append(((loss(hi) - loss(lo)) / (float(hi.reshape(-1)[j]) - float(lo.reshape(-1)[j])), float(r["grad"].reshape(-1)[j])))
        big = max(abs(g) for _, g in pairs)
        for d, g in pairs:
            print(f"through the fit {through_fit}: central difference {d:+.6e} restatement {g:+.6e}")
            assert abs(d - g) <= 2e-3 * big + 1e-9


def test_who_holds_the_maximum():
    """Each branch of the maximum's rule, on items of four pixels."""
    f = lambda a, t, k: S.item_max(np.array([a], np.float32), np.array([t], np.float32), np.array([k], bool))
    name = lambda r: (S.HOLDERS[int(r[1][0])], float(r[2][0]), int(r[3][0]))
    assert name(f([1, 3, 3, 2], [1, 1, 1, 1], [1, 1, 1, 1])) == ("prediction", 1.0, 1)          # the lowest index among equals
    assert name(f([1, 3, 2, 2], [1, 4, 1, 1], [1, 1, 1, 1])) == ("target", 0.0, 1)
    assert name(f([1, 3, 2, 2], [1, 3, 1, 1], [1, 1, 1, 1])) == ("tie", 0.5, 1)
    assert name(f([-1, -3, 9, -2], [-1, -1, 9, -1], [1, 1, 0, 1])) == ("dropped", 0.0, -1)       # all kept values negative: a dropped pixel's 0
    assert name(f([0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1])) == ("clamp", 0.0, 0)
    assert name(f([9, 3, 2, 2], [9, 1, 1, 1], [0, 1, 1, 1])) == ("prediction", 1.0, 1)           # a dropped pixel's value is not read
    assert name(f([0, -3, 0, -2], [-1, -1, -1, -1], [0, 1, 1, 1])) == ("dropped", 0.0, -1)       # the dropped 0 comes before the kept one
    assert name(f([-1, 0, 0, -2], [-1, -1, -1, -1], [1, 1, 0, 1])) == ("clamp", 0.0, 1)          # the kept 0 comes first, below the clamp
    r = f([-1, -3, 9, -2], [-1, -1, 9, -1], [1, 1, 0, 1])
    assert float(r[0][0]) == float(np.float32(1e-8))


def _device_cases():
    import test_gpu_ssim as Gs
    return Gs


@pytest.mark.parametrize("name", _device_cases().PAST_ONE_RING)
def test_the_device_tests_larger_inputs_are_what_they_are_named_for(name):
    """The cases tests/test_gpu_ssim.py takes past one ring of tiles and one trip of the sweeps, checked where no device is: the
    restatement gives the holder, index and gated count the table expects, the placed maxima are kept pixels of equal bits,
    the shapes reach what they are there for, and the measured floor is a number."""
    Gs = _device_cases()
    _, aligned, holders, gated = Gs.CASES[name]
    c, fit, r, floor = Gs.oracle(name)
    f = r["fwd"]
    Gs.reach(name, c["pred"].shape)
    print(f"[{name}] holder {[S.HOLDERS[int(h)] for h in f['holder']]} index {f['index'].tolist()} gated {f['gated']} cs {f['cs'].ravel().tolist()} "
          f"floor {floor:.2e}")
    assert (fit is not None) == aligned and f["gated"] == gated and np.isfinite(floor) and 0 < floor < 1e-12
    assert np.isfinite(r["grad"]).all() and r["grad"].any()
    if holders is not None:
        assert tuple(S.HOLDERS[int(h)] for h in f["holder"]) == holders and r["hold"][0] != 0
    if name == "strip-gated-aligned":
        assert f["cs"][0, 1] < 0 < f["cs"][0, 0] and not c["mask"][0, 1].any() and not r["grad"][0, 1].any()
    if name.startswith("holder-"):
        at = Gs.placed(name)
        pred, keep = c["pred"][0, 0].reshape(-1), c["mask"][0, 0].reshape(-1)
        assert len(at) == (2 if name == "holder-tie-across-blocks" else 1) and len(set(at)) == len(at) and max(at) < pred.size
        assert all(keep[i] and pred[i].tobytes() == pred[at[0]].tobytes() for i in at)
        assert (pred[at[0]] > np.delete(c["pred"][0].reshape(-1), at)).all() and pred[at[0]] > c["target"].max()
        assert f["index"][0] == min(at) and f["max_val"][0] == pred[at[0]]
        # the placed indices sit where the names say: the later one on a lane's second trip, the earlier in another block
        assert at[-1] // Gs.trip(True) == 1 and at[0] // Gs.trip(True) == (1 if len(at) == 1 else 0)


def test_signatures_keys_and_argument_errors():
    """Fails without the feature: the classes do not exist. Every error comes before the device is touched (this machine has
    none)."""
    from vdn import loss as L
    sig = lambda f: [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()][1:]
    kw, pk = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert sig(L.DepthShallowSSIMLoss.__init__) == [("reduction", "batch-based", pk), ("weights", [1.0, 0.0, 0.0, 0.0, 0.0], pk),
                                                    ("device", "cuda", kw)]
    assert sig(L.SSIMVideoDepthLoss.__init__) == [("alpha", 0.5, pk), ("scales", 4, pk), ("trim", 0.0, pk), ("stable_scale", 10, pk),
                                                  ("ssim_loss_scale", 0.0, pk), ("device", "cuda", kw)]
    assert L.SSIMVideoDepthLoss(0.5, 4, 0.0, 10, 0.3).keys == ("spatial_loss", "stable_loss", "ssim_loss", "absRel_loss", "d1", "total_loss")
    assert L.SSIMVideoDepthLoss(stable_scale=0, ssim_loss_scale=0.3).keys == ("spatial_loss", "ssim_loss", "absRel_loss", "d1", "total_loss")
    assert L.SSIMVideoDepthLoss().keys == L.TrimmedVideoDepthLoss(trim=0.0).keys == L.VideoDepthLoss().keys
    c = L.SSIMVideoDepthLoss(0.25, 3, 0.2, 5, 0.1)
    assert (c.initial_alpha, c.scales, c.trim, c.stable_scale, c.ssim_loss_scale, c._keep) == (0.25, 3, 0.2, 5, 0.1, 1.0 - 0.2)
    with pytest.raises(NotImplementedError):
        L.DepthShallowSSIMLoss(reduction="image-based")
    for w in ([0.5, 0.5, 0, 0, 0], [1.0, 0, 0, 0], [2.0, 0, 0, 0, 0], [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]):
        with pytest.raises(NotImplementedError):
            L.DepthShallowSSIMLoss(weights=w)
    L.DepthShallowSSIMLoss(weights=(1, 0, 0, 0, 0))
    for bad in (dict(trim=1.0), dict(trim=-0.1), dict(ssim_loss_scale="0.1"), dict(ssim_loss_scale=float("nan"))):
        with pytest.raises(ValueError):
            L.SSIMVideoDepthLoss(**bad)
    with pytest.raises(NotImplementedError):
        L.SSIMVideoDepthLoss(scales=5)
    p = torch.zeros(1, 2, 160, 200)
    for crit in (L.DepthShallowSSIMLoss(), L.SSIMVideoDepthLoss(ssim_loss_scale=0.1)):
        with pytest.raises(ValueError, match="160"):
            crit(p, p, p > -1)                                   # the library asserts min(H, W) > 160
        with pytest.raises(ValueError):
            crit(p, p[:, :1], p > -1)
    for fn in (L.ssim_loss, L.ssim_loss_grad):
        with pytest.raises(ValueError, match="11"):
            fn(torch.zeros(1, 1, 10, 30), torch.zeros(1, 1, 10, 30), torch.ones(1, 1, 10, 30))
    q = torch.zeros(1, 2, 161, 161, requires_grad=True)
    with pytest.raises(NotImplementedError):
        L.DepthShallowSSIMLoss()(torch.zeros(1, 2, 161, 161), q, q > -1)      # a target that requires a gradient


def test_the_older_classes_keep_their_refusals():
    from vdn import loss as L
    with pytest.raises(NotImplementedError):
        L.VideoDepthLoss(ssim_loss_scale=0.5)
    crit = L.VideoDepthLoss()
    crit.ssim_loss_scale = 0.5                                   # the attribute is public
    with pytest.raises(NotImplementedError):
        crit(torch.zeros(1, 2, 161, 161), torch.zeros(1, 2, 161, 161), torch.ones(1, 2, 161, 161))
    assert "ssim_loss_scale" not in inspect.signature(L.TrimmedVideoDepthLoss.__init__).parameters


def test_header_declares_what_the_library_exports():
    import re
    from vdn import _abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "vdn.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vdn_ssim_[a-z_]+)\s*\(", hdr))
    assert declared == {"vdn_ssim_tile", "vdn_ssim_loss_workspace_bytes", "vdn_ssim_loss", "vdn_ssim_loss_backward_workspace_bytes",
                        "vdn_ssim_loss_backward"}
    assert declared == {n for n in _abi.EXPORTS if n.startswith("vdn_ssim_")}
    for n in declared:
        assert hasattr(_abi.lib, n)
    from vdn import loss as L
    th, tw = L.ssim_tile()
    assert th > 0 and tw > 0
    # sizes the entry points refuse before anything is launched have no workspace
    assert _abi.lib.vdn_ssim_loss_workspace_bytes(1, 1, 10, 11) == 0 and _abi.lib.vdn_ssim_loss_workspace_bytes(1, 1, 11, 11) > 0
    assert _abi.lib.vdn_ssim_loss_backward_workspace_bytes(1, 2, 11, 11) >= 8 * 2 * (3 * 1 + 121)
    assert _abi.lib.vdn_ssim_loss(None, None, None, None, 1, 1, 11, 11, None, None, None, None, None) == -1   # VDN_EINVAL
