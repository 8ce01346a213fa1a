"""Host-side checks of the normal criterion's gradient (vdn.normals, csrc/normals_grad.hip): the CPU restatement
tests/normal_grad_ref.py against prediction.grad of the reference's VideoNormalLoss as recorded in
tests/golden/normal_grad_cases.npz, against central differences of the forward restatement, on and under the clamp of
F.cosine_similarity, and the rejected-argument paths of the new entry point. Nothing here launches a kernel.

Bars. The reference's autograd runs in float32 and the restatement in float64. tools/make_golden_normal_grad.py measured, per
recorded gradient, the restatement's rel-L2 deviation and its largest absolute deviation over the reference's largest component
(1.1e-6 at most) and stored both; the bar is four times each, to cover float32 differences across torch builds, the convention
of tests/test_loss_grad_host.py. The generator refuses a deviation above 1e-4, which would mean a wrong restatement rather
than rounding. Central differences: below."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import normal_grad_ref as G
import normal_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "normal_grad_cases.npz")
Z = np.load(GOLD)
CASES = [dict(seed=int(Z["seed"][i]), shape=tuple(int(s) for s in Z["shape"][i]), mask_kind=str(Z["mask_kind"][i]),
              target_kind=str(Z["target_kind"][i]), empty=tuple(int(e) for e in Z["empty"][i] if e >= 0), checksum=Z["checksum"][i])
         for i in range(len(Z["seed"]))]
SPECIAL = len(CASES)                      # the index of the case on and under the clamp, recorded on its own
KINDS = ("stored", "depth")
RECORDED = [(i, k) for i in range(len(CASES) + 1) for k in KINDS]


def case_id(i) -> str:
    if i == SPECIAL:
        return f"seed{int(Z['special_seed'])}-special"
    c = CASES[i]
    return f"seed{c['seed']}-{c['mask_kind']}-{c['target_kind']}"


def case_seed(i) -> int:
    return int(Z["special_seed"]) if i == SPECIAL else CASES[i]["seed"]


@functools.lru_cache(maxsize=None)
def inputs(i):
    """Recorded case i (SPECIAL: the last), drawn once, shared and never written."""
    if i == SPECIAL:
        case, idx = G.make_special(int(Z["special_seed"]), tuple(int(s) for s in Z["special_shape"]))
        assert all(np.array_equal(idx[k], Z[f"special_{k}"]) for k in idx), "the seeded generator no longer picks the recorded pixels"
        want = Z["special_checksum"]
    else:
        c = CASES[i]
        case, want = R.make_case(c["seed"], c["shape"], c["mask_kind"], c["target_kind"], c["empty"]), c["checksum"]
    assert np.allclose(R.checksum(case), want, rtol=1e-12, atol=0), "the seeded generator no longer draws the recorded case"
    for a in case.values():
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def oracle(i, kind="stored", coeff=1.0):
    """-> (case, grad, mag) of the restatement on recorded case i against its stored target or its depth, computed once."""
    case = inputs(i)
    grad, mag = G.normal_loss_grad_ref(case["pred"], case["depth" if kind == "depth" else "target"], case["mask"], kind == "depth", coeff)
    grad.setflags(write=False)
    mag.setflags(write=False)
    return case, grad, mag


def test_fixture_covers_every_branch():
    kinds = [c["mask_kind"] for c in CASES]
    assert {"none", "bool", "float", "allfalse"} <= set(kinds) and any(c["target_kind"] == "scaled" for c in CASES)
    assert any(c["shape"][0] > 1 for c in CASES) and any(c["empty"] for c in CASES)
    assert os.path.getsize(GOLD) < 200_000
    for i in range(len(CASES) + 1):
        case = inputs(i)
        B, T, _, H, W = case["pred"].shape
        assert B * T * H * W <= 4000 and (H, W) != (224, 224)
        keep = R.erode_ref(case["mask"])
        for k in KINDS:
            g = Z[f"grad_{case_seed(i)}_{k}"]
            assert g.dtype == np.float32 and g.size == case["pred"].size
            dev = Z[f"deviation_{case_seed(i)}_{k}"]
            assert dev.shape == (2,) and (dev >= 0).all() and (dev <= 1e-4).all()
        if i == SPECIAL:
            continue
        c = CASES[i]
        per_frame = keep.reshape(B * T, -1).mean(1)
        if c["mask_kind"] in ("bool", "float"):
            full = [f for f in range(B * T) if f not in c["empty"]]
            assert 0.25 <= per_frame[full].mean() <= 0.90 and all(per_frame[f] == 0 for f in c["empty"])
        if c["mask_kind"] == "allfalse":
            assert not keep.any()
        if keep.any():
            assert np.sqrt((case["pred"].astype(np.float64) ** 2).sum(2))[keep].min() >= 1e-3


@pytest.mark.parametrize("i,kind", RECORDED, ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_restatement_reproduces_the_references_gradient(i, kind):
    case, got, _ = oracle(i, kind)
    want = Z[f"grad_{case_seed(i)}_{kind}"].reshape(case["pred"].shape).astype(np.float64)
    rel_dev, max_dev = (float(v) for v in Z[f"deviation_{case_seed(i)}_{kind}"])
    assert np.isfinite(got).all()
    diff, scale = got - want, float(np.abs(want).max())
    if scale == 0:
        assert not got.any() and not R.erode_ref(case["mask"]).any()
        return
    rel = float(np.sqrt((diff ** 2).sum() / (want ** 2).sum()))
    mx = float(np.abs(diff).max()) / scale
    print(f"rel-L2 {rel:.2e} (bar {4 * rel_dev:.2e}), max-abs / max {mx:.2e} (bar {4 * max_dev:.2e}), max |g| {scale:.3g}")
    assert rel <= 4 * rel_dev and mx <= 4 * max_dev


def test_zero_under_every_dropped_pixel_and_in_an_empty_batch():
    for i, kind in RECORDED:
        case, grad, mag = oracle(i, kind)
        drop = np.broadcast_to(~R.erode_ref(case["mask"])[:, :, None], grad.shape)
        assert not grad[drop].any() and not np.signbit(grad[drop]).any() and not mag[drop].any(), case_id(i)
    i = next(i for i, c in enumerate(CASES) if c["mask_kind"] == "allfalse")
    assert not oracle(i)[1].any()
    i = next(i for i, c in enumerate(CASES) if c["empty"])
    f = CASES[i]["empty"][0]
    g = oracle(i)[1].reshape((-1,) + oracle(i)[1].shape[2:])
    assert not g[f].any() and g[f - 1].any()


def test_restatement_against_central_differences():
    """The forward in float64, (L(p + h e) - L(p - h e)) / 2h with h = 1e-6 * max(1, |p_c|) for every component of a small case,
    stored target and depth target: relative error below 1e-6 of the largest gradient entry. The difference quotient is good to
    about 1e-9 there: its truncation is h^2 |L'''| / 6, some 1e-12 of the gradient, and the rounding of the two losses,
    2^-53 |L| / h = 1e-10, is some 3e-9 of a largest entry of 0.04.
    normal_ref.normal_loss_ref rounds its prediction to float32, which would swallow the step, so the float64 loss is composed
    here from the same functions in the same way (erode_ref, cosine_ref, select, sum, 1 - sum / count) and is first held to
    normal_loss_ref's value at the unperturbed point, bit for bit."""
    case = R.make_case(71, (1, 2, 5, 6), "bool", "scaled", false_rate=0.04)
    keep = R.erode_ref(case["mask"])
    assert 4 <= keep.sum() < keep.size
    for from_depth in (False, True):
        target = case["depth"] if from_depth else case["target"]
        b = R.normal_vector_ref(target) if from_depth else target.astype(np.float64)
        n = int(keep.sum())

        def loss64(a):
            return 1.0 - float(np.where(keep, R.cosine_ref(a, b), 0.0).sum((-1, -2)).sum()) / n

        p = case["pred"].astype(np.float64)
        assert loss64(p) == R.normal_loss_ref(case["pred"], target, case["mask"], from_depth)[0]
        got, _ = G.normal_loss_grad_ref(case["pred"], target, case["mask"], from_depth)
        fd = np.zeros_like(p)
        for j in range(p.size):
            h = 1e-6 * max(1.0, abs(p.flat[j]))
            hi, lo = p.copy(), p.copy()
            hi.flat[j] += h
            lo.flat[j] -= h
            fd.flat[j] = (loss64(hi) - loss64(lo)) / (hi.flat[j] - lo.flat[j])
        scale = float(np.abs(got).max())
        err = float(np.abs(got - fd).max()) / scale
        print(f"from_depth={from_depth}: max |grad - difference quotient| / max |grad| = {err:.2e}, max |grad| {scale:.3g}")
        assert scale > 0 and err < 1e-6


def test_on_and_under_the_clamp():
    """The special case, restatement and recorded reference alike: a prediction under the clamp gets
    -(1 / N) * (that - (p . that) / n * p / |p|) / n with n = 1e-8 (for p = (3e-9, 0, 0): 0.7 of that_x / 1e-8 in x, all of
    that_y / 1e-8 in y), a zero prediction gets -(1 / N) * that / 1e-8 (the norm's derivative is 0 at the origin), and a zero
    target gives a zero gradient."""
    case, got, _ = oracle(SPECIAL, "stored")
    B, T, _, H, W = case["pred"].shape
    want = Z[f"grad_{case_seed(SPECIAL)}_stored"].reshape(B * T, 3, H * W).astype(np.float64)
    got = got.reshape(B * T, 3, H * W)
    pred, target = (case[k].reshape(B * T, 3, H * W).astype(np.float64) for k in ("pred", "target"))
    n_kept = int(R.erode_ref(case["mask"]).sum())
    at = lambda a, flat: a[flat // (H * W), :, flat % (H * W)]
    for k, flat in enumerate(Z["special_tiny"]):
        p, t = at(pred, flat), at(target, flat)
        assert 0 < np.linalg.norm(p) < 1e-8 and np.array_equal(p, G.TINY[k].astype(np.float64))
        that = t / np.linalg.norm(t)
        expect = -(1.0 / n_kept) * (that - (p @ that) / 1e-8 * p / np.linalg.norm(p)) / 1e-8
        for name, g in (("restatement", at(got, flat)), ("reference", at(want, flat))):
            assert np.abs(g - expect).max() <= (1e-12 if name == "restatement" else 1e-6) * np.abs(expect).max(), (name, k, g, expect)
        if k == 0:                                            # p = (3e-9, 0, 0)
            plain = -(1.0 / n_kept) * that / 1e-8
            factor = 1.0 - float(np.float32(3e-9)) / 1e-8
            assert abs(factor - 0.7) < 1e-7
            assert abs(at(got, flat)[0] / plain[0] - factor) < 1e-12 and abs(at(want, flat)[0] / plain[0] - factor) < 1e-6
            assert abs(at(got, flat)[1] / plain[1] - 1.0) < 1e-12 and abs(at(want, flat)[1] / plain[1] - 1.0) < 1e-6
    for flat in Z["special_zero_pred"]:
        p, t = at(pred, flat), at(target, flat)
        assert not p.any()
        expect = -(1.0 / n_kept) * (t / np.linalg.norm(t)) / 1e-8
        assert np.abs(at(got, flat) - expect).max() <= 1e-12 * np.abs(expect).max()
        assert np.abs(at(want, flat) - expect).max() <= 1e-6 * np.abs(expect).max()
    for flat in Z["special_zero_target"]:
        assert not at(target, flat).any() and at(pred, flat).any()
        assert not at(got, flat).any() and not at(want, flat).any()


def test_backward_entry_point_rejects_bad_arguments():
    """The codes of vdn_normal_loss_backward, returned before anything is launched: no GPU is needed."""
    from vdn import _abi, normals as N
    L, P = _abi.lib, 4096                                   # P: a non-null, aligned stand-in; nothing is launched
    assert L.vdn_normal_loss_backward_trip(1) == 4 * L.vdn_normal_loss_backward_trip(0) == N.grad_trip_pixels(True) > 0
    #     pred target is_depth mask frames H W count coeff grad stream
    ok = [P, P, 0, None, 2, 3, 4, P, P, P, None]

    def call(**changes):
        args = list(ok)
        for idx, val in changes.items():
            args[int(idx[1:])] = val
        return L.vdn_normal_loss_backward(*args)

    for idx in (0, 1, 7, 8, 9):                              # every pointer but the mask is required
        assert call(**{f"a{idx}": None}) == -1, idx
    for idx, val in dict(a4=0, a4_=-3, a5=1, a6=1).items():
        assert call(**{idx.rstrip("_"): val}) == -1, (idx, val)
    assert call(a5=65536, a6=65536) == -2                    # H * W past INT32_MAX
    for idx in (0, 1, 9):
        assert call(**{f"a{idx}": P + 2}) == -3, idx         # a float pointer off by 2 bytes
    for idx in (7, 8):
        assert call(**{f"a{idx}": P + 4}) == -3, idx         # a double pointer off by 4
    assert call(a2=1, a1=P + 2) == -3 and call(a0=None, a5=65536, a6=65536) == -1   # the order of vdn_normal_eval
