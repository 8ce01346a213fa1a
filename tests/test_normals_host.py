"""Host-side checks of the normal evaluation (vdn.normals, csrc/normals.hip): the CPU restatement tests/normal_ref.py against
the values the reference recorded in tests/golden/normal_cases.npz, the fixture's coverage, the wrapper's argument errors
and the rejected-argument paths of the new entry points. Nothing here launches a kernel.

Bars. Loss: 2e-6 absolute. The reference computes in float32: each cosine carries a few ulp, at most 4e-7, and a pairwise
float32 sum over at most 1.1e6 terms in [-1, 1] adds at most about log2(N) * 2^-24 = 1.2e-6 to the mean. Recorded normals:
4 * 2^-24 * max(1, max|d|) per component: float32 rounding in a six-term stencil, passed through a map whose derivative
is at most 1."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import normal_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "normal_cases.npz")
LOSS_ATOL = 2e-6


def golden_cases():
    z = np.load(GOLD)
    for i in range(len(z["seed"])):
        yield dict(seed=int(z["seed"][i]), shape=tuple(int(s) for s in z["shape"][i]), mask_kind=str(z["mask_kind"][i]),
                   target_kind=str(z["target_kind"][i]), empty=tuple(int(e) for e in z["empty"][i] if e >= 0),
                   checksum=z["checksum"][i], expected=float(z["expected"][i]), expected_depth=float(z["expected_depth"][i]),
                   kept_share=float(z["kept_share"][i]))


def case_inputs(c):
    case = R.make_case(c["seed"], c["shape"], c["mask_kind"], c["target_kind"], c["empty"])
    assert np.allclose(R.checksum(case), c["checksum"], rtol=1e-12, atol=0), "the seeded generator no longer draws the recorded case"
    return case


def recorded_normals():
    z = np.load(GOLD)
    for i in range(len(z["nv_seed"])):
        shape = tuple(int(s) for s in z["nv_shape"][i])
        d = R.make_depth(np.random.default_rng(int(z["nv_seed"][i])), shape)
        assert np.isclose(d.astype(np.float64).sum(), float(z[f"nv{i}_depth_checksum"]), rtol=1e-12, atol=0)
        nk, sxy, sz, eps = z["nv_args"][i]
        yield d, dict(normalize_kernel=bool(nk), scale_xy=float(sxy), scale_z=float(sz), eps=float(eps)), z[f"nv{i}"]


def normals_bar(d) -> float:
    return 4 * 2.0 ** -24 * max(1.0, float(np.abs(d).max()))


CASES = list(golden_cases())


@pytest.mark.parametrize("c", CASES, ids=lambda c: f"seed{c['seed']}-{c['mask_kind']}-{c['target_kind']}")
def test_normal_ref_reproduces_the_reference(c):
    case = case_inputs(c)
    got = R.normal_loss_ref(case["pred"], case["target"], case["mask"])[0]
    got_depth = R.normal_loss_ref(case["pred"], case["depth"], case["mask"], target_is_depth=True)[0]
    print(f"stored target: {got!r} vs {c['expected']!r} diff {got - c['expected']:+.2e}; "
          f"from depth: {got_depth!r} vs {c['expected_depth']!r} diff {got_depth - c['expected_depth']:+.2e}")
    assert abs(got - c["expected"]) <= LOSS_ATOL
    assert abs(got_depth - c["expected_depth"]) <= LOSS_ATOL


def test_normal_vector_ref_reproduces_the_recorded_normals():
    n = 0
    for d, args, want in recorded_normals():
        got = R.normal_vector_ref(d, **args)
        assert want.shape == got.shape and want.dtype == np.float32 and want.size < 1000
        diff = float(np.abs(got - want).max())
        print(f"{d.shape}: max abs diff {diff:.2e}, bar {normals_bar(d):.2e}")
        assert diff <= normals_bar(d)
        n += 1
    assert n == 2


def test_fixture_covers_every_branch():
    kinds = [c["mask_kind"] for c in CASES]
    assert len(CASES) >= 6 and {"none", "bool", "float", "allfalse"} <= set(kinds)
    assert any(c["shape"][0] > 1 for c in CASES) and any(c["empty"] for c in CASES)
    assert any(c["target_kind"] == "scaled" for c in CASES)
    for c in CASES:
        case = case_inputs(c)
        keep = R.erode_ref(case["mask"])
        assert np.isclose(keep.mean(), c["kept_share"], atol=1e-6)        # the reference's own eroded_mask, recorded
        if c["mask_kind"] == "none":
            assert case["mask"].dtype == bool and case["mask"].all() and keep.all()
        if c["mask_kind"] == "float":
            assert case["mask"].dtype == np.float32 and set(np.unique(case["mask"])) <= {0.0, 1.0}
        if c["mask_kind"] == "allfalse":
            assert not keep.any() and c["expected"] == 1.0 and c["expected_depth"] == 1.0
        if c["mask_kind"] in ("bool", "float"):
            B, T, H, W = c["shape"]
            per_frame = keep.reshape(B * T, -1).mean(1)
            full = [f for f in range(B * T) if f not in c["empty"]]
            assert 0.25 <= per_frame[full].mean() <= 0.90, per_frame
            assert all(per_frame[f] == 0 for f in c["empty"])
        if c["target_kind"] == "scaled":
            length = np.sqrt((case["target"].astype(np.float64) ** 2).sum(2))
            assert length.min() < 0.5 and length.max() > 2.0


def test_restatement_corner_semantics():
    ones = np.ones((1, 1, 5, 6), bool)
    assert R.erode_ref(ones).all()                                        # an all-true mask keeps the whole border
    for (y, x), dropped in (((0, 0), 4), ((0, 3), 6), ((2, 3), 9)):
        m = ones.copy()
        m[0, 0, y, x] = False
        assert (~R.erode_ref(m)).sum() == dropped
    pred = np.zeros((1, 1, 3, 2, 2), np.float32)                          # a zero vector: cosine 0, loss 1
    loss, mean, count = R.normal_loss_ref(pred, np.ones((1, 1, 2, 2), np.float32), None, target_is_depth=True)
    assert loss == 1.0 and mean[0, 0] == 0.0 and count[0, 0] == 4
    with pytest.raises(ValueError):
        R.sobel_ref(np.ones((1, 5), np.float32))


def test_wrapper_argument_errors():
    """Every ValueError and NotImplementedError comes before the device is touched; a CPU device is a VdnError."""
    from vdn import _abi, normals as N
    p, t, d, m = torch.ones(1, 2, 3, 4, 5), torch.ones(1, 2, 3, 4, 5), torch.ones(1, 2, 4, 5), torch.ones(1, 2, 4, 5, dtype=torch.bool)
    loss = N.VideoNormalLoss(trim=0.2)
    with pytest.raises(NotImplementedError):
        N.VideoNormalLoss(reduction="image-based")
    with pytest.raises(ValueError, match="prediction"):
        loss(p[0], t[0], m)
    with pytest.raises(ValueError, match="prediction"):
        loss(p[:, :, :2], t[:, :, :2], m)
    with pytest.raises(ValueError, match="target"):
        loss(p, t[:, :1], m)
    with pytest.raises(ValueError, match="target"):
        loss(p, d, m)
    with pytest.raises(ValueError, match="mask"):
        loss(p, t, m[:, :, :3])
    with pytest.raises(ValueError, match="at least 2"):
        loss(p[..., :1], t[..., :1], m[..., :1])
    with pytest.raises(ValueError, match="gt_depth"):
        N.normal_loss_from_depth(p, t)
    with pytest.raises(ValueError, match="mask"):
        N.normal_loss_from_depth(p, d, m[0])
    with pytest.raises(ValueError, match="at least 2"):
        N.normal_loss_from_depth(p[:, :, :, :1], d[:, :, :1])
    with pytest.raises(ValueError, match="mask"):
        loss.eroded_mask(m[0, 0])
    for fn in (N.normal_vector, N.sobel_ix_iy):
        with pytest.raises(ValueError, match=r"\(B,S,1,Y,X\)"):
            fn(d)
        with pytest.raises(ValueError, match=r"\(B,S,1,Y,X\)"):
            fn(t)
        with pytest.raises(ValueError, match="at least 2"):
            fn(d[:, :, None, :1])
        with pytest.raises(_abi.VdnError):
            fn(d[:, :, None], device="cpu")
    with pytest.raises(_abi.VdnError):
        N.normal_loss_from_depth(p, d, device="cpu")
    with pytest.raises(_abi.VdnError):
        N.VideoNormalLoss(device="cpu")(p, t, m)


def test_normal_entry_points_reject_bad_arguments():
    from vdn import _abi
    L, P = _abi.lib, 4096                                   # P: a non-null, aligned stand-in; nothing is launched
    assert L.vdn_normal_eval_workspace_bytes(0) == 0 and L.vdn_normal_eval_workspace_bytes(3) % 8 == 0
    assert L.vdn_normal_eval_workspace_bytes(32) == 32 * L.vdn_normal_eval_workspace_bytes(1)
    sob_ok = [P, P, P, 2, 3, 4, 1, None]
    nv_ok = [P, P, 2, 3, 4, 1, 1.0, 1.0, 1e-8, None]
    er_ok = [P, P, 2, 3, 4, None]
    ev_ok = [P, P, 1, None, 2, 3, 4, P, None, None, P, None]

    def bad(fn, ok, **changes):
        for idx, val in changes.items():
            args = list(ok)
            args[int(idx[1:])] = val
            assert fn(*args) == -1, (fn.__name__, idx, val)

    bad(L.vdn_sobel_ix_iy, sob_ok, a0=None, a1=None, a2=None, a3=0, a4=1, a5=1)
    bad(L.vdn_normal_vector, nv_ok, a0=None, a1=None, a2=0, a3=1, a4=1)
    bad(L.vdn_erode_mask3, er_ok, a0=None, a1=None, a2=-1, a3=1, a4=0)
    bad(L.vdn_normal_eval, ev_ok, a0=None, a1=None, a4=0, a5=1, a6=1, a7=None, a10=None)
    assert L.vdn_normal_vector(*[P + 2 if i == 0 else a for i, a in enumerate(nv_ok)]) == -3     # a float pointer off by 2 bytes
    assert L.vdn_normal_eval(*[P + 4 if i == 10 else a for i, a in enumerate(ev_ok)]) == -3      # a double pointer off by 4
    assert L.vdn_normal_eval(*[65536 if i in (5, 6) else a for i, a in enumerate(ev_ok)]) == -2  # H * W past INT32_MAX
