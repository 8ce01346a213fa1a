"""The batch preparation on the device (csrc/prep.hip, vdn.prep) against the numpy restatement tests/prep_ref.py, which
tests/test_prep_host.py holds to the arrays the reference's own functions recorded.

Bar throughout: np.array_equal(device, restatement, equal_nan=True). Both sides take the same float32 IEEE operations, one
per reference operation, and min / max are exact in any order, so there is no tolerance. The comparison is numeric: the sign
of a zero is not part of the contract. Where two device results are compared with each other, their bytes are."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import prep_ref as R
from test_prep_host import RECORDED, case_id, case_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def same_bits(a, b):
    a, b = (x.detach().cpu().numpy() for x in (a, b))
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def equal(got, want):
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == want.shape, (got.dtype, got.shape, want.shape)
    g = got.cpu().numpy()
    bad = ~((g == want) | (np.isnan(g) & np.isnan(want)))
    print(f"{want.shape}: {int(bad.sum())} of {want.size} elements differ; nan {int(np.isnan(want).sum())}")
    assert np.array_equal(g, want, equal_nan=True)


def run(c, x, mask):
    """The case's composition through vdn.prep; x and mask are torch tensors (any device) or None."""
    from vdn import prep
    op = c["op"]
    if op == "rgb":
        return prep.preprocess_rgb_sequences(x)
    if op == "viz":
        return prep.preprocess_rgb_viz_sequences(x)
    if op == "pre":
        return prep.preprocess_depth_sequences(x, mask, c["norm"])
    if op == "bwn":
        return prep.batch_wise_min_max_norm(x.squeeze(2), None if mask is None else mask.squeeze(2))
    if op == "inv":
        return prep.inverse_depth(x)
    return prep.preprocess_inverse_depth_sequences(x, mask, c["norm"])


@functools.lru_cache(maxsize=None)
def extra(op, shape, mask="bool", special="plain", norm=True, seed=900):
    """A case the reference is not consulted for and the restatement on it, computed once, shared and never written."""
    c = dict(op=op, seed=seed, shape=shape, mask=mask, special=special, norm=norm)
    case = R.make_case(c)
    want = R.restate(c, case)
    for a in (case["x"], case["mask"], want):
        if a is not None:
            a.setflags(write=False)
    return c, case, want


def device_result(op, shape, **kw):
    c, case, want = extra(op, shape, **kw)
    return run(c, dev(case["x"]), dev(case["mask"])), want


@pytest.mark.parametrize("rec", RECORDED, ids=case_id)
def test_recorded_cases(rec):
    _, c, checksum, _ = rec
    case = case_inputs(c, checksum)
    equal(run(c, dev(case["x"]), dev(case["mask"])), R.restate(c, case))


#                                      non-square and odd: one element per lane, two items; whole quads; one pixel per item
@pytest.mark.parametrize("shape", [(2, 3, 1, 17, 13), (1, 2, 1, 16, 16), (2, 2, 1, 1, 1)], ids=str)
@pytest.mark.parametrize("op,mask,special,norm", [("pre", "bool", "negative", True), ("pre", "uint8", "plain", False),
                                                  ("bwn", "none", "negative", True), ("inv", "none", "gt_small", False),
                                                  ("invpre", "bool", "plain", True), ("pre", "bool", "empty_item", True)])
def test_depth_shapes(shape, op, mask, special, norm):
    if shape[-1] == 1 and special == "gt_small":
        special = "plain"                      # one pixel per item: nowhere to plant three values
    equal(*device_result(op, shape, mask=mask, special=special, norm=norm))


#                  35 pixels a plane: an element's channel changes inside a run of four; whole quads; one pixel a plane
@pytest.mark.parametrize("shape", [(2, 2, 3, 5, 7), (1, 2, 3, 4, 4), (1, 3, 3, 1, 1), (1, 1, 3, 2, 6)], ids=str)
@pytest.mark.parametrize("op", ["rgb", "viz"])
def test_rgb_shapes(shape, op):
    equal(*device_result(op, shape, mask="none", special="outside", norm=op == "rgb"))


@pytest.mark.parametrize("trips", [1, 8], ids=["one-trip", "eight-trips"])
@pytest.mark.parametrize("wide", [True, False], ids=["quads", "single"])
def test_past_one_grid_trip(wide, trips):
    """One frame per item, longer than one trip of the grid (and than the eight trips whose loads a lane issues together, which
    sends it round its outer loop again); each item's kept extremes sit in its last four pixels and differ between the items,
    so a lost tail or a leak between the items changes every element."""
    from vdn import prep
    n = trips * prep.trip_elements(wide) + (4 if wide else 5)
    assert (n % 4 == 0) == wide
    rng = np.random.default_rng(77)
    x = rng.uniform(1.0, 2.0, (2, 1, 1, 1, n)).astype(np.float32)
    m = rng.random(x.shape) < 0.7
    x[0, ..., -4:] = (0.5, 3.0, 1.5, 1.5)
    x[1, ..., -4:] = (1.25, 1.5, 5.0, 0.25)
    m[..., -4:] = True
    want, mm = R.prep_depth_ref(x, m, False, True, True)
    assert mm.tolist() == [[0.5, 3.0], [0.25, 5.0]]
    equal(prep.preprocess_depth_sequences(dev(x), dev(m)), want.squeeze(2))
    hw = (trips * prep.trip_elements(wide) // 12 + 1) * 4 + (0 if wide else 1)    # 3 * H * W just past the trips as well
    assert 3 * hw > trips * prep.trip_elements(wide) and (hw % 4 == 0) == wide
    rgb = rng.uniform(-0.5, 1.5, (2, 1, 3, 1, hw)).astype(np.float32)
    equal(prep.preprocess_rgb_sequences(dev(rgb)), R.prep_rgb_ref(rgb, True))


def test_misaligned_pointers():
    """Planes that start 4 bytes past a 16-byte boundary (the mask 1 byte past a 4-byte one) take the one-element path of a
    shape that otherwise takes the quads: the same values."""
    from vdn import prep
    c, case, want = extra("pre", (1, 2, 1, 16, 16), special="negative")
    x, m = dev(case["x"]), dev(case["mask"])
    aligned = prep.preprocess_depth_sequences(x, m)
    buf = torch.empty(x.numel() + 4, dtype=torch.float32, device=DEV)
    mbuf = torch.empty(m.numel() + 4, dtype=torch.bool, device=DEV)
    off = 1 + (-(buf.data_ptr() // 4) % 4)                   # the first element that is 4 bytes past a 16-byte boundary
    xs = buf[off:off + x.numel()].view(x.shape).copy_(x)
    ms = mbuf[1:1 + m.numel()].view(m.shape).copy_(m)
    assert xs.data_ptr() % 16 == 4 and xs.is_contiguous()
    got = prep.preprocess_depth_sequences(xs, ms)
    equal(got, want)
    same_bits(got, aligned)
    same_bits(prep.preprocess_depth_sequences(x, ms), aligned)          # the mask alone off its boundary
    c, case, want = extra("rgb", (1, 2, 3, 4, 4), mask="none", special="outside")
    r = dev(case["x"])
    rbuf = torch.empty(r.numel() + 4, dtype=torch.float32, device=DEV)
    off = 1 + (-(rbuf.data_ptr() // 4) % 4)
    rs = rbuf[off:off + r.numel()].view(r.shape).copy_(r)
    assert rs.data_ptr() % 16 == 4
    equal(prep.preprocess_rgb_sequences(rs), want)
    same_bits(prep.preprocess_rgb_sequences(rs), prep.preprocess_rgb_sequences(r))


def test_views_mask_types_and_host_tensors():
    from vdn import prep
    c, case, want = extra("pre", (2, 3, 1, 17, 13), special="negative")
    x, m = dev(case["x"]), dev(case["mask"])
    base = prep.preprocess_depth_sequences(x, m)
    equal(base, want)
    wide = torch.zeros(2, 3, 1, 17, 26, device=DEV)
    wide[..., ::2] = x
    mwide = torch.zeros(2, 3, 1, 17, 26, dtype=torch.bool, device=DEV)
    mwide[..., ::2] = m
    assert not wide[..., ::2].is_contiguous()
    same_bits(prep.preprocess_depth_sequences(wide[..., ::2], mwide[..., ::2]), base)
    xt = x.permute(1, 0, 2, 3, 4).contiguous().permute(1, 0, 2, 3, 4)                     # a transposed view
    assert not xt.is_contiguous()
    same_bits(prep.preprocess_depth_sequences(xt, m), base)
    for mask in (m.to(torch.uint8), m.to(torch.uint8) * 7, m.to(torch.float32) * 0.5, m.cpu(), torch.from_numpy(case["mask"].copy())):
        same_bits(prep.preprocess_depth_sequences(x, mask), base)
    same_bits(prep.preprocess_depth_sequences(torch.from_numpy(case["x"].copy()), m.cpu()), base)   # host tensors
    same_bits(prep.preprocess_depth_sequences(x.double(), m), base)                       # float32 values held in float64
    same_bits(prep.preprocess_depth_sequences(x, torch.ones_like(m)), prep.preprocess_depth_sequences(x, None))
    c, case, want = extra("rgb", (2, 2, 3, 5, 7), mask="none", special="outside")
    r = dev(case["x"])
    rbase = prep.preprocess_rgb_sequences(r)
    rt = r.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not rt.is_contiguous()
    same_bits(prep.preprocess_rgb_sequences(rt), rbase)
    same_bits(prep.preprocess_rgb_sequences(torch.from_numpy(case["x"].copy())), rbase)


@pytest.mark.parametrize("shape", [(2, 2, 3, 5, 7), (1, 2, 3, 4, 4)], ids=str)
def test_rgb_in_place(shape):
    from vdn.normals import _runtime_for
    rt = _runtime_for(DEV)
    for op in ("rgb", "viz"):
        c, case, want = extra(op, shape, mask="none", special="outside", norm=op == "rgb")
        x = dev(case["x"]).view(-1, 3, *shape[-2:])
        rt.prep_rgb(x, x, op == "rgb")
        equal(x.view(shape), want)


def test_two_runs_give_the_same_bits():
    for args in (("pre", (2, 3, 1, 17, 13)), ("invpre", (1, 2, 1, 16, 16)), ("rgb", (2, 2, 3, 5, 7))):
        c, case, _ = extra(*args, mask="none" if args[0] == "rgb" else "bool", special="outside" if args[0] == "rgb" else "plain")
        x, m = dev(case["x"]), dev(case["mask"])
        same_bits(run(c, x, m), run(c, x, m))


@pytest.mark.parametrize("shape", [(2, 3, 1, 17, 13), (1, 2, 1, 16, 16)], ids=str)
def test_nan_and_inf_under_dropped_pixels_change_nothing(shape):
    from vdn import prep
    c, case, want = extra("pre", shape, special="dropped_nan")
    x, m = case["x"], case["mask"]
    bad = ~np.isfinite(x)
    assert bad.sum() == 3 * shape[0] and not m[bad].any()
    clean = np.where(bad, np.float32(1.0), x)
    got, mm = prep.batch_wise_min_max_norm(dev(x).squeeze(2), dev(m).squeeze(2), return_minmax=True)
    ref, mm_ref = prep.batch_wise_min_max_norm(dev(clean).squeeze(2), dev(m).squeeze(2), return_minmax=True)
    same_bits(mm, mm_ref)
    keep = torch.from_numpy(~bad.squeeze(2))
    same_bits(got.cpu()[keep], ref.cpu()[keep])                       # every other pixel: not a bit changes
    equal(prep.preprocess_depth_sequences(dev(x), dev(m)), want)      # under them: NaN, 1 and 0, as the reference writes


def test_nan_at_a_kept_pixel_stays_in_its_item():
    from vdn import prep
    c, case, want = extra("pre", (2, 3, 1, 17, 13), special="nan_kept")
    x, m = case["x"], case["mask"]
    assert np.isnan(x[0]).sum() == 1 and not np.isnan(x[1]).any()
    got, mm = prep.batch_wise_min_max_norm(dev(x).squeeze(2), dev(m).squeeze(2), return_minmax=True)
    clean, _ = prep.batch_wise_min_max_norm(dev(np.nan_to_num(x, nan=1.0)).squeeze(2), dev(m).squeeze(2), return_minmax=True)
    assert torch.isnan(got[0]).all() and torch.isnan(mm[0]).all()
    same_bits(got[1], clean[1])
    equal(prep.preprocess_depth_sequences(dev(x), dev(m)), want)


@pytest.mark.parametrize("special", ["plain", "empty_item", "constant_item", "nan_kept"])
def test_minmax_output(special):
    from vdn import prep
    c, case, _ = extra("bwn", (2, 3, 1, 17, 13), special=special)
    want, mm = R.prep_depth_ref(case["x"], case["mask"], False, False, True)
    got, got_mm = prep.batch_wise_min_max_norm(dev(case["x"]).squeeze(2), dev(case["mask"]).squeeze(2), return_minmax=True)
    equal(got, want.squeeze(2))
    equal(got_mm, mm)
    if special == "empty_item":
        assert got_mm[1].tolist() == [np.inf, -np.inf] and not got[1].any() and not torch.signbit(got[1]).any()


@pytest.mark.parametrize("shape", [(2, 3, 1, 17, 13), (1, 2, 1, 16, 16)], ids=str)
def test_fused_reciprocal_normalise(shape):
    from vdn import prep
    c, case, want = extra("invpre", shape, special="gt_small")
    x, m = dev(case["x"]), dev(case["mask"])
    fused = prep.preprocess_inverse_depth_sequences(x, m)
    equal(fused, want)
    inv = prep.inverse_depth(x)
    same_bits(fused, prep.batch_wise_min_max_norm(inv.squeeze(2), m.squeeze(2)))
    same_bits(fused, prep.preprocess_depth_sequences(inv, m))
    same_bits(prep.preprocess_inverse_depth_sequences(x, m, False), inv.squeeze(2))
