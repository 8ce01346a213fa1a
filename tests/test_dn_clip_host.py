"""Host side of the depth + normal model's clip driver (VideoDepthEstimationModel.infer_video): the window table and the
numpy restatement of the stitch in vdn.util against tests/dn_clip_ref.py, the overlap rule, and the refusals that need no GPU."""
import numpy as np
import pytest
import torch

import dn_clip_ref as R

CONFIGS = [(4, 2), (6, 3), (16, 4), (16, 0)]


@pytest.mark.parametrize("S,overlap", CONFIGS)
def test_window_table_is_the_brute_force_table(S, overlap):
    from vdn import util
    step = S - overlap
    for N in range(1, 3 * S + 1):
        table = util.dn_window_table(N, S, overlap)
        assert table == R.window_table(N, S, overlap), (N, S, overlap)
        assert all(len(row) == S for row in table)
        assert [row[0] for row in table] == [k * step for k in range(len(table))]      # starts 0, step, 2 step, ..
        seen = [sum(f in row for row in table) for f in range(N)]                       # windows a frame lies in
        assert min(seen) >= 1, (N, "a frame is in no window")
        assert max(seen) <= 2, (N, "a frame is in three windows")
        covered = set(table[0])
        for row in table[1:]:
            assert set(row) - covered, (N, "a later window brings no new frame")
            covered |= set(row)
        for k, row in enumerate(table):
            for i, f in enumerate(row):
                assert f == (k * step + i if k * step + i < N else N - 1)                 # pad slots show the last frame


def test_overlap_rule():
    from vdn import util
    assert util.dn_check_overlap(16, None) == 4 and util.dn_check_overlap(8, None) == 2
    assert util.dn_check_overlap(16, 0) == 0 and util.dn_check_overlap(16, 8) == 8 and util.dn_check_overlap(4, 2) == 2
    for S, ov in [(16, 1), (16, 9), (16, -1), (4, 3), (16, 2.5), (16, True), (4, None)]:   # S // 4 = 1 is no overlap either
        with pytest.raises(ValueError):
            util.dn_check_overlap(S, ov)
    with pytest.raises(ValueError):
        util.dn_window_table(0, 4, 2)


def _windows(N, S, overlap, H, W, seed, signed):
    rng = np.random.default_rng(seed)
    table = R.window_table(N, S, overlap)
    base = rng.normal(size=(N, H, W)) + (0.0 if signed else 3.0)
    depths, normals = [], []
    for k, row in enumerate(table):   # every window sees the clip through an affine map of its own, plus noise
        a, b = 1.0 + 0.2 * k, (-0.3 * k if signed else 0.1 * k)
        depths.append((a * base[row] + b + 0.05 * rng.normal(size=(S, H, W))).astype(np.float32))
        n = rng.normal(size=(S, 3, H, W)).astype(np.float32)
        n[:, 2] = 1
        normals.append(n)
    return depths, normals


@pytest.mark.parametrize("clamp0", [False, True])
@pytest.mark.parametrize("S,overlap,N,align", [(4, 2, 7, True), (6, 3, 11, True), (16, 4, 41, True), (4, 0, 9, True), (6, 3, 11, False),
                                              (4, 2, 3, True)])
def test_dn_stitch_float32_against_float64(S, overlap, N, align, clamp0):
    """util.dn_stitch evaluates in float32 what dn_clip_ref.stitch64 evaluates in float64, the rule for normals and the clamp
    included. Bar: 1e-5 of the largest value. A result takes a fit (sums of at most 4 * 35 float32 products, conditioning
    asserted below: relative error of a few 1e-6), one multiply-add and one blend, each with a 6e-8 rounding, per window, and
    the error of a window enters the next fit once: a few 1e-6 for the three or four windows here."""
    from vdn import util
    depths, normals = _windows(N, S, overlap, 5, 7, seed=S * 100 + N, signed=clamp0)
    d, n, c = util.dn_stitch(depths, normals, N, overlap, align=align, clamp0=clamp0)
    d64, n64, c64, fits = R.stitch64(depths, normals, N, overlap, align=align, clamp0=clamp0)
    assert d.dtype == n.dtype == c.dtype == np.float32 and d.shape == (N, 5, 7) and n.shape == (N, 3, 5, 7)
    assert len(fits) == (len(depths) - 1 if align and overlap else 0)
    for det, s0, s2 in fits:
        assert det >= 0.05 * s0 * s2
    if not (align and overlap):
        assert np.array_equal(c, np.tile(np.float32([1, 0]), (len(depths), 1)))
    if clamp0:
        assert (d64 == 0).any() and (d64 > 0).any() and (d >= 0).all()     # the clamp cuts some values and not others
    for name, g, w in (("depth", d, d64), ("normal", n, n64), ("coefs", c, c64)):
        assert np.isfinite(w).all(), name
        err = np.abs(g - w).max() / np.abs(w).max()
        assert err < 1e-5, (name, err)
    assert (n[:, 2] == 1).all()
    if len(depths) > 1 and align and overlap:                            # normals follow the depth's scale, not its shift
        k = len(depths) - 1
        start, keep = k * (S - overlap), min(S, N - k * (S - overlap))
        assert np.array_equal(n[start + overlap:start + keep, 0], (normals[k][overlap:keep, 0] * c[k, 0]).astype(np.float32))


def _cpu_model():
    import vdn
    from vdn import synth
    sizes = ((8, 8), (4, 4), (2, 2), (1, 1))
    return vdn.VideoDepthEstimationModel(8, trunk=synth.dn_trunk(sizes=sizes), img_trunk=synth.dn_trunk(sizes=sizes))


@pytest.mark.parametrize("case", ["rank", "frames_rank", "n_mismatch", "hw_mismatch", "n0", "bool", "complex", "numpy_bool", "list",
                                  "overlap1", "overlap5"])
def test_refusals_come_before_the_device(case):
    """Every malformed call raises ValueError while the model still sits on the CPU: no runtime exists, nothing was launched."""
    m = _cpu_model()
    d, f, kw = torch.zeros(5, 32, 32), torch.zeros(5, 3, 32, 32), {}
    if case == "rank":
        d = d[None]
    elif case == "frames_rank":
        f = f[:, 0]
    elif case == "n_mismatch":
        f = f[:4]
    elif case == "hw_mismatch":
        f = torch.zeros(5, 3, 32, 30)
    elif case == "n0":
        d, f = d[:0], f[:0]
    elif case == "bool":
        d = d.bool()
    elif case == "complex":
        f = f.to(torch.complex64)
    elif case == "numpy_bool":
        d = np.zeros((5, 32, 32), bool)
    elif case == "list":
        d = d.tolist()
    elif case == "overlap1":
        kw = dict(overlap=1)
    elif case == "overlap5":
        kw = dict(overlap=5)     # sequence_length // 2 = 4
    for call in (m.infer_video, m.infer_video_vis):
        with pytest.raises(ValueError):
            call(d, f, **kw)
    assert m._eng is None
    from vdn._abi import VdnError
    with pytest.raises(VdnError):     # a well-formed call gets as far as the runtime, which has no CPU path
        m.infer_video(torch.zeros(5, 32, 32), torch.zeros(5, 3, 32, 32), overlap=4)


def test_abi_entry_is_declared_and_bound():
    import ctypes
    from vdn import _abi
    res, params = _abi.EXPORTS["vdn_dn_stitch_apply"]
    assert res is ctypes.c_int and len(params) == 11 and params[5] is ctypes.c_size_t
    assert hasattr(_abi.lib, "vdn_dn_stitch_apply")
