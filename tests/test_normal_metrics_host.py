"""vdn.normal_metrics and vdn.vis.colorize_normals without a device: the restatement the GPU tests compare with
(tests/normal_angle_ref.py) on values worked out by hand, the public surface, every argument error (raised with CPU tensors
before a device is looked for), and the agreement of header, binding table and library on the new entry points."""
from __future__ import annotations

import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import normal_angle_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vdn_normal_angle_map", "vdn_normal_angle_stats_workspace_bytes", "vdn_normal_angle_stats", "vdn_normal_colorize")


def px(*v):
    """One pixel: the vector v as [3, 1, 1]."""
    return np.array(v, np.float64).reshape(3, 1, 1)


def angle(a, b):
    return float(A.angle_ref(px(*a), px(*b))[0, 0])


# ------------------------------------------------------------------------------------------------ the restatement
def test_angle_on_hand_values():
    assert angle((0.3, -0.2, 0.9), (0.6, -0.4, 1.8)) == 0.0            # parallel, any length
    assert angle((0.25, 0.5, -1.0), (-0.5, -1.0, 2.0)) == 180.0        # antiparallel: exactly 180
    assert abs(angle((1, 0, 0), (1, 1, 0)) - 45.0) <= 1e-13
    assert abs(angle((0, 0, 2), (0, 3, 0)) - 90.0) <= 1e-13
    assert angle((0, 0, 0), (0, 0, 1)) == 90.0 and angle((0, 1, 0), (0, 0, 0)) == 90.0    # a zero vector: 90
    for bad in (np.nan, np.inf, -np.inf):
        assert np.isnan(angle((bad, 0, 1), (0, 0, 1))) and np.isnan(angle((0, 0, 1), (0, bad, 1)))
        assert np.isnan(angle((bad, 0, 1), (0, 0, 0)))                 # not finite wins over the zero vector


def test_small_angle_keeps_its_digits_where_acos_gives_zero():
    a = np.array([0.25, -0.5, 1.0])
    e = np.array([1.0, 0.5, -0.75])
    b = (a.astype(np.float32).astype(np.float64) + 1e-7 * e).astype(np.float32).astype(np.float64)   # float32 inputs
    eperp = (b - a) - ((b - a) @ a) / (a @ a) * a                      # what the rounding to float32 left of 1e-7 e, across a
    want = np.sqrt(eperp @ eperp) / np.sqrt(a @ a) * 180.0 / np.pi
    got = angle(a, b)
    assert want > 1e-6 and abs(got - want) <= 1e-6 * want, (got, want)
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    cos32 = np.float32(a32 @ b32) / (np.sqrt(np.float32(a32 @ a32)) * np.sqrt(np.float32(b32 @ b32)))
    lost = float(np.degrees(np.arccos(np.minimum(cos32, np.float32(1.0)))))   # acos of the float cosine: 0, or the last bit's 0.02
    assert lost == 0.0 or lost > 1000 * want, lost


def test_from_depth_target_is_the_unnormalised_stencil():
    d = np.array([[[1.0, 2.0, 4.0], [2.0, 3.0, 5.0], [4.0, 5.0, 9.0]]], np.float32)
    n = A.depth_normal_ref(d)
    ix, iy = A.R.sobel_ref(d)
    assert n.shape == (1, 3, 3, 3) and np.array_equal(n[0, 0], -ix[0]) and np.array_equal(n[0, 1], -iy[0]) and (n[0, 2] == 1).all()
    # the centre: Ix = ((1-4) + 2 (2-5) + (4-9)) / 8, Iy = ((1-4) + 2 (2-5) + (4-9)) / 8
    assert n[0, 0, 1, 1] == 14 / 8 and n[0, 1, 1, 1] == 14 / 8
    unit = A.R.normal_vector_ref(d)
    assert np.abs(A.angle_ref(n, unit)).max() <= 1e-6                  # the same direction as normal_vector's


def test_rows_medians_and_empty_and_nan_sets():
    ang = np.array([[[[1.0, 4.0, 6.0, 40.0]], [[2.0, 2.0, 8.0, 20.0]]]])      # [1, 2, 1, 4]
    keep = np.ones_like(ang, bool)
    rows = A.stats_ref(ang, keep)
    assert rows.shape == (4, 9)
    assert rows[2].tolist() == [4.0, 12.75, 5.0, np.sqrt((1 + 16 + 36 + 1600) / 4), 0.5, 0.75, 0.75, 0.75, 0.75]   # even n: (4 + 6) / 2
    assert rows[3, 2] == 5.0 and rows[3, 4] == 0.5                     # ties below the middle: (2 + 8) / 2
    assert rows[0, 0] == 8 and rows[0, 2] == 5.0 and np.array_equal(rows[0], rows[1])   # one item: the batch
    keep[0, 1, 0, 3] = False
    odd = A.stats_ref(ang, keep)
    assert odd[3, 0] == 3 and odd[3, 2] == 2.0 and odd[0, 2] == 4.0    # odd n: the middle value itself (1 2 2 4 6 8 40)
    assert A.row_ref(np.array([5.0]), np.array([True]))[4:] == [0.0, 1.0, 1.0, 1.0, 1.0]   # strict comparisons
    # the median is taken over the angles rounded to float32
    v = np.array([1.0 + 2.0 ** -30, 3.0])
    assert A.row_ref(v, np.ones(2, bool))[2] == 2.0 and A.row_ref(v, np.ones(2, bool))[1] > 2.0
    keep[0, 0] = False
    empty = A.stats_ref(ang, keep)
    assert empty[2, 0] == 0 and np.isnan(empty[2, 1:]).all() and not np.isnan(empty[3]).any()
    ang[0, 1, 0, 0] = np.nan
    keep[:] = True
    nan = A.stats_ref(ang, keep)
    assert nan[3, 0] == 4 and np.isnan(nan[3, 1:]).all() and np.isnan(nan[0, 1:]).all() and np.array_equal(nan[2], rows[2])


def test_dropped_pixels_are_selected_away():
    c = A.make_case(3, (1, 2, 6, 7))
    pred = c["pred"].copy()
    ang, keep = A.angle_map_ref(pred, c["target"], c["mask"])
    assert keep.sum() < c["mask"].sum() <= keep.size and np.array_equal(keep, A.R.erode_ref(c["mask"]))
    pred[np.broadcast_to(~keep[:, :, None], pred.shape)] = np.nan
    ang2, _ = A.angle_map_ref(pred, c["target"], c["mask"])
    assert np.array_equal(ang, ang2, equal_nan=True) and np.isnan(ang[~keep]).all() and not np.isnan(ang[keep]).any()
    plain, kept = A.angle_map_ref(c["pred"], c["target"], c["mask"], erode=False)
    assert np.array_equal(kept, c["mask"]) and np.array_equal(plain[keep], ang[keep])


def test_cases_span_every_threshold():
    c = A.make_case(11, (2, 3, 12, 14))
    ang, keep = A.angle_map_ref(c["pred"], c["target"], None)
    assert ang.min() < 5.0 and ang.max() > 30.0 and ang.max() < 60.0
    rows = A.stats_ref(ang, keep)
    assert (np.diff(rows[0, 4:]) > 0).all() and 0 < rows[0, 4] and rows[0, 8] < 1
    again = A.make_case(11, (2, 3, 12, 14))
    assert all(np.array_equal(c[k], again[k]) for k in c)


def test_picture_bytes():
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0]], np.float32)
    x = (axes * np.array([[0.5], [3], [1], [7], [0.25], [2], [1]], np.float32)).T.reshape(1, 3, 1, 7)   # any length
    byte, v = A.colorize_ref(x)
    assert byte.shape == (1, 1, 7, 3)
    assert byte[0, 0].tolist() == [[255, 128, 128], [0, 128, 128], [128, 255, 128], [128, 0, 128], [128, 128, 255], [128, 128, 0],
                                   [128, 128, 128]]
    assert v[0, 0, 0].tolist() == [255.0, 127.5, 127.5] and np.isnan(v[0, 0, 6]).all()
    assert A.colorize_ref(x, bgr=True)[0][0, 0, 4].tolist() == [255, 128, 128]
    x[0, 1, 0, 2] = np.inf
    assert A.colorize_ref(x)[0][0, 0, 2].tolist() == [128, 128, 128]
    flat = np.full((1, 4, 5), 3.0, np.float32)                          # a constant depth: the normal is +z
    assert (A.colorize_ref(flat, from_depth=True)[0] == np.array([128, 128, 255], np.uint8)).all()


def test_from_depth_picture_differs_from_the_stored_normals_within_the_cap():
    """colorize_ref(from_depth) against colorize_ref(normal_vector_ref rounded to float32): the bytes differ only where that
    rounding crosses a half-integer, fewer than 1e-4 of them at the GPU test's seed and shape."""
    depth = A.make_depth(29, (1, 2, 64, 67))[0]
    a, _ = A.colorize_ref(depth, from_depth=True)
    b, _ = A.colorize_ref(A.R.normal_vector_ref(depth).astype(np.float32))
    differ = int((a != b).sum())
    print(f"bytes that differ: {differ} of {a.size}")
    assert differ <= 1e-4 * a.size and int(np.abs(a.astype(int) - b.astype(int)).max()) <= 1


# ------------------------------------------------------------------------------------------------ the public surface
def test_names_and_signatures():
    import vdn
    from vdn import normal_metrics as M, steps, vis
    assert vdn.normal_metrics is M
    assert M.normal_metric_names == ["n", "mean", "median", "rmse", "a5", "a7_5", "a11_25", "a22_5", "a30"] == A.NAMES
    for fn in (M.angular_error_map, M.angular_error, M.angular_error_values):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["prediction", "target", "mask", "from_depth", "erode", "device"], fn.__name__
        assert [sig.parameters[k].default for k in ("mask", "from_depth", "erode", "device")] == [None, False, True, "cuda"]
        assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("from_depth", "erode", "device"))
    sig = inspect.signature(vis.colorize_normals)
    assert list(sig.parameters) == ["normals", "from_depth", "order", "device"]
    assert [sig.parameters[k].default for k in ("from_depth", "order", "device")] == [False, "rgb", "cuda"]
    sig = inspect.signature(steps.evaluate_normals_step)
    assert list(sig.parameters) == ["model", "batch", "meter", "erode", "input_key", "device"]
    assert [sig.parameters[k].default for k in ("meter", "erode", "input_key", "device")] == [None, True, "depth_anything_v2", "cuda"]


def test_argument_errors_are_raised_before_any_device():
    from vdn import normal_metrics as M, vis
    p, m = torch.zeros(2, 3, 3, 4, 5), torch.ones(2, 3, 4, 5)
    for fn in (M.angular_error_map, M.angular_error, M.angular_error_values):
        with pytest.raises(ValueError, match="prediction must be"):
            fn(torch.zeros(2, 3, 4, 5), p)
        with pytest.raises(ValueError, match="prediction must be"):
            fn(torch.zeros(2, 3, 2, 4, 5), p)
        with pytest.raises(ValueError, match="prediction must be"):
            fn(p.numpy(), p)
        with pytest.raises(ValueError, match="target shape"):
            fn(p, torch.zeros(2, 3, 3, 4, 6))
        with pytest.raises(ValueError, match="target shape"):
            fn(p, m)                                                    # a depth map without from_depth
        with pytest.raises(ValueError, match="target must be"):
            fn(p, None)
        with pytest.raises(ValueError, match="gt_depth must be"):
            fn(p, p, from_depth=True)
        with pytest.raises(ValueError, match="gt_depth must be"):
            fn(p, [1.0], from_depth=True)
        with pytest.raises(ValueError, match="mask shape"):
            fn(p, p, torch.ones(2, 3, 1, 4, 5))
        with pytest.raises(ValueError, match="mask must be"):
            fn(p, p, 1)
        with pytest.raises(ValueError, match="empty"):
            fn(torch.zeros(0, 3, 3, 4, 5), torch.zeros(0, 3, 3, 4, 5))
        with pytest.raises(ValueError, match="at least 2"):
            fn(torch.zeros(1, 1, 3, 1, 5), torch.zeros(1, 1, 3, 1, 5))
    with pytest.raises(ValueError, match="order"):
        vis.colorize_normals(p, order="xyz")
    with pytest.raises(ValueError, match="torch tensor"):
        vis.colorize_normals(p.numpy())
    with pytest.raises(ValueError, match="normals must be"):
        vis.colorize_normals(torch.ones(2, 4, 4, 5))
    with pytest.raises(ValueError, match="normals must be"):
        vis.colorize_normals(torch.zeros(3, 4, 5))
    with pytest.raises(ValueError, match="depth must be"):
        vis.colorize_normals(p, from_depth=True)
    with pytest.raises(ValueError, match="at least 2"):
        vis.colorize_normals(torch.zeros(2, 1, 5), from_depth=True)
    with pytest.raises(ValueError, match="empty"):
        vis.colorize_normals(torch.zeros(0, 3, 4, 5))


def test_there_is_no_cpu_path():
    from vdn import _abi, normal_metrics as M, vis
    p = torch.zeros(1, 2, 3, 4, 5)
    for fn in (M.angular_error_map, M.angular_error, M.angular_error_values):
        with pytest.raises(_abi.VdnError, match="no CPU path"):
            fn(p, p, device="cpu")
    with pytest.raises(_abi.VdnError, match="no CPU path"):
        vis.colorize_normals(p, device="cpu")


# ------------------------------------------------------------------------------------------------ header, table, library
def test_header_bindings_and_library_agree():
    from vdn import _abi
    with open(os.path.join(ROOT, "include", "vdn.h")) as f:
        hdr = f.read()
    for s in SYMBOLS:
        m = re.search(r"\b(int|size_t) " + s + r"\(([^;]*)\);", hdr)
        assert m, s
        assert len(m.group(2).split(",")) == len(_abi.EXPORTS[s][1]), s
        assert _abi.EXPORTS[s][0] is (ctypes.c_int if m.group(1) == "int" else ctypes.c_size_t), s
        assert getattr(_abi.lib, s).argtypes == _abi.EXPORTS[s][1]
    from vdn._build import SOURCES
    assert "normal_metrics.hip" in SOURCES


def test_entry_points_reject_bad_arguments_without_launch():
    from vdn import _abi
    L = _abi.lib
    p, odd2, odd4 = ctypes.c_void_p(256), ctypes.c_void_p(258), ctypes.c_void_p(260)
    EINVAL, EUNSUP = -1, -2
    assert L.vdn_normal_angle_map(None, p, 0, None, 1, 1, 4, 4, p, None) == EINVAL
    assert L.vdn_normal_angle_map(p, None, 0, None, 1, 1, 4, 4, p, None) == EINVAL
    assert L.vdn_normal_angle_map(p, p, 0, None, 1, 1, 4, 4, None, None) == EINVAL
    assert L.vdn_normal_angle_map(p, p, 0, None, 1, 0, 4, 4, p, None) == EINVAL
    assert L.vdn_normal_angle_map(p, p, 0, None, 1, 1, 1, 4, p, None) == EINVAL
    assert L.vdn_normal_angle_map(p, p, 1, None, 1, 1, 4, 1, p, None) == EINVAL
    assert L.vdn_normal_angle_map(p, p, 0, None, 1, 1, 65536, 65536, p, None) == EUNSUP
    assert L.vdn_normal_angle_map(p, p, 0, None, 1, 65536, 4, 4, p, None) == EUNSUP
    ealign = L.vdn_normal_angle_map(odd2, p, 0, None, 1, 1, 4, 4, p, None)
    assert ealign not in (0, EINVAL, EUNSUP) and ealign > -1000
    assert L.vdn_normal_angle_map(p, p, 0, None, 1, 1, 4, 4, odd2, None) == ealign
    assert L.vdn_normal_angle_stats(p, p, 0, None, 1, 1, 1, 4, 4, None, p, None) == EINVAL
    assert L.vdn_normal_angle_stats(p, p, 0, None, 1, 1, 1, 4, 4, p, None, None) == EINVAL
    assert L.vdn_normal_angle_stats(None, p, 0, None, 1, 1, 1, 4, 4, p, p, None) == EINVAL
    assert L.vdn_normal_angle_stats(p, p, 0, None, 1, 0, 1, 4, 4, p, p, None) == EINVAL
    assert L.vdn_normal_angle_stats(p, p, 0, None, 1, 1, 1, 4, 1, p, p, None) == EINVAL
    assert L.vdn_normal_angle_stats(p, p, 0, None, 1, 256, 256, 4, 4, p, p, None) == EUNSUP      # B T > 65535
    assert L.vdn_normal_angle_stats(p, p, 0, None, 1, 1, 1, 65536, 65536, p, p, None) == EUNSUP
    assert L.vdn_normal_angle_stats(p, p, 0, None, 1, 1, 4, 32768, 32768, p, p, None) == EUNSUP  # 2^32 pixels in the batch
    assert L.vdn_normal_angle_stats(p, p, 0, None, 1, 1, 1, 4, 4, odd4, p, None) == ealign       # workspace off 8 bytes
    assert L.vdn_normal_angle_stats(p, p, 0, None, 1, 1, 1, 4, 4, p, odd4, None) == ealign
    assert L.vdn_normal_angle_stats(p, odd2, 0, None, 1, 1, 1, 4, 4, p, p, None) == ealign
    assert L.vdn_normal_angle_stats_workspace_bytes(0, 1, 4, 4) == 0 and L.vdn_normal_angle_stats_workspace_bytes(256, 256, 4, 4) == 0
    small, large = L.vdn_normal_angle_stats_workspace_bytes(1, 1, 2, 2), L.vdn_normal_angle_stats_workspace_bytes(2, 3, 8, 8)
    assert 0 < small < large and small % 8 == 0 and large % 8 == 0
    assert L.vdn_normal_colorize(None, 0, 0, p, 1, 4, 4, None) == EINVAL
    assert L.vdn_normal_colorize(p, 0, 0, None, 1, 4, 4, None) == EINVAL
    assert L.vdn_normal_colorize(p, 0, 0, p, 0, 4, 4, None) == EINVAL
    assert L.vdn_normal_colorize(p, 1, 0, p, 1, 1, 4, None) == EINVAL
    assert L.vdn_normal_colorize(p, 0, 0, p, 1, 65536, 65536, None) == EUNSUP
    assert L.vdn_normal_colorize(odd2, 0, 0, p, 1, 4, 4, None) == ealign
