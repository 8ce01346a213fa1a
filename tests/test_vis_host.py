"""Host-side checks of the colourised depth output (vdn.vis, csrc/vis.hip): the palette literals, the VDN_EINVAL / VDN_EALIGN
paths of the two entry points, and that the numpy restatement tests/vis_ref.py tells the reference's choices from their
neighbours. Nothing here launches a kernel."""
from __future__ import annotations

import numpy as np
import pytest

import vis_ref as R


def test_palette_literals_equal_the_fixture():
    from vdn._palettes import PALETTES
    gold = R.tables()
    assert sorted(PALETTES) == sorted(gold) == ["Spectral", "Spectral_r", "inferno"]
    for name, t in gold.items():
        assert t.shape == (256, 3) and t.dtype == np.uint8
        assert len(PALETTES[name]) == 768 and all(isinstance(v, int) and 0 <= v <= 255 for v in PALETTES[name])
        assert np.array_equal(np.array(PALETTES[name], np.uint8).reshape(256, 3), t), name
    # matplotlib interpolates the reversed map on its own: after truncation it is close to, not equal to, the flipped table
    assert (gold["Spectral_r"] != gold["Spectral"]).any()
    assert np.abs(gold["Spectral_r"].astype(int) - gold["Spectral"][::-1].astype(int)).max() <= 1


def test_palettes_equal_the_generating_expressions():
    matplotlib = pytest.importorskip("matplotlib")
    gold = R.tables()
    idx = np.arange(256, dtype=np.uint8)
    for name in ("Spectral_r", "Spectral"):
        cmap = matplotlib.colormaps.get_cmap(name)
        assert np.array_equal((cmap(idx)[:, :3] * 255).astype(np.uint8), gold[name]), name
    inferno = (np.array(matplotlib.colormaps.get_cmap("inferno").colors) * 255).astype(np.uint8)
    assert np.array_equal(inferno, gold["inferno"])
    # the per-pixel cmap call of run.py:65 is the table lookup vis_ref makes of it
    d = np.arange(256, dtype=np.uint8).reshape(16, 16)
    cmap = matplotlib.colormaps.get_cmap("Spectral_r")
    assert np.array_equal((cmap(d)[:, :, :3] * 255)[:, :, ::-1].astype(np.uint8), gold["Spectral_r"][d][:, :, ::-1])


def test_vis_entry_points_reject_bad_arguments():
    from vdn import _abi
    L, P = _abi.lib, 4096                                   # P: a non-null, aligned stand-in; nothing is launched
    assert L.vdn_minmax_workspace_bytes(0) == 0 and L.vdn_minmax_workspace_bytes(-1) == 0
    sizes = [L.vdn_minmax_workspace_bytes(g) for g in range(1, 40)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and all(s % 4 == 0 for s in sizes)
    mm_ok = [P, 3, 12, P, P, None]
    # depth, minmax, per_frame, lut, ch, raw, margin, out, N, H, W, stream
    col_ok = [P, P, 1, P, 3, None, 0, P, 2, 3, 4, None]
    raw_ok = [P, P, 1, P, 3, P, 50, P, 2, 3, 4, None]

    def bad(fn, ok, **changes):
        for idx, val in changes.items():
            args = list(ok)
            args[int(idx[1:])] = val
            assert fn(*args) == -1, (fn.__name__, idx, val)

    bad(L.vdn_minmax_f32, mm_ok, a0=None, a1=0, a2=0, a3=None, a4=None)
    bad(L.vdn_minmax_f32, mm_ok, a1=-2)
    bad(L.vdn_colorize, col_ok, a0=None, a1=None, a3=None, a4=2, a7=None, a8=0, a9=0, a10=0)
    bad(L.vdn_colorize, col_ok, a4=0, a8=-1, a9=-1, a10=-5)
    bad(L.vdn_colorize, raw_ok, a4=1, a6=-1)                # raw with one channel; a negative margin
    for i in (0, 3, 4):                                     # a float / workspace pointer off by 2 bytes
        assert L.vdn_minmax_f32(*[P + 2 if k == i else a for k, a in enumerate(mm_ok)]) == -3, i
    for i in (0, 1):
        assert L.vdn_colorize(*[P + 2 if k == i else a for k, a in enumerate(col_ok)]) == -3, i


def test_wrapper_argument_errors():
    """Every ValueError comes before the device is touched; a CPU tensor is refused like everywhere in the package."""
    import torch
    from vdn import vis
    d = torch.ones(2, 3, 4)
    with pytest.raises(ValueError, match="palette"):
        vis.colorize(d, palette="viridis")
    with pytest.raises(ValueError, match="order"):
        vis.colorize(d, order="gbr")
    with pytest.raises(ValueError, match="scope"):
        vis.colorize(d, scope="window")
    with pytest.raises(ValueError, match="scope"):
        vis.minmax(d, scope="window")
    with pytest.raises(ValueError, match="gray_channels"):
        vis.colorize(d, grayscale=True, gray_channels=2)
    with pytest.raises(Exception, match="no CPU path"):
        vis.colorize(d)
    with pytest.raises(Exception, match="no CPU path"):
        vis.minmax(d)


def teeth_input():
    """[3, 5, 7] in [0.1, 80] with distinct per-frame ranges: frame f spans [0.1 + 3 f, 80 - 20 f]."""
    rng = np.random.default_rng(20240607)
    u = rng.random((3, 5, 7))
    d = np.empty((3, 5, 7), np.float32)
    for f in range(3):
        lo, hi = 0.1 + 3.0 * f, 80.0 - 20.0 * f
        d[f] = (lo + (hi - lo) * u[f]).astype(np.float32)
        d[f].reshape(-1)[f] = lo
        d[f].reshape(-1)[-1 - f] = hi
    raw = rng.integers(0, 256, (3, 5, 7, 3), dtype=np.uint8)
    return d, raw


def test_vis_ref_has_teeth():
    """On one fixed input each neighbouring choice changes at least one output byte of the restatement: rounding instead
    of truncating, the clip's min/max instead of the frame's, RGB instead of BGR, Spectral instead of Spectral_r."""
    d, raw = teeth_input()
    assert d.min() >= np.float32(0.1) and d.max() <= np.float32(80)
    T = R.tables()
    want = np.stack([R.run_frame(d[f], raw[f], True, False, T["Spectral_r"]) for f in range(3)])
    assert want.shape == (3, 5, 7, 3) and want.dtype == np.uint8

    def frame_variant(f, rounding=False, clip=False, rgb=False, table="Spectral_r"):
        mn, mx = (d.min(), d.max()) if clip else (d[f].min(), d[f].max())
        x = (d[f] - mn) / (mx - mn) * 255.0
        idx = (np.rint(x) if rounding else x).astype(np.uint8)
        out = T[table][idx]
        return out if rgb else out[:, :, ::-1]

    same = np.stack([frame_variant(f) for f in range(3)])
    assert np.array_equal(same, want), "the variant builder itself restates run_frame"
    for kw in (dict(rounding=True), dict(clip=True), dict(rgb=True), dict(table="Spectral")):
        other = np.stack([frame_variant(f, **kw) for f in range(3)])
        assert (other != want).any(), kw
    # the concatenated form: raw verbatim, 50 columns of 255, then the depth picture
    full = R.run_frame(d[1], raw[1], False, False, T["Spectral_r"])
    assert full.shape == (5, 7 + 50 + 7, 3)
    assert np.array_equal(full[:, :7], raw[1]) and (full[:, 7:57] == 255).all() and np.array_equal(full[:, 57:], want[1])
    grey = R.run_frame(d[1], raw[1], True, True, T["Spectral_r"])
    assert grey.shape == (5, 7, 3) and (grey[..., 0] == grey[..., 1]).all() and (grey[..., 0] == grey[..., 2]).all()
    # save_video: clip-wide range, RGB, inferno; the grey form is the index itself
    sv = R.save_video_frames(d, False, T["inferno"])
    idx = R.save_video_frames(d, True, T["inferno"])
    assert sv.shape == (3, 5, 7, 3) and idx.shape == (3, 5, 7) and np.array_equal(sv, T["inferno"][idx])
    assert idx.min() == 0 and idx.max() == 255
    per_frame = np.stack([R.run_frame(d[f], raw[f], True, True, None)[..., 0] for f in range(3)])
    assert (per_frame != idx).any()
