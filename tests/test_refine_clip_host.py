"""The depth refiners' clip driver without a GPU: the fixtures RC5_vits / RC3_vits / RC2_vits (the imported reference's
`forward`, `compute_scale_and_shift` and `get_interpolate_frames` joined by the loop of v5:215-283 on depth windows,
tools/make_golden_refine_clip.py) against the CPU restatement tests/refine_clip_ref.restate, the conditions that make the
fixtures worth having, the public surface, and the slot tables vdn_refine_window_tail indexes the clip with."""
import importlib

import numpy as np
import pytest

import refine_clip_ref as RC
from common import rel_l2


@pytest.mark.parametrize("name", list(RC.FIXTURES))
def test_fixture_agrees_with_the_restatement_and_its_clamp_acts(name):
    """<= 1e-5 (rel-L2, the fixture tool's measure) between what the reference's halves wrote and per-window forward
    restatement + vdn.util.stitch. v3 / v5: the stitcher's clamp acts on the later windows (exact zeros among the frames >= 32
    between 0.5 % and 50 %), on the fixture alone. v2: each ReLU of final_res clips 5 % .. 95 %, the second on the fixture's
    frames in front of the first cross-fade (window 0 as `forward` gave it), the first on the restatement's trace."""
    g, version, clip, sd = RC.fixture(name)
    out = g["out"]
    assert out.shape == clip.shape == (50, *clip.shape[1:]) and out.dtype == np.float32 and np.isfinite(out).all() and (out[32:] >= 0).all()
    traces = []
    mine, per_window = RC.restate(sd, clip, "vits", version, traces)
    e = rel_l2(mine, out)
    print(f"[{name}] restatement vs fixture rel-L2 {e:.2e}")
    assert per_window.shape[0] == 3 and e <= 1e-5
    if version == 2:
        clipped, zero = float((traces[0]["pre_relu1"] < 0).float().mean()), float((out[:RC.RAW] == 0).mean())
        print(f"[{name}] first ReLU clips {clipped:.3f} of window 0, outputs exactly zero {zero:.3f} of the frames < {RC.RAW}")
        assert np.array_equal(out[:RC.RAW], per_window[0][:RC.RAW]) or rel_l2(per_window[0][:RC.RAW], out[:RC.RAW]) <= 1e-5
        assert RC.RELU_SHARE[0] <= clipped <= RC.RELU_SHARE[1] and RC.RELU_SHARE[0] <= zero <= RC.RELU_SHARE[1]
    else:
        z = RC.zero_share(out)
        print(f"[{name}] exact zeros among the frames >= 32: {z:.4f}")
        assert RC.ZERO_SHARE[0] <= z <= RC.ZERO_SHARE[1]
        assert RC.FIXTURES[name][2] in {k[3:] for k in g.files if k.startswith("sd/")}   # the shifted bias travels with the fixture


@pytest.mark.parametrize("version", [2, 3, 4, 5])
def test_every_refiner_has_the_clip_driver_and_no_infer_video_depth(version):
    cls = importlib.import_module(f"vdn.video_depth_model_v{version}").VideoDepthAnything
    for attr in ("refine_video_depth", "refine_video_depth_vis", "_refine_video_depth_device"):
        assert callable(getattr(cls, attr)), attr
    assert not hasattr(cls, "infer_video_depth")   # the reference's RGB signature is not offered


@pytest.mark.parametrize("n,windows", [(1, 1), (22, 1), (23, 2), (50, 3)])
def test_slot_tables(n, windows):
    """util.window_slots: int32 [windows, 32], every entry a clip frame; the tail is padded with copies of the last frame and
    slots 0..9 of a later window are the previous window's inputs at KEYFRAMES, so slots repeat exactly there."""
    from vdn import util
    s = util.window_slots(n)
    assert s.dtype == np.int32 and s.shape == (windows, util.INFER_LEN) and s.flags["C_CONTIGUOUS"]
    assert s.min() == 0 and s.max() == n - 1 and s.tolist() == util.window_table(n)
    step = util.INFER_LEN - util.OVERLAP
    for w in range(windows):
        fresh = s[w] if w == 0 else s[w, util.OVERLAP:]
        first = 0 if w == 0 else w * step + util.OVERLAP
        assert fresh.tolist() == [min(first + i, n - 1) for i in range(len(fresh))]          # new frames, then the padding
        if w:
            assert s[w, :util.OVERLAP].tolist() == [int(s[w - 1, k]) for k in util.KEYFRAMES]   # the keyframe copies
    distinct = [len(set(r.tolist())) for r in s]
    assert distinct == {1: [1], 22: [22], 23: [23, 3], 50: [32, 28, 6]}[n]   # 23: frame 0, keyframe 12, and the last frame 30 times


def test_slot_table_rejects_an_empty_clip():
    from vdn import util
    with pytest.raises(ValueError):
        util.window_slots(0)


def test_window_tail_entry_rejects_bad_arguments_without_a_gpu():
    """vdn_refine_window_tail returns before anything is launched: null pointers, sizes, an unknown kind, a finish that reads
    `scaled` without one, a map beyond INT32_MAX pixels, a misaligned pointer; and its trip hook reports the grid's reach."""
    import ctypes
    from vdn import _abi
    L = _abi.lib
    assert L.vdn_refine_window_tail_trip(1) == 4 * L.vdn_refine_window_tail_trip(0) == 4 * 64 * 256
    slots = ctypes.cast(64, ctypes.POINTER(ctypes.c_int32))

    def call(net=16, scaled=32, slots=slots, T=32, OH=8, OW=8, kind=_abi.TAIL_SHIFT, residual=1, out=48, frames=4, IH=8, IW=8):
        return L.vdn_refine_window_tail(net, IH, IW, scaled, frames, slots, T, OH, OW, kind, residual, 1.0, 0.0, 1.0, 0.0, 0.0, out, None)

    assert call(net=None) == call(out=None) == call(slots=None) == call(T=0) == call(T=65536) == call(frames=0) == call(OH=0) == -1
    assert call(kind=2) == -1 and call(scaled=None) == -1 and call(scaled=None, kind=_abi.TAIL_MIX, residual=0) == -1
    assert call(OH=65536, OW=32768) == -2 and call(IH=65536, IW=32768) == -2
    assert call(out=50) == -3 and call(scaled=34) == -3
