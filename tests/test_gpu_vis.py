"""vdn.vis on the device (csrc/vis.hip) against the numpy restatement of the reference's front ends (tests/vis_ref.py).

The bar everywhere is equality: every output byte, and for min/max the fp32 bits of numpy.min / numpy.max. The index
arithmetic is three fp32 operations, each correctly rounded on both sides, a truncation and a table lookup: there is
nothing to tolerate."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import vis_ref as R
from common import synth_sd

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 0xA5


@functools.lru_cache(maxsize=None)
def runtime():
    from vdn.runtime import Runtime
    return Runtime(torch.device("cuda", torch.cuda.current_device()))


def dev(a, dtype=None):
    """A device copy of a (possibly read-only) numpy array."""
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ vdn_minmax_f32
def ragged(a, n):
    """(head, first tail element) of a group of n floats that starts at float a of a 16-byte aligned allocation."""
    head = min((-a) % 4, n)
    return head, head + 4 * ((n - head) // 4)


@functools.lru_cache(maxsize=None)
def minmax_case(groups, n):
    """x [groups, n] in [0.1, 80): group 0 has its minimum in element 0 and its maximum in its last element, group 1 its
    extremes after the last 16-byte boundary (the kernel's per-element tail). Never written after this."""
    rng = np.random.default_rng(groups * 100003 + n)
    x = (0.1 + 79.9 * rng.random((groups, n))).astype(np.float32)
    x[0, 0], x[0, -1] = np.float32(0.05), np.float32(90.5)
    if groups > 1 and n >= 3:
        _, tail0 = ragged(1 + n, n)
        assert n - tail0 >= 2, "the case is meant to have a ragged tail"
        x[1, tail0], x[1, -1] = np.float32(0.01), np.float32(123.25)
    x.setflags(write=False)
    return x


def device_minmax(x):
    """vdn_minmax_f32 on a copy of x that starts one float into its allocation: 4-byte, not 16-byte aligned."""
    groups, n = x.shape
    buf = torch.empty(groups * n + 9, dtype=torch.float32, device=DEV)
    view = buf[1:1 + groups * n]
    assert view.data_ptr() % 16 == 4
    view.copy_(dev(x).reshape(-1))
    out = torch.full((groups + 1, 2), -777.0, dtype=torch.float32, device=DEV)
    runtime().minmax(view, groups, out[:groups])
    got = out.cpu().numpy()
    assert (got[groups] == -777.0).all(), "wrote past out[groups][2]"
    return got[:groups]


@pytest.mark.parametrize("groups,n", [(3, 1), (3, 3), (3, 5), (3, 257), (3, 4099), (1, 2 * 270 * 480)])
def test_minmax_bits_equal_numpy(groups, n):
    x = minmax_case(groups, n)
    want = np.stack([x.min(axis=1), x.max(axis=1)], axis=1)
    got = device_minmax(x)
    print(f"[minmax {groups}x{n}] got {got.tolist()} want {want.tolist()}")
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(device_minmax(x)), bits(got)), "two runs differ"


def test_minmax_nan_and_inf():
    x = minmax_case(3, 257).copy()
    x[1, 128] = np.nan
    got = device_minmax(x)
    assert np.isnan(got[1]).all(), got
    for g in (0, 2):
        assert np.array_equal(bits(got[g]), bits([x[g].min(), x[g].max()]))
    x = minmax_case(3, 4099).copy()
    x[2, 2000] = np.inf
    x[0, 7] = -np.inf
    got = device_minmax(x)
    want = np.stack([x.min(axis=1), x.max(axis=1)], axis=1)
    assert got[2, 1] == np.inf and got[0, 0] == -np.inf and np.array_equal(bits(got), bits(want))


def test_minmax_wrapper_scopes():
    from vdn import vis
    x = minmax_case(3, 4099)[:, :4095].reshape(3, 45, 91)
    d = dev(x)
    per = vis.minmax(d).cpu().numpy()
    assert per.shape == (3, 2) and np.array_equal(bits(per), bits(np.stack([x.min((1, 2)), x.max((1, 2))], 1)))
    clip = vis.minmax(d, scope="clip").cpu().numpy()
    assert clip.shape == (1, 2) and np.array_equal(bits(clip), bits([[x.min(), x.max()]]))
    one = vis.minmax(d[1]).cpu().numpy()
    assert np.array_equal(bits(one), bits(per[1:2]))


# ------------------------------------------------------------------------------------------------------ vdn_colorize
SHAPES = [(3, 5, 7), (2, 3, 9), (1, 1, 1), (2, 17, 64)]


def scaled(d, mn, mx):
    """The reference's fp32 arithmetic (run.py:59, dc_utils.py:79) before the cast."""
    return (np.asarray(d, np.float32) - np.float32(mn)) / (np.float32(mx) - np.float32(mn)) * np.float32(255.0)


def edge_values(mn, mx, ks):
    """For each integer k: the depth with the largest scaled position below k and the one with the smallest at or above it,
    found among the floats next to mn + (mx - mn) k / 255: scaled positions k -+ an ulp or so."""
    out = []
    for k in ks:
        d0 = np.float32(mn + (float(mx) - float(mn)) * k / 255.0)
        chain = [d0]
        for _ in range(8):
            chain.append(np.nextafter(chain[-1], np.float32(np.inf), dtype=np.float32))
        lo = d0
        for _ in range(8):
            lo = np.nextafter(lo, np.float32(-np.inf), dtype=np.float32)
            chain.insert(0, lo)
        chain = np.array(chain, np.float32)
        t = scaled(chain, mn, mx)
        below, above = chain[t < k], chain[t >= k]
        assert len(below) and len(above), (mn, mx, k)
        out += [below[-1], above[0]]
    return np.array(out, np.float32)


@functools.lru_cache(maxsize=None)
def depth_case(shape):
    """depth f32 [N, H, W] and raw u8 [N, H, W, 3]. Frame f spans exactly [0.1 + 3.3 f, 80 - 17.7 f] (both present: indices
    0 and 255); as many pixels as fit sit an ulp either side of an integer scaled position, the rest are random."""
    N, H, W = shape
    rng = np.random.default_rng(N * 10007 + H * 101 + W)
    d = np.empty(shape, np.float32)
    for f in range(N):
        mn, mx = np.float32(0.1 + 3.3 * f), np.float32(80.0 - 17.7 * f)
        v = (mn + (mx - mn) * rng.random(H * W)).astype(np.float32)
        v = np.clip(v, mn, mx)
        e = edge_values(mn, mx, [1, 2, 37, 64, 100, 127, 128, 129, 200, 254])
        if H * W > 2:
            v[2:2 + len(e)] = e[:max(0, H * W - 2)]
            v = rng.permutation(v)
        if H * W > 1:
            v[W // 2], v[-1] = mn, mx
        d[f] = v.reshape(H, W)
    raw = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    d.setflags(write=False)
    raw.setflags(write=False)
    return d, raw


def device_colorize(depth, minmax, lut, raw=None, margin=0, pad=16):
    """vdn_colorize into a buffer with `pad` guard bytes before and 13 after; the guards must come back untouched."""
    N, H, W = depth.shape
    ch = lut.shape[1]
    shape = (N, H, W, ch) if raw is None else (N, H, 2 * W + margin, 3)
    total = int(np.prod(shape))
    buf = torch.full((pad + total + 13,), CANARY, dtype=torch.uint8, device=DEV)
    out = buf[pad:pad + total]
    rt = runtime()
    rt.colorize(dev(depth), dev(minmax, np.float32), dev(lut), out, None if raw is None else dev(raw), margin)
    got = buf.cpu().numpy()
    assert (got[:pad] == CANARY).all() and (got[pad + total:] == CANARY).all(), "guard bytes were written"
    return got[pad:pad + total].reshape(shape)


def expected(depth, raw, table, ch, per_frame, margin):
    """Through vis_ref alone. `table` [256, ch] is in the channel order of the wanted output; run_frame flips to BGR, so it
    gets the flipped table. A one-pixel frame has max == min, where the reference divides 0 by 0 and casts the NaN, which
    no platform defines: there the expectation is what include/vdn.h defines as departure (1), palette index 0, stated
    directly; the raw frame and the margin around it are still the reference's."""
    if depth[0].size == 1:
        assert (depth.max((1, 2)) == depth.min((1, 2))).all()
        pic = np.broadcast_to(table[0], depth.shape + (ch,)).copy()
        if margin is None:
            return pic
        return np.concatenate([raw, np.full(depth.shape[:2] + (margin, 3), 255, np.uint8), pic], axis=2)
    return _expected(depth, raw, table, ch, per_frame, margin)


def _expected(depth, raw, table, ch, per_frame, margin):
    N = depth.shape[0]
    if per_frame:
        if ch == 1:
            pic = np.stack([R.run_frame(depth[f], None, True, True, None)[..., :1] for f in range(N)])
        elif margin is None:
            pic = np.stack([R.run_frame(depth[f], None, True, False, table[:, ::-1]) for f in range(N)])
        else:
            return np.stack([R.run_frame(depth[f], raw[f], False, False, table[:, ::-1], margin) for f in range(N)])
        return pic
    pic = R.save_video_frames(depth, ch == 1, table)
    if ch == 1:
        return pic[..., None]
    if margin is None:
        return pic
    white = np.full((N, depth.shape[1], margin, 3), 255, np.uint8)
    return np.concatenate([raw, white, pic], axis=2)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_colorize_bytes_equal_the_reference(shape):
    depth, raw = depth_case(shape)
    N, H, W = shape
    T = R.tables()
    rgb, bgr = T["Spectral_r"], np.ascontiguousarray(T["Spectral_r"][:, ::-1])
    grey = np.arange(256, dtype=np.uint8)[:, None]
    if H * W >= 30:   # the input can tell truncation from rounding and a division from a reciprocal multiply
        rounded = recip = 0
        for f in range(N):
            mn, mx = depth[f].min(), depth[f].max()
            t = scaled(depth[f], mn, mx).astype(np.uint8)
            rounded += int((np.rint(scaled(depth[f], mn, mx)).astype(np.uint8) != t).sum())
            recip += int((((depth[f] - mn) * (np.float32(1.0) / (mx - mn)) * np.float32(255.0)).astype(np.uint8) != t).sum())
            recip += int((((depth[f] - mn) * (np.float32(255.0) / (mx - mn))).astype(np.uint8) != t).sum())
        print(f"[colorize {shape}] pixels on another index with rounding: {rounded}, with a reciprocal multiply: {recip}")
        assert rounded > 0 and recip > 0
    mm_frame = np.stack([depth.min((1, 2)), depth.max((1, 2))], axis=1)
    mm_clip = np.array([[depth.min(), depth.max()]], np.float32)
    pads = (16, 17, 18, 19)   # every alignment of the output pointer
    for per_frame, mm in ((True, mm_frame), (False, mm_clip)):
        for name, lut, ch, margin in (("bgr", bgr, 3, None), ("rgb", rgb, 3, None), ("grey", grey, 1, None),
                                      ("raw50", bgr, 3, 50), ("raw0", bgr, 3, 0), ("raw1", bgr, 3, 1)):
            want = expected(depth, raw, lut, ch, per_frame, margin)
            for pad in pads:
                got = device_colorize(depth, mm, lut, raw if margin is not None else None, margin or 0, pad)
                assert got.shape == want.shape, (name, got.shape, want.shape)
                bad = int((got != want).sum())
                assert bad == 0, (shape, name, "per frame" if per_frame else "clip", pad, bad, np.argwhere(got != want)[:5].tolist())
    # the min/max the kernel pair computes itself, through the public entry
    from vdn import vis
    d = dev(depth)
    inferno = T["inferno"]
    assert np.array_equal(vis.colorize(d).cpu().numpy(), expected(depth, raw, bgr, 3, True, None))
    assert np.array_equal(vis.colorize(d, palette="inferno", order="rgb", scope="clip").cpu().numpy(),
                          expected(depth, raw, inferno, 3, False, None))
    assert np.array_equal(vis.colorize(d, raw=dev(raw)).cpu().numpy(), expected(depth, raw, bgr, 3, True, 50))
    assert np.array_equal(vis.colorize(d[0], palette="Spectral", grayscale=True, gray_channels=1, scope="clip").cpu().numpy(),
                          expected(depth[:1], raw[:1], grey, 1, False, None)[0])


def test_colorize_documented_departures():
    """What include/vdn.h defines where the reference casts NaN or an out-of-range float to uint8."""
    depth, _ = depth_case((2, 17, 64))
    lut = np.ascontiguousarray(R.tables()["Spectral_r"][:, ::-1])
    # (1) a constant frame: index 0 everywhere (frame 1 keeps its own range)
    d = depth.copy()
    d[0] = np.float32(3.25)
    mm = np.stack([d.min((1, 2)), d.max((1, 2))], axis=1)
    got = device_colorize(d, mm, lut)
    assert (got[0] == lut[0]).all()
    assert np.array_equal(got[1], R.run_frame(depth[1], None, True, False, lut[:, ::-1]))
    # (2) a supplied range narrower than the data clamps to 0 / 255; inside, the arithmetic is unchanged
    mn, mx = np.float32(10.0), np.float32(40.0)
    t = scaled(depth, mn, mx)
    idx = np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.uint8))).astype(np.uint8)
    assert (t < 0).any() and (t > 255).any() and ((t > 0) & (t < 255)).any()
    got = device_colorize(depth, np.array([[mn, mx]], np.float32), lut)
    assert np.array_equal(got, lut[idx])
    # (3) a NaN pixel: index 0, its neighbours untouched
    d = depth.copy()
    mm = np.stack([d.min((1, 2)), d.max((1, 2))], axis=1)
    want = np.stack([R.run_frame(d[f], None, True, False, lut[:, ::-1]) for f in range(2)])
    d[1, 8, 31] = np.nan
    want[1, 8, 31] = lut[0]
    assert (want[1, 8, 30] != lut[0]).any() or (want[1, 8, 32] != lut[0]).any()
    got = device_colorize(d, mm, lut)
    assert np.array_equal(got, want)


def test_colorize_argument_errors():
    from vdn import vis
    from vdn._abi import VdnError
    with pytest.raises(VdnError, match="no CPU path"):
        vis.colorize(torch.ones(2, 3, 4))
    d = torch.ones(2, 3, 4, device=DEV)
    with pytest.raises(ValueError, match="palette"):
        vis.colorize(d, palette="viridis")
    with pytest.raises(ValueError, match="order"):
        vis.colorize(d, order="xyz")
    with pytest.raises(ValueError, match="three channels"):
        vis.colorize(d, grayscale=True, gray_channels=1, raw=torch.zeros(2, 3, 4, 3, dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------------ model level
def test_infer_image_vis_equals_the_script_on_infer_image():
    """run.py's host stage applied to infer_image's depth, against infer_image_vis after clear_memory(): ViT-S, synthetic
    weights, input_size 266, a 120 x 120 BGR frame, so that the resize back to the frame runs. The frame is square because
    the memory block takes square grids only (memory_block.py:85; MemoryEngine.prepare asserts it): a 120 x 160 frame runs
    neither through infer_image nor through the reference. Non-square pictures are covered at the kernel level above."""
    import vdn
    from vdn import synth
    model = vdn.DepthAnythingV2(**vdn.MODEL_CONFIGS["vits"])
    model.load_state_dict(synth_sd("A", "vits"), strict=True)
    model = model.to(DEV).eval()
    raw = np.ascontiguousarray(synth.frames_u8(1234, 1, 120, 120)[0][:, :, ::-1])
    depth = model.infer_image(raw, 266)
    assert depth.shape == (120, 120) and depth.dtype == np.float32 and depth.max() > depth.min()
    T = R.tables()
    model.clear_memory()
    got = model.infer_image_vis(raw, 266, pred_only=False)
    want = R.run_frame(depth, raw, False, False, T["Spectral_r"])
    assert got.shape == (120, 2 * 120 + 50, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want), int((got != want).sum())
    model.clear_memory()
    got = model.infer_image_vis(raw, 266, pred_only=True, grayscale=True)
    assert got.shape == (120, 120, 3) and np.array_equal(got, R.run_frame(depth, raw, True, True, T["Spectral_r"]))
    model.clear_memory()
    got = model.infer_image_vis(raw, 266, pred_only=True, palette="Spectral")   # metric_depth/run.py
    assert np.array_equal(got, R.run_frame(depth, raw, True, False, T["Spectral"]))
    with pytest.raises(ValueError, match="palette"):
        model.infer_image_vis(raw, 266, palette="viridis")


def test_infer_video_depth_vis_equals_save_video_on_infer_video_depth():
    """save_video's frames from infer_video_depth's clip, against infer_video_depth_vis on the same frames: ViT-S, 34 frames of
    60 x 100 at input_size 70 (two windows: the stitched result), the smallest clip of the video-driver tests."""
    import vdn
    from vdn import synth
    model = vdn.VideoDepthAnything(**vdn.MODEL_CONFIGS["vits"])
    model.load_state_dict(synth_sd("B", "vits"), strict=True)
    model = model.to(DEV).eval()
    frames = synth.frames_u8(1234, 34, 60, 100)
    d, _ = model.infer_video_depth(frames, 24, input_size=70)
    d = d.copy()   # the driver's result aliases a reused pinned buffer
    T = R.tables()
    got, fps = model.infer_video_depth_vis(frames, 24, input_size=70)
    want = R.save_video_frames(d, False, T["inferno"])
    assert fps == 24 and got.shape == (34, 60, 100, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want), int((got != want).sum())
    got, _ = model.infer_video_depth_vis(frames, 24, input_size=70, grayscale=True)
    assert got.shape == (34, 60, 100) and np.array_equal(got, R.save_video_frames(d, True, T["inferno"]))
