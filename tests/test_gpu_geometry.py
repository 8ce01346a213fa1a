"""Frame geometry of the video drivers on the MI355X: how a u8 frame gets into the network (`vdn_preprocess`: cubic resize +
normalisation) and how the depth gets back out (`vdn_upsample_bilinear_f32`, the stitcher's fh / fw), at the shapes a real
clip has: not square, scaled down on the way in, scaled up on the way out, wide enough for the drivers' ratio rule.

Every bar below is arithmetic only, a multiple of U = 2^-24 (the largest relative error of one fp32 rounding): it holds for
any frame size, and none of it is taken from what the kernels return.

PREPROCESS BAR, |device - float64 oracle| <= 332 U max|ref|. With the source coordinate split exactly into floor and
fraction t, what is left is (pixels p = u8 / 255 in [0, 1], weights |w| <= 1, sum |w| <= S = 1.375, reached at t = 1/2):
  * t = fl(r / den) is off by U/2, and 1 + t, 1 - t, 2 - t by another U: the cubic's arguments by 1.5 U, times |w'| <= 1.35;
  * an outer weight ((A x - 5A) x + 8A) x - 4A, x in [1, 2]: roundings of U, 2U, 4U, 2U at A x (< 2), + 3.75 (< 4), . x (<= 4.5)
    and the last product (<= 4) (the additions of -6 and +3 are exact, Sterbenz), the first three multiplied by x <= 2 once or
    twice on the way: (((U) + 2U) 2 + 4U) 2 + 2U = 22 U at x = 2, where w' = 0, and ((U + 2U) + 2U) + 2U + 0.75 . 1.5 U <= 9 U
    at x = 1; where one outer tap has x near 2 the other has x near 1: 31 U the pair (24 U at x = 1.5 for both);
  * an inner weight ((A + 2) x - (A + 3)) x x + 1, x in [0, 1]: roundings U, 2U, U, U/2, U/2 = 5 U and the argument's
    1.35 . 1.5 U: 7.1 U, 14.2 U the pair; so W = sum |dw| <= 46 U per axis;
  * a row  sum_b wx[b] p[b]: W + S U/2 (p's own rounding) + 8 U (4 products, 4 sums, all below 2) <= 55 U, |row| <= S;
  * the column sum over 4 rows: S 55 U + W S + 8 U <= 147 U on the resized value v;
  * (v - mean) * (1 / std): 147 U / 0.224 = 657 U absolute, plus 3 roundings relative to the result: 3 U max|ref|.
Every case's content holds both 0 and 255, so max|ref| >= 2 (asserted): 657 U <= 329 U max|ref|, in all 332 U max|ref| —
6e-5 at max|ref| = 3. An fp32 coordinate adds in / out * o * U to t, 1e-4 and more in the output at a 300-row frame.

UPSAMPLE BAR, |device - torch's fp32 CPU result| <= 16 U max|x|: both evaluate (1 - ly) ((1 - lx) a + lx b) + ly (...) from the
same fp32 scale * o: per evaluation U/2 on each 1 - l (two levels), and 3 roundings per level (2 products, 1 sum) of values
below max|x|: 3.5 U + 4 U = 7.5 U max|x| from the exactly evaluated lerp of the same l, twice that between the two."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from common import rel_l2, synth_sd, worst_px

pytestmark = pytest.mark.gpu
TOL = 1e-3            # the project's bar on rel-L2 and on the worst pixel (tests/test_gpu_e2e.py)
U = 2.0 ** -24
PRE_BAR, UP_BAR = 332, 16
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SENTINEL, PAD = -12345.0, 4096   # floats on either side of an output (16 KiB: the views stay 16-byte aligned)


def net_size(fh, fw, input_size):
    """(input_size after the drivers' ratio rule, H, W) of the network input for an fh x fw frame."""
    from vdn import util
    ratio = max(fh, fw) / min(fh, fw)
    if ratio > 1.78:
        input_size = round(int(input_size * 1.777 / ratio) / 14) * 14
    W, H = util.get_size(fw, fh, input_size)
    return input_size, H, W


@pytest.fixture(scope="module")
def rt():
    from vdn import _abi
    from vdn.runtime import Runtime
    assert torch.cuda.is_available() and _abi.lib.vdn_arch_ok() == 1
    return Runtime(torch.device("cuda:0"), torch.float16)


def guarded(shape):
    """(whole buffer, view of `shape` in its middle): the buffer is pre-filled with SENTINEL, PAD floats on either side."""
    numel = int(np.prod(shape))
    whole = torch.full((numel + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    return whole, whole[PAD:PAD + numel].view(shape)


def margins_untouched(whole):
    w = whole.cpu()
    return bool((w[:PAD] == SENTINEL).all() and (w[-PAD:] == SENTINEL).all())


# --------------------------------------------------------------------------------------------- vdn_preprocess
# frame h x w at input_size -> network input H x W
PRE_CASES = {
    "landscape_up": (60, 100, 70, 70, 112),
    "portrait_down": (300, 180, 140, 238, 140),
    "wide_ratio_branch": (40, 100, 140, 98, 252),      # ratio 2.5 > 1.78 -> input_size 98
    "up_14x": (37, 53, 518, 518, 742),                 # the border clamp covers 7 output pixels
    "identity": (98, 98, 98, 98, 98),
    "1080p_grid_stride": (1080, 1920, 518, 518, 924),  # 3 x 518 x 924 = 1.43 M pixels > 4096 blocks x 256 threads
}


def frames_for(h, w):
    """Three frames of different content: uniform noise; a one-pixel 0/255 checkerboard (cubic overshoot outside [0, 1]);
    three different constants per channel (which channel went where, and whose mean / std it got)."""
    rng = np.random.default_rng(h * 10007 + w)
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    noise[0, 0], noise[-1, -1] = 0, 255
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    const = np.empty((h, w, 3), np.uint8)
    const[:] = (0, 90, 255)
    return np.ascontiguousarray(np.stack([noise, checker, const]))


@functools.lru_cache(maxsize=None)
def pre_case(name):
    """(frames u8 [3,h,w,3], float64 cubic resize of frames / 255 [3,H,W,3]) — computed once per case, never written to."""
    from oracle import ref_cpu as O
    h, w, _, H, W = PRE_CASES[name]
    fr = frames_for(h, w)
    rs = np.stack([O.resize_cubic(f / 255.0, W, H) for f in fr])
    fr.setflags(write=False)
    rs.setflags(write=False)
    return fr, rs


def pre_reference(resized, swap_rb):
    """float64 [n,3,H,W]: output channel c reads source channel 2 - c under swap_rb, and is normalised with mean[c], std[c]."""
    src = resized[..., ::-1] if swap_rb else resized
    return ((src - np.array(MEAN)) / np.array(STD)).transpose(0, 3, 1, 2)


@pytest.mark.parametrize("swap_rb", [False, True])
@pytest.mark.parametrize("name", list(PRE_CASES))
def test_preprocess_against_fp64_oracle(rt, name, swap_rb):
    h, w, size, H, W = PRE_CASES[name]
    assert net_size(h, w, size)[1:] == (H, W)
    fr, resized = pre_case(name)
    ref = pre_reference(resized, swap_rb)
    whole, out = guarded((3, 3, H, W))
    got = rt.preprocess_u8(torch.from_numpy(fr).cuda(), H, W, MEAN, STD, swap_rb, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert margins_untouched(whole)
    got = out.cpu().numpy().astype(np.float64)
    m = float(np.abs(ref).max())
    assert m >= 2.0, m     # the bar's derivation leans on it
    bar = PRE_BAR * U * m
    per_frame = np.abs(got - ref).reshape(3, -1).max(1)
    print(f"[geometry] preprocess {name} {h}x{w} -> {H}x{W} swap_rb={int(swap_rb)}: max |device - fp64 oracle| per frame "
          f"{per_frame[0]:.2e} {per_frame[1]:.2e} {per_frame[2]:.2e}, bar {bar:.2e} (max|ref| {m:.2f})")
    assert np.isfinite(got).all() and per_frame.max() <= bar, (name, swap_rb, per_frame.tolist(), bar)
    if (h, w) == (H, W):   # identity geometry: weights {0, 1, 0, 0}, so the fp32 normalisation of the pixel itself, bit for bit
        f32 = np.float32
        src = fr[..., ::-1] if swap_rb else fr
        host = (src.astype(f32) / f32(255.0) - np.array(MEAN, f32)) * (f32(1.0) / np.array(STD, f32))
        assert host.dtype == f32
        assert np.array_equal(out.cpu().numpy(), host.transpose(0, 3, 1, 2))


# --------------------------------------------------------------------------------------------- vdn_upsample_bilinear_f32
UP_CASES = {
    "down_b2": (2, 70, 112, 60, 100),              # a small frame at a larger input_size
    "wide_down": (1, 98, 252, 40, 100),
    "to_1080p_grid_stride": (1, 518, 924, 1080, 1920),   # 2.07 M outputs > 4096 blocks x 256 threads
    "one_output": (2, 5, 7, 1, 1),                 # OH = OW = 1: both scales 0
    "one_output_row": (1, 6, 7, 1, 5),
    "one_output_col": (1, 6, 7, 5, 1),
    "one_input_row": (1, 1, 9, 4, 6),              # IH = 1: scale 0, y1 = y0
    "one_input_col": (1, 9, 1, 6, 4),
}


@functools.lru_cache(maxsize=None)
def up_case(name):
    """(signed x [B,IH,IW], torch's fp32 CPU bilinear align_corners result, the float64 one)."""
    B, IH, IW, OH, OW = UP_CASES[name]
    x = torch.randn(B, IH, IW, generator=torch.Generator().manual_seed(IH * 1009 + IW)) * 2.5
    ref = F.interpolate(x[:, None], (OH, OW), mode="bilinear", align_corners=True)[:, 0]
    ref64 = F.interpolate(x.double()[:, None], (OH, OW), mode="bilinear", align_corners=True)[:, 0]
    return x, ref, ref64


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("name", list(UP_CASES))
def test_upsample_f32_against_torch_fp32(rt, name, relu):
    B, IH, IW, OH, OW = UP_CASES[name]
    x, ref, ref64 = up_case(name)
    if relu:
        ref, ref64 = torch.relu(ref), torch.relu(ref64)
    assert float(x.min()) < 0 < float(x.max())
    whole, out = guarded((B, OH, OW))
    rt.upsample_f32(x.cuda(), out, B, IH, IW, OH, OW, relu=bool(relu))
    torch.cuda.synchronize()
    assert margins_untouched(whole)
    got = out.cpu()
    bar = UP_BAR * U * float(x.abs().max())
    err = float((got.double() - ref.double()).abs().max())
    err64 = float((got.double() - ref64).abs().max())
    print(f"[geometry] upsample {name} B={B} {IH}x{IW} -> {OH}x{OW} relu={relu}: max |device - torch fp32| {err:.2e}, bar {bar:.2e}; "
          f"for information, to torch float64 {err64:.2e} (torch's own fp32 is {float((ref.double() - ref64).abs().max()):.2e} from it)")
    assert torch.isfinite(got).all() and err <= bar, (name, relu, err, bar)
    if relu:
        assert float(got.min()) >= 0


# --------------------------------------------------------------------------------------------- drivers on non-square frames
@pytest.fixture(scope="module")
def model():
    import vdn
    m = vdn.VideoDepthAnything(**vdn.MODEL_CONFIGS["vits"])
    m.load_state_dict(synth_sd("B", "vits"), strict=True)
    return m.to("cuda").eval()


def oracle_preprocess(frames, H, W):
    """RGB u8 [n,h,w,3] -> f32 [n,3,H,W] on the host: the float64 oracle, narrowed once at the end."""
    from oracle import ref_cpu as O
    rs = np.stack([O.resize_cubic(f / 255.0, W, H) for f in frames])
    return torch.from_numpy(pre_reference(rs, False).astype(np.float32))


def host_chain(model, net, n, fh, fw):
    """Per-window forward of the pre-processed clip `net`, torch's CPU resize to the frame size, the host stitcher."""
    from vdn import util
    per_window = []
    for idxs in util.window_table(n):
        d = model.forward(net[torch.tensor(idxs, device=net.device)][None])[0].cpu()
        d = F.interpolate(d[:, None], (fh, fw), mode="bilinear", align_corners=True)[:, 0].numpy()
        per_window += [d[i] for i in range(util.INFER_LEN)]
    return util.stitch(per_window, n)


@pytest.mark.parametrize("fh,fw,size,H,W", [(60, 100, 70, 70, 112), (40, 100, 140, 98, 252)])
def test_infer_video_depth_nonsquare(model, fh, fw, size, H, W):
    """34 frames = two windows. (a) isolates resize_depth and the stitcher's geometry: same device pre-processing, host resize
    and stitch. (b) adds the pre-processing: the same chain fed from the oracle's.

    Measured: (a) 4.8e-7 and 7.2e-7 of maxima of 3.3 and 3.5; (b) rel-L2 1.3e-5 / 6.0e-6, worst pixel 3.2e-5 / 1.8e-5.
    (a) is also what holds the driver's tap cache to whole encoder batches: with the clip's last two frames encoded as a
    batch of 2, where `forward` encodes 32, vdn_gemm lands on another kernel and (a) read 4.2e-5 and 1.7e-5."""
    from vdn import synth, util
    n = 34
    frames = synth.frames_u8(1234, n, fh, fw)
    eff, nH, nW = net_size(fh, fw, size)
    assert (nH, nW) == (H, W) and len(util.window_table(n)) == 2
    d, fps = model.infer_video_depth(frames, 24, input_size=size)
    d = d.copy()   # the driver's result aliases a reused pinned buffer
    assert d.shape == (n, fh, fw) and d.dtype == np.float32 and fps == 24 and np.isfinite(d).all() and (d >= 0).all()
    net = model.preprocess_frames(frames, eff)
    assert tuple(net.shape) == (n, 3, H, W)
    ref = host_chain(model, oracle_preprocess(frames, H, W).cuda(), n, fh, fw)
    e, wp = rel_l2(d, ref), worst_px(d, ref)
    print(f"[geometry] infer_video_depth {fh}x{fw} at {size} -> {H}x{W}: (b) vs the chain fed from the oracle's pre-processing, "
          f"rel-L2 {e:.2e} worst pixel {wp:.2e}")
    assert e < TOL and wp < TOL, (e, wp)
    host = host_chain(model, net, n, fh, fw)
    print(f"[geometry] infer_video_depth {fh}x{fw} at {size} -> {H}x{W}: (a) device resize + stitcher vs host, max |diff| "
          f"{float(np.abs(d - host).max()):.2e} of max {float(np.abs(host).max()):.2e}")
    assert np.allclose(d, host, rtol=2e-5, atol=1e-6), float(np.abs(d - host).max())


def test_infer_video_depth_one_wide_frames(model, monkeypatch):
    """The streaming driver on 40 x 100 frames: ratio branch -> 98 x 252 per call, depth back at 40 x 100."""
    from vdn import synth
    fh, fw, size = 40, 100, 140
    _, H, W = net_size(fh, fw, size)
    assert (H, W) == (98, 252)
    frames = synth.frames_u8(1234, 3, fh, fw)
    seen, step = [], model.stream_step
    monkeypatch.setattr(model, "stream_step", lambda x, *a, **k: (seen.append(tuple(x.shape)), step(x, *a, **k))[1])
    model.reset_stream()
    got = [model.infer_video_depth_one(f, input_size=size) for f in frames]
    assert seen == [(1, 1, 3, H, W)] * 3
    monkeypatch.undo()
    model.reset_stream()
    x = oracle_preprocess(frames, H, W)
    for t in range(3):
        d = model.stream_step(x[t][None, None].cuda()).cpu()
        ref = F.interpolate(d[None, None], (fh, fw), mode="bilinear", align_corners=True)[0, 0].numpy()
        e, wp = rel_l2(got[t], ref), worst_px(got[t], ref)
        print(f"[geometry] infer_video_depth_one frame {t} {fh}x{fw} -> {H}x{W}: rel-L2 {e:.2e} worst pixel {wp:.2e}")
        assert got[t].shape == (fh, fw) and np.isfinite(got[t]).all() and (got[t] >= 0).all()
        assert e < TOL and wp < TOL, (t, e, wp)
    model.reset_stream()


def test_window_sharded_driver_single_rank_nonsquare(model):
    """Holds the one-rank sharded driver to the plain driver's encoder batches: in chunks of 8 frames (320 rows at 5 x 8
    patches, another vdn_gemm kernel than 32 frames' 1280 rows) the two were 5.5e-5 apart here, bit-equal at 98x252 and 140x140."""
    from vdn import synth
    from vdn.dist import infer_video_depth_sharded
    frames = synth.frames_u8(1234, 34, 60, 100)
    d0, _ = model.infer_video_depth(frames, 24, input_size=70)
    d0 = d0.copy()
    d1, _ = infer_video_depth_sharded(model, frames, 24, input_size=70)
    assert d0.shape == d1.shape == (34, 60, 100)
    assert np.allclose(d0, d1, rtol=1e-5, atol=1e-6), float(np.abs(d0 - d1).max())
