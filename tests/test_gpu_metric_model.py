"""The metric-depth model on the MI355X (vdn.metric_depth, vdn.points), through the C-ABI: the sigmoid ending of the two DPT
tails against fp64, the model against the fixtures tools/make_golden_metric_model.py wrote from the imported reference
(metric_depth/depth_anything_v2: DINOv2 + DPTHead, times max_depth), its statelessness, max_depth as a launch argument, the
image drivers, the point cloud against numpy bit for bit, and metric_depth/train.py's validation-loop body on top of it."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from common import GOLD, inputs, rel_l2, sample_idx, schema, stats, synth_sd, worst_px
from test_gpu_ops import close, h, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3                       # the project's parity bar (tests/test_gpu_e2e.py): rel-L2 and worst pixel
NONE, RELU, SIGMOID = 0, 1, 2    # VDN_OUT_* (include/vdn.h)


@pytest.fixture(scope="module")
def rt():
    from vdn.runtime import Runtime
    from vdn import _abi
    assert torch.cuda.is_available() and _abi.lib.vdn_arch_ok() == 1, "GPU tests need the MI355X"
    return Runtime(torch.device("cuda:0"), torch.float16)


@pytest.fixture(scope="module")
def rt3():
    from vdn.runtime import Runtime
    return Runtime(torch.device("cuda:0"), torch.float16, split=True)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ 1. fused tail
def _tail_case(B, IH, IW, C, OH, OW, w1_gain):
    """The inputs and the fp64 restatement of test_depth_tail_fused_against_fp64_and_unfused (same seeds), the 1x1 weights
    times w1_gain; returns the fp64 logits."""
    x = rnd(B, IH, IW, C, seed=900)
    w2 = rnd(32, C, 3, 3, seed=901, scale=1 / math.sqrt(9 * C))
    b2 = rnd(32, seed=902, scale=0.1)
    w1 = rnd(32, seed=903, scale=0.3)
    w1 = (w1 - w1.mean()) * w1_gain
    b1 = 0.2
    up = F.interpolate(x.double().permute(0, 3, 1, 2), (OH, OW), mode="bilinear", align_corners=True)
    mid = F.relu(F.conv2d(up, w2.double(), b2.double(), padding=1))
    ref = (mid * w1.double().reshape(1, 32, 1, 1)).sum(1) + b1
    return x, w2, b2, w1, b1, ref


def _tail_act(rt3, x, wt, b2, w1, b1, d, shape, act, out_scale):
    from vdn import _abi
    B, IH, IW, C, OH, OW = shape
    rc = _abi.lib.vdn_depth_tail_act(_abi.F16, x.data_ptr(), B, IH, IW, C, wt.hi.data_ptr(), wt.lo.data_ptr(), wt.hi.shape[1],
                                     b2.data_ptr(), w1.data_ptr(), b1, d.data_ptr(), OH, OW, act, out_scale, _stream())
    assert rc == 0, rc
    return d


@pytest.mark.parametrize("shape,out_scale", [((2, 76, 76, 32, 133, 133), 20.0), ((1, 40, 24, 64, 70, 42), 80.0)])
def test_depth_tail_sigmoid_against_fp64(rt3, shape, out_scale):
    """vdn_depth_tail_act(VDN_OUT_SIGMOID) = out_scale * sigmoid(logits) against the fp64 restatement of the existing tail test:
    tile tails (133 = 8 x 16 + 5), a non-square map, 1 and 2 channel passes. The 1x1 weights are 4 times that test's, the
    smallest whole factor at which the fp64 logits of both shapes pass -6 and +6 (they span -2.25 .. 2.49 and -1.91 .. 2.27
    unscaled), so both flat ends of the sigmoid carry pixels. Bar: that test's close(.., 2e-5): |sigmoid'| <= 1/4, and in fp32
    arithmetic the same pipeline is 8e-7 .. 3e-6 from fp64 at this gain. Then act 0 / 1 through the new entry are the bits of
    vdn_depth_tail(relu = 0 / 1)."""
    from vdn import pack, _abi
    B, IH, IW, C, OH, OW = shape
    x, w2, b2, w1, b1, ref = _tail_case(*shape, w1_gain=4.0)
    assert float(ref.min()) < -6 and float(ref.max()) > 6, (float(ref.min()), float(ref.max()))
    xf = x.reshape(-1, C).to(DEV).contiguous()
    wt = pack.conv3x3_taps(w2.to(DEV), rt3.prec)
    b2d, w1d = b2.to(DEV), w1.to(DEV)
    d = torch.empty(B, OH, OW, device=DEV)
    _tail_act(rt3, xf, wt, b2d, w1d, b1, d, shape, SIGMOID, out_scale)
    want = (out_scale * torch.sigmoid(ref)).float()
    got = d.cpu()
    print(f"[tail sigmoid {shape}] rel-L2 {rel_l2(got, want):.2e} worst {worst_px(got, want):.2e}; logits {float(ref.min()):.1f} .. {float(ref.max()):.1f}")
    close(d, want, 2e-5)
    assert float(got.min()) >= 0.0 and float(got.max()) <= out_scale
    # Runtime.depth_tail(act=...) is the same launch
    d_rt = torch.empty_like(d)
    rt3.depth_tail(xf, wt, b2d, w1d, b1, d_rt, B, IH, IW, C, OH, OW, act=SIGMOID, out_scale=out_scale)
    assert torch.equal(d_rt, d)
    # the two older endings: bit-equal to the entry that existing callers and bench.py use, and out_scale is not read
    for relu in (0, 1):
        old, new = torch.empty_like(d), torch.empty_like(d)
        rc = _abi.lib.vdn_depth_tail(_abi.F16, xf.data_ptr(), B, IH, IW, C, wt.hi.data_ptr(), wt.lo.data_ptr(), wt.hi.shape[1],
                                     b2d.data_ptr(), w1d.data_ptr(), b1, old.data_ptr(), OH, OW, relu, _stream())
        assert rc == 0
        _tail_act(rt3, xf, wt, b2d, w1d, b1, new, shape, RELU if relu else NONE, 7.0)
        assert torch.equal(old, new)
        close(new, (F.relu(ref) if relu else ref).float(), 2e-5)
        rt3.depth_tail(xf, wt, b2d, w1d, b1, old, B, IH, IW, C, OH, OW, relu=bool(relu))   # the keyword existing callers pass
        assert torch.equal(old, new)


def test_depth_tail_sigmoid_saturates_exactly_and_passes_nan(rt3):
    """One 16 x 16 tile whose logits are forced (zero 1x1 weights, the bias alone): -100 gives exactly 0 (e^100 overflows to
    +inf, 1 / inf), +100 exactly out_scale (e^-100 vanishes beside 1), NaN gives NaN; no NaN from inf / inf."""
    from vdn import pack
    shape = (1, 9, 9, 32, 16, 16)
    B, IH, IW, C, OH, OW = shape
    x, w2, b2, _, _, _ = _tail_case(*shape, w1_gain=1.0)
    xf = x.reshape(-1, C).to(DEV).contiguous()
    wt = pack.conv3x3_taps(w2.to(DEV), rt3.prec)
    w1 = torch.zeros(32, device=DEV)
    d = torch.empty(B, OH, OW, device=DEV)
    for out_scale in (20.0, 80.0):
        assert torch.equal(_tail_act(rt3, xf, wt, b2.to(DEV), w1, -100.0, d, shape, SIGMOID, out_scale).cpu(), torch.zeros(B, OH, OW))
        assert torch.equal(_tail_act(rt3, xf, wt, b2.to(DEV), w1, 100.0, d, shape, SIGMOID, out_scale).cpu(),
                           torch.full((B, OH, OW), out_scale))
        assert bool(torch.isnan(_tail_act(rt3, xf, wt, b2.to(DEV), w1, float("nan"), d, shape, SIGMOID, out_scale)).all())
    from vdn import _abi
    assert _abi.lib.vdn_depth_tail_act(_abi.F16, xf.data_ptr(), B, IH, IW, C, wt.hi.data_ptr(), wt.lo.data_ptr(), wt.hi.shape[1],
                                       b2.to(DEV).data_ptr(), w1.data_ptr(), 0.0, d.data_ptr(), OH, OW, 3, 1.0, _stream()) == -1


# ------------------------------------------------------------------------------------------------ 2. unfused ending
def test_head_out_act_against_fp64(rt, rt3):
    """vdn_head_out_act, M = 1000 (3 blocks of 256 and a partial one): the three activations against fp64 to the existing
    head_out test's close(.., 1e-5), on one half plane and on split planes; act 0 / 1 are the bits of vdn_head_out. The weights
    are 3 times that test's so that the logits pass -6 and +6."""
    from vdn import _abi
    M, C = 1000, 32
    f = F.relu(h(rnd(M, C, seed=140)))
    w = rnd(C, seed=141) * 3.0
    ref = f.double() @ w.double() + 0.3
    assert float(ref.min()) < -6 and float(ref.max()) > 6, (float(ref.min()), float(ref.max()))
    fd, wd = f.half().to(DEV), w.to(DEV)
    d = torch.empty(M, device=DEV)
    for out_scale in (20.0, 80.0):
        rt.head_out(fd, wd, 0.3, d, M, C, act=SIGMOID, out_scale=out_scale)
        close(d, (out_scale * torch.sigmoid(ref)).float(), 1e-5)
    for relu in (0, 1):
        old, new = torch.empty_like(d), torch.empty_like(d)
        assert _abi.lib.vdn_head_out(_abi.F16, fd.data_ptr(), None, wd.data_ptr(), 0.3, old.data_ptr(), M, C, relu, _stream()) == 0
        assert _abi.lib.vdn_head_out_act(_abi.F16, fd.data_ptr(), None, wd.data_ptr(), 0.3, new.data_ptr(), M, C, RELU if relu else NONE,
                                         7.0, _stream()) == 0
        assert torch.equal(old, new)
        close(new, (F.relu(ref) if relu else ref).float(), 1e-5)
        rt.head_out(fd, wd, 0.3, old, M, C, relu=bool(relu))
        assert torch.equal(old, new)
    # split planes: a value the half plane alone cannot hold
    f2 = F.relu(rnd(M, C, seed=142))
    fs = rt3.to_half(f2.to(DEV))
    ref2 = fs.float().cpu().double() @ w.double() - 0.1
    rt3.head_out(fs, wd, -0.1, d, M, C, act=SIGMOID, out_scale=20.0)
    close(d, (20.0 * torch.sigmoid(ref2)).float(), 1e-5)
    # forced logits: exact ends and NaN
    wz = torch.zeros(C, device=DEV)
    rt.head_out(fd, wz, -100.0, d, M, C, act=SIGMOID, out_scale=80.0)
    assert torch.equal(d.cpu(), torch.zeros(M))
    rt.head_out(fd, wz, 100.0, d, M, C, act=SIGMOID, out_scale=80.0)
    assert torch.equal(d.cpu(), torch.full((M,), 80.0))
    rt.head_out(fd, wz, float("nan"), d, M, C, act=SIGMOID, out_scale=80.0)
    assert bool(torch.isnan(d).all())
    assert _abi.lib.vdn_head_out_act(_abi.F16, fd.data_ptr(), None, wd.data_ptr(), 0.3, d.data_ptr(), M, C, 3, 1.0, _stream()) == -1


# ------------------------------------------------------------------------------------------------ 3. model vs fixtures
_BASE = {"M": "A", "Mf": "Af", "Mh": "Ah"}   # the relative model's synthetic weights: same keys, same values, plus a memory block


def _fixture(name):
    return np.load(os.path.join(GOLD, f"{name}.npz"))


def _state_dict(which, enc, g):
    """common.synth_sd's weights under the metric model's keys (parameter values depend on the key alone, so the relative
    model's cached state dict serves: its memory_block.* entries are dropped), with the fixture's final 1x1 layer on top."""
    sch = schema(which, enc)
    base = synth_sd(_BASE[which], enc)
    sd = {k: base[k] for k, _ in sch["params"] + sch["buffers"]}
    sd["depth_head.scratch.output_conv2.2.weight"] = torch.from_numpy(g["last_weight"])
    sd["depth_head.scratch.output_conv2.2.bias"] = torch.from_numpy(g["last_bias"])
    return sd


def _model(which, enc, g, precision=None):
    import vdn
    from vdn.metric_depth.depth_anything_v2.dpt import DepthAnythingV2
    flags = dict(use_bn=True, use_clstoken=True) if which == "Mf" else {}
    m = DepthAnythingV2(**dict(vdn.MODEL_CONFIGS[enc], **flags), max_depth=float(g["max_depth"]))
    m.load_state_dict(_state_dict(which, enc, g), strict=True)
    if precision:
        m.set_precision(precision)
    return m.to(DEV).eval()


def _against_fixture(name, model, g, bar=TOL, depth_l2_only=False):
    B, H, W, sub, ls, _ = [int(v) for v in g["meta"]]
    x = inputs(B, H, W).cuda()
    logits = model.forward(x, _pre_act=True).cpu()
    depth = model.forward(x).cpu()
    assert tuple(depth.shape) == (B, H, W) and torch.isfinite(logits).all() and torch.isfinite(depth).all()
    md = float(g["max_depth"])
    assert float(depth.min()) >= 0.0 and float(depth.max()) <= md
    e_l, w_l = rel_l2(logits[:, ::ls, ::ls], g["logits"]), worst_px(logits[:, ::ls, ::ls], g["logits"])
    e_d, w_d = rel_l2(depth[:, ::sub, ::sub], g["depth"]), worst_px(depth[:, ::sub, ::sub], g["depth"])
    print(f"[{name}] vs reference fixture: logits rel-L2 {e_l:.2e} worst pixel {w_l:.2e}; depth rel-L2 {e_d:.2e} worst pixel {w_d:.2e}")
    assert e_d <= bar, (name, e_d)
    if not depth_l2_only:
        assert e_l <= bar and w_l <= bar and w_d <= bar, (name, e_l, w_l, e_d, w_d)
    return logits, depth


def _samples_close(name, k, v, g):
    ref = g[f"{k}_samp"]
    err = rel_l2(v.reshape(-1)[sample_idx(v.numel(), len(ref))], ref)
    st, rs = stats(v), g[f"{k}_stats"]
    print(f"[{name}] stage {k} {tuple(v.shape)}: samples rel-L2 {err:.2e}, mean {st[0]:.5f} / {rs[0]:.5f}, std {st[1]:.5f} / {rs[1]:.5f}")
    return err, st, rs


def test_M_vits_266x350_fused_unfused_and_stages(monkeypatch):
    """vits, B = 2, 19 x 25 patches (not square: tile tails of the fused tail in both directions). Logits and depth against the
    fixture at 1e-3 (rel-L2 and worst pixel); the four taps as tests/test_gpu_e2e.py holds a token-level feature (2e-3 on the
    samples) and path_1 / output_conv1 as its stage test holds them. Then the same with VDN_TAIL_UNFUSED=1 set before the engines
    are built (ending in vdn_head_out_act): the two agree to the existing tail test's close(.., 3e-5)."""
    name = "M_vits_266x350"
    g = _fixture(name)
    B, H, W = [int(v) for v in g["meta"][:3]]
    ph, pw, C, Fh = H // 14, W // 14, 384, 64
    model = _model("M", "vits", g)
    logits, depth = _against_fixture(name, model, g)
    e = model._eng
    assert e["head"].oc2_taps is not None, "the fused tail did not run"
    rt = e["rt"]
    # the batch in one pass (set_batch_invariant(False)) against the fixture too; its arena then holds both frames' stages
    model.set_batch_invariant(False)
    _against_fixture(name + " one pass", model, g)
    for j in range(4):
        err, st, rs = _samples_close(name, f"tap{j}", rt.hbuf(f"tap{j}", (B * ph * pw, C)).float().cpu(), g)
        assert err < 2e-3, (j, err)
    for k, v in (("path1", rt.hbuf("path1", (B * 64 * ph * pw, Fh)).float().cpu()), ("oc1", rt.fbuf("out1_f32", (B * 64 * ph * pw, Fh // 2)).cpu())):
        err, st, rs = _samples_close(name, k, v, g)
        assert err < TOL and abs(st[1] - rs[1]) <= 1e-3 * rs[1] and abs(st[0] - rs[0]) <= 1e-3 * rs[1], (k, err, st, rs)
    monkeypatch.setenv("VDN_TAIL_UNFUSED", "1")
    unfused = _model("M", "vits", g)
    logits_u, depth_u = _against_fixture(name + " unfused", unfused, g)
    assert unfused._eng["head"].oc2_taps is None, "VDN_TAIL_UNFUSED=1 was not seen by the engine"
    close(logits_u, logits, 3e-5)
    close(depth_u, depth, 3e-5)


def test_M_vits_266x350_f16():
    """The single-product mode (it ends in vdn_head_out_act: the fused tail needs split planes), to the 3e-3 that
    test_single_pass_modes_error_is_reported_and_bounded gives f16: like that test, the rel-L2 of the returned map (the mode is
    not fp32-faithful; the logits' and the worst pixel's distances are printed)."""
    g = _fixture("M_vits_266x350")
    model = _model("M", "vits", g, precision="f16")
    _against_fixture("M_vits_266x350 f16", model, g, bar=3e-3, depth_l2_only=True)
    assert model._eng["head"].oc2_taps is None


def test_Mf_use_bn_and_use_clstoken():
    """use_bn=True, use_clstoken=True (BatchNorm with non-trivial statistics folded, cls-token readout on all four taps right
    after the encoder), max_depth = 80."""
    g = _fixture("Mf_vits_266")
    _against_fixture("Mf_vits_266", _model("Mf", "vits", g), g)


def test_M_vitl_518_checkpoint_like_weights():
    """ViT-L at 518 x 518 with vdn/synth.heavy_overlay: the size at which output_conv1 runs at the low resolution and the fused
    tail follows it. Final maps only, as the relative model's heavy fixture is held."""
    g = _fixture("M_vitl_518_heavy")
    model = _model("Mh", "vitl", g)
    _against_fixture("M_vitl_518_heavy", model, g)
    head = model._eng["head"]
    assert head.oc2_taps is not None and head.oc1_low is not None


# ------------------------------------------------------------------------------------------------ 4 / 5. state, max_depth
@pytest.fixture(scope="module")
def vits_model():
    g = _fixture("M_vits_266x350")
    return _model("M", "vits", g)


def test_no_state_between_calls(vits_model):
    """The same batch twice: equal bits. Row 1 of a batch of two alone as a batch of one: equal bits. A 266 x 350 call followed
    by a 266 x 266 call needs no reset. A batch of THREE against each of its frames alone: equal bits too, although a one-pass
    batch of three would cross the row count (65536 rows of the 8x map; a frame here has 30400) from which output_conv1 runs at
    the low resolution: the default runs a batch frame by frame. The opt-out (one pass) agrees with it to rounding: 1e-5 at
    batch 2, what test_determinism_and_memory_reset gives a batch against a single frame; 3e-5 at batch 3, where the head also
    takes its other, equally fp32-faithful ending, the bar the existing tail test gives two such endings."""
    x3 = inputs(3, 266, 350).cuda()
    x = x3[:2].contiguous()
    a = vits_model.forward(x)
    b = vits_model.forward(x)
    assert torch.equal(a, b)
    one = vits_model.forward(x[1:2])
    assert torch.equal(one[0], a[1])
    sq = vits_model.forward(inputs(1, 266, 266).cuda())
    assert tuple(sq.shape) == (1, 266, 266) and torch.isfinite(sq).all()
    assert torch.equal(vits_model.forward(x), a)
    a3 = vits_model.forward(x3)
    assert torch.equal(a3[:2], a)
    for i in range(3):
        assert torch.equal(vits_model.forward(x3[i:i + 1])[0], a3[i]), i
    eng = vits_model._eng
    try:
        vits_model.set_batch_invariant(False)
        e2, e3 = rel_l2(vits_model.forward(x), a), rel_l2(vits_model.forward(x3), a3)
        print(f"[metric no state] one pass against frame by frame: batch 2 rel-L2 {e2:.2e}, batch 3 (low-resolution output_conv1) {e3:.2e}")
        assert vits_model._eng is eng
        took_lowres = ("oc1_z", (3 * 76 * 100, 9 * 32), torch.float32) in eng["rt"]._bufs
        assert took_lowres, "the one-pass batch of three did not cross the low-resolution threshold"
        assert e2 < 1e-5 and e3 < 3e-5
    finally:
        vits_model.set_batch_invariant(True)
    assert torch.equal(vits_model.forward(x), a)


def test_max_depth_is_read_at_launch(vits_model):
    x = inputs(1, 266, 350).cuda()
    assert vits_model.max_depth == 20.0
    d20 = vits_model.forward(x)
    eng = vits_model._eng
    vits_model.max_depth = 80
    try:
        d80 = vits_model.forward(x)
        assert vits_model._eng is eng, "changing max_depth rebuilt the engines"
        assert torch.equal(d80, 4.0 * d20)   # x 4 is exact in binary floating point
        assert float(d80.max()) > 20.0
    finally:
        vits_model.max_depth = 20.0


# ------------------------------------------------------------------------------------------------ 6. image drivers
def test_infer_image_and_vis(vits_model):
    """infer_image = the align-corners bilinear resize of forward(image2tensor(frame)) back to the frame, to the 1e-3 that
    test_image2tensor_and_infer_image_against_oracle gives that step; (240, 320), values in [0, max_depth];
    infer_image_vis(palette='Spectral', pred_only=True) = vdn.vis.colorize of that map, byte for byte."""
    from vdn import synth, vis
    img = np.ascontiguousarray(synth.frames_u8(1234, 1, 240, 320)[0][:, :, ::-1])
    x, (hh, ww) = vits_model.image2tensor(img, input_size=266)
    assert (hh, ww) == (240, 320) and tuple(x.shape) == (1, 3, 266, 350)
    net = vits_model.forward(x)
    want = F.interpolate(net[:, None].cpu(), (240, 320), mode="bilinear", align_corners=True)[0, 0]
    d = vits_model.infer_image(img, input_size=266)
    e = rel_l2(d, want)
    print(f"[metric infer_image] 240x320 -> 266x350 -> 240x320: rel-L2 vs torch's resize of the forward {e:.2e}")
    assert d.shape == (240, 320) and d.dtype == np.float32 and np.isfinite(d).all() and e < TOL
    assert d.min() >= 0.0 and d.max() <= vits_model.max_depth
    pic = vits_model.infer_image_vis(img, input_size=266, pred_only=True, palette="Spectral")
    ref = vis.colorize(torch.from_numpy(d).cuda(), palette="Spectral").cpu().numpy()
    assert pic.dtype == np.uint8 and pic.shape == (240, 320, 3) and np.array_equal(pic, ref)
    assert inspect_default(vits_model.infer_image_vis, "palette") == "Spectral"
    both = vits_model.infer_image_vis(img, input_size=266)
    assert both.shape == (240, 2 * 320 + 50, 3) and np.array_equal(both[:, :320], img) and np.array_equal(both[:, 370:], pic)
    pts, col = vits_model.infer_image_points(img, input_size=266, fx=470.4, fy=431.7)
    assert pts.is_cuda and pts.dtype == torch.float64 and tuple(pts.shape) == (240 * 320, 3) and tuple(col.shape) == (240 * 320, 3)
    wp, wc = _points_numpy(d, img[:, :, ::-1], 470.4, 431.7)
    assert np.array_equal(pts.cpu().numpy(), wp) and np.array_equal(col.cpu().numpy(), wc)


def inspect_default(fn, name):
    import inspect
    return inspect.signature(fn).parameters[name].default


# ------------------------------------------------------------------------------------------------ 7. points
def _points_numpy(pred, color_image, focal_length_x, focal_length_y):
    """depth_to_pointcloud.py:99-104, as written there."""
    height, width = pred.shape
    x, y = np.meshgrid(np.arange(width), np.arange(height))
    x = (x - width / 2) / focal_length_x
    y = (y - height / 2) / focal_length_y
    z = np.array(pred)
    points = np.stack((np.multiply(x, z), np.multiply(y, z), z), axis=-1).reshape(-1, 3)
    colors = np.array(color_image).reshape(-1, 3) / 255.0
    return points, colors


@pytest.mark.parametrize("hw", [(23, 37), (133, 260)])
def test_depth_to_points_is_numpy_bit_for_bit(hw):
    """23 x 37 = 851 pixels: one partial block and an odd last pixel; 133 x 260: several blocks, even count. fx != fy. A zero,
    a very large and a denormal depth are planted. Bar: np.array_equal on both outputs."""
    from vdn.points import depth_to_points
    hh, ww = hw
    rs = np.random.RandomState(hh * 1000 + ww)
    depth = (rs.rand(hh, ww) * 20.0).astype(np.float32)
    depth[0, 0], depth[hh // 2, ww // 3], depth[-1, -1], depth[1, 2] = 0.0, 3.0e38, 1.0e30, 1.0e-40
    rgb = rs.randint(0, 256, (hh, ww, 3)).astype(np.uint8)
    rgb[0, 0], rgb[-1, -1] = (0, 255, 1), (255, 0, 254)
    wp, wc = _points_numpy(depth, rgb, 470.4, 431.7)
    pts, col = depth_to_points(torch.from_numpy(depth).to(DEV), torch.from_numpy(rgb).to(DEV), 470.4, 431.7)
    assert pts.dtype == col.dtype == torch.float64 and tuple(pts.shape) == tuple(col.shape) == (hh * ww, 3)
    assert wp.dtype == np.float64 and np.array_equal(pts.cpu().numpy(), wp)
    assert np.array_equal(col.cpu().numpy(), wc)
    # host tensors are copied once; the result stays on the device
    pts2, _ = depth_to_points(torch.from_numpy(depth), torch.from_numpy(rgb), 470.4, 431.7)
    assert pts2.is_cuda and torch.equal(pts2, pts)


# ------------------------------------------------------------------------------------------------ 8. loop body
def test_metric_validate_step_runs_on_the_model(vits_model):
    """metric_depth/train.py:160-177 with the new model as `model`: a 266 x 350 image, a 300 x 400 target, a mask that drops
    pixels. [B, 10]; column 0 is the mask count; the nine scores are tests/metric_ref.py's on the model's own prediction, to the
    bars of tests/test_gpu_metric.py. Plumbing only: the model's precision is held above."""
    import metric_ref as R
    from test_gpu_metric import check_rows
    from vdn.steps import DepthMetricMeter, metric_validate_step
    B, H, W = 2, 300, 400
    image = inputs(B, 266, 350)
    rs = np.random.RandomState(7)
    target = (rs.rand(B, H, W) * 24.0).astype(np.float32)      # some above max_depth = 20, some below min_depth
    target[:, :5] = 0.0
    mask = (rs.rand(B, H, W) > 0.2)
    sample = dict(image=image, depth=torch.from_numpy(target).cuda(), valid_mask=torch.from_numpy(mask).cuda())
    meter = DepthMetricMeter()
    rows = metric_validate_step(vits_model, sample, min_depth=0.001, max_depth=20, meter=meter)
    assert tuple(rows.shape) == (B, 10) and rows.dtype == torch.float64 and rows.is_cuda
    pred = vits_model(image.cuda()).cpu().numpy()
    keep = R.keep_mask(mask, target, 0.001, 20)
    assert 0 < keep.sum() < mask.sum() < mask.size
    assert rows[:, 0].cpu().tolist() == [float(keep[b].sum()) for b in range(B)]
    check_rows(rows, R.eval_rows(pred, target, mask, 0.001, 20))
    from vdn.metric import KEYS
    means = meter.means()
    assert tuple(means) == KEYS and all(np.isfinite(v) for v in means.values())
