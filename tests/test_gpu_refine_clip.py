"""The depth refiners' windowed clip driver on the MI355X: `refine_video_depth` against the fixtures the imported reference's
halves wrote (RC5_vits, RC3_vits, RC2_vits: 50 frames, three windows, the last mostly padding), vdn_refine_window_tail against
the launches it fuses, bit for bit, and the driver's parts (clip-level tap cache, front once per distinct frame, device
stitcher, the per-window fallback, the colourised variant, the input checks) against `forward` and the host restatements.
ViT-S throughout. Tolerances: 1e-3 on rel-L2 and worst pixel against the reference (README); rel-L2 < 1e-5 and worst pixel <
1e-4 of max for the cache against `forward`, and rtol 5e-5 / atol 1e-5 max|host| for the stitcher chain, the bounds of
test_gpu_e2e.test_infer_video_depth_256_frames_vitl_518_full_size."""
import importlib
from functools import lru_cache

import numpy as np
import pytest
import torch

import refine_clip_ref as RC
from common import rel_l2, synth_sd, worst_px

pytestmark = pytest.mark.gpu
TOL = 1e-3
DEV = "cuda"
PAD, CANARY = 8, -777.0


@pytest.fixture(scope="module")
def rt():
    from vdn.runtime import Runtime
    from vdn import _abi
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    assert _abi.lib.vdn_arch_ok() == 1, "not a gfx950 device"
    return Runtime(torch.device("cuda:0"), torch.float16)


def _cls(version):
    return importlib.import_module(f"vdn.video_depth_model_v{version}").VideoDepthAnything


@lru_cache(maxsize=None)
def _model(name):
    """The refiner of a fixture, or "R4": v4 with the plain synthetic draw (no fixture)."""
    import vdn
    version, sd = (4, synth_sd("R4", "vits")) if name == "R4" else (RC.fixture(name)[1], RC.fixture(name)[3])
    m = _cls(version)(**vdn.MODEL_CONFIGS["vits"])
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


@lru_cache(maxsize=None)
def _clip(name):
    from vdn import synth
    return synth.depth_clip(77, 50, 42, 56) if name == "R4" else RC.fixture(name)[2]


@lru_cache(maxsize=None)
def _windows(name):
    """Per window of the 50-frame clip: (what the clip driver's generator yields, a fresh `forward` of the same 32 gathered
    frames), both on the host; computed once and shared."""
    from vdn import util
    m, x = _model(name), torch.from_numpy(_clip(name)).to(DEV)
    new = [d.clone() for d in m._refined_windows(x)]   # the generator rewrites one buffer
    fresh = [m.forward(x[torch.tensor(idxs, device=DEV)][None])[0] for idxs in util.window_table(x.shape[0])]
    return [d.cpu().numpy() for d in new], [d.cpu().numpy() for d in fresh]


@lru_cache(maxsize=None)
def _result(name):
    d, fps = _model(name).refine_video_depth(_clip(name), 24)
    assert fps == 24
    return d.copy()   # the driver's result aliases a reused pinned buffer


# ------------------------------------------------------------------------------------------------ 1. reference parity
@pytest.mark.parametrize("name", list(RC.FIXTURES))
def test_refine_video_depth_against_reference_fixture(name):
    g = RC.fixture(name)[0]
    d = _result(name)
    e, w = rel_l2(d, g["out"]), worst_px(d, g["out"])
    print(f"[{name}] refine_video_depth vs reference fixture: rel-L2 {e:.2e} worst pixel {w:.2e}; zeros among frames >= 32: "
          f"{RC.zero_share(d):.4f} (fixture {RC.zero_share(g['out']):.4f})")
    assert d.shape == g["out"].shape and d.dtype == np.float32 and np.isfinite(d).all()
    assert e <= TOL and w <= TOL


# ------------------------------------------------------------------------------------------------ 2. the tail kernel
def _placed(values, off):
    """`values` at float offset `off` of a canary-filled device allocation: (whole buffer, the view the kernel gets)."""
    buf = torch.full((off + values.numel() + PAD,), CANARY, dtype=torch.float32, device=DEV)
    view = buf[off:off + values.numel()].view(values.shape)
    view.copy_(values)
    return buf, view


def _tail_cases():
    from vdn import _abi
    narrow, wide = _abi.lib.vdn_refine_window_tail_trip(0), _abi.lib.vdn_refine_window_tail_trip(1)
    assert (narrow, wide) == (16384, 65536)   # what the two large shapes below were chosen for
    cases = []
    for kind in ("shift", "unit", "mix"):
        cases += [
            (kind, (37, 53), (37, 53), 0),        # same size, odd row: one pixel per lane
            (kind, (40, 56), (40, 56), 0),        # same size, rows of 4 pixels: 16-byte accesses
            (kind, (224, 224), (37, 53), 0),      # the v5 resample to an odd size, row tail
            (kind, (224, 224), (36, 52), 0),      # the resample with four pixels per lane
        ]
    cases += [
        ("shift", (40, 56), (40, 56), 1),         # a base off 16 bytes: rows of 4 pixels on the one-pixel path
        ("shift", (131, 127), (131, 127), 0),     # 16 637 pixels: past the first grid round, one pixel per lane
        ("mix", (30, 28), (131, 127), 0),         # the same, resampled
        ("shift", (260, 256), (260, 256), 0),     # 66 560 pixels: past the first round of the 4-pixel lanes
        ("mix", (65, 64), (260, 256), 0),         # the same, resampled
    ]
    return cases


@pytest.mark.parametrize("kind,net_hw,out_hw,off", _tail_cases())
def test_window_tail_equals_the_unfused_launches(rt, kind, net_hw, out_hw, off):
    """vdn_refine_window_tail == index_select by slots -> vdn_upsample_bilinear_f32(relu) where the sizes differ ->
    vdn_refine_finish / vdn_refine_mix, with torch.equal: the kernels share their per-pixel device functions. A slot table
    with repeats over a 4-frame clip; nothing is written outside the output."""
    from vdn import _abi
    slots = [3, 0, 3, 1, 0] if out_hw[0] * out_hw[1] < 60000 else [1, 1]
    T, frames = len(slots), 4
    gen = torch.Generator().manual_seed(out_hw[0] * 1000 + net_hw[1])
    net = torch.randn((T, *net_hw), generator=gen).to(DEV)              # signed: the second rectification matters
    scaled = torch.rand((frames, *out_hw), generator=gen).to(DEV)
    st = torch.tensor(slots, dtype=torch.int32, device=DEV)
    if kind == "mix":
        from vdn.refiner import fold_final_res
        import refiner_ref as R
        import torch.nn as nn
        seq = nn.Sequential(nn.Conv2d(2, 1, 1), nn.BatchNorm2d(1), nn.ReLU(), nn.Conv2d(1, 1, 1), nn.BatchNorm2d(1), nn.ReLU()).eval()
        seq.load_state_dict(R.with_final_res(seq.state_dict(), {k[10:]: v for k, v in R.R2_FINAL_RES.items()}))
        coef = fold_final_res(seq)
    else:
        coef = (0.37, -0.21, 65535.0, 0.0, 0.0)
    # the unfused composition
    gathered = scaled.index_select(0, st.long()).contiguous()
    if net_hw != out_hw:
        d0 = torch.empty((T, *out_hw), dtype=torch.float32, device=DEV)
        rt.upsample_f32(net, d0, T, *net_hw, *out_hw, relu=True)
    else:
        d0 = net
    want = torch.empty((T, *out_hw), dtype=torch.float32, device=DEV)
    if kind == "mix":
        rt.refine_mix(d0, gathered, *coef, want)
    else:
        rt.refine_finish(gathered if kind == "shift" else None, d0, coef[0], coef[1], coef[2], kind == "shift", want)
    # the fused kernel, into a canary-framed output
    obuf, out = _placed(torch.zeros((T, *out_hw)), off)
    rt.refine_window_tail(net, None if kind == "unit" else scaled, st, _abi.TAIL_MIX if kind == "mix" else _abi.TAIL_SHIFT,
                          kind == "shift", coef, out)
    n = out.numel()
    assert bool((obuf[:off] == CANARY).all()) and bool((obuf[off + n:] == CANARY).all())
    if kind == "mix":   # both kinks of the mix are exercised
        assert 0.02 < float((want == 0).float().mean()) < 0.98
    assert torch.equal(out, want), int((out != want).sum())


def test_window_tail_rejects_wrong_operands(rt):
    from vdn import _abi
    net, scaled = torch.zeros((2, 8, 8), device=DEV), torch.zeros((3, 8, 8), device=DEV)
    out, st = torch.empty((2, 8, 8), device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    coef = (1.0, 0.0, 1.0, 0.0, 0.0)
    with pytest.raises(_abi.VdnError):
        rt.refine_window_tail(net, scaled[:, :7], st, _abi.TAIL_SHIFT, True, coef, out)        # scaled of another frame size
    with pytest.raises(_abi.VdnError):
        rt.refine_window_tail(net, scaled, st.long(), _abi.TAIL_SHIFT, True, coef, out)        # int64 slots
    with pytest.raises(_abi.VdnError):
        rt.refine_window_tail(net, None, st, _abi.TAIL_MIX, True, coef, out)                   # the mix reads scaled
    with pytest.raises(_abi.VdnError):
        rt.refine_window_tail(net, scaled, st[:1], _abi.TAIL_SHIFT, True, coef, out)           # one slot for two maps


# ------------------------------------------------------------------------------------------------ 3. cache and front-once
@pytest.mark.parametrize("name", ["R4", "RC5_vits"])
def test_windows_from_the_tap_cache_equal_a_fresh_forward(name):
    """Every window of the 50-frame clip from the new path (front once per distinct frame, encoder taps from the clip-level
    cache, the fused tail) against `forward` of the same 32 gathered frames."""
    new, fresh = _windows(name)
    assert len(new) == len(fresh) == 3
    for w, (a, b) in enumerate(zip(new, fresh)):
        e, worst = rel_l2(a, b), float(np.abs(a - b).max() / np.abs(b).max())
        print(f"[{name}] window {w}: clip path vs fresh forward rel-L2 {e:.2e}, worst pixel {worst:.2e} of max")
        assert e < 1e-5 and worst < 1e-4, (w, e, worst)


# ------------------------------------------------------------------------------------------------ 4. stitcher chain
@pytest.mark.parametrize("name", ["R4", "RC5_vits"])
def test_clip_equals_host_stitch_of_the_forward_windows(name):
    from vdn import util
    _, fresh = _windows(name)
    d = _result(name)
    host = util.stitch([w[i] for w in fresh for i in range(util.INFER_LEN)], d.shape[0])
    err = float(np.abs(d - host).max() / np.abs(host).max())
    print(f"[{name}] refine_video_depth vs util.stitch of the per-window forwards: worst pixel {err:.2e} of max")
    assert d.shape == host.shape and np.allclose(d, host, rtol=5e-5, atol=1e-5 * float(np.abs(host).max())), err


# ------------------------------------------------------------------------------------------------ 5. one padded window
@pytest.mark.parametrize("name", ["RC3_vits", "RC5_vits"])
@pytest.mark.parametrize("n", [22, 1])
def test_short_clip_is_forward_of_the_padded_window(name, n):
    """N <= 22 is one window: the clip, then copies of its last frame. Its encoder batch is that window itself and the tail
    has the bits of the unfused launches, so the result EQUALS `forward` of the padded window, cut to N."""
    m = _model(name)
    x = torch.from_numpy(_clip(name)[:n]).to(DEV)
    d, _ = m.refine_video_depth(x)
    d = d.copy()
    padded = torch.cat([x, x[-1:].expand(32 - n, -1, -1)])[None]
    want = m.forward(padded)[0, :n].cpu().numpy()
    assert d.shape == want.shape == (n, *x.shape[1:])
    assert np.array_equal(d, want), (rel_l2(d, want), worst_px(d, want))


# ------------------------------------------------------------------------------------------------ 6. the fallback
def test_tap_cache_budget_zero_falls_back_to_forward_per_window(monkeypatch):
    name = "RC5_vits"
    monkeypatch.setenv("VDN_TAP_CACHE_GB", "0")
    d, _ = _model(name).refine_video_depth(_clip(name))
    d = d.copy()
    monkeypatch.delenv("VDN_TAP_CACHE_GB")
    ref = _result(name)
    e, worst = rel_l2(d, ref), float(np.abs(d - ref).max() / np.abs(ref).max())
    print(f"[{name}] VDN_TAP_CACHE_GB=0 vs the cached path: rel-L2 {e:.2e}, worst pixel {worst:.2e} of max")
    assert e < 1e-5 and worst < 1e-4


# ------------------------------------------------------------------------------------------------ 7. the colourised variant
def test_refine_video_depth_vis_is_colorize_of_the_clip():
    from vdn import vis
    name = "RC5_vits"
    m, d = _model(name), torch.from_numpy(_result(name)).to(DEV)
    got, fps = m.refine_video_depth_vis(_clip(name), 24)
    assert fps == 24 and got.dtype == np.uint8 and got.shape == (*d.shape, 3)
    assert np.array_equal(got, vis.colorize(d, palette="inferno", order="rgb", scope="clip").cpu().numpy())
    got, _ = m.refine_video_depth_vis(_clip(name), 24, grayscale=True)
    assert got.shape == tuple(d.shape)
    assert np.array_equal(got, vis.colorize(d, scope="clip", grayscale=True, gray_channels=1)[..., 0].cpu().numpy())
    with pytest.raises(ValueError):
        m.refine_video_depth_vis(_clip(name), 24, palette="viridis")


# ------------------------------------------------------------------------------------------------ 8. input checks
def test_input_checks_raise_before_any_launch(monkeypatch):
    m3, m5 = _model("RC3_vits"), _model("RC5_vits")

    def launched(*a, **k):
        raise RuntimeError("the engines were asked for: a launch would follow")

    for m in (m3, m5):
        monkeypatch.setattr(m, "_engines", launched)
    with pytest.raises(AssertionError, match="multiple of the patch size 14"):
        m3.refine_video_depth(np.zeros((3, 40, 56), np.float32))
    for m in (m3, m5):
        with pytest.raises(ValueError):
            m.refine_video_depth(np.zeros((1, 3, 42, 56), np.float32))
        with pytest.raises(ValueError):
            m.refine_video_depth(torch.zeros((0, 42, 56)))
        with pytest.raises(ValueError):
            m.refine_video_depth_vis(np.zeros((42, 56), np.float32))
        with pytest.raises(ValueError):
            m.refine_video_depth([[[1.0]]])


def test_any_real_dtype_and_container_is_staged(monkeypatch):
    """numpy or tensor, host or device, f64 / u16-range integers: the same clip gives the same result."""
    m = _model("RC3_vits")
    clip = np.round(_clip("RC3_vits")[:5])
    want = m.refine_video_depth(clip)[0].copy()
    for other in (clip.astype(np.float64), clip.astype(np.int32), torch.from_numpy(clip).to(DEV), torch.from_numpy(clip).double()):
        got = m.refine_video_depth(other)[0]
        assert np.array_equal(got, want)
