"""VideoDepthEstimationModel.infer_video on the MI355X: vdn_dn_stitch_apply value for value against the
float32 numpy expression, one window against `forward` bit for bit, several windows against the restated loop (`forward` on
each window's gathered frames, then the float64 host stitch of tests/dn_clip_ref.py), the fallback without a cache, native
trunks, repeat calls, the pictures and the refusals. Stand-in trunks (synth.dn_trunk) on 32 x 32 frames with 8 x 8 .. 1 x 1
feature maps, the smallest the head's kernels take; synthetic weights from dn_fixture.state_dict."""
import numpy as np
import pytest
import torch

import dn_clip_ref as R
import dn_fixture as DF
from common import rel_l2, worst_px
from test_gpu_dn_head import TOL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PAD, CANARY = 64, -777.0
EINVAL = -1
HW = 32
SIZES = ((8, 8), (4, 4), (2, 2), (1, 1))
SEED = 4321   # of the input clip; test_several_windows asserts that every fit of the reference is well conditioned with it


def _rt():
    from vdn.runtime import Runtime
    return Runtime(DEV, torch.float16, True)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fresh(shape, fill=CANARY):
    """(whole allocation, the output the kernel gets): `shape` filled with `fill`, PAD canaries behind it."""
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), CANARY, dtype=torch.float32, device=DEV)
    buf[:n] = fill
    return buf, buf[:n].view(shape)


def _pad_intact(*bufs):
    torch.cuda.synchronize()
    return all(bool((b[-PAD:] == CANARY).all()) for b in bufs)


# ================================================================================================ 1. vdn_dn_stitch_apply
def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _apply_case(T, hw, overlap, keep, clamp0, seed, extra=2):
    """The clip has `extra` frames behind the window's T: they and the frames keep .. T-1 hold canaries that must survive."""
    rt = _rt()
    depth, normal = _rnd(T, 1, hw, seed=seed), _rnd(T, 3, 1, hw, seed=seed + 1)     # both signs
    scale, shift = np.float32(1.3), np.float32(-0.2)
    (db, od), (nb, on) = _fresh((T + extra, 1, hw)), _fresh((T + extra, 3, 1, hw))
    if overlap:
        od[:overlap] = _rnd(overlap, 1, hw, seed=seed + 2).abs().to(DEV)
        on[:overlap] = _rnd(overlap, 3, 1, hw, seed=seed + 3).to(DEV)
    before_d, before_n = od.cpu().numpy().reshape(T + extra, hw), on.cpu().numpy().reshape(T + extra, 3, hw)
    want_d, want_n = R.stitch_apply32(depth.numpy().reshape(T, hw), normal.numpy().reshape(T, 3, hw), scale, shift, before_d, before_n,
                                      overlap, keep, clamp0)
    assert np.array_equal(want_d[keep:], before_d[keep:]) and (want_d[keep:] == CANARY).all()
    mapped = depth.numpy().reshape(T, hw)[overlap:keep] * scale + shift
    if clamp0:
        assert (want_d[overlap:keep] == 0).any() and (want_d[overlap:keep] > 0).any() and (mapped < 0).any()   # the clamp cut some
    else:
        assert (want_d[overlap:keep] < 0).any()
    coef = torch.tensor([float(scale), float(shift)], dtype=torch.float32, device=DEV)
    rt.dn_stitch_apply(depth.to(DEV), normal.to(DEV), coef, od, on, overlap, keep, clamp0)
    assert _pad_intact(db, nb)
    got_d, got_n = od.cpu().numpy().reshape(T + extra, hw), on.cpu().numpy().reshape(T + extra, 3, hw)
    for name, g, w in (("out_depth", got_d, want_d), ("out_normal", got_n, want_n)):
        assert np.array_equal(g, w), (name, int((g != w).sum()), float(np.abs(g - w).max()))
    assert (got_n[:keep, 2] == 1).all()


@pytest.mark.parametrize("T,hw,overlap,keep,clamp0", [
    (5, 5, 2, 5, True),       # two blend frames: the weights are 0 and 1
    (5, 5, 2, 5, False),
    (6, 8, 0, 6, True),       # a first window: nothing of the clip is read (hw % 4 == 0: 16-byte accesses)
    (8, 12, 4, 6, True),      # keep < T: the pad slots behind the end of the clip stay out; weights 0, 1/3, 2/3, 1
    (8, 7, 3, 4, False),      # an odd overlap, one stored frame
], ids=["w01_clamp", "w01", "first_window", "keep<T", "odd_overlap"])
def test_dn_stitch_apply_is_the_float32_expression(T, hw, overlap, keep, clamp0):
    _apply_case(T, hw, overlap, keep, clamp0, seed=100 * T + hw)


@pytest.mark.parametrize("vec", [False, True], ids=["4-byte", "16-byte"])
def test_dn_stitch_apply_second_grid_trip(vec):
    """The smallest planes whose last pixel groups fall to the second trip of the grid-stride loop, on the 4-byte path with
    hw % 4 != 0 and on the 16-byte path, from the launch grid include/vdn.h states."""
    T, keep = 5, 5
    _, lanes, _ = R.launch_grid(1 << 30, keep, vec)
    hw = lanes + 5 if not vec else 4 * (lanes + 3)
    assert (hw % 4 != 0) == (not vec)
    gx, lanes, groups = R.launch_grid(hw, keep, vec)
    assert lanes < groups <= 2 * lanes and gx * 256 == lanes      # a second trip, for fewer lanes than a block
    _apply_case(T, hw, 2, keep, True, seed=7 + vec)


def test_dn_stitch_apply_unaligned_clip_frame_takes_the_4_byte_path():
    """hw % 4 == 0 but the clip frame the window starts at is not 16-byte aligned: same values."""
    rt = _rt()
    T, hw = 4, 8
    depth, normal = _rnd(T, 1, hw, seed=1).to(DEV), _rnd(T, 3, 1, hw, seed=2).to(DEV)
    coef = torch.tensor([0.7, 0.1], dtype=torch.float32, device=DEV)
    outs = []
    for shift in (0, 1):
        db, nb = torch.full((T * hw + 4 + PAD,), CANARY, device=DEV), torch.full((T * 3 * hw + 4 + PAD,), CANARY, device=DEV)
        od, on = db[shift:shift + T * hw].view(T, 1, hw), nb[shift:shift + 3 * T * hw].view(T, 3, 1, hw)
        assert od.data_ptr() % 16 == 4 * shift
        rt.dn_stitch_apply(depth, normal, coef, od, on, 0, T, False)
        assert _pad_intact(db, nb) and bool((db[:shift] == CANARY).all()) and bool((nb[:shift] == CANARY).all())
        outs.append((od.cpu(), on.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("T,overlap,keep,hw", [(8, 1, 8, 5), (8, 5, 8, 5), (9, 5, 9, 5), (8, 2, 2, 5), (8, 4, 3, 5), (8, 2, 9, 5), (8, 0, 0, 5),
                                               (8, 2, 8, 0), (8, -2, 8, 5)],
                         ids=["overlap=1", "overlap>T/2", "overlap>T/2_odd", "keep=overlap", "keep<overlap", "keep>T", "keep<1", "hw=0",
                              "overlap<0"])
def test_dn_stitch_apply_rejects(T, overlap, keep, hw):
    from vdn import _abi
    px = max(hw, 5)
    depth, normal, coef = torch.ones(T, px, device=DEV), torch.ones(T, 3, px, device=DEV), torch.ones(2, device=DEV)
    (db, od), (nb, on) = _fresh((T + 2, px)), _fresh((T + 2, 3, px))
    rc = _abi.lib.vdn_dn_stitch_apply(depth.data_ptr(), normal.data_ptr(), coef.data_ptr(), od.data_ptr(), on.data_ptr(), hw, T, overlap,
                                      keep, 1, _stream())
    torch.cuda.synchronize()
    assert rc == EINVAL and bool((db == CANARY).all()) and bool((nb == CANARY).all())


# ================================================================================================ the model
_MODELS, _CLIPS = {}, {}


def _model(S, relu=False, res=False):
    key = (S, relu, res)
    if key not in _MODELS:
        import vdn
        from vdn import synth
        m = vdn.VideoDepthEstimationModel(S, use_residual=res, use_final_relu=relu, trunk=synth.dn_trunk(sizes=SIZES),
                                          img_trunk=synth.dn_trunk(sizes=SIZES))
        m.load_state_dict(DF.state_dict(m), strict=True)
        _MODELS[key] = m.to(DEV).eval()
    return _MODELS[key]


def _clip(N, hw=HW, gamma=1):
    """(depths f32 [N, hw, hw] in (0, 1), frames f32 [N, 3, hw, hw]) on the device, computed once per length. gamma = 2 squares
    the depth: more contrast, for a model whose output is little more than its input (a flat map has no well-conditioned fit)."""
    if (N, hw, gamma) not in _CLIPS:
        from vdn import synth
        d = synth.depth_clip(SEED, N, hw, hw, max_depth=1.0).astype(np.float32) ** gamma
        f = synth.normalize_frames(synth.frames_u8(SEED, N, hw, hw)).astype(np.float32)
        _CLIPS[N, hw, gamma] = torch.from_numpy(d).to(DEV), torch.from_numpy(f).to(DEV)
    return _CLIPS[N, hw, gamma]


def _restated_loop(m, d, f, S, overlap, align):
    """`forward` on every window's gathered frames, then the float64 host stitch -> (depth, normal, coefs, fits)."""
    N = d.shape[0]
    wd, wn = [], []
    for row in R.window_table(N, S, overlap):
        idx = torch.tensor(row, device=DEV)
        dd, nn = m(d[idx][None], f[idx][None])
        wd.append(dd[0].double().cpu().numpy())
        wn.append(nn[0].double().cpu().numpy())
    return R.stitch64(wd, wn, N, overlap, align=align, clamp0=m.use_final_relu)


def _hold(where, got_d, got_n, coefs, ref):
    ref_d, ref_n, ref_c, fits = ref
    for det, s0, s2 in fits:
        assert det >= 0.05 * s0 * s2, (where, "an ill-conditioned fit in the reference", det / (s0 * s2))
    gd, gn = got_d.double().cpu(), got_n.double().cpu()
    rd, rn = torch.from_numpy(ref_d), torch.from_numpy(ref_n)
    assert torch.isfinite(rd).all() and torch.isfinite(rn).all()
    for name, g, r in (("depth", gd, rd), ("nx", gn[:, 0], rn[:, 0]), ("ny", gn[:, 1], rn[:, 1]),
                       ("coefs", coefs.double().cpu(), torch.from_numpy(ref_c))):
        e, w = rel_l2(g, r), worst_px(g, r)
        print(f"[dn_clip {where}] {name}: rel-L2 {e:.2e} worst {w:.2e} (bar {TOL:.0e})")
        assert e < TOL and w < TOL, (where, name, e, w)
    assert bool((got_n[:, 2] == 1).all())
    if fits:
        print(f"[dn_clip {where}] coefs {ref_c.tolist()} det/(s0 s2) {[f[0] / (f[1] * f[2]) for f in fits]}")


# ------------------------------------------------------------------------------------------------ 2. one window is forward
@pytest.mark.parametrize("N", [4, 3], ids=["N=S", "N=S-1"])
@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
def test_one_window_is_forward(N, res):
    S = 4
    m = _model(S, relu=True, res=res)
    d, f = _clip(N)
    idx = torch.tensor([min(i, N - 1) for i in range(S)], device=DEV)
    want_d, want_n = m(d[idx][None], f[idx][None])
    got_d, got_n = m.infer_video(d, f, overlap=2)
    assert got_d.shape == (N, HW, HW) and got_n.shape == (N, 3, HW, HW) and got_d.dtype == got_n.dtype == torch.float32
    assert torch.equal(got_d, want_d[0, :N]) and torch.equal(got_n, want_n[0, :N])
    assert torch.equal(m._clip_coefs.cpu(), torch.tensor([[1.0, 0.0]]))
    assert float(got_d.abs().max()) > 0 and float(got_n[:, :2].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 3. several windows
CASES = [(4, 2, 7, False, False, True), (4, 2, 7, True, False, True), (6, 3, 11, False, False, True), (6, 3, 11, True, True, True),
         (4, 0, 9, True, False, True), (4, 2, 7, False, True, True), (6, 3, 11, False, False, False)]
IDS = ["S4o2N7", "S4o2N7_relu", "S6o3N11", "S6o3N11_relu_res", "S4o0N9_relu", "S4o2N7_res", "S6o3N11_noalign"]


@pytest.mark.parametrize("S,overlap,N,relu,res,align", CASES, ids=IDS)
def test_several_windows_against_the_restated_loop(S, overlap, N, relu, res, align):
    m = _model(S, relu=relu, res=res)
    d, f = _clip(N)
    ref = _restated_loop(m, d, f, S, overlap, align)
    assert len(ref[3]) == (len(R.window_table(N, S, overlap)) - 1 if align and overlap else 0)
    got_d, got_n = m.infer_video(d, f, overlap=overlap, align=align)
    assert m._clip_coefs.shape == (len(R.window_table(N, S, overlap)), 2)
    _hold(f"S={S} overlap={overlap} N={N} relu={relu} res={res} align={align}", got_d, got_n, m._clip_coefs, ref)
    if not (align and overlap):
        assert torch.equal(m._clip_coefs.cpu(), torch.tensor([[1.0, 0.0]]).repeat(len(ref[2]), 1))


# ------------------------------------------------------------------------------------------------ 4. fallback equals cached
@pytest.mark.parametrize("S,overlap,N,relu,res", [(4, 2, 7, True, False), (6, 3, 11, False, True)], ids=["S4o2N7_relu", "S6o3N11_res"])
def test_fallback_without_a_cache_equals_cached(S, overlap, N, relu, res, monkeypatch):
    m = _model(S, relu=relu, res=res)
    d, f = _clip(N)
    cached = tuple(t.clone() for t in m.infer_video(d, f, overlap=overlap))
    coefs = m._clip_coefs.clone()
    calls = []
    fwd = m.forward
    monkeypatch.setattr(m, "forward", lambda *a: (calls.append(1), fwd(*a))[1])
    monkeypatch.setenv("VDN_TAP_CACHE_GB", "0")
    got_d, got_n = m.infer_video(d, f, overlap=overlap)
    assert len(calls) == len(R.window_table(N, S, overlap)), "the fallback did not run: forward once per window"
    for name, g, r in (("depth", got_d, cached[0]), ("nx", got_n[:, 0], cached[1][:, 0]), ("ny", got_n[:, 1], cached[1][:, 1]),
                       ("coefs", m._clip_coefs, coefs)):
        e, w = rel_l2(g.double().cpu(), r.double().cpu()), worst_px(g.double().cpu(), r.double().cpu())
        print(f"[dn_clip fallback S={S} N={N}] {name}: rel-L2 {e:.2e} worst {w:.2e}")
        assert e < TOL and w < TOL, (name, e, w)
    assert bool((got_n[:, 2] == 1).all())


# ------------------------------------------------------------------------------------------------ 5. native trunks
def test_native_trunks_against_the_restated_loop():
    """Both Hiera trunks through the clip cache. use_residual with a squared input depth: without them the synthetic weights
    give a nearly flat depth (det = 0.013 s0 s2 measured) whose fit the reference itself does not determine."""
    import vdn
    S, overlap, N = 4, 2, 6
    m = vdn.VideoDepthEstimationModel.with_native_trunks(S, encoder="hiera_tiny_224", use_residual=True)
    m.load_state_dict(DF.state_dict(m), strict=True)
    m = m.to(DEV).eval()
    d, f = _clip(N, 224, gamma=2)
    ref = _restated_loop(m, d, f, S, overlap, True)
    got_d, got_n = m.infer_video(d, f, overlap=overlap)
    _hold("native hiera_tiny_224 S=4 overlap=2 N=6", got_d, got_n, m._clip_coefs, ref)


# ------------------------------------------------------------------------------------------------ 6. repeat calls
def test_repeat_call_allocates_nothing_and_is_bitwise_equal():
    m = _model(4, relu=True, res=True)
    d, f = _clip(7)
    d0, n0 = (t.clone() for t in m.infer_video(d, f, overlap=2))
    c0 = m._clip_coefs.clone()
    rt = m._eng["rt"]
    nbufs, nbytes = len(rt._bufs), rt.workspace_bytes()
    torch.cuda.synchronize()
    reserved = torch.cuda.memory_reserved(DEV)
    d1, n1 = m.infer_video(d, f, overlap=2)
    torch.cuda.synchronize()
    assert len(rt._bufs) == nbufs and rt.workspace_bytes() == nbytes
    assert torch.cuda.memory_reserved(DEV) == reserved
    assert torch.equal(d0, d1) and torch.equal(n0, n1) and torch.equal(c0, m._clip_coefs)


# ------------------------------------------------------------------------------------------------ 7. pictures
def test_infer_video_vis_is_the_coloured_result():
    from vdn import vis
    m = _model(4, relu=True, res=False)
    d, f = _clip(7)
    res_d, res_n = m.infer_video(d, f, overlap=2)
    pic_d, pic_n = m.infer_video_vis(d, f, overlap=2)
    assert isinstance(pic_d, np.ndarray) and isinstance(pic_n, np.ndarray) and pic_d.dtype == pic_n.dtype == np.uint8
    assert pic_d.shape == pic_n.shape == (7, HW, HW, 3)
    assert np.array_equal(pic_d, vis.colorize(res_d, "inferno", "rgb", "clip").cpu().numpy())
    assert np.array_equal(pic_n, vis.colorize_normals(res_n).cpu().numpy())
    assert len(np.unique(pic_d)) > 8 and len(np.unique(pic_n)) > 2
    gray, _ = m.infer_video_vis(d, f, overlap=2, grayscale=True)
    assert np.array_equal(gray, vis.colorize(res_d, "inferno", "rgb", "clip", grayscale=True, gray_channels=1).cpu().numpy()[..., 0])


# ------------------------------------------------------------------------------------------------ 8. refusals
@pytest.mark.parametrize("case", ["rank", "n_mismatch", "n0", "bool", "overlap1", "overlap>S//2"])
def test_refusals_launch_nothing(case, monkeypatch):
    from vdn.runtime import Runtime
    m = _model(4)
    m._engines()
    d, f = _clip(7)
    kw = dict(overlap=2)
    if case == "rank":
        d = d[None]
    elif case == "n_mismatch":
        f = f[:6]
    elif case == "n0":
        d, f = d[:0], f[:0]
    elif case == "bool":
        d = d > 0.5
    elif case == "overlap1":
        kw = dict(overlap=1)
    else:
        kw = dict(overlap=3)
    launched = []
    launch = Runtime._launch
    monkeypatch.setattr(Runtime, "_launch", lambda self, fn, *a, **k: (launched.append(fn.__name__), launch(self, fn, *a, **k))[1])
    for call in (m.infer_video, m.infer_video_vis):
        with pytest.raises(ValueError):
            call(d, f, **kw)
    assert launched == []
    m.infer_video(*_clip(7), overlap=2)           # the recorder does see the launches of a well-formed call
    assert "vdn_dn_stitch_apply" in launched and "vdn_stitch_fit" in launched
