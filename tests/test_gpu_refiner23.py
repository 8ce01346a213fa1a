"""The v2 / v3 depth-refiner wrappers and pe='rope' through all four, on the MI355X: vdn_refine_mix and
vdn_refine_normalize against fp64 / torch, the wrappers against the imported reference's fixtures (R2_vits, R3_vits,
R5r_vits) and, for the constructor flags and v4 + rope, against the CPU restatements. Tolerance as in test_gpu_e2e.py:
1e-3 on the rel-L2 of the map and on its worst pixel."""
import importlib
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import refiner_ref as R
from common import GOLD, rel_l2, synth_sd, worst_px

pytestmark = pytest.mark.gpu
TOL = 1e-3
DEV = "cuda"
# (n, offset in floats of depth, x, out inside their allocations): one lane, less than a block, the fixture's frame (a
# multiple of 4 but not of 1024), a vector body with a 3-float head and a 4-float tail behind a pointer offset by one
# float, and arrays whose alignments differ (everything on the one-float path)
MIX_CASES = [(1, (0, 0, 0)), (255, (0, 0, 0)), (21168, (0, 0, 0)), (21171, (1, 1, 1)), (21171, (0, 1, 2))]
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


def _fixture(name):
    from vdn import synth
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    v, S, H, W, seed = [int(t) for t in g["meta"]]
    return g, v, torch.from_numpy(synth.depth_clip(seed, S, H, W))[None]


def _state_dict(name):
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    return {"R2_vits": lambda: R.r2_state_dict(g, synth_sd("R2", "vits")), "R3_vits": lambda: synth_sd("R3", "vits"), "R5r_vits": lambda: synth_sd("R5r", "vits")}[name]()


@lru_cache(maxsize=None)
def _model(name):
    import vdn
    version = int(name[1])
    m = _cls(version)(**dict(vdn.MODEL_CONFIGS["vits"], **(dict(pe="rope") if name.startswith("R5r") else {})))
    m.load_state_dict(_state_dict(name), strict=True)
    return m.to(DEV).eval()


def _placed(values, off):
    """`values` at float offset `off` of a canary-filled device allocation: (whole buffer, the view the kernel gets)."""
    buf = torch.full((off + values.numel() + PAD,), CANARY, dtype=torch.float32, device=DEV)
    view = buf[off:off + values.numel()]
    view.copy_(values)
    return buf, view


def _canaries_intact(buf, off, n):
    return bool((buf[:off] == CANARY).all()) and bool((buf[off + n:] == CANARY).all())


@pytest.mark.parametrize("n,offs", MIX_CASES)
def test_refine_mix_against_fp64(rt, n, offs):
    """vdn_refine_mix = relu(a2 relu(a0 d + a1 x + c0) + c1) with the R2 fixture's folded scalars. Bar 2e-6 of max |out|:
    the scalars' and three fused operations' fp32 roundings of O(1) quantities, 2^-24 each. NaN in, NaN out."""
    import torch.nn as nn
    from vdn.refiner import fold_final_res
    seq = nn.Sequential(nn.Conv2d(2, 1, 1), nn.BatchNorm2d(1), nn.ReLU(), nn.Conv2d(1, 1, 1), nn.BatchNorm2d(1), nn.ReLU()).eval()
    seq.load_state_dict(R.with_final_res(seq.state_dict(), {k[10:]: v for k, v in R.R2_FINAL_RES.items()}))
    a0, a1, c0, a2, c1 = fold_final_res(seq)
    gen = torch.Generator().manual_seed(n)
    d, x = 2.0 * torch.rand(n, generator=gen), torch.rand(n, generator=gen)   # the network's rectified depth, the normalised input
    nan_at = [n // 2, n - 1] if n > 2 else []                                 # one in the vector body (depth), one in the tail (x)
    if nan_at:
        d[nan_at[0]], x[nan_at[1]] = float("nan"), float("nan")
    inner = a0 * d.double() + a1 * x.double() + c0
    ref = torch.relu(a2 * torch.relu(inner) + c1)
    ok = ~torch.isnan(ref)
    assert int((~ok).sum()) == len(nan_at)
    if n >= 255:   # the inputs straddle both kinks
        assert 0.05 < float((inner[ok] < 0).double().mean()) < 0.95 and 0.05 < float((ref[ok] == 0).double().mean()) < 0.95
    (_, dv), (_, xv) = _placed(d, offs[0]), _placed(x, offs[1])
    obuf, ov = _placed(torch.zeros(n), offs[2])
    rt.refine_mix(dv, xv, a0, a1, c0, a2, c1, ov)
    got = ov.cpu()
    assert _canaries_intact(obuf, offs[2], n)
    assert torch.equal(torch.isnan(got), ~ok)
    err = float((got.double() - ref)[ok].abs().max()) / max(float(ref[ok].abs().max()), 1e-30)
    print(f"[refine_mix n={n} offsets={offs}] max abs error / max |out| = {err:.2e}")
    assert err <= 2e-6


@pytest.mark.parametrize("n,offs", MIX_CASES)
def test_refine_normalize_is_torch_div(rt, n, offs):
    """vdn_refine_normalize is bit-equal to torch.div(x, 65535.0): the correctly rounded fp32 quotient."""
    gen = torch.Generator().manual_seed(n + 1)
    x = 65535.0 * torch.rand(n, generator=gen)
    x[: min(n, 4)] = torch.tensor([65535.0, 0.0, 1.0, 32767.5])[: min(n, 4)]
    (_, xv) = _placed(x, offs[1])
    obuf, ov = _placed(torch.zeros(n), offs[2])
    rt.refine_normalize(xv, 65535.0, ov)
    assert _canaries_intact(obuf, offs[2], n)
    assert torch.equal(ov.cpu(), torch.div(x, 65535.0))


@pytest.mark.parametrize("name", ["R2_vits", "R3_vits", "R5r_vits"])
def test_refiner_against_reference_fixture(name):
    """The wrapper against the output the imported reference model wrote: rel-L2 and worst pixel within 1e-3, finite,
    deterministic, and two clips in one batch independent."""
    g, version, x = _fixture(name)
    m = _model(name)
    out = m.forward(x.to(DEV))[0].cpu()
    e, w = rel_l2(out, g["out"]), worst_px(out, g["out"])
    print(f"[{name}] refined depth vs reference fixture: rel-L2 {e:.2e} worst pixel {w:.2e}")
    assert torch.isfinite(out).all()
    assert e < TOL and w <= TOL
    assert torch.equal(m.forward(x.to(DEV))[0].cpu(), out)
    both = m.forward(torch.cat([x, x * 0.5 + 100.0]).to(DEV)).cpu()
    assert rel_l2(both[0], g["out"]) < TOL


def test_refiner_v3_median_and_scale(rt):
    """v3:175-176 on the device (vdn_frame_median, vdn_refine_scale with final_scale2's weight and bias, max_depth 65535)
    against the reference's per-frame median of the normalised clip and its scale."""
    g, _, x = _fixture("R3_vits")
    sd = synth_sd("R3", "vits")
    xd = x[0].to(DEV).contiguous()
    med = torch.empty(xd.shape[0], dtype=torch.float32, device=DEV)
    rt.frame_median(xd, med)
    scaled, sc = torch.empty_like(xd), torch.empty_like(med)
    rt.refine_scale(xd, med, float(sd["final_scale2.feat.1.weight"]), float(sd["final_scale2.feat.1.bias"]), 1.0, 65535.0, scaled, sc)
    e_med, e_sc = rel_l2(med.cpu().double() / 65535.0, g["median"]), rel_l2(sc.cpu(), g["scale"])
    print(f"[R3_vits] median {e_med:.2e} scale {e_sc:.2e}")
    assert e_med <= 1e-6 and e_sc <= 1e-6


@pytest.mark.parametrize("version", [2, 3])
@pytest.mark.parametrize("use_residual,input_normal", [(False, True), (True, False)])
def test_refiner_v2_v3_flags_against_restatement(version, use_residual, input_normal):
    """v2:79-83,94 / v3:180-184,195: without the residual the result is the rectified network depth (not multiplied by
    65535); without normals the depth is broadcast to 3 channels."""
    import vdn
    from vdn import synth
    name = f"R{version}_vits"
    sd = _state_dict(name)
    m = _cls(version)(use_residual=use_residual, input_normal=input_normal, **vdn.MODEL_CONFIGS["vits"])
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    x = torch.from_numpy(synth.depth_clip(77, 2, 70, 98))[None]
    tr = {}
    with torch.no_grad():
        ref = R.refiner23_forward(sd, x, "vits", version=version, use_residual=use_residual, input_normal=input_normal, trace=tr)
    if not use_residual:
        assert torch.equal(ref, tr["net_depth"])
    out = m.forward(x.to(DEV)).cpu()
    e, w = rel_l2(out, ref), worst_px(out, ref)
    print(f"[refiner v{version} residual={use_residual} normals={input_normal}] vs restatement: rel-L2 {e:.2e} worst pixel {w:.2e}")
    assert torch.isfinite(out).all() and e < TOL and w <= TOL


def test_refiner_v4_rope_against_oracle():
    """pe='rope' with the network at the input resolution: v4's weights without the pos_encoder.pe tables."""
    import vdn
    from oracle import ref_cpu as O
    from vdn import synth
    sd = {k: v for k, v in synth_sd("R4", "vits").items() if "pos_encoder.pe" not in k}
    m = _cls(4)(pe="rope", **vdn.MODEL_CONFIGS["vits"])
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    x = torch.from_numpy(synth.depth_clip(77, 2, 70, 98))[None]
    with torch.no_grad():
        ref = O.depth_refiner_forward(sd, x, "vits", version=4)
        ape = O.depth_refiner_forward(synth_sd("R4", "vits"), x, "vits", version=4)
    assert rel_l2(ape, ref) > 10 * TOL   # the two position schemes differ by far more than the tolerance on this clip
    out = m.forward(x.to(DEV)).cpu()
    e, w = rel_l2(out, ref), worst_px(out, ref)
    print(f"[refiner v4 rope] vs oracle: rel-L2 {e:.2e} worst pixel {w:.2e}")
    assert torch.isfinite(out).all() and e < TOL and w <= TOL
