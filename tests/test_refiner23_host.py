"""The v2 / v3 depth-refiner wrappers and pe='rope' on all four, without a GPU: state-dict schemas and import paths against
the imported reference's key lists, the CPU restatement (tests/refiner_ref.py) against the reference fixtures, and the fp64
BatchNorm fold behind vdn_refine_mix against the module chain it replaces."""
import importlib
import os

import numpy as np
import pytest
import torch

import refiner_ref as R
from common import GOLD, rel_l2, schema, synth_sd


def _cls(version):
    return importlib.import_module(f"vdn.video_depth_model_v{version}").VideoDepthAnything


def _clip(g):
    from vdn import synth
    v, S, H, W, seed = [int(t) for t in g["meta"]]
    return v, torch.from_numpy(synth.depth_clip(seed, S, H, W))[None]


def r2_state_dict(g):
    return R.r2_state_dict(g, synth_sd("R2", "vits"))


@pytest.mark.parametrize("version", [2, 3])
def test_refiner_v2_v3_state_dict_schema_matches_reference(version):
    """Same parameter / buffer keys and shapes as models/video_depth_model_v{2,3}.VideoDepthAnything: `head.*` (not
    `temporal_head.*`), v2's final_res.{0,1,3,4} with both BatchNorms' buffers, v3's final_res2.0 and final_scale2.feat.1."""
    import vdn
    m = _cls(version)(**vdn.MODEL_CONFIGS["vits"])
    sch = schema(f"R{version}", "vits")
    assert {k: tuple(v.shape) for k, v in m.named_parameters()} == {k: tuple(s) for k, s in sch["params"]}
    assert {k: tuple(v.shape) for k, v in m.named_buffers()} == {k: tuple(s) for k, s in sch["buffers"]}
    m.load_state_dict(m.state_dict(), strict=True)
    m.load_state_dict(synth_sd(f"R{version}", "vits"), strict=True)


@pytest.mark.parametrize("version", [2, 3])
def test_refiner_v2_v3_constructor_is_the_references(version):
    """v2:38-49 / v3:129-140: nine arguments in this order, no max_depth."""
    import inspect
    names = list(inspect.signature(_cls(version).__init__).parameters)[1:]
    assert names == ["encoder", "features", "out_channels", "use_bn", "use_clstoken", "num_frames", "pe", "use_residual", "input_normal"]


def test_refiner_v2_v3_import_paths_exist():
    for version in (2, 3):
        c = _cls(version)
        assert callable(c.forward) and not hasattr(c, "infer_video_depth")   # the reference's cannot run


@pytest.mark.parametrize("version", [2, 3, 4, 5])
def test_refiner_rope_builds_without_position_tables(version):
    """pe='rope' (motion_module.py:236-240) has no pos_encoder.pe buffer; any other value raises as video_depth.py:19 does."""
    import vdn
    m = _cls(version)(pe="rope", **vdn.MODEL_CONFIGS["vits"])
    keys = list(m.state_dict())
    assert keys and not any("pos_encoder.pe" in k for k in keys)
    assert any("pos_encoder.pe" in k for k in _cls(version)(**vdn.MODEL_CONFIGS["vits"]).state_dict())
    with pytest.raises(NotImplementedError):
        _cls(version)(pe="sine", **vdn.MODEL_CONFIGS["vits"])


def test_refiner_v5_rope_schema_and_64_frames():
    import vdn
    m = _cls(5)(pe="rope", **vdn.MODEL_CONFIGS["vits"])
    sch = schema("R5r", "vits")
    assert {k: tuple(v.shape) for k, v in m.named_parameters()} == {k: tuple(s) for k, s in sch["params"]}
    assert {k: tuple(v.shape) for k, v in m.named_buffers()} == {k: tuple(s) for k, s in sch["buffers"]}
    m.load_state_dict(synth_sd("R5r", "vits"), strict=True)
    m64 = _cls(5)(num_frames=64, pe="rope", **vdn.MODEL_CONFIGS["vits"])
    att = m64.temporal_head.motion_modules[0].temporal_transformer.transformer_blocks[0].attention_blocks[0]
    assert att.max_len == 64   # the rotation table is built for max_len frames (TemporalEngine)


@pytest.mark.parametrize("name", ["R2_vits", "R3_vits", "R5r_vits"])
def test_restatement_agrees_with_reference_fixture(name):
    from oracle import ref_cpu as O
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    version, x = _clip(g)
    tr = {}
    with torch.no_grad():
        if version == 5:
            out = O.depth_refiner_forward(synth_sd("R5r", "vits"), x, "vits", version=5, trace=tr)
        else:
            sd = r2_state_dict(g) if version == 2 else synth_sd("R3", "vits")
            out = R.refiner23_forward(sd, x, "vits", version=version, trace=tr)
    e, e_net = rel_l2(out[0], g["out"]), rel_l2(tr["net_depth"][0], g["net_depth"])
    print(f"[{name}] restatement vs reference fixture: out {e:.2e} net_depth {e_net:.2e}")
    assert e <= 1e-5 and e_net <= 1e-5
    if "median" in g.files:
        assert rel_l2(tr["median"], g["median"]) < 1e-6 and rel_l2(tr["scale"], g["scale"]) < 1e-6


def test_r2_fixture_is_not_degenerate():
    """Conditions on the reference alone: both ReLUs of final_res are partly active on the fixture clip."""
    g = np.load(os.path.join(GOLD, "R2_vits.npz"))
    assert {k[3:]: g[k].reshape(-1).tolist() for k in g.files if k.startswith("sd/")} == \
        {k: np.asarray(v, np.float32).tolist() for k, v in R.R2_FINAL_RES.items()}
    _, x = _clip(g)
    tr = {}
    R.final_res(r2_state_dict(g), torch.from_numpy(g["net_depth"]), x[0] / 65535.0, tr)
    clipped = float((tr["pre_relu1"] < 0).float().mean())
    zero = float((torch.from_numpy(g["out"]) == 0).float().mean())
    print(f"[R2_vits] clipped by the first ReLU {clipped:.3f}, outputs exactly zero {zero:.3f}")
    assert 0.05 <= clipped <= 0.95
    assert 0.05 <= zero <= 0.95


def test_final_res_fold_equals_the_module_chain_in_fp64():
    """vdn.refiner.fold_final_res: (a0, a1, c0, a2, c1) with relu(a2 relu(a0 d + a1 x + c0) + c1) equal to torch's
    Conv2d - BatchNorm2d - ReLU - Conv2d - BatchNorm2d - ReLU in eval mode, fp64, on inputs that straddle both kinks."""
    import torch.nn as nn
    from vdn.refiner import fold_final_res
    gen = torch.Generator().manual_seed(5)
    for trial in range(4):
        seq = nn.Sequential(nn.Conv2d(2, 1, 1), nn.BatchNorm2d(1), nn.ReLU(), nn.Conv2d(1, 1, 1), nn.BatchNorm2d(1), nn.ReLU()).double().eval()
        with torch.no_grad():
            for p in seq.parameters():
                p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64))
            for i in (1, 4):
                seq[i].running_mean.copy_(torch.randn(1, generator=gen, dtype=torch.float64))
                seq[i].running_var.copy_(0.5 + torch.rand(1, generator=gen, dtype=torch.float64))
            if trial == 0:
                seq.load_state_dict({k: torch.tensor(v, dtype=torch.float64).reshape(seq.state_dict()[k[10:]].shape)
                                     for k, v in R.R2_FINAL_RES.items()}, strict=False)
        d, x = 3.0 * torch.randn(2, 4096, generator=gen, dtype=torch.float64)
        if trial:   # put the second kink at the median of what the first ReLU passes: c1 moves one for one with the last beta
            a0, a1, c0, a2, c1 = fold_final_res(seq)
            r = torch.relu(a0 * d + a1 * x + c0)
            with torch.no_grad():
                seq[4].bias += -a2 * float(r[r > 0].median()) - c1
        a0, a1, c0, a2, c1 = fold_final_res(seq)
        with torch.no_grad():
            ref = seq(torch.stack([d, x])[None].reshape(1, 2, 64, 64)).reshape(-1)
        inner = a0 * d + a1 * x + c0
        got = torch.relu(a2 * torch.relu(inner) + c1)
        kink1 = float((inner < 0).double().mean())
        kink2 = float((got == 0).double().mean())
        assert 0.02 < kink1 < 0.98, kink1                    # the first ReLU clips some and passes some
        assert 0.02 < kink2 < 0.98, kink2                    # and so does the second
        assert float((got - ref).abs().max()) <= 1e-12
