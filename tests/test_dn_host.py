"""Depth + normal model (vdn.VideoDepthEstimationModel / vdn.VideoDepthAnythingHeadV2): host-side checks, no GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _model(**kw):
    import vdn
    from vdn import synth
    return vdn.VideoDepthEstimationModel(8, trunk=synth.dn_trunk(), img_trunk=synth.dn_trunk(), **kw)


def test_state_dict_matches_reference_schema():
    """Keys and shapes equal the reference wrapper's (with the stand-in trunks), so a reference checkpoint loads strict."""
    with open(os.path.join(GOLD, "schema_dn_wrapper.json")) as f:
        sch = json.load(f)
    m = _model(use_residual=True, use_final_relu=True)
    want = {k: tuple(s) for k, s in sch["params"] + sch["buffers"]}
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert sum(k.startswith("head.") for k in got) == 818
    from dn_fixture import state_dict
    m.load_state_dict(state_dict(m), strict=True)


def test_head_state_dict_keys_and_pe_none():
    import vdn
    h = vdn.VideoDepthAnythingHeadV2(sequence_length=32)
    assert tuple(h.pos_embeds[3].shape) == (32, 768)
    assert len(h.state_dict()) == 818
    n = vdn.VideoDepthAnythingHeadV2(pe="none")
    assert n.pos_embeds is None and len(n.state_dict()) == 814


def test_pe_sine_raises():
    import vdn
    with pytest.raises(NotImplementedError):
        vdn.VideoDepthAnythingHeadV2(pe="sine")
    with pytest.raises(ValueError):
        vdn.VideoDepthAnythingHeadV2(attention_feature_levels=[4])


def test_missing_trunk_raises_without_hub(monkeypatch):
    import vdn
    from vdn import synth

    def no_hub(*a, **k):
        raise AssertionError("torch.hub must never be called")

    monkeypatch.setattr(torch.hub, "load", no_hub)
    with pytest.raises(ValueError, match="trunk"):
        vdn.VideoDepthEstimationModel(8)
    with pytest.raises(ValueError, match="img_trunk"):
        vdn.VideoDepthEstimationModel(8, trunk=synth.dn_trunk())


def test_finetune_modes_only_flip_requires_grad():
    m = _model()
    m.set_finetune_modes(encoder_finetune=True, head_finetune=True)
    assert all(p.requires_grad for p in m.encoder.parameters()) and all(p.requires_grad for p in m.head.parameters())
    m.set_finetune_modes(encoder_finetune=False, head_finetune=False)
    assert not any(p.requires_grad for p in m.encoder.parameters()) and not any(p.requires_grad for p in m.head.parameters())


def test_dn_entry_points_reject_bad_arguments_without_launch():
    """Every malformed call returns a vdn_status before anything is launched (no GPU here: a launch would fail)."""
    from vdn import _abi
    L = _abi.lib
    p = ctypes.c_void_p(256)
    # attention: missing buffers, split planes half given, a sequence past the last row, unsupported head dims
    assert L.vdn_dn_attn(0, None, None, p, None, 8, 96, 8, 4, 1, 1, 0, 2, 4, 0.3, None) == -1
    assert L.vdn_dn_attn(0, p, p, p, None, 8, 96, 8, 4, 1, 1, 0, 2, 4, 0.3, None) == -1
    assert L.vdn_dn_attn(0, p, None, p, None, 8, 96, 8, 4, 1, 1, 0, 2, 5, 0.3, None) == -1
    assert L.vdn_dn_attn(0, p, None, p, None, 8, 96, 8, 5, 1, 1, 0, 2, 4, 0.3, None) == -1
    assert L.vdn_dn_attn(0, p, None, p, None, 8, 64 * 8, 8, 4, 1, 1, 0, 2, 4, 0.3, None) == -2
    assert L.vdn_dn_attn(0, p, None, p, None, 8, 100, 8, 4, 1, 1, 0, 2, 4, 0.3, None) == -1
    assert L.vdn_dn_attn(2, p, None, p, None, 8, 96, 8, 4, 1, 1, 0, 2, 4, 0.3, None) == -2
    # prologue: no input, no output, lo without hi, ape without S, f32 planes
    assert L.vdn_dn_prologue(0, None, None, 2, 96, 49, None, 1, p, None, None, None) == -1
    assert L.vdn_dn_prologue(0, p, None, 2, 96, 49, None, 1, None, None, None, None) == -1
    assert L.vdn_dn_prologue(0, p, None, 2, 96, 49, None, 1, None, None, p, None) == -1
    assert L.vdn_dn_prologue(0, p, None, 2, 96, 49, p, 0, p, None, None, None) == -1
    assert L.vdn_dn_prologue(2, p, None, 2, 96, 49, None, 1, None, p, None, None) == -2
    # tail: no output, depth without normal, residual without depth, too many input channels
    assert L.vdn_dn_tail(p, 1, 8, 8, 48, p, p, 8, 8, None, 0, None, None, None, None) == -1
    assert L.vdn_dn_tail(p, 1, 8, 8, 48, p, p, 8, 8, None, 0, None, p, None, None) == -1
    assert L.vdn_dn_tail(p, 1, 8, 8, 48, p, p, 8, 8, p, 0, p, None, None, None) == -1
    assert L.vdn_dn_tail(p, 1, 8, 8, 256, p, p, 8, 8, None, 0, p, None, None, None) == -2


def test_view_reinterpretation_index_map():
    """The prologue's index map token[(f hw + p), c] = flat_f[c hw + p] is what `.view(B, S, D, H, W)` of an NHWC buffer
    followed by the head's rearranges yields (video_depth_model.py:101-103, then "b s c h w -> (b s) (h w) c")."""
    from dn_fixture import tokens_as_maps
    B, S, h, w, C = 2, 3, 4, 5, 8
    nhwc = torch.randn(B * S, h, w, C)
    viewed = nhwc.view(B, S, C, h, w)                                     # the reference's reinterpretation
    tokens_ref = viewed.permute(0, 1, 3, 4, 2).reshape(B * S * h * w, C)  # (b s) (h w) c
    flat = nhwc.reshape(B * S, C * h * w)
    f, p, c = torch.meshgrid(torch.arange(B * S), torch.arange(h * w), torch.arange(C), indexing="ij")
    tokens = flat[f, c * h * w + p].reshape(B * S * h * w, C)             # the kernel's map
    assert torch.equal(tokens, tokens_ref)
    assert not torch.equal(tokens, nhwc.reshape(-1, C))                    # it is NOT a permute back to channels-last
    assert torch.equal(tokens_as_maps(tokens, B * S, C, h * w), viewed.reshape(B * S, C, h * w))


def test_fixtures_present_and_small():
    for n in ("dn_head_s4", "dn_head_s32", "dn_head_s2_all", "dn_model_b2", "dn_model_nope"):
        path = os.path.join(GOLD, n + ".npz")
        assert os.path.getsize(path) <= 1 << 20
        with np.load(path) as z:
            assert "levels" in z.files and "meta" in z.files
