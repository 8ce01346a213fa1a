"""Drop-in for models/video_depth_head_v2_sangyu.py:187-317 (VideoDepthAnythingHeadV2): same constructor, module tree
and state-dict keys; the forward pass runs on libvdn_hip.so (vdn/dn_engine.py, csrc/dn_head.hip), never on torch ops."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import modules
from .depth_anything_v2 import _EngineOwner
from .dn_engine import CHANNELS, DNHeadEngine


class _MHA(nn.Module):
    """nn.MultiheadAttention(C, 8, batch_first=True)'s parameters: packed q|k|v in_proj + out_proj."""

    def __init__(self, c):
        super().__init__()
        self.in_proj_weight = modules._param(3 * c, c)
        self.in_proj_bias = modules._param(3 * c)
        self.out_proj = modules.Lin(c, c)


class TransformerBlock(nn.Module):
    """Pre-LN block (:33-75): x + MHA(LN(x)), then + Linear(GELU(Linear(LN(x))))."""

    def __init__(self, c):
        super().__init__()
        self.multi_head_attention = _MHA(c)
        self.norm1 = modules.Norm(c)
        self.norm2 = modules.Norm(c)
        self.ffn = nn.Sequential(modules.Lin(c, 4 * c), nn.GELU(), modules.Lin(4 * c, c))


class _Layer(nn.Module):
    """TemporalLayer / SpatialLayer (:77-185): four TransformerBlocks."""

    def __init__(self, c, blocks=4):
        super().__init__()
        self.transformer_blocks = nn.ModuleList([TransformerBlock(c) for _ in range(blocks)])


class UpSampleAdd(nn.Module):
    """(:17-31) x2 bilinear -> conv3x3 (no bias) + BN + ReLU -> + skip_proj(skip)."""

    def __init__(self, in_ch, skip_ch, out_ch):
        super().__init__()
        self.conv = nn.Sequential(modules.Conv(in_ch, out_ch, 3, bias=False), modules.BatchNorm(out_ch), nn.ReLU(inplace=True))
        self.skip_proj = modules.Conv(skip_ch, out_ch, 1)


class VideoDepthAnythingHeadV2(_EngineOwner):
    def __init__(self, sequence_length: int = 8, pe="ape", attention_feature_levels: list = [2, 3]):
        super().__init__()
        if pe == "sine":
            raise NotImplementedError("pe='sine' is not supported (the reference's sinusoid table cannot run: math is not imported)")
        if pe not in ("ape", "none"):
            raise ValueError(f"pe must be 'ape' or 'none', got {pe!r}")
        self.feature_channels = list(CHANNELS)
        self.pos_embedding_type = pe
        if pe == "ape":
            self.pos_embeds = nn.ParameterList([modules._param(sequence_length, c) for c in CHANNELS])
        else:
            self.register_parameter("pos_embeds", None)
        for name in ("temporal_layers_first", "temporal_layers_second", "spatial_layers_first", "spatial_layers_second"):
            setattr(self, name, nn.ModuleList([_Layer(c) for c in CHANNELS]))
        self.attention_feature_levels = list(attention_feature_levels)
        for lvl in self.attention_feature_levels:
            if lvl not in range(len(CHANNELS)):
                raise ValueError("attention_feature_levels must contain indices between 0 and 3 inclusive")
        c0, c1, c2, c3 = CHANNELS
        self.upscale_layers = nn.ModuleList([UpSampleAdd(c3, c2, c2), UpSampleAdd(c2, c1, c1), UpSampleAdd(c1, c0, c0)])
        self.final_upscale_layer = nn.Sequential(
            nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True),
            modules.Conv(c0, c0, 3, bias=False), modules.BatchNorm(c0), nn.ReLU(True),
            nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True),
            modules.Conv(c0, c0, 3, bias=False), modules.BatchNorm(c0), nn.ReLU(True),
            modules.Conv(c0, 48, 3), nn.ReLU(True),
            modules.Conv(48, 3, 3))
        self.fusion_layer = nn.ModuleList([modules.Conv(c1, c0, 3), modules.Conv(c2, c1, 3), modules.Conv(c3, c2, 3)])  # unused (:251-255)

    def _engines(self):
        if self._eng is None:
            self._eng = dict(rt=(rt := self._runtime()), head=DNHeadEngine(rt, self))
        return self._eng

    def set_finetune(self, finetune: bool):
        """Training is out of scope: only the requires_grad flags change."""
        for p in self.parameters():
            p.requires_grad_(bool(finetune))

    @torch.no_grad()
    def forward(self, features) -> torch.Tensor:
        """four f32 [B, S, C_l, h_l, w_l] maps (C = 96 / 192 / 384 / 768, strides 4..32) -> [B, S, 3, 4 h0, 4 w0]."""
        if len(features) != 4:
            raise ValueError("Expected 4 levels of encoder features (stride 4→32)")
        e = self._engines()
        rt = e["rt"]
        feats = []
        for lvl, f in enumerate(features):
            if f.dim() != 5 or f.shape[2] != CHANNELS[lvl] or f.shape[:2] != features[0].shape[:2]:
                raise ValueError(f"level {lvl}: expected [B, S, {CHANNELS[lvl]}, h, w], got {tuple(f.shape)}")
            feats.append(f.to(device=rt.device, dtype=torch.float32).contiguous())
        B, S = feats[0].shape[:2]
        h0, w0 = feats[0].shape[-2:]
        out = torch.empty((B, S, 3, 4 * h0, 4 * w0), dtype=torch.float32, device=rt.device)
        self._taps = e["head"].run_head(feats, out)
        return out


__all__ = ["VideoDepthAnythingHeadV2"]
