"""Drop-in for models/video_depth_model.py:19-125 (VideoDepthEstimationModel, the depth + normal model).

The reference builds its two Hiera trunks with torch.hub (models/hiera_image_encoder.py:35), which needs the network; here
`with_native_trunks` builds them from vdn.HieraImageEncoder (csrc/hiera.hip), or the caller injects any other module
(`trunk=` for the depth branch, `img_trunk=` for the RGB branch). They are registered as
`encoder` / `img_encoder`, so state-dict keys equal the reference's. A trunk is any module whose forward(x [N, 3, H, W])
returns (anything, [4 f32 NHWC maps [N, h_l, w_l, C_l]]) with C = 96 / 192 / 384 / 768 at strides 4 / 8 / 16 / 32
(hiera_image_encoder.py:53-58). Everything after the trunks runs on libvdn_hip.so: the Sobel normals of the input
depth (vdn_refine_pack), the head (vdn/dn_engine.py) and the resize / residual / normal tail (vdn_dn_tail)."""
from __future__ import annotations

import torch
import torch.nn as nn

from .depth_anything_v2 import _EngineOwner
from .dn_engine import CHANNELS, DNHeadEngine
from .video_depth_head_v2_sangyu import VideoDepthAnythingHeadV2


class VideoDepthEstimationModel(_EngineOwner):
    def __init__(self, sequence_length, attention_feature_levels=[2, 3], encoder="hiera_base_224", encoder_finetune=False,
                 use_residual=False, use_final_relu=False, use_depth_feature=True, use_rgb_feature=True, *, trunk=None,
                 img_trunk=None, pe="ape"):
        super().__init__()
        if trunk is None or img_trunk is None:
            missing = " and ".join(n for n, t in (("trunk", trunk), ("img_trunk", img_trunk)) if t is None)
            raise ValueError(
                f"VideoDepthEstimationModel needs its {encoder} trunks injected ({missing} missing): the reference fetches "
                "them with torch.hub, which this package never calls. Pass trunk=<depth-branch module> and "
                "img_trunk=<RGB-branch module> (see INTEGRATION.md).")
        if not (use_depth_feature or use_rgb_feature):
            raise ValueError("at least one of use_depth_feature / use_rgb_feature must be set")
        self.use_residual = use_residual
        self.use_final_relu = use_final_relu
        self.use_depth_feature = use_depth_feature
        self.use_rgb_feature = use_rgb_feature
        self.encoder_name = encoder
        self.img_encoder = img_trunk
        self.encoder = trunk
        self.head = VideoDepthAnythingHeadV2(sequence_length=sequence_length, pe=pe, attention_feature_levels=attention_feature_levels)
        self.set_finetune_modes(encoder_finetune=encoder_finetune)

    @classmethod
    def with_native_trunks(cls, sequence_length, encoder="hiera_base_224", **kw):
        """The model with both Hiera trunks built here (vdn.HieraImageEncoder, csrc/hiera.hip) instead of injected: the
        module tree and state-dict keys of the reference (`encoder.model.*`, `img_encoder.model.*`), nothing fetched."""
        from .hiera_image_encoder import HieraImageEncoder
        finetune = kw.get("encoder_finetune", False)
        trunk = HieraImageEncoder(encoder, finetune=finetune)
        img_trunk = HieraImageEncoder(encoder, finetune=finetune).share_runtime(trunk)   # one workspace arena for both
        return cls(sequence_length, encoder=encoder, trunk=trunk, img_trunk=img_trunk, **kw)

    def set_precision(self, name: str):
        """The native trunks are engine owners of their own: they follow the model's precision."""
        super().set_precision(name)
        for t in (self.encoder, self.img_encoder):
            if isinstance(t, _EngineOwner):
                t.set_precision(name)
        return self

    def _engines(self):
        if self._eng is None:
            rt = self._runtime()
            self._eng = dict(rt=rt, head=DNHeadEngine(rt, self.head))
        return self._eng

    def set_finetune_modes(self, encoder_finetune: bool = None, head_finetune: bool = None):
        """Inference only: the flags set requires_grad and nothing else."""
        if encoder_finetune is not None:
            for p in self.encoder.parameters():
                p.requires_grad_(bool(encoder_finetune))
        if head_finetune is not None:
            self.head.set_finetune(head_finetune)

    @staticmethod
    def _features(out, F: int):
        feats = list(out[1])
        if len(feats) != 4:
            raise ValueError(f"a trunk must return (_, [4 NHWC maps]); got {len(feats)} maps")
        for lvl, f in enumerate(feats):
            if f.dim() != 4 or f.shape[0] != F or f.shape[3] != CHANNELS[lvl]:
                raise ValueError(f"trunk level {lvl}: expected NHWC [{F}, h, w, {CHANNELS[lvl]}], got {tuple(f.shape)}")
        return [f.float().contiguous() for f in feats]

    @torch.no_grad()
    def forward(self, depth: torch.Tensor, img):
        """depth f32 [B, S, H, W], img [B, S, 3, H, W] -> (depth [B, S, H, W], normal [B, S, 3, H, W])."""
        e = self._engines()
        rt, eng = e["rt"], e["head"]
        B, S, H, W = depth.shape
        F = B * S
        d = depth.to(device=rt.device, dtype=torch.float32).reshape(F, H, W).contiguous()
        a = b = None
        if self.use_depth_feature:
            d3 = rt.fbuf("dn_in", (F, 3, H, W))
            rt.refine_pack(d, d3, normals=True)   # (d, nx, ny) of the raw depth (utils/normal_utils.py, :78-82)
            a = self._features(self.encoder(d3), F)
        if self.use_rgb_feature:
            i = self._features(self.img_encoder(img.to(rt.device).reshape(F, 3, H, W)), F)
            a, b = (i, None) if a is None else (a, i)
        sizes = [tuple(f.shape[1:3]) for f in a]
        if b is not None and [tuple(f.shape[1:3]) for f in b] != sizes:
            raise ValueError("the two trunks' feature maps differ in size")
        out_d = torch.empty((B, S, H, W), dtype=torch.float32, device=rt.device)
        out_n = torch.empty((B, S, 3, H, W), dtype=torch.float32, device=rt.device)
        self._taps = eng.run_model(a, b, B, S, sizes, H, W, d if self.use_residual else None, self.use_final_relu, out_d, out_n)
        return out_d, out_n
