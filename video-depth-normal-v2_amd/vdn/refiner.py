"""Depth-refiner wrappers: drop-ins for models/video_depth_model_v2.py:37-100, _v3.py:128-206,
_v4.py:83-148 and _v5.py:124-192 — same constructor, `forward(input_depth)` and state-dict keys. The network itself is the
same DINOv2 encoder + temporal DPT head as `vdn.VideoDepthAnything`; what the wrappers add runs in csrc/refine.hip:
per-frame median (exact radix select), tanh/exp scale, Sobel normals, then the version's finish step.

One class runs all four; a version supplies its module tree and key names, whether it has a scale head, where the
network runs and its finish step:

  version  head keys        scale head       network input       finish                                      result
  v2       head.*           -                the clip (H,W%14)   final_res.{0,1,3,4}: conv-BN-ReLU-conv-BN-   normalised
                                                                 ReLU on [depth, x]  (vdn_refine_mix)
  v3       head.*           final_scale2.*   the clip            x + final_res2.0 (depth)                     normalised
  v4       temporal_head.*  scale_head.*     the clip            x + shift_head.0 (depth)                     x max_depth
  v5       temporal_head.*  scale_head.*     224 x 224 resize    x + shift_head.0 (depth)                     x max_depth

v2 and v3 take no `max_depth`: 65535 is hard-wired there (v2:77, v3:169). None of the four has `infer_video_depth`: the
reference's copies feed a 5-D RGB window into `forward`, whose first line unpacks four dimensions."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import modules
from .depth_anything_v2 import _EngineOwner
from .engine import DPTEngine, EncoderEngine, ReadoutEngine


def fold_final_res(seq):
    """v2's final_res = Conv2d(2,1,1), BatchNorm2d(1), ReLU, Conv2d(1,1,1), BatchNorm2d(1), ReLU (video_depth_model_v2.py:64-72)
    in inference: eval-mode BatchNorm (eps 1e-5) is an affine map, so the chain on stack([d, x]) is
    relu(a2 * relu(a0 * d + a1 * x + c0) + c1). Returns (a0, a1, c0, a2, c1), folded in fp64."""
    def f(t):
        return t.detach().double().reshape(-1)

    def bn(m):
        s = f(m.weight) / torch.sqrt(f(m.running_var) + 1e-5)
        return s, f(m.bias) - f(m.running_mean) * s   # y -> s * y + t

    s1, t1 = bn(seq[1])
    s2, t2 = bn(seq[4])
    w0, w3 = f(seq[0].weight), f(seq[3].weight)
    return tuple(float(v) for v in (w0[0] * s1, w0[1] * s1, f(seq[0].bias) * s1 + t1, w3[0] * s2, f(seq[3].bias) * s2 + t2))


def _scalar_conv():
    return modules.Conv(1, 1, 1)   # the reference's 1x1 'ZeroConv' on one channel: a weight and a bias


class _DepthRefiner(_EngineOwner):
    VERSION = 5
    HEAD = "temporal_head"        # attribute (= state-dict prefix) of the temporal DPT head
    SCALE_HEAD = "scale_head"     # attribute of the GlobalScaleHead, None: the clip is only divided by max_depth
    NET_HW = (224, 224)           # the network sees a bilinear resize of the clip; None: the clip itself (H, W multiples of 14)
    FINISH = ("shift", "shift_head")   # ("shift", attr): x + (w * depth + b); ("mix", attr): fold_final_res on [depth, x]
    DENORMALISE = True            # the result is multiplied back by max_depth

    def __init__(self, encoder="vitl", features=256, out_channels=[256, 512, 1024, 1024], use_bn=False, use_clstoken=False,
                 num_frames=32, max_depth=65535, pe="ape", use_residual=True, input_normal=True):
        super().__init__()
        if pe not in ("ape", "rope"):
            raise NotImplementedError(pe)   # motion_module.py:242
        if encoder not in ("vits", "vitl"):
            raise KeyError(encoder)
        self.intermediate_layer_idx = {"vits": [2, 5, 8, 11], "vitl": [4, 11, 17, 23]}
        self.max_depth, self.use_residual, self.input_normal = max_depth, use_residual, input_normal
        self.encoder = encoder
        cfg = modules.ENCODERS[encoder]
        self.pretrained = modules.dinov2(encoder)
        if self.SCALE_HEAD:
            sh = modules.Holder()
            sh.feat = nn.Sequential(nn.Identity(), _scalar_conv())  # quantile pool has no weights
            setattr(self, self.SCALE_HEAD, sh)
        setattr(self, self.HEAD, modules.dpt_head_temporal(cfg["dim"], features, out_channels, num_frames, use_bn, use_clstoken, pe))
        kind, attr = self.FINISH
        if kind == "shift":
            setattr(self, attr, nn.Sequential(_scalar_conv()))
        else:
            setattr(self, attr, nn.Sequential(modules.Conv(2, 1, 1), modules.BatchNorm(1), nn.ReLU(), _scalar_conv(),
                                              modules.BatchNorm(1), nn.ReLU()))
        self._features, self._out_channels = features, list(out_channels)

    def _engines(self):
        if self._eng is None:
            rt = self._runtime()
            cfg = modules.ENCODERS[self.encoder]
            head = getattr(self, self.HEAD)

            def wb(conv):
                return float(conv.weight.reshape(()).item()), float(conv.bias.reshape(()).item())

            self._eng = dict(rt=rt, enc=EncoderEngine(rt, self.pretrained, cfg),
                             head=DPTEngine(rt, head, cfg["dim"], self._features, self._out_channels, temporal=True),
                             scale_wb=wb(getattr(self, self.SCALE_HEAD).feat[1]) if self.SCALE_HEAD else None)
            kind, attr = self.FINISH
            if kind == "shift":
                self._eng["shift_wb"] = wb(getattr(self, attr)[0])
            else:
                self._eng["mix"] = fold_final_res(getattr(self, attr))
            if hasattr(head, "readout_projects"):   # use_clstoken
                self._eng["enc"].readout = ReadoutEngine(rt, head.readout_projects, cfg["dim"])
        return self._eng

    @torch.no_grad()
    def forward(self, input_depth: torch.Tensor) -> torch.Tensor:
        """input_depth f32 [B,S,H,W] in [0, max_depth] -> refined depth [B,S,H,W] (v5:160-192 / v4:117-148 / v3:167-206 /
        v2:75-100); v2 and v3 return it normalised, v4 and v5 in the input's units."""
        e = self._engines()
        rt, enc, head = e["rt"], e["enc"], e["head"]
        B, S, H0, W0 = input_depth.shape
        F = B * S
        x = input_depth.to(device=rt.device, dtype=torch.float32).reshape(F, H0, W0).contiguous()
        scaled = torch.empty_like(x)
        if e["scale_wb"] is not None:
            med = torch.empty(F, dtype=torch.float32, device=rt.device)
            rt.frame_median(x, med)
            rt.refine_scale(x, med, e["scale_wb"][0], e["scale_wb"][1], 1.0, float(self.max_depth), scaled)
        else:
            rt.refine_normalize(x, float(self.max_depth), scaled)
        if self.NET_HW is not None:
            H, W = self.NET_HW
            r = torch.empty((F, H, W), dtype=torch.float32, device=rt.device)
            rt.upsample_f32(scaled, r, F, H0, W0, H, W)
        else:
            if H0 % 14 or W0 % 14:
                raise AssertionError(f"input resolution {H0}x{W0} must be a multiple of the patch size 14")  # patch_embed.py:73-74
            H, W, r = H0, W0, scaled
        net_in = torch.empty((F, 3, H, W), dtype=torch.float32, device=rt.device)
        rt.refine_pack(r, net_in, normals=self.input_normal)
        taps, _, (ph, pw) = enc.run(net_in)
        depth = head.run(taps, F, ph, pw, T=S, relu=True).reshape(F, H, W)  # rectified before the resize, as the head does
        if (H, W) != (H0, W0):
            d0 = torch.empty((F, H0, W0), dtype=torch.float32, device=rt.device)
            rt.upsample_f32(depth.contiguous(), d0, F, H, W, H0, W0, relu=True)
        else:
            d0 = depth.contiguous()
        out = torch.empty((F, H0, W0), dtype=torch.float32, device=rt.device)
        unit = float(self.max_depth) if self.DENORMALISE else 1.0
        if "shift_wb" in e:
            rt.refine_finish(scaled, d0, e["shift_wb"][0], e["shift_wb"][1], unit, self.use_residual, out)
        elif self.use_residual:
            rt.refine_mix(d0, scaled, *e["mix"], out)
        else:   # v2 without final_res: the rectified depth itself
            rt.refine_finish(None, d0, 0.0, 0.0, unit, False, out)
        return out.reshape(B, S, H0, W0)


class _DepthRefiner65535(_DepthRefiner):
    """v2 / v3: the reference's constructor has no `max_depth` there; the clip is divided by 65535 and the result stays normalised."""
    DENORMALISE = False

    def __init__(self, encoder="vitl", features=256, out_channels=[256, 512, 1024, 1024], use_bn=False, use_clstoken=False,
                 num_frames=32, pe="ape", use_residual=True, input_normal=True):
        super().__init__(encoder, features, out_channels, use_bn, use_clstoken, num_frames, 65535, pe, use_residual, input_normal)
