"""Drop-in for the metric-depth model of metric_depth/depth_anything_v2/dpt.py — same class name, constructor and
state-dict keys (`pretrained.*`, `depth_head.*`: an upstream depth_anything_v2_metric_* checkpoint loads with strict=True);
the forward pass runs on libvdn_hip.so (MI355X), never on torch ops.

The reference keeps the class itself commented out (dpt.py:152-222) and ships its two halves live: DINOv2 (dinov2.py, the main
copy's) and a DPTHead whose output_conv2 ends in nn.Sigmoid() (dpt.py:38-149). What joins them is restated here, not imported:

    features = self.pretrained.get_intermediate_layers(x, idx[encoder], return_class_token=True)
    depth = self.depth_head(features, patch_h, patch_w) * self.max_depth
    return depth.squeeze(1)

as the commented class spells it (dpt.py:178-185) and as every caller relies on it (metric_depth/train.py:88,131,165-166,
run.py:38,60, depth_to_pointcloud.py:66,93). The sigmoid and the factor are the final activation of the head's last kernel
(include/vdn.h VDN_OUT_SIGMOID): max_depth is a launch argument, so changing model.max_depth rebuilds nothing.

There is no memory block: a call keeps no state, and the batch or the resolution may change between calls. By default a batch
is run frame by frame, each frame through the launches a batch of one gets: the library picks kernels by row count in many
places (split-K slicing, GEMM tile and kernel family, the 8-bit cross-term kernel from 4096 rows, the low-resolution
output_conv1 from 65536), so only then is a frame's depth the same bits whatever batch it arrives in. That is also how the
reference's scripts call the model (run.py, depth_to_pointcloud.py and train.py's validation: one image per call).
set_batch_invariant(False) runs the batch in one pass instead, for throughput; results then agree to rounding.
Inference only: model.train(), gradients, SyncBatchNorm and the optimiser of train.py stay outside."""
from __future__ import annotations

import numpy as np
import torch

from ... import _abi as abi
from ... import modules
from ...depth_anything_v2 import _SingleImage
from ...engine import DPTEngine, EncoderEngine, ReadoutEngine


class DepthAnythingV2(_SingleImage):
    def __init__(self, encoder="vitl", features=256, out_channels=[256, 512, 1024, 1024], use_bn=False, use_clstoken=False,
                 max_depth=20.0):
        super().__init__()
        self.intermediate_layer_idx = {k: v["taps"] for k, v in modules.ENCODERS.items()}
        self.max_depth = max_depth
        self.encoder = encoder
        cfg = modules.ENCODERS[encoder]
        self.pretrained = modules.dinov2(encoder)
        self.depth_head = modules.dpt_head(cfg["dim"], features, out_channels, use_bn, use_clstoken)
        self._features, self._out_channels = features, list(out_channels)
        self.batch_invariant = True

    def set_batch_invariant(self, flag: bool):
        """True (default): a batch runs frame by frame, so a frame's depth is the same bits in any batch. False: the batch runs
        in one pass (profiles/metric_model.md has both at ViT-L 518 x 518, batch 8); a frame's result then follows the kernels its
        batch's row count selects and agrees with the default to rounding only. No engine rebuild."""
        self.batch_invariant = bool(flag)
        return self

    def _engines(self):
        if self._eng is None:
            rt = self._runtime()
            cfg = modules.ENCODERS[self.encoder]
            self._eng = dict(
                rt=rt, enc=EncoderEngine(rt, self.pretrained, cfg),
                head=DPTEngine(rt, self.depth_head, cfg["dim"], self._features, self._out_channels, temporal=False))
            if hasattr(self.depth_head, "readout_projects"):   # use_clstoken: every tap gets its readout right after the encoder
                self._eng["enc"].readout = ReadoutEngine(rt, self.depth_head.readout_projects, cfg["dim"])
        return self._eng

    @torch.no_grad()
    def forward(self, x: torch.Tensor, _pre_act: bool = False) -> torch.Tensor:
        """x f32 [B,3,H,W] (H, W multiples of 14, not necessarily square) -> f32 [B,H,W] in metres: max_depth * sigmoid of the
        head's logits. `_pre_act` (tests only) returns the logits in front of the sigmoid."""
        e = self._engines()
        rt = e["rt"]
        x = x.to(device=rt.device, dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        out = torch.empty((B, H, W), dtype=torch.float32, device=rt.device)   # the one allocation of a forward: its result
        rt.cu_hint = 0
        act, n = abi.OUT_NONE if _pre_act else abi.OUT_SIGMOID, 1 if self.batch_invariant else max(B, 1)
        with torch.cuda.device(rt.device):
            for b in range(0, B, n):   # frame by frame (module docstring), or the whole batch at once
                taps, _, (ph, pw) = e["enc"].run(x[b:b + n])
                e["head"].run(taps, n, ph, pw, act=act, out_scale=float(self.max_depth), out=out[b:b + n])
        return out

    @torch.no_grad()
    def infer_image(self, raw_image: np.ndarray, input_size: int = 518) -> np.ndarray:
        """BGR u8 [h,w,3] -> f32 [h,w] in metres (dpt.py:187-195)."""
        return self._infer_image_device(raw_image, input_size, "infer_image")[0][0].cpu().numpy()

    @torch.no_grad()
    def infer_image_vis(self, raw_image: np.ndarray, input_size: int = 518, pred_only: bool = False, grayscale: bool = False,
                        palette: str = "Spectral") -> np.ndarray:
        """BGR u8 [h,w,3] -> BGR u8 [h,w,3] (pred_only) or [h, 2w+50, 3] (raw | 50 white columns | depth): the array
        metric_depth/run.py:60-78 builds on the host from infer_image's result ('Spectral', not the relative model's
        'Spectral_r') and hands to cv2.imwrite, byte for byte, made on the device (vdn.vis); only the uint8 picture is
        copied back."""
        return self._infer_image_vis(raw_image, input_size, pred_only, grayscale, palette)

    @torch.no_grad()
    def infer_image_points(self, raw_image: np.ndarray, input_size: int = 518, fx: float = 470.4, fy: float = 470.4):
        """BGR u8 [h,w,3] -> (points, colors), float64 [h*w, 3] each, on the device: depth_to_pointcloud.py:92-104 from
        infer_image on (vdn.points.depth_to_points). The colours are the frame's, its channels swapped to RGB (the script
        reads the same file a second time through PIL); its Image.NEAREST resize of line 96 is the identity, because
        infer_image already returns the frame's (height, width)."""
        from ...points import depth_to_points
        depth, img = self._infer_image_device(raw_image, input_size, "infer_image_points")
        return depth_to_points(depth[0], img[0].flip(-1).contiguous(), fx, fy, device=depth.device)
