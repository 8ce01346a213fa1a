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
reference's copies feed a 5-D RGB window into `forward`, whose first line unpacks four dimensions. Its loop
(v5:215-283) runs here on DEPTH windows instead, for all four:

  method                                   input                    result
  forward(input_depth)                     [B,S,H,W]                [B,S,H,W] on the device, one window
  refine_video_depth(depths, fps)          [N,H,W], N >= 1, any     (f32 [N,H,W] on the host, fps): 32-frame windows, 10 overlapping,
                                           real dtype, numpy/tensor  forward per window, aligned, clamped and cross-faded on the device
  refine_video_depth_vis(depths, fps, ..)  the same                 (u8 [N,H,W,3] RGB or [N,H,W] grey, fps): that clip through vdn.vis

The clip driver runs everything in front of the temporal head once per distinct frame (scaled clip and encoder tap cache of
vdn/clip.py stay on the device) and ends each window in one launch, vdn_refine_window_tail, which finishes window slot t
against the scaled input of the clip frame that slot shows."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _abi as abi
from . import clip, modules, util
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

    def _scaled(self, x: torch.Tensor) -> torch.Tensor:
        """f32 x [F,H0,W0] on the device -> the normalised clip, times the scale head's per-frame factor where the version has
        one (v5:162-166): per frame, so a clip's frames may be scaled together or window by window."""
        e = self._engines()
        rt = e["rt"]
        scaled = torch.empty_like(x)
        if e["scale_wb"] is not None:
            med = torch.empty(x.shape[0], dtype=torch.float32, device=rt.device)
            rt.frame_median(x, med)
            rt.refine_scale(x, med, e["scale_wb"][0], e["scale_wb"][1], 1.0, float(self.max_depth), scaled)
        else:
            rt.refine_normalize(x, float(self.max_depth), scaled)
        return scaled

    def _check_hw(self, H0: int, W0: int):
        if self.NET_HW is None and (H0 % 14 or W0 % 14):
            raise AssertionError(f"input resolution {H0}x{W0} must be a multiple of the patch size 14")  # patch_embed.py:73-74

    def _net_input(self, scaled: torch.Tensor) -> torch.Tensor:
        """The scaled frames [F,H0,W0] -> the encoder's input [F,3,H,W]: resized to NET_HW where the version has one, then
        (d, nx, ny) (v5:168-179)."""
        rt = self._engines()["rt"]
        F, H0, W0 = scaled.shape
        if self.NET_HW is not None:
            H, W = self.NET_HW
            r = torch.empty((F, H, W), dtype=torch.float32, device=rt.device)
            rt.upsample_f32(scaled, r, F, H0, W0, H, W)
        else:
            self._check_hw(H0, W0)
            H, W, r = H0, W0, scaled
        net_in = torch.empty((F, 3, H, W), dtype=torch.float32, device=rt.device)
        rt.refine_pack(r, net_in, normals=self.input_normal)
        return net_in

    def _tail(self):
        """(kind, residual, five coefficients) of the version's finish step, as vdn_refine_window_tail takes them."""
        e = self._engines()
        unit = float(self.max_depth) if self.DENORMALISE else 1.0
        if "shift_wb" in e:
            return abi.TAIL_SHIFT, self.use_residual, (e["shift_wb"][0], e["shift_wb"][1], unit, 0.0, 0.0)
        if self.use_residual:
            return abi.TAIL_MIX, True, e["mix"]
        return abi.TAIL_SHIFT, False, (0.0, 0.0, unit, 0.0, 0.0)   # v2 without final_res: the rectified depth itself

    @torch.no_grad()
    def forward(self, input_depth: torch.Tensor) -> torch.Tensor:
        """input_depth f32 [B,S,H,W] in [0, max_depth] -> refined depth [B,S,H,W] (v5:160-192 / v4:117-148 / v3:167-206 /
        v2:75-100); v2 and v3 return it normalised, v4 and v5 in the input's units."""
        e = self._engines()
        rt, enc, head = e["rt"], e["enc"], e["head"]
        B, S, H0, W0 = input_depth.shape
        F = B * S
        x = input_depth.to(device=rt.device, dtype=torch.float32).reshape(F, H0, W0).contiguous()
        scaled = self._scaled(x)
        net_in = self._net_input(scaled)
        H, W = net_in.shape[-2:]
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

    # ------------------------------------------------------------------ the windowed clip driver (v5:215-283 on depth windows)
    @torch.no_grad()
    def refine_video_depth(self, depths, target_fps=None):
        """A depth clip [N,H,W] (N >= 1; numpy array or tensor of any real dtype, in `forward`'s units [0, max_depth]) ->
        (f32 [N,H,W] in `forward`'s result units, target_fps): the loop of the reference's `infer_video_depth` (v5:215-283, the
        same text in v2 .. v4) with the depth clip in place of the RGB frames and without the RGB transform, which cannot run
        there. 32-slot windows of `util.window_table`, slots 0..9 of a later window holding the previous
        window's INPUTS at KEYFRAMES; `forward` per window; scale/shift on the two alignment frames, clamp at 0 and the
        8-frame cross-fade on the device (`DeviceStitcher`); one pinned device-to-host copy. v2 .. v4 need H and W to be
        multiples of 14 and raise as `forward` does; a wrong rank or N = 0 raises ValueError before any launch."""
        return util.to_host(self._refine_video_depth_device(depths, "refine_video_depth")), target_fps

    @torch.no_grad()
    def refine_video_depth_vis(self, depths, target_fps=None, grayscale: bool = False, palette: str = "inferno"):
        """refine_video_depth's clip as the frames save_video(depths, is_depths=True) of utils/dc_utils.py:72-81 writes: u8
        [N,H,W,3] RGB, or [N,H,W] with `grayscale`, one min/max for the clip, coloured on the device (vdn.vis); the clip's only
        device-to-host copy is the uint8 frames. Built as `VideoDepthAnything.infer_video_depth_vis` is."""
        from . import vis
        vis._check(palette, "rgb", "clip", grayscale, 1)
        res = self._refine_video_depth_device(depths, "refine_video_depth_vis")
        with torch.cuda.device(res.device):
            out = vis._colorize(self._engines()["rt"], res.contiguous(), palette, "rgb", "clip", grayscale, 1, None, 0, None)
        return util.to_host(out[..., 0] if grayscale else out), target_fps

    def _refine_video_depth_device(self, depths, what: str) -> torch.Tensor:
        """refine_video_depth up to its device-to-host copy: the stitched, range-checked clip f32 [N,H,W] on the device.
        Everything in front of the temporal head depends on one frame alone, so it runs once per DISTINCT clip frame: the
        median and scale over the whole clip (the scaled clip stays on the device), then resize, normals and encoder in
        batches of INFER_LEN into the clip-level tap cache of vdn/clip.py. A window's head reads its 32 slots from the cache and
        vdn_refine_window_tail finishes slot t against the scaled input of the clip frame it shows. Where the cache does not
        fit (VDN_TAP_CACHE_GB) every window goes through `forward`."""
        from ._device import stage
        from .video_depth import DeviceStitcher
        shape = tuple(getattr(depths, "shape", ()))
        if not isinstance(depths, (np.ndarray, torch.Tensor)) or len(shape) != 3 or shape[0] < 1 or shape[1] < 1 or shape[2] < 1:
            raise ValueError(f"{what}: expected a depth clip [N,H,W] with N >= 1 (numpy array or tensor), got "
                             f"{type(depths).__name__} {list(shape)}")
        if isinstance(depths, torch.Tensor) and (depths.is_complex() or depths.dtype == torch.bool):
            raise ValueError(f"{what}: expected a real dtype, got {depths.dtype}")
        if isinstance(depths, np.ndarray) and depths.dtype.kind not in "fiu":
            raise ValueError(f"{what}: expected a real dtype, got {depths.dtype}")
        N, H0, W0 = shape
        self._check_hw(H0, W0)
        rt = self._engines()["rt"]
        x = stage(depths, rt.device, torch.float32)
        st = DeviceStitcher(rt, len(util.window_table(N)), H0, W0)
        for d in self._refined_windows(x):
            st.push(d)
        res = st.result(N)
        util.check_finite(res, what)
        return res

    def _refined_windows(self, x: torch.Tensor):
        """Yields the refined window [32,H,W] (what `forward` returns for the window's 32 gathered frames) of every window of the
        clip x f32 [N,H,W] on the device, in order; one buffer, rewritten for the next window."""
        e = self._engines()
        rt, enc, head = e["rt"], e["enc"], e["head"]
        N, H0, W0 = x.shape
        table = util.window_table(N)
        windows = list(range(len(table)))
        H, W = self.NET_HW if self.NET_HW is not None else (H0, W0)
        need, fits = clip.tap_cache_plan(rt, self.pretrained.embed_dim, H, W, table, windows)
        if not fits:
            for w in windows:
                yield self.forward(x[torch.tensor(table[w], device=rt.device)][None])[0]
            return
        scaled = self._scaled(x)
        slots = torch.from_numpy(util.window_slots(N)).to(rt.device)   # int32 [windows, 32], range-checked, one upload per clip

        def net_batch(fr):
            run = fr == list(range(fr[0], fr[0] + len(fr)))
            return self._net_input((scaled[fr[0]:fr[0] + len(fr)] if run else scaled[torch.tensor(fr, device=rt.device)]).contiguous())

        kind, residual, coef = self._tail()
        out = rt.buf("refine_window_out", (util.INFER_LEN, H0, W0), torch.float32)
        for w, d in zip(windows, clip.cached_window_depths(rt, enc, head, self.pretrained.embed_dim, net_batch, H, W, table, windows, need)):
            rt.refine_window_tail(d.contiguous(), scaled, slots[w], kind, residual, coef, out)
            yield out


class _DepthRefiner65535(_DepthRefiner):
    """v2 / v3: the reference's constructor has no `max_depth` there; the clip is divided by 65535 and the result stays normalised."""
    DENORMALISE = False

    def __init__(self, encoder="vitl", features=256, out_channels=[256, 512, 1024, 1024], use_bn=False, use_clstoken=False,
                 num_frames=32, pe="ape", use_residual=True, input_normal=True):
        super().__init__(encoder, features, out_channels, use_bn, use_clstoken, num_frames, 65535, pe, use_residual, input_normal)
