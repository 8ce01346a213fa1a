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

from . import clip
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
        self.sequence_length = int(sequence_length)
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

    def _trunk_features(self, rt, d: torch.Tensor, img: torch.Tensor):
        """The per-frame front of the model on F frames, d f32 [F, H, W] and img [F, 3, H, W] on the device -> (a, b, sizes):
        the 4 NHWC maps of the first branch in use, those of the second or None, and the maps' (h, w)."""
        F, H, W = d.shape
        a = b = None
        if self.use_depth_feature:
            d3 = rt.fbuf("dn_in", (F, 3, H, W))
            rt.refine_pack(d, d3, normals=True)   # (d, nx, ny) of the raw depth (utils/normal_utils.py, :78-82)
            a = self._features(self.encoder(d3), F)
        if self.use_rgb_feature:
            i = self._features(self.img_encoder(img), F)
            a, b = (i, None) if a is None else (a, i)
        sizes = [tuple(f.shape[1:3]) for f in a]
        if b is not None and [tuple(f.shape[1:3]) for f in b] != sizes:
            raise ValueError("the two trunks' feature maps differ in size")
        return a, b, sizes

    @torch.no_grad()
    def forward(self, depth: torch.Tensor, img):
        """depth f32 [B, S, H, W], img [B, S, 3, H, W] -> (depth [B, S, H, W], normal [B, S, 3, H, W])."""
        e = self._engines()
        rt, eng = e["rt"], e["head"]
        B, S, H, W = depth.shape
        F = B * S
        d = depth.to(device=rt.device, dtype=torch.float32).reshape(F, H, W).contiguous()
        a, b, sizes = self._trunk_features(rt, d, img.to(rt.device).reshape(F, 3, H, W))
        out_d = torch.empty((B, S, H, W), dtype=torch.float32, device=rt.device)
        out_n = torch.empty((B, S, 3, H, W), dtype=torch.float32, device=rt.device)
        self._taps = eng.run_model(a, b, B, S, sizes, H, W, d if self.use_residual else None, self.use_final_relu, out_d, out_n)
        return out_d, out_n

    # ------------------------------------------------------------------ the windowed clip driver
    @torch.no_grad()
    def infer_video(self, depths, frames, *, overlap=None, align=True):
        """A clip of any length through the model: depths [N, H, W] and frames [N, 3, H, W] as vdn.steps.prepare_batch makes
        them (numpy array or tensor of any real dtype, N >= 1) -> (depth f32 [N, H, W], normal f32 [N, 3, H, W]) on the device.

        The reference has no such loop for this model (its scripts see sequence_length-frame dataset items); this one is
        built from its conventions. Windows of S = sequence_length slots start every S - overlap frames
        (util.dn_window_table; overlap = S // 4 by default, 0 or 2 .. S // 2), the last one filled up with copies of the last
        frame (v5:215-283). Window 0 is stored. A later window's depth is mapped by the least-squares (scale, shift) of its
        first `overlap` frames onto the clip's (compute_scale_and_shift_full with an all-ones mask, vdn_stitch_fit; {1, 0}
        with align=False or overlap 0) and clamped at 0 if and only if use_final_relu; its normals (-dx, -dy, 1) become
        (scale nx, scale ny, 1), the gradient of the mapped depth (the clamp leaves them alone: where the clamp cuts, the
        normal is still the unclamped surface's, as `forward`'s is under its ReLU); the overlap frames are cross-faded into
        what the clip holds (get_interpolate_frames' weights 0 .. 1 on depth, nx and ny), the others stored
        (vdn_dn_stitch_apply, one launch per window). The coefficients stay on the device as self._clip_coefs [windows, 2].

        Everything in front of the head's temporal stacks depends on one frame alone, so both trunks run once per frame of
        the padded clip, in batches of S (for N <= S exactly `forward`'s batch), into a per-clip cache of their four f32 NHWC
        levels that the head reads window by window: every window is a contiguous slice of it. Where the cache does not fit
        (VDN_TAP_CACHE_GB, vdn/clip.py) every window goes through `forward` and the same stitcher. Nothing synchronises with
        the host before the final range check (util.check_finite). A wrong rank, mismatched N / H / W, a bool or complex
        dtype, N = 0 or an overlap outside its range raises ValueError before any launch."""
        return self._infer_video_device(depths, frames, overlap, align, "infer_video")

    @torch.no_grad()
    def infer_video_vis(self, depths, frames, *, overlap=None, align=True, palette="inferno", grayscale=False):
        """infer_video's clip as pictures, coloured on the device: (the depth frames as refine_video_depth_vis makes them, u8
        [N, H, W, 3] RGB or [N, H, W] with `grayscale`, one min / max for the clip; the normals as vis.colorize_normals paints
        them, u8 [N, H, W, 3]), both numpy arrays. Only uint8 crosses to the host."""
        from . import util, vis
        vis._check(palette, "rgb", "clip", grayscale, 1)
        d, n = self._infer_video_device(depths, frames, overlap, align, "infer_video_vis")
        with torch.cuda.device(d.device):
            pic = vis._colorize(self._engines()["rt"], d, palette, "rgb", "clip", grayscale, 1, None, 0, None)
        normals = vis.colorize_normals(n)
        return util.to_host(pic[..., 0] if grayscale else pic), util.to_host(normals)

    @staticmethod
    def _check_clip(depths, frames, what: str):
        import numpy as np
        for name, x, rank in (("depths", depths, 3), ("frames", frames, 4)):
            if not isinstance(x, (np.ndarray, torch.Tensor)) or len(x.shape) != rank:
                raise ValueError(f"{what}: expected {name} {'[N,H,W]' if rank == 3 else '[N,3,H,W]'} (numpy array or tensor), got "
                                 f"{type(x).__name__} {list(getattr(x, 'shape', ()))}")
            real = x.dtype.kind in "fiu" if isinstance(x, np.ndarray) else not (x.is_complex() or x.dtype == torch.bool)
            if not real:
                raise ValueError(f"{what}: expected a real dtype for {name}, got {x.dtype}")
        N, H, W = (int(v) for v in depths.shape)
        if N < 1 or H < 1 or W < 1:
            raise ValueError(f"{what}: expected a clip of N >= 1 non-empty frames, got depths {list(depths.shape)}")
        if tuple(int(v) for v in frames.shape) != (N, 3, H, W):
            raise ValueError(f"{what}: depths {list(depths.shape)} need frames [{N}, 3, {H}, {W}], got {list(frames.shape)}")
        return N, H, W

    def _infer_video_device(self, depths, frames, overlap, align: bool, what: str):
        from . import util
        from ._device import stage
        N, H, W = self._check_clip(depths, frames, what)
        S = self.sequence_length
        overlap = util.dn_check_overlap(S, overlap)
        table = util.dn_window_table(N, S, overlap)
        e = self._engines()
        rt = e["rt"]
        with torch.cuda.device(rt.device):
            d = stage(depths, rt.device, torch.float32)
            img = stage(frames, rt.device, torch.float32)
            out_d = torch.empty((N, H, W), dtype=torch.float32, device=rt.device)
            out_n = torch.empty((N, 3, H, W), dtype=torch.float32, device=rt.device)
            coefs = rt.fbuf("dn_clip_coefs", (len(table), 2))
            coefs[:, 0].fill_(1.0)
            coefs[:, 1].fill_(0.0)
            step = S - overlap
            for k, (wd, wn) in enumerate(self._clip_windows(d, img, table)):
                start = k * step
                ov = overlap if k else 0
                if ov and align:
                    target = out_d[start:start + ov]
                    if target.data_ptr() % 16:   # vdn_stitch_fit reads 16-byte vectors
                        target = rt.fbuf("dn_fit_target", (ov, H, W)).copy_(target)
                    rt.stitch_fit(wd[:ov], target, coefs[k])
                rt.dn_stitch_apply(wd, wn, coefs[k], out_d[start:], out_n[start:], ov, min(S, N - start), self.use_final_relu)
            self._clip_coefs = coefs
            util.check_finite(out_d, what)
            util.check_finite(out_n, what)
        return out_d, out_n

    def _clip_windows(self, d: torch.Tensor, img: torch.Tensor, table):
        """Yields (depth f32 [S, H, W], normal f32 [S, 3, H, W]), what `forward` returns for the window's S gathered frames, of
        every window of `table` over the staged clip, in order: two arena buffers, rewritten for the next window."""
        e = self._engines()
        rt, eng = e["rt"], e["head"]
        N, H, W = d.shape
        S = len(table[0])
        step = table[1][0] if len(table) > 1 else S
        chunks = -(-(step * (len(table) - 1) + S) // S)   # batches of S frames of the padded clip that the windows reach

        def padded(x, lo, name):
            """Frames lo .. lo + S - 1 of the padded clip: a view, or past the end of the clip an arena buffer."""
            if lo + S <= N:
                return x[lo:lo + S]
            buf = rt.fbuf(name, (S,) + tuple(x.shape[1:]))
            have = max(0, N - lo)
            if have:
                buf[:have].copy_(x[lo:N])
            buf[have:].copy_(x[N - 1:N].expand(S - have, *x.shape[1:]))
            return buf

        wd, wn = rt.fbuf("dn_win_depth", (S, H, W)), rt.fbuf("dn_win_normal", (S, 3, H, W))
        cache = None
        for c in range(chunks):
            a, b, sizes = self._trunk_features(rt, padded(d, c * S, "dn_clip_pad_d"), padded(img, c * S, "dn_clip_pad_img"))
            if cache is None:
                per_frame = sum(f[0].numel() * 4 for f in a) * (1 if b is None else 2)
                if chunks * S * per_frame > clip.cache_budget_bytes():
                    break
                cache = [[rt.fbuf(f"dn_clip_{n}{lvl}", (chunks * S,) + tuple(f.shape[1:])) for lvl, f in enumerate(t)]
                         for n, t in (("a", a), ("b", b)) if t is not None]
            for dst, src in zip(cache, (a, b)):
                for lvl in range(4):
                    dst[lvl][c * S:(c + 1) * S].copy_(src[lvl])
        if cache is None:   # the cache does not fit: `forward` on every window's frames
            for row in table:
                yield tuple(t[0] for t in self.forward(padded(d, row[0], "dn_clip_pad_d")[None], padded(img, row[0], "dn_clip_pad_img")[None]))
            return
        for row in table:
            lo = row[0]
            a, b = ([t[lo:lo + S] for t in side] for side in (cache[0], cache[-1]))
            din = padded(d, lo, "dn_clip_pad_d") if self.use_residual else None
            self._taps = eng.run_model(a, b if len(cache) == 2 else None, 1, S, sizes, H, W, din, self.use_final_relu, wd, wn)
            yield wd, wn
