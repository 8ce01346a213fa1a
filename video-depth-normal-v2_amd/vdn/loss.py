"""The depth criterion on the device: the reference's loss.loss.VideoDepthLoss as its scripts construct it, computed by the
kernels of csrc/loss.hip on tensors that can stay in HBM. In the `validate` of scripts/train.py, train_v2.py, train_v3.py and
train_v4.py, replace

    from loss.loss import VideoDepthLoss
by
    from vdn.loss import VideoDepthLoss

Forward only: nothing here records a gradient. Tensors are taken as float32 (masks as "non-zero = keep"; bool, uint8 and
float masks all do); a CUDA tensor of the right type is used in place, anything else is copied to `device` once, and results
stay on the device unless a function says otherwise. include/vdn.h (vdn_depth_loss) states the arithmetic: the fit and all
sums are fp64 on the device, and exactly the operations the reference's float32 tensors decide something with (the
alignment scale * p + shift, medians, thresholds, the quotients of d1) are the same float32 operations. Sums have a fixed
order, so two runs give the same bits.

One difference from the reference: a dropped pixel is skipped, where the reference multiplies it by the mask. NaN or inf
under a dropped pixel therefore reaches nothing here, and poisons the reference's sums.

Not computed, each raising NotImplementedError: trim != 0 (a global k-smallest selection the scripts never ask for),
reduction != "batch-based" (the reference's image-based branch indexes a 1-D vector with the mask's coordinates) and
ssim_loss_scale > 0 (the reference's term needs pytorch_msssim). scales above 4 (the reference's default) likewise."""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from .normals import _on_device, _runtime_for

OUT_SLOTS = 20   # include/vdn.h: the layout of vdn_depth_loss's out
MAX_SCALES = 4


def _check(prediction, target, mask, dims: int) -> tuple:
    if not isinstance(prediction, torch.Tensor) or prediction.dim() != dims:
        want = "[B, T, H, W]" if dims == 4 else "[B, H, W]"
        raise ValueError(f"prediction must be {want}, got {tuple(getattr(prediction, 'shape', ()))}")
    for name, t in (("target", target), ("mask", mask)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(prediction.shape):
            raise ValueError(f"{name} shape {tuple(getattr(t, 'shape', ()))} is not the prediction's {tuple(prediction.shape)}")
    if prediction.numel() == 0:
        raise ValueError("empty input")
    return tuple(prediction.shape)


def _check_args(alpha, scales, trim, stable_scale, ssim_loss_scale, reduction):
    if trim != 0:
        raise NotImplementedError(f"trim={trim!r}: the trimmed losses need a global k-smallest selection, which the "
                                  "reference's scripts never ask for; only trim=0.0 is computed")
    if reduction != "batch-based":
        raise NotImplementedError(f"reduction={reduction!r}: the reference's image-based branch indexes a 1-D vector with the "
                                  "mask's coordinates; only 'batch-based' is defined")
    if ssim_loss_scale > 0:
        raise NotImplementedError(f"ssim_loss_scale={ssim_loss_scale!r}: the reference's SSIM term needs pytorch_msssim; "
                                  "only ssim_loss_scale=0.0 is computed")
    if int(scales) != scales or not 0 <= scales <= MAX_SCALES:
        raise NotImplementedError(f"scales={scales!r}: 0 .. {MAX_SCALES} gradient grids are computed")


def _launch(prediction, target, mask, alpha, scales, stable_scale, device, per_frame: bool):
    """-> (runtime, res): res float64 on the device, out[20] | frame_stats [F][4] | frame_counts [F] (int64) when per_frame."""
    B, T, H, W = _check(prediction, target, mask, 4)
    if stable_scale > 0 and T < 2:
        raise ValueError("stable_scale > 0 needs T >= 2: the temporal term of a single frame divides by a count of zero")
    rt = _runtime_for(device, prediction, target, mask)
    p = _on_device(prediction, rt.device, torch.float32)
    t = _on_device(target, rt.device, torch.float32)
    m = _on_device(mask, rt.device, torch.uint8)
    F = B * T
    with torch.cuda.device(rt.device):
        res = rt.buf("depth_loss_res", (OUT_SLOTS + 5 * F,), torch.float64)
        stats = res[OUT_SLOTS:OUT_SLOTS + 4 * F] if per_frame else None
        counts = res[OUT_SLOTS + 4 * F:].view(torch.int64) if per_frame else None
        rt.depth_loss(p, t, m, res[:OUT_SLOTS], alpha, int(scales), stable_scale, None, stats, counts)
    return rt, res


class VideoDepthLoss(torch.nn.Module):
    """loss/loss.py:326-367, forward only, with the reference's constructor signature and attributes. trim != 0,
    reduction != "batch-based" and ssim_loss_scale > 0 raise NotImplementedError (see the module's text)."""

    def __init__(self, alpha=0.5, scales=4, trim=0.0, stable_scale=10, ssim_loss_scale=0.0, reduction="batch-based", *,
                 device="cuda"):
        super().__init__()
        _check_args(alpha, scales, trim, stable_scale, ssim_loss_scale, reduction)
        self.stable_scale = stable_scale
        self.ssim_loss_scale = ssim_loss_scale
        self.initial_alpha = alpha
        self.initial_stable_scale = stable_scale
        self._alpha = float(alpha)   # fixed at construction, as in the reference's TrimmedProcrustesLoss; initial_alpha is a record
        self.scales = int(scales)
        self.device = device

    @property
    def keys(self) -> Tuple[str, ...]:
        """The keys of forward's dictionary, in the reference's order: 'stable_loss' only when stable_scale > 0."""
        return (("spatial_loss",) + (("stable_loss",) if self.stable_scale > 0 else ()) + ("absRel_loss", "d1", "total_loss"))

    def forward(self, prediction, target, mask) -> Dict[str, torch.Tensor]:
        """prediction, target, mask [B, T, H, W] -> {'spatial_loss', 'stable_loss' (when stable_scale > 0), 'absRel_loss',
        'd1', 'total_loss'}: 0-dim float32 tensors on the device, no host synchronisation. ValueError when T == 1 and
        stable_scale > 0, where the reference divides by zero."""
        if self.ssim_loss_scale > 0:      # the attribute is public, as in the reference
            raise NotImplementedError("ssim_loss_scale > 0 is not computed")
        rt, res = _launch(prediction, target, mask, self._alpha, self.scales, float(self.stable_scale),
                          self.device, False)
        with torch.cuda.device(rt.device):
            v = res[:5].to(torch.float32)   # a copy: the buffer is reused by the next call
        slot = {"spatial_loss": 0, "stable_loss": 1, "absRel_loss": 2, "d1": 3, "total_loss": 4}
        return {k: v[slot[k]] for k in self.keys}


def compute_scale_and_shift(prediction, target, mask, *, device="cuda"):
    """loss/loss.py:74-96 for [B, H, W] tensors -> float32 (scale [B], shift [B]) on the device: the masked least-squares
    fit of scale * prediction + shift to target per item, sums in fp64, rounded once (the fit pass of vdn_depth_loss alone)."""
    B, H, W = _check(prediction, target, mask, 3)
    rt = _runtime_for(device, prediction, target, mask)
    # An item's H * W pixels are handed to the kernel as `parts` frames of equal length (the most, up to 64, that leave 32768
    # pixels each, four for every lane of a frame's blocks): the fit sums an item's frames, and a frame is what the kernel
    # spreads over blocks.
    n = H * W
    parts = next((c for c in range(64, 1, -1) if n % c == 0 and n // c >= 32768 and B * c <= 65535), 1)
    p = _on_device(prediction, rt.device, torch.float32).view(B, parts, 1, n // parts)
    t = _on_device(target, rt.device, torch.float32).view(B, parts, 1, n // parts)
    m = _on_device(mask, rt.device, torch.uint8).view(B, parts, 1, n // parts)
    with torch.cuda.device(rt.device):
        ss = torch.empty((B, 2), dtype=torch.float32, device=rt.device)
        rt.depth_loss(p, t, m, None, scale_shift=ss)
    return ss[:, 0], ss[:, 1]


def depth_loss(prediction, target, mask, alpha=0.5, scales=4, stable_scale=10, *, device="cuda") -> dict:
    """The fp64 values of one launch, read with one synchronising copy. prediction, target, mask [B, T, H, W]. Returns
    Python floats 'spatial_loss', 'stable_loss' (when stable_scale > 0), 'absRel_loss', 'd1', 'total_loss', 'data', and CPU
    tensors 'g' float64 [4] and 'M' int64 [4] (the gradient term and kept points of each grid; zeros beyond `scales`),
    'm_pred', 's_pred', 'm_target', 's_target' float64 [B, T] (median and scale of the robust normalisation per frame) and
    'count' int64 [B, T], and the integers 'stable_count', 'absrel_count' and 'd1_hits' (the pixels behind those three means)."""
    _check_args(alpha, scales, 0.0, stable_scale, 0.0, "batch-based")
    B, T = prediction.shape[:2] if isinstance(prediction, torch.Tensor) and prediction.dim() == 4 else (0, 0)
    rt, res = _launch(prediction, target, mask, float(alpha), scales, float(stable_scale), device, True)
    host = res.cpu()
    F = B * T
    out = {k: float(host[i]) for i, k in enumerate(("spatial_loss", "stable_loss", "absRel_loss", "d1", "total_loss", "data"))}
    if not stable_scale > 0:
        del out["stable_loss"]
    out.update(stable_count=int(host[16]), absrel_count=int(host[17]), d1_hits=int(host[18]))
    stats = host[OUT_SLOTS:OUT_SLOTS + 4 * F].view(B, T, 4)
    out.update(g=host[8:12].clone(), M=host[12:16].to(torch.int64), m_pred=stats[..., 0].clone(), s_pred=stats[..., 1].clone(),
               m_target=stats[..., 2].clone(), s_target=stats[..., 3].clone(),
               count=host[OUT_SLOTS + 4 * F:].view(torch.int64).view(B, T).clone())
    return out
