"""The depth criterion on the device: the reference's loss.loss.VideoDepthLoss as its scripts construct it, computed by the
kernels of csrc/loss.hip on tensors that can stay in HBM, with its gradient with respect to the prediction by the kernels of
csrc/loss_grad.hip. In scripts/train.py, train_v2.py, train_v3.py and train_v4.py, which build the criterion once and use it
in `validate` (under no_grad) and in the training step (total_loss.backward()), replace

    from loss.loss import VideoDepthLoss
by
    from vdn.loss import VideoDepthLoss

Gradients. A prediction that requires a gradient (with gradients enabled) goes through a torch.autograd.Function: the
forward is the same launch, the backward is one launch of vdn_depth_loss_backward for whatever combination of the
dictionary's entries was differentiated (d1 is piecewise constant and contributes zero). It is once differentiable. Without
a gradient to record, forward is what it was: the same launches and tensors, nothing extra. A target that requires a
gradient raises NotImplementedError: the reference would differentiate it and none of its scripts does. depth_loss_grad
returns the same gradient without autograd.

Tensors are taken as float32 (masks as "non-zero = keep"; bool, uint8 and
float masks all do); a CUDA tensor of the right type is used in place, anything else is copied to `device` once, and results
stay on the device unless a function says otherwise. include/vdn.h (vdn_depth_loss) states the arithmetic: the fit and all
sums are fp64 on the device, and exactly the operations the reference's float32 tensors decide something with (the
alignment scale * p + shift, medians, thresholds, the quotients of d1) are the same float32 operations. Sums have a fixed
order, so two runs give the same bits.

One difference from the reference: a dropped pixel is skipped, where the reference multiplies it by the mask. NaN or inf
under a dropped pixel therefore reaches nothing here, and poisons the reference's sums.

The trimmed criterion. The reference's VideoDepthLoss takes `trim` as its third argument: each of the data, temporal and
absRel terms then sums only the int(n * (1 - trim)) smallest of its n residuals (and still divides by n). Here that is
TrimmedVideoDepthLoss (and the keyword `trim` of depth_loss and depth_loss_grad): one batch-wide exact selection on the
device per term, the rank computed on the device, forward and backward (include/vdn.h, vdn_depth_loss_trimmed).
VideoDepthLoss itself keeps refusing trim != 0.

Not computed, each raising NotImplementedError: trim != 0 in VideoDepthLoss (use TrimmedVideoDepthLoss),
reduction != "batch-based" (the reference's image-based branch indexes a 1-D vector with the mask's coordinates) and
ssim_loss_scale > 0 (the reference's term needs pytorch_msssim). scales above 4 (the reference's default) likewise."""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from ._device import runtime_for, stage, wants_grad

OUT_SLOTS = 20   # include/vdn.h: the layout of vdn_depth_loss's out
TRIM_SLOTS = 40  # ... and of vdn_depth_loss_trimmed's: 20 + 5 * term: k | n_less | n_tied | threshold | weight
MAX_SCALES = 4
_SLOT = {"spatial_loss": 0, "stable_loss": 1, "absRel_loss": 2, "d1": 3, "total_loss": 4}


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


def _check_trim(trim) -> float:
    """-> keep = 1.0 - trim as the reference computes it, for 0 <= trim < 1."""
    if isinstance(trim, bool) or not isinstance(trim, (int, float)) or not 0 <= trim < 1:
        raise ValueError(f"trim={trim!r}: a number in [0, 1) (the share of the largest residuals that each term drops)")
    return 1.0 - float(trim)


def _launch(prediction, target, mask, alpha, scales, stable_scale, device, per_frame: bool, state: bool = False, keep: float = 1.0):
    """-> (runtime, res): res float64 on the device, out[N] | frame_stats [F][4] | frame_counts [F] (int64) when per_frame;
    N = 20, or 40 when keep < 1 (the trimmed launch).
    state: -> (runtime, res, the fit f32 [B, 2] in a tensor of its own, and the float32 prediction, target and uint8 mask the
    kernels read), what the backward needs."""
    B, T, H, W = _check(prediction, target, mask, 4)
    if stable_scale > 0 and T < 2:
        raise ValueError("stable_scale > 0 needs T >= 2: the temporal term of a single frame divides by a count of zero")
    rt = runtime_for(device, prediction, target, mask)
    p = stage(prediction, rt.device, torch.float32)
    t = stage(target, rt.device, torch.float32)
    m = stage(mask, rt.device, torch.uint8)
    F = B * T
    with torch.cuda.device(rt.device):
        N = TRIM_SLOTS if keep < 1.0 else OUT_SLOTS
        res = rt.buf("depth_loss_res", (N + 5 * F,), torch.float64)
        stats = res[N:N + 4 * F] if per_frame else None
        counts = res[N + 4 * F:].view(torch.int64) if per_frame else None
        ss = torch.empty((B, 2), dtype=torch.float32, device=rt.device) if state else None
        rt.depth_loss(p, t, m, res[:N], alpha, int(scales), stable_scale, ss, stats, counts, keep=keep)
    return (rt, res, ss, p, t, m) if state else (rt, res)


def _backward(rt, p, t, m, alpha, scales, stable_scale, ss, res, coeff, keep: float = 1.0) -> torch.Tensor:
    """One launch of vdn_depth_loss_backward (vdn_depth_loss_trimmed_backward when keep < 1) -> float32 [B, T, H, W]. res:
    out | frame_stats | frame_counts as _launch left them for these inputs and this keep (a copy: the runtime's buffer is reused
    by the next call); coeff float32 [3] on the device."""
    F = p.shape[0] * p.shape[1]
    N = TRIM_SLOTS if keep < 1.0 else OUT_SLOTS
    with torch.cuda.device(rt.device):
        grad = torch.empty_like(p)
        rt.depth_loss_backward(p, t, m, alpha, int(scales), stable_scale, ss, res[N:N + 4 * F], res[N + 4 * F:].view(torch.int64),
                               res[:N], coeff, grad, keep=keep)
    return grad


class _DepthLossFn(torch.autograd.Function):
    """The five values of the criterion as one float32 [5] tensor (slots of _SLOT), differentiable in `prediction`."""

    @staticmethod
    def forward(ctx, prediction, target, mask, alpha, scales, stable_scale, device, keep=1.0):
        rt, res, ss, p, t, m = _launch(prediction, target, mask, alpha, scales, stable_scale, device, True, state=True, keep=keep)
        with torch.cuda.device(rt.device):
            res = res.clone()   # the O(B T) state, kept: the runtime's buffer is reused by the next call
            v = res[:5].to(torch.float32)
        ctx.save_for_backward(p, t, m, ss, res)
        ctx.args = (rt, alpha, scales, stable_scale, prediction.dtype, prediction.device, keep)
        return v

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        p, t, m, ss, res = ctx.saved_tensors
        rt, alpha, scales, stable_scale, dtype, device, keep = ctx.args
        with torch.cuda.device(rt.device):
            g = g.to(device=rt.device, dtype=torch.float32)
            coeff = torch.stack((g[4] + g[0], g[4] * stable_scale + g[1], g[2]))   # c_sp, c_st, c_ar; d1 contributes zero
        grad = _backward(rt, p, t, m, alpha, scales, stable_scale, ss, res, coeff, keep)
        return grad.to(device=device, dtype=dtype), None, None, None, None, None, None, None


class VideoDepthLoss(torch.nn.Module):
    """loss/loss.py:326-367 with the reference's constructor signature and attributes, differentiable in the prediction.
    trim != 0, reduction != "batch-based" and ssim_loss_scale > 0 raise NotImplementedError (see the module's text)."""

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
        self._keep = 1.0             # nothing is trimmed; TrimmedVideoDepthLoss sets 1 - trim

    @property
    def keys(self) -> Tuple[str, ...]:
        """The keys of forward's dictionary, in the reference's order: 'stable_loss' only when stable_scale > 0."""
        return (("spatial_loss",) + (("stable_loss",) if self.stable_scale > 0 else ()) + ("absRel_loss", "d1", "total_loss"))

    def forward(self, prediction, target, mask) -> Dict[str, torch.Tensor]:
        """prediction, target, mask [B, T, H, W] -> {'spatial_loss', 'stable_loss' (when stable_scale > 0), 'absRel_loss',
        'd1', 'total_loss'}: 0-dim float32 tensors on the device, no host synchronisation. ValueError when T == 1 and
        stable_scale > 0, where the reference divides by zero. With gradients enabled and a prediction that requires one, the
        values carry a grad_fn whose backward gives prediction.grad in the prediction's dtype and shape."""
        if self.ssim_loss_scale > 0:      # the attribute is public, as in the reference
            raise NotImplementedError("ssim_loss_scale > 0 is not computed")
        if wants_grad(prediction, target):
            v = _DepthLossFn.apply(prediction, target, mask, self._alpha, self.scales, float(self.stable_scale), self.device,
                                   self._keep)
            return {k: v[_SLOT[k]] for k in self.keys}
        rt, res = _launch(prediction, target, mask, self._alpha, self.scales, float(self.stable_scale),
                          self.device, False, keep=self._keep)
        with torch.cuda.device(rt.device):
            v = res[:5].to(torch.float32)   # a copy: the buffer is reused by the next call
        return {k: v[_SLOT[k]] for k in self.keys}


class TrimmedVideoDepthLoss(VideoDepthLoss):
    """The reference's VideoDepthLoss(alpha, scales, trim, stable_scale) with trim > 0: the data term, the temporal term and
    absRel each sum the int(n * (1.0 - trim)) smallest of their n counted residuals and divide by n (loss/loss.py:164-219); the
    regulariser and d1 are not trimmed. Same forward, keys and dictionary as VideoDepthLoss, differentiable in the prediction
    (one forward and one backward launch: vdn_depth_loss_trimmed and its backward). Residuals that share the threshold's
    float32 key are weighted equally, where the reference's unstable sort keeps an arbitrary subset of them. 0 <= trim < 1,
    ValueError otherwise; trim == 0 is VideoDepthLoss, bit for bit."""

    def __init__(self, alpha=0.5, scales=4, trim=0.2, stable_scale=10, *, device="cuda"):
        keep = _check_trim(trim)
        super().__init__(alpha, scales, 0.0, stable_scale, device=device)
        self.trim = trim
        self._keep = keep


def compute_scale_and_shift(prediction, target, mask, *, device="cuda"):
    """loss/loss.py:74-96 for [B, H, W] tensors -> float32 (scale [B], shift [B]) on the device: the masked least-squares
    fit of scale * prediction + shift to target per item, sums in fp64, rounded once (the fit pass of vdn_depth_loss alone)."""
    B, H, W = _check(prediction, target, mask, 3)
    rt = runtime_for(device, prediction, target, mask)
    # An item's H * W pixels are handed to the kernel as `parts` frames of equal length (the most, up to 64, that leave 32768
    # pixels each, four for every lane of a frame's blocks): the fit sums an item's frames, and a frame is what the kernel
    # spreads over blocks.
    n = H * W
    parts = next((c for c in range(64, 1, -1) if n % c == 0 and n // c >= 32768 and B * c <= 65535), 1)
    p = stage(prediction, rt.device, torch.float32).view(B, parts, 1, n // parts)
    t = stage(target, rt.device, torch.float32).view(B, parts, 1, n // parts)
    m = stage(mask, rt.device, torch.uint8).view(B, parts, 1, n // parts)
    with torch.cuda.device(rt.device):
        ss = torch.empty((B, 2), dtype=torch.float32, device=rt.device)
        rt.depth_loss(p, t, m, None, scale_shift=ss)
    return ss[:, 0], ss[:, 1]


def depth_loss(prediction, target, mask, alpha=0.5, scales=4, stable_scale=10, *, trim=0.0, device="cuda") -> dict:
    """The fp64 values of one launch, read with one synchronising copy. prediction, target, mask [B, T, H, W]. Returns
    Python floats 'spatial_loss', 'stable_loss' (when stable_scale > 0), 'absRel_loss', 'd1', 'total_loss', 'data', and CPU
    tensors 'g' float64 [4] and 'M' int64 [4] (the gradient term and kept points of each grid; zeros beyond `scales`),
    'm_pred', 's_pred', 'm_target', 's_target' float64 [B, T] (median and scale of the robust normalisation per frame) and
    'count' int64 [B, T], and the integers 'stable_count', 'absrel_count' and 'd1_hits' (the pixels behind those three means).
    trim > 0: the trimmed criterion, and for the terms (data, stable, absRel) also 'trim_k', 'trim_less', 'trim_tied' int64 [3]
    (kept residuals, residuals below the threshold key, residuals at it) and 'trim_threshold', 'trim_weight' float64 [3]."""
    _check_args(alpha, scales, 0.0, stable_scale, 0.0, "batch-based")
    keep = _check_trim(trim)
    B, T = prediction.shape[:2] if isinstance(prediction, torch.Tensor) and prediction.dim() == 4 else (0, 0)
    rt, res = _launch(prediction, target, mask, float(alpha), scales, float(stable_scale), device, True, keep=keep)
    host = res.cpu()
    F = B * T
    if keep < 1.0:
        tr = host[OUT_SLOTS:OUT_SLOTS + 15].view(3, 5)
        host = torch.cat((host[:OUT_SLOTS], host[TRIM_SLOTS:]))
    out = {k: float(host[i]) for i, k in enumerate(("spatial_loss", "stable_loss", "absRel_loss", "d1", "total_loss", "data"))}
    if not stable_scale > 0:
        del out["stable_loss"]
    out.update(stable_count=int(host[16]), absrel_count=int(host[17]), d1_hits=int(host[18]))
    stats = host[OUT_SLOTS:OUT_SLOTS + 4 * F].view(B, T, 4)
    out.update(g=host[8:12].clone(), M=host[12:16].to(torch.int64), m_pred=stats[..., 0].clone(), s_pred=stats[..., 1].clone(),
               m_target=stats[..., 2].clone(), s_target=stats[..., 3].clone(),
               count=host[OUT_SLOTS + 4 * F:].view(torch.int64).view(B, T).clone())
    if keep < 1.0:
        out.update(trim_k=tr[:, 0].to(torch.int64), trim_less=tr[:, 1].to(torch.int64), trim_tied=tr[:, 2].to(torch.int64),
                   trim_threshold=tr[:, 3].clone(), trim_weight=tr[:, 4].clone())
    return out


def depth_loss_grad(prediction, target, mask, alpha=0.5, scales=4, stable_scale=10, *, weights=(1, 0, 0, 0), trim=0.0,
                    device="cuda"):
    """The gradient with respect to prediction of weights[0] * total_loss + weights[1] * spatial_loss + weights[2] *
    stable_loss + weights[3] * absRel_loss, without autograd: float32 [B, T, H, W] on the device (the forward's launch and one
    of vdn_depth_loss_backward). What VideoDepthLoss's backward computes, for tools and tests; with trim > 0 what
    TrimmedVideoDepthLoss's does."""
    _check_args(alpha, scales, 0.0, stable_scale, 0.0, "batch-based")
    keep = _check_trim(trim)
    if len(weights) != 4:
        raise ValueError(f"weights are (total, spatial, stable, absRel), got {weights!r}")
    w = [float(x) for x in weights]
    rt, res, ss, p, t, m = _launch(prediction, target, mask, float(alpha), scales, float(stable_scale), device, True, state=True,
                                   keep=keep)
    with torch.cuda.device(rt.device):
        coeff = torch.tensor([w[0] + w[1], float(stable_scale) * w[0] + w[2], w[3]], dtype=torch.float32, device=rt.device)
    return _backward(rt, p, t, m, float(alpha), scales, float(stable_scale), ss, res, coeff, keep)
