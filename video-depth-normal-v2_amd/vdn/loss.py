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

The SSIM term. The reference's VideoDepthLoss takes `ssim_loss_scale` as its fifth argument (the scripts' --ssim_loss_scale):
with it above 0 the dictionary gains 'ssim_loss' = DepthShallowSSIMLoss of the aligned prediction and total_loss gains
ssim_loss_scale times it. Here DepthShallowSSIMLoss is the term alone and SSIMVideoDepthLoss the criterion with all of its
terms (and `trim`), both differentiable in the prediction: csrc/ssim.hip, include/vdn.h (vdn_ssim_loss and its backward).
pytorch_msssim's MS_SSIM is restated from its published algorithm, not linked: with the weights [1, 0, 0, 0, 0] the reference
uses, it is 1 - mean over frames of relu(mean of the contrast-structure map of an 11-tap Gaussian window, SSIM_WINDOW), and
the four pooled levels are factors of exactly 1. Parity with the library's own file cannot be pinned without it (DESIGN.md
5.18). The library asserts min(H, W) > 160 for its four downsamplings; the classes raise ValueError there, the functions
ssim_loss and ssim_loss_grad take any frame of 11 x 11 or more. VideoDepthLoss and TrimmedVideoDepthLoss keep refusing
ssim_loss_scale > 0: the criterion with the term is SSIMVideoDepthLoss.

Not computed, each raising NotImplementedError: trim != 0 in VideoDepthLoss (use TrimmedVideoDepthLoss), ssim_loss_scale > 0
in VideoDepthLoss (use SSIMVideoDepthLoss), reduction != "batch-based" (the reference's image-based branch indexes a 1-D
vector with the mask's coordinates, and cannot run), weights of the SSIM term other than [1, 0, 0, 0, 0] (they need the four
pooled levels). scales above 4 (the reference's default) likewise."""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from ._device import runtime_for, stage, wants_grad

OUT_SLOTS = 20   # include/vdn.h: the layout of vdn_depth_loss's out
TRIM_SLOTS = 40  # ... and of vdn_depth_loss_trimmed's: 20 + 5 * term: k | n_less | n_tied | threshold | weight
MAX_SCALES = 4
_SLOT = {"spatial_loss": 0, "stable_loss": 1, "absRel_loss": 2, "d1": 3, "total_loss": 4}
# The eleven taps of the SSIM term's window: the float32 values of exp(-(k - 5)^2 / (2 * 1.5^2)) / sum as torch computes them
# (pytorch_msssim's _fspecial_gauss_1d(11, 1.5)), widened to double. csrc/ssim.hip holds the same literals.
SSIM_WINDOW = tuple(float.fromhex(h) for h in (
    "0x1.0d9570p-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.106560p-2", "0x1.b43c3ep-3",
    "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8", "0x1.0d9570p-10"))
SSIM_MIN_SIDE = 160   # the library asserts min(H, W) > (11 - 1) * 2 ** 4 for its four downsamplings
SSIM_HOLDERS = ("prediction", "target", "dropped", "clamp", "tie")   # who holds an item's maximum (include/vdn.h, item_max)


def trip_pixels(wide: bool) -> int:
    """The pixels of one frame that one trip of a criterion's sweep covers (vdn_depth_loss_trip): a larger frame sends every
    lane round its stride loop again. wide: the four-pixel path. The SSIM term's sweeps share the figure."""
    from . import _abi as abi
    return int(abi.lib.vdn_depth_loss_trip(int(wide)))


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
            raise NotImplementedError("ssim_loss_scale > 0 is not computed here: SSIMVideoDepthLoss is the criterion with the term")
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


# ------------------------------------------------------------------------------------------------ the SSIM term
def ssim_tile() -> Tuple[int, int]:
    """(rows, columns) of the outputs one block of the SSIM kernels takes (vdn_ssim_tile): a frame of tile + 10 is one tile."""
    import ctypes
    from . import _abi as abi
    th, tw = ctypes.c_int(), ctypes.c_int()
    abi.check(abi.lib.vdn_ssim_tile(ctypes.byref(th), ctypes.byref(tw)), "vdn_ssim_tile")
    return th.value, tw.value


def _check_ssim(prediction, target, mask, library_rule: bool) -> tuple:
    B, T, H, W = _check(prediction, target, mask, 4)
    if library_rule and min(H, W) <= SSIM_MIN_SIDE:
        raise ValueError(f"the SSIM term needs min(H, W) > {SSIM_MIN_SIDE} (pytorch_msssim asserts it for its four "
                         f"downsamplings), got {H} x {W}")
    if min(H, W) < len(SSIM_WINDOW):
        raise ValueError(f"the SSIM term needs frames of {len(SSIM_WINDOW)} x {len(SSIM_WINDOW)} or more, got {H} x {W}")
    return B, T, H, W


def _ssim_launch(rt, p, t, m, ss):
    """One launch of vdn_ssim_loss on staged tensors -> its state, float64 on the device in a tensor of its own: out [4] |
    frame_cs [B T] | item_max [B, 4]."""
    B, T = p.shape[:2]
    with torch.cuda.device(rt.device):
        st = torch.empty((4 + B * T + 4 * B,), dtype=torch.float64, device=rt.device)
        rt.ssim_loss(p, t, m, ss, st[:4], st[4:4 + B * T], st[4 + B * T:])
    return st


def _ssim_backward(rt, p, t, m, ss, st, coeff, grad, accumulate: bool):
    F = p.shape[0] * p.shape[1]
    with torch.cuda.device(rt.device):
        rt.ssim_loss_backward(p, t, m, ss, st[:4], st[4:4 + F], st[4 + F:], coeff, grad, accumulate)
    return grad


def _ssim_stage(prediction, target, mask, device, aligned: bool):
    """-> runtime, the staged f32 prediction, target and u8 mask, and the fit f32 [B, 2] when `aligned` (else None)."""
    rt = runtime_for(device, prediction, target, mask)
    p = stage(prediction, rt.device, torch.float32)
    t = stage(target, rt.device, torch.float32)
    m = stage(mask, rt.device, torch.uint8)
    ss = None
    if aligned:
        with torch.cuda.device(rt.device):
            ss = torch.empty((p.shape[0], 2), dtype=torch.float32, device=rt.device)
            rt.depth_loss(p, t, m, None, scale_shift=ss)
    return rt, p, t, m, ss


class _SsimLossFn(torch.autograd.Function):
    """The SSIM term alone as a 0-dim float32 tensor, differentiable in `prediction`."""

    @staticmethod
    def forward(ctx, prediction, target, mask, device):
        rt, p, t, m, _ = _ssim_stage(prediction, target, mask, device, False)
        st = _ssim_launch(rt, p, t, m, None)
        ctx.save_for_backward(p, t, m, st)
        ctx.args = (rt, prediction.dtype, prediction.device)
        with torch.cuda.device(rt.device):
            return st[0].to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        p, t, m, st = ctx.saved_tensors
        rt, dtype, device = ctx.args
        with torch.cuda.device(rt.device):
            coeff = g.to(device=rt.device, dtype=torch.float32).reshape(1)
            grad = torch.empty_like(p)
        _ssim_backward(rt, p, t, m, None, st, coeff, grad, False)
        return grad.to(device=device, dtype=dtype), None, None, None


class DepthShallowSSIMLoss(torch.nn.Module):
    """loss/loss.py:296-323 with the reference's constructor signature: 1 - MS_SSIM(data_range=1, channel=1, weights)(x, y) of
    the prediction and target divided by the item's masked maximum, for the weights [1, 0, 0, 0, 0] the reference's criterion
    uses. reduction other than "batch-based" and any other weights raise NotImplementedError."""

    def __init__(self, reduction="batch-based", weights=[1.0, 0.0, 0.0, 0.0, 0.0], *, device="cuda"):
        super().__init__()
        if reduction != "batch-based":
            raise NotImplementedError(f"reduction={reduction!r}: only 'batch-based' is computed")
        w = [float(x) for x in weights]
        if w != [1.0, 0.0, 0.0, 0.0, 0.0]:
            raise NotImplementedError(f"weights={list(weights)!r}: only [1, 0, 0, 0, 0] is computed; other weights need the four "
                                      "pooled levels of MS_SSIM")
        self.device = device

    def forward(self, prediction, target, mask) -> torch.Tensor:
        """prediction, target, mask [B, S, H, W] -> a 0-dim float32 tensor on the device, no host synchronisation. ValueError for
        min(H, W) <= 160, where the library asserts. With gradients enabled and a prediction that requires one, the value
        carries a grad_fn (once differentiable); a target that requires one raises NotImplementedError."""
        _check_ssim(prediction, target, mask, True)
        if wants_grad(prediction, target):
            return _SsimLossFn.apply(prediction, target, mask, self.device)
        rt, p, t, m, _ = _ssim_stage(prediction, target, mask, self.device, False)
        st = _ssim_launch(rt, p, t, m, None)
        with torch.cuda.device(rt.device):
            return st[0].to(torch.float32)


class _SsimDepthLossFn(torch.autograd.Function):
    """The criterion with the SSIM term as one float32 [6] tensor: the slots of _SLOT (total_loss without the term) and the term
    in slot 5, differentiable in `prediction`."""

    @staticmethod
    def forward(ctx, prediction, target, mask, alpha, scales, stable_scale, device, keep):
        rt, res, ss, p, t, m = _launch(prediction, target, mask, alpha, scales, stable_scale, device, True, state=True, keep=keep)
        st = _ssim_launch(rt, p, t, m, ss)
        with torch.cuda.device(rt.device):
            res = res.clone()
            v = torch.cat((res[:5], st[:1])).to(torch.float32)
        ctx.save_for_backward(p, t, m, ss, res, st)
        ctx.args = (rt, alpha, scales, stable_scale, prediction.dtype, prediction.device, keep)
        return v

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        p, t, m, ss, res, st = ctx.saved_tensors
        rt, alpha, scales, stable_scale, dtype, device, keep = ctx.args
        with torch.cuda.device(rt.device):
            g = g.to(device=rt.device, dtype=torch.float32)
            coeff = torch.stack((g[4] + g[0], g[4] * stable_scale + g[1], g[2]))
            c_ssim = g[5:6].contiguous()
        grad = _backward(rt, p, t, m, alpha, scales, stable_scale, ss, res, coeff, keep)
        _ssim_backward(rt, p, t, m, ss, st, c_ssim, grad, True)   # added to the other terms' gradient in fp64, rounded once
        return grad.to(device=device, dtype=dtype), None, None, None, None, None, None, None


class SSIMVideoDepthLoss(VideoDepthLoss):
    """The reference's VideoDepthLoss(alpha, scales, trim, stable_scale, ssim_loss_scale) with all of its terms, in its
    positional order: the fit, the criterion's launch (trimmed when trim > 0), then with ssim_loss_scale > 0 the SSIM term on
    the aligned prediction (loss/loss.py:358-360). The dictionary then holds 'ssim_loss' after 'stable_loss', and total_loss
    is the float32 sum the reference forms: spatial_loss + stable_loss * stable_scale + ssim_loss * ssim_loss_scale.
    Differentiable in the prediction: the criterion's backward launch, then the term's, which adds its gradient to the first's.
    ValueError for min(H, W) <= 160 when the term is on. With ssim_loss_scale == 0 this is TrimmedVideoDepthLoss bit for bit,
    and launches nothing else."""

    def __init__(self, alpha=0.5, scales=4, trim=0.0, stable_scale=10, ssim_loss_scale=0.0, *, device="cuda"):
        keep = _check_trim(trim)
        if isinstance(ssim_loss_scale, bool) or not isinstance(ssim_loss_scale, (int, float)) or ssim_loss_scale != ssim_loss_scale:
            raise ValueError(f"ssim_loss_scale={ssim_loss_scale!r}: a number (the term is computed when it is above 0)")
        super().__init__(alpha, scales, 0.0, stable_scale, device=device)
        self.trim = trim
        self._keep = keep
        self.ssim_loss_scale = ssim_loss_scale

    @property
    def keys(self) -> Tuple[str, ...]:
        """The keys of forward's dictionary, in the reference's order."""
        return (("spatial_loss",) + (("stable_loss",) if self.stable_scale > 0 else ())
                + (("ssim_loss",) if self.ssim_loss_scale > 0 else ()) + ("absRel_loss", "d1", "total_loss"))

    def forward(self, prediction, target, mask) -> Dict[str, torch.Tensor]:
        if not self.ssim_loss_scale > 0:      # zero or negative: the reference adds no term either
            return super().forward(prediction, target, mask)
        _check_ssim(prediction, target, mask, True)
        args = (self._alpha, self.scales, float(self.stable_scale), self.device, self._keep)
        if wants_grad(prediction, target):
            v = _SsimDepthLossFn.apply(prediction, target, mask, *args)
        else:
            rt, res, ss, p, t, m = _launch(prediction, target, mask, *args[:4], False, state=True, keep=self._keep)
            st = _ssim_launch(rt, p, t, m, ss)
            with torch.cuda.device(rt.device):
                v = torch.cat((res[:5], st[:1])).to(torch.float32)
        total = v[0]
        if self.stable_scale > 0:
            total = total + v[1] * self.stable_scale
        total = total + v[5] * self.ssim_loss_scale
        return {k: (total if k == "total_loss" else v[5] if k == "ssim_loss" else v[_SLOT[k]]) for k in self.keys}


def ssim_loss(prediction, target, mask, *, aligned=False, device="cuda") -> dict:
    """The fp64 values of one launch of the SSIM term, read with one synchronising copy. prediction, target, mask [B, T, H, W]
    with H, W >= 11 (the library's rule min(H, W) > 160 is the classes'). aligned: on scale * prediction + shift of the masked
    fit, as SSIMVideoDepthLoss takes it. Returns Python floats 'ssim_loss' and 'mean_cs', the integer 'gated' (frames whose cs
    relu sets to 0) and CPU tensors 'cs' float64 [B, T], 'max_val' float64 [B] (a float32 value), 'holder' int64 [B] (an index
    into SSIM_HOLDERS), 'weight' float64 [B] and 'index' int64 [B] (include/vdn.h, item_max)."""
    B, T, _, _ = _check_ssim(prediction, target, mask, False)
    rt, p, t, m, ss = _ssim_stage(prediction, target, mask, device, aligned)
    host = _ssim_launch(rt, p, t, m, ss).cpu()
    im = host[4 + B * T:].view(B, 4)
    return dict(ssim_loss=float(host[0]), mean_cs=float(host[1]), gated=int(host[2]), cs=host[4:4 + B * T].view(B, T).clone(),
                max_val=im[:, 0].clone(), holder=im[:, 1].to(torch.int64), weight=im[:, 2].clone(), index=im[:, 3].to(torch.int64))


def ssim_loss_grad(prediction, target, mask, *, aligned=False, coeff=1.0, prior=None, device="cuda") -> torch.Tensor:
    """The gradient of coeff * ssim_loss with respect to prediction without autograd: float32 [B, T, H, W] on the device (the
    forward's launch and one of vdn_ssim_loss_backward); what DepthShallowSSIMLoss's backward computes, and with `aligned` the
    term's part of SSIMVideoDepthLoss's. prior: a float32 gradient the result is added to in fp64 and rounded once (the
    accumulating write; `prior` itself is left as it is)."""
    _check_ssim(prediction, target, mask, False)
    rt, p, t, m, ss = _ssim_stage(prediction, target, mask, device, aligned)
    st = _ssim_launch(rt, p, t, m, ss)
    with torch.cuda.device(rt.device):
        c = torch.tensor([float(coeff)], dtype=torch.float32, device=rt.device)
        grad = torch.empty_like(p) if prior is None else stage(prior, rt.device, torch.float32).clone().view(p.shape)
    return _ssim_backward(rt, p, t, m, ss, st, c, grad, prior is not None)


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
