"""Normal evaluation on the device: the reference's utils.normal_utils (normal_vector, sobel_ix_iy) and its
loss.loss.VideoNormalLoss, computed by the kernels of csrc/normals.hip on tensors that can stay in HBM, with the criterion's
gradient with respect to the prediction by the kernel of csrc/normals_grad.hip. In scripts/train.py, train_v2.py and
train_v3.py, which build the criterion once and use it in `validate` (under no_grad) and in the training step
(total_loss.backward()), replace

    from loss.loss import VideoNormalLoss
    from utils.normal_utils import normal_vector
by
    from vdn.normals import VideoNormalLoss
    from vdn.normals import normal_vector

Gradients. A prediction that requires a gradient (with gradients enabled) goes through a torch.autograd.Function: the
forward is the same launch and the value has the same bits, the backward is one launch of vdn_normal_loss_backward. It is
once differentiable. The incoming gradient, float32 as the loss is, is widened to float64 exactly and read by the kernel from
device memory. Without a gradient to record, forward is what it was: the same launches and tensors, nothing extra. A target
that requires a gradient raises NotImplementedError: the reference would differentiate it and none of its scripts does.
VideoNormalLoss.forward_from_depth is the same criterion against normal_vector(gt_depth), made per pixel and never stored;
normal_loss_grad returns the gradient without autograd. normal_vector and sobel_ix_iy record no gradient.

One difference from the reference: a dropped pixel is skipped, where the reference multiplies it by the selection's zero. NaN
or inf under a dropped pixel therefore reaches nothing here, and its gradient is +0.0 where the reference's is NaN.

Tensors are taken as float32 (masks as "non-zero = use"); a CUDA tensor of the right type is used in place, anything else is
copied to `device` once, and results stay on the device unless a function says otherwise. The stencil, the normalisation, the
cosine and its gradient are fp64 on the device, where the reference computes in the float32 of its inputs; sums have a fixed
order, so two runs give the same bits."""
from __future__ import annotations

import torch

from . import _abi as abi
from ._device import runtime_for as _runtime_for, stage, wants_grad


def _check_size(H: int, W: int):
    if H < 2 or W < 2:
        raise ValueError(f"H and W must be at least 2 (the reflect pad of the Sobel stencil), got {H} x {W}")


def _check_img(img) -> tuple:
    if not isinstance(img, torch.Tensor) or img.dim() != 5 or img.shape[2] != 1:
        raise ValueError(f"input is expected (B,S,1,Y,X) shape, got {tuple(getattr(img, 'shape', ()))}")
    B, S, _, Y, X = img.shape
    if B * S == 0:
        raise ValueError("empty input")
    _check_size(Y, X)
    return B, S, Y, X


def sobel_ix_iy(img: torch.Tensor, normalize_kernel: bool = True, *, device="cuda"):
    """img (B, S, 1, Y, X) -> Ix, Iy (B, S, 1, Y, X): the 3 x 3 Sobel kernels of utils/normal_utils.py:23-52 (divided by 8
    when normalize_kernel) on the reflect-padded map. ValueError for another rank, or Y < 2 or X < 2, where the
    reference's pad raises."""
    B, S, Y, X = _check_img(img)
    rt = _runtime_for(device, img)
    d = stage(img, rt.device, torch.float32).view(B * S, Y, X)
    with torch.cuda.device(rt.device):
        ix, iy = torch.empty_like(d), torch.empty_like(d)
        rt.sobel_ix_iy(d, ix, iy, normalize_kernel)
    return ix.view(B, S, 1, Y, X), iy.view(B, S, 1, Y, X)


def normal_vector(img: torch.Tensor, normalize_kernel: bool = True, scale_xy: float = 1.0, scale_z: float = 1.0,
                  eps: float = 1e-8, *, device="cuda") -> torch.Tensor:
    """img (B, S, 1, Y, X) -> unit normals (B, S, 3, Y, X) = (-scale_xy Ix, -scale_xy Iy, scale_z) / sqrt(|.|^2 + eps), as
    utils/normal_utils.py:4-20. scale_xy, scale_z and eps are rounded to float32 first, as the reference's float32 tensor
    arithmetic does."""
    B, S, Y, X = _check_img(img)
    rt = _runtime_for(device, img)
    d = stage(img, rt.device, torch.float32).view(B * S, Y, X)
    with torch.cuda.device(rt.device):
        out = torch.empty((B * S, 3, Y, X), dtype=torch.float32, device=rt.device)
        rt.normal_vector(d, out, normalize_kernel, float(scale_xy), float(scale_z), float(eps))
    return out.view(B, S, 3, Y, X)


def _check_loss_shapes(prediction, target, mask, target_is_depth: bool) -> tuple:
    if not isinstance(prediction, torch.Tensor) or prediction.dim() != 5 or prediction.shape[2] != 3:
        raise ValueError(f"prediction must be [B, T, 3, H, W], got {tuple(getattr(prediction, 'shape', ()))}")
    B, T, _, H, W = prediction.shape
    if target_is_depth:
        if tuple(target.shape) not in ((B, T, H, W), (B, T, 1, H, W)):
            raise ValueError(f"gt_depth must be [B, T, H, W] or [B, T, 1, H, W] = {(B, T, H, W)}, got {tuple(target.shape)}")
    elif tuple(target.shape) != (B, T, 3, H, W):
        raise ValueError(f"target shape {tuple(target.shape)} is not the prediction's {(B, T, 3, H, W)}")
    if mask is not None and tuple(mask.shape) != (B, T, H, W):
        raise ValueError(f"mask shape {tuple(mask.shape)} is not {(B, T, H, W)}")
    if B * T == 0:
        raise ValueError("empty input")
    _check_size(H, W)
    return B, T, H, W


def grad_trip_pixels(wide: bool) -> int:
    """The pixels of one frame that one trip of the backward's grid covers (vdn_normal_loss_backward_trip): a larger frame
    sends every lane round its stride loop again. wide: the four-pixel path."""
    return int(abi.lib.vdn_normal_loss_backward_trip(int(wide)))


def _launch(prediction, target, mask, target_is_depth: bool, device):
    """The forward's launch -> (runtime, out float64 [2] = loss, kept count: the runtime's buffer, reused by the next call;
    and the float32 prediction [F, 3, H, W], target [F, 3, H, W] or [F, H, W] and uint8 mask [F, H, W] or None the kernel read)."""
    B, T, H, W = _check_loss_shapes(prediction, target, mask, target_is_depth)
    rt = _runtime_for(device, prediction, target, mask)
    F = B * T
    p = stage(prediction, rt.device, torch.float32).view(F, 3, H, W)
    t = stage(target, rt.device, torch.float32).view((F, H, W) if target_is_depth else (F, 3, H, W))
    m = None if mask is None else stage(mask, rt.device, torch.uint8).view(F, H, W)
    with torch.cuda.device(rt.device):
        out = rt.buf("normal_out", (2,), torch.float64)
        rt.normal_eval(p, t, m, out)
    return rt, out, p, t, m


def _backward(rt, p, t, m, count, coeff) -> torch.Tensor:
    """One launch of vdn_normal_loss_backward -> float32 [F, 3, H, W]. count, coeff: float64 [1] on the device."""
    with torch.cuda.device(rt.device):
        grad = torch.empty_like(p)
        rt.normal_loss_backward(p, t, m, count, coeff, grad)
    return grad


class _NormalLossFn(torch.autograd.Function):
    """normal_loss as a 0-dim float32 tensor, differentiable in `prediction`. mask may be None."""

    @staticmethod
    def forward(ctx, prediction, target, mask, target_is_depth, device):
        rt, out, p, t, m = _launch(prediction, target, mask, target_is_depth, device)
        with torch.cuda.device(rt.device):
            count = out[1:2].clone()   # a tensor of its own: the runtime's buffer is reused by the next call
            v = out[0].to(torch.float32)
        ctx.save_for_backward(p, t, count, *(() if m is None else (m,)))
        ctx.args = (rt, prediction.dtype, prediction.device, tuple(prediction.shape))
        return v

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        p, t, count, *m = ctx.saved_tensors
        rt, dtype, device, shape = ctx.args
        with torch.cuda.device(rt.device):
            coeff = g.to(device=rt.device, dtype=torch.float64).reshape(1)   # float32 widened: exact
        grad = _backward(rt, p, t, m[0] if m else None, count, coeff)
        return grad.view(shape).to(device=device, dtype=dtype), None, None, None, None


class VideoNormalLoss(torch.nn.Module):
    """loss/loss.py:370-409, differentiable in the prediction: one minus the mean cosine between prediction and target over
    the pixels the 3 x 3 erosion of the mask keeps.

    reduction="image-based" raises NotImplementedError: in the reference that branch (reduction_image_based) indexes the
    1-D vector of kept cosines, and the 4-D mask along its batch axis, with the mask's [n, 4] pixel coordinates. It raises
    IndexError as soon as a coordinate reaches the batch size (checked on the CPU with torch 2.x; tools/make_golden_normals.py
    prints it), so there is no behaviour to reproduce. `trim` is accepted and unused, as in the reference."""

    def __init__(self, trim=0.0, reduction="batch-based", *, device="cuda"):
        super().__init__()
        if reduction != "batch-based":
            raise NotImplementedError(f"reduction={reduction!r}: the reference's image-based branch cannot run; "
                                      "only 'batch-based' is defined")
        self.device = device

    def eroded_mask(self, mask: torch.Tensor) -> torch.Tensor:
        """mask [B, T, H, W] -> bool [B, T, H, W]: true where the pixel and all of its 3 x 3 neighbours inside the image are
        non-zero (positions outside the image erode nothing)."""
        if not isinstance(mask, torch.Tensor) or mask.dim() != 4:
            raise ValueError(f"mask must be [B, T, H, W], got {tuple(getattr(mask, 'shape', ()))}")
        B, T, H, W = mask.shape
        if B * T == 0:
            raise ValueError("empty input")
        _check_size(H, W)
        rt = _runtime_for(self.device, mask)
        m = stage(mask, rt.device, torch.uint8).view(B * T, H, W)
        with torch.cuda.device(rt.device):
            out = torch.empty_like(m)
            rt.erode_mask3(m, out)
        return out.view(B, T, H, W).view(torch.bool)

    def _value(self, prediction, target, mask, target_is_depth: bool, name: str):
        if wants_grad(prediction, target, name):
            return {"normal_loss": _NormalLossFn.apply(prediction, target, mask, target_is_depth, self.device)}
        rt, out, _, _, _ = _launch(prediction, target, mask, target_is_depth, self.device)
        with torch.cuda.device(rt.device):
            return {"normal_loss": out[0].to(torch.float32)}   # a copy: the buffer is reused by the next call

    def forward(self, prediction, target, mask):
        """prediction [B, T, 3, H, W], target [B, T, 3, H, W] (unit length or not), mask [B, T, H, W] ->
        {'normal_loss': 0-dim float32 tensor on the device}; 1.0 when the erosion keeps no pixel. No host synchronisation.
        With gradients enabled and a prediction that requires one, the value carries a grad_fn whose backward gives
        prediction.grad in the prediction's dtype and shape."""
        return self._value(prediction, target, mask, False, "target")

    def forward_from_depth(self, prediction, gt_depth, mask):
        """forward(prediction, normal_vector(gt_depth), mask) without the target tensor: gt_depth [B, T, H, W] or
        [B, T, 1, H, W]; the target normal of each kept pixel is made from the depth stencil in fp64 and never stored. The
        same dictionary and the same autograd behaviour; gt_depth is a constant of the differentiation."""
        if not isinstance(gt_depth, torch.Tensor):
            raise ValueError("gt_depth must be a tensor [B, T, H, W] or [B, T, 1, H, W]")
        return self._value(prediction, gt_depth, mask, True, "gt_depth")


def _loss(prediction, target, mask, target_is_depth: bool, per_frame: bool, device):
    B, T, H, W = _check_loss_shapes(prediction, target, mask, target_is_depth)
    rt = _runtime_for(device, prediction, target, mask)
    F = B * T
    p = stage(prediction, rt.device, torch.float32).view(F, 3, H, W)
    t = stage(target, rt.device, torch.float32).view((F, H, W) if target_is_depth else (F, 3, H, W))
    m = None if mask is None else stage(mask, rt.device, torch.uint8).view(F, H, W)
    with torch.cuda.device(rt.device):
        res = rt.buf("normal_res", (2 + 2 * F,), torch.float64)   # out[2] | frame sums [F] | frame counts [F] (int64)
        sums, counts = res[2:2 + F], res[2 + F:].view(torch.int64)
        rt.normal_eval(p, t, m, res[:2], sums if per_frame else None, counts if per_frame else None)
        if not per_frame:
            return float(res[:1].cpu()[0])
        host = res.cpu()
    n = host[2 + F:].view(torch.int64).clone()
    return float(host[0]), (host[2:2 + F] / n.double()).view(B, T), n.view(B, T)


def normal_loss(prediction, target, mask=None, *, per_frame=False, device="cuda"):
    """The value of VideoNormalLoss()(prediction, target, mask) in float64, as a Python float (one synchronising copy):
    prediction and target [B, T, 3, H, W], mask [B, T, H, W] or None (all ones). per_frame as in normal_loss_from_depth."""
    return _loss(prediction, target, mask, False, per_frame, device)


def normal_loss_from_depth(prediction, gt_depth, mask=None, *, per_frame=False, device="cuda"):
    """VideoNormalLoss()(prediction, normal_vector(gt_depth), mask) in one pass, without the target tensor: the target
    normal of each kept pixel is made from the depth stencil in fp64 and never stored.

    prediction [B, T, 3, H, W]; gt_depth [B, T, H, W] or [B, T, 1, H, W]; mask [B, T, H, W] or None (all ones). Returns the
    loss as a Python float (one synchronising copy). With per_frame=True returns (loss, per-frame mean cosine [B, T] float64,
    per-frame kept pixels [B, T] int64), CPU tensors from the same copy; a frame without a kept pixel has mean NaN."""
    return _loss(prediction, gt_depth, mask, True, per_frame, device)


def normal_loss_grad(prediction, target, mask=None, *, from_depth=False, coeff=1.0, device="cuda"):
    """The gradient of coeff * normal_loss with respect to prediction, without autograd: float32 [B, T, 3, H, W] on the device
    (the forward's launch for the kept count, then one of vdn_normal_loss_backward). target is [B, T, 3, H, W], or with
    from_depth a depth map [B, T, H, W] or [B, T, 1, H, W]. coeff is rounded to float32 first, as the gradient that autograd
    hands the float32 loss is, and crosses to the kernel widened to float64. What VideoNormalLoss's backward computes, for
    tools and tests."""
    rt, out, p, t, m = _launch(prediction, target, mask, bool(from_depth), device)
    with torch.cuda.device(rt.device):
        c = torch.tensor([float(coeff)], dtype=torch.float32, device=rt.device).to(torch.float64)
        grad = _backward(rt, p, t, m, out[1:2], c)
    return grad.view(prediction.shape)
