"""The metric-depth branch's criterion and scores on the device: the reference's metric_depth/util/loss.py (SiLogLoss) and
metric_depth/util/metric.py (eval_depth), computed by the kernels of csrc/metric.hip on tensors that stay in HBM. In
metric_depth/train.py replace

    from util.loss import SiLogLoss
    from util.metric import eval_depth
by
    from vdn.metric import SiLogLoss, eval_depth

and see vdn.steps.metric_validate_step for the body of its validation loop, which calls eval_depth_batch: the resize of the
prediction to the ground truth's size, the mask (valid_mask == 1) & (depth >= min_depth) & (depth <= max_depth), the two
boolean-indexed copies and the nine .item() calls of the script are one launch there, and nothing crosses to the host.

Kept pixels. A mask keeps a pixel where it EQUALS 1, the script's `valid_mask == 1`: bool and uint8 masks on the device are
used in place (a uint8 value of 2 drops), anything else becomes `mask == 1` once. This is not the "non-zero = keep" rule of
vdn.loss. A dropped pixel is skipped, and the reference indexes with the mask, so a NaN under a dropped pixel reaches nothing
on either side.

Arithmetic (include/vdn.h, vdn_metric_eval): the resampled prediction, thresh and the quotients d1, d2, d3 are the reference's
float32 operations; the other six metrics, the loss and its gradient are fp64 from the float32 inputs on, where the reference
computes them in the inputs' float32. Sums have a fixed order, so two runs give the same bits.

SiLogLoss is differentiable in the prediction through a torch.autograd.Function: the forward is the same launch, the backward
one launch of vdn_silog_loss_backward, once differentiable. A target that requires a gradient raises NotImplementedError: the
reference would differentiate it and its script does not. Edge cases as the reference's autograd gives them: no kept pixel,
loss NaN and a zero gradient; pred == target at every kept pixel, loss 0 and a NaN gradient at the kept pixels; a negative
radicand, NaN in both.

Tensors are taken as float32; a CUDA tensor of the right type is used in place (made contiguous if it is a view), anything
else is copied to `device` once, and results stay on the device unless a function says otherwise. A wrong shape raises
ValueError before the device is touched; a CPU device raises VdnError."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from ._device import runtime_for, stage, wants_grad

KEYS = ("d1", "d2", "d3", "abs_rel", "sq_rel", "rmse", "rmse_log", "log10", "silog")   # eval_depth's, in its order
ROW = 1 + len(KEYS)   # a row of eval_depth_batch: n, then the nine


def trip_elements(wide: bool) -> int:
    """The elements of one item that one trip of the grid covers (vdn_metric_trip); a lane issues the loads of four trips
    together, and a longer item sends it round its loop again. wide: the four-floats-per-lane path."""
    from . import _abi as abi
    return int(abi.lib.vdn_metric_trip(int(wide)))


def _tensor(t, name: str) -> tuple:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    return tuple(t.shape)


def _same(pred, target, mask=None) -> tuple:
    shape = _tensor(pred, "pred")
    for name, t in (("target", target),) + ((("valid_mask", mask),) if mask is not None else ()):
        if _tensor(t, name) != shape:
            raise ValueError(f"{name} shape {tuple(t.shape)} is not the prediction's {shape}")
    if pred.numel() == 0:
        raise ValueError("empty input")
    return shape


def _bounds(min_depth, max_depth) -> Optional[Tuple[float, float]]:
    if min_depth is None and max_depth is None:
        return None
    if min_depth is None or max_depth is None:
        raise ValueError("min_depth and max_depth come together")
    lo, hi = float(min_depth), float(max_depth)
    if lo != lo or hi != hi:
        raise ValueError(f"min_depth={min_depth!r}, max_depth={max_depth!r}: a bound is NaN")
    return lo, hi


def _mask_u8(mask: torch.Tensor, device: torch.device) -> torch.Tensor:
    """uint8 whose bytes equal 1 exactly where `mask == 1`: bool and uint8 tensors on the device in place."""
    if mask.dtype not in (torch.bool, torch.uint8):
        mask = mask == 1
    return stage(mask, device, torch.uint8)


def eval_depth_batch(pred, depth, valid_mask, *, min_depth, max_depth, device="cuda") -> torch.Tensor:
    """pred [B, h, w], depth [B, H, W], valid_mask [B, H, W] -> float64 [B, 10] on the device: per item the kept pixels n and
    d1 d2 d3 abs_rel sq_rel rmse rmse_log log10 silog of eval_depth(pred[keep], depth[keep]) with keep = (valid_mask == 1) &
    (depth >= min_depth) & (depth <= max_depth). (h, w) != (H, W): pred is sampled at the ground truth's pixels as
    F.interpolate(pred[:, None], (H, W), mode='bilinear', align_corners=True) places it. An item without a kept pixel gets nine
    NaN. One launch, no host synchronisation."""
    if len(_tensor(pred, "pred")) != 3 or len(_tensor(depth, "depth")) != 3 or pred.shape[0] != depth.shape[0]:
        raise ValueError(f"pred must be [B, h, w] and depth [B, H, W], got {tuple(pred.shape)} and {tuple(depth.shape)}")
    if _tensor(valid_mask, "valid_mask") != tuple(depth.shape):
        raise ValueError(f"valid_mask shape {tuple(valid_mask.shape)} is not the depth's {tuple(depth.shape)}")
    if pred.numel() == 0 or depth.numel() == 0:
        raise ValueError("empty input")
    bounds = _bounds(min_depth, max_depth)
    if bounds is None:
        raise ValueError("min_depth and max_depth are required")
    rt = runtime_for(device, pred, depth, valid_mask)
    p = stage(pred, rt.device, torch.float32)
    d = stage(depth, rt.device, torch.float32)
    m = _mask_u8(valid_mask, rt.device)
    with torch.cuda.device(rt.device):
        out = torch.empty((d.shape[0], ROW), dtype=torch.float64, device=rt.device)
        rt.metric_eval(p, d, m, out, bounds)
    return out


def eval_depth(pred, target, *, device="cuda") -> Dict[str, float]:
    """metric_depth/util/metric.py:eval_depth: pred and target of one shape (the script passes the 1-D pred[valid_mask],
    depth[valid_mask]), every element kept -> {'d1', 'd2', 'd3', 'abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'log10', 'silog'} as
    Python floats, read with one synchronising copy."""
    _same(pred, target)
    rt = runtime_for(device, pred, target)
    p = stage(pred, rt.device, torch.float32).view(1, 1, -1)
    t = stage(target, rt.device, torch.float32).view(1, 1, -1)
    with torch.cuda.device(rt.device):
        out = torch.empty((1, ROW), dtype=torch.float64, device=rt.device)
        rt.metric_eval(p, t, None, out)
    return dict(zip(KEYS, out[0, 1:].cpu().tolist()))


def _forward(pred, target, mask, lambd, bounds, device):
    """-> (runtime, state float64 [4] = loss | n | sum dl | sum dl^2 in a tensor of its own, and the float32 prediction, target
    and uint8 mask the kernels read)."""
    _same(pred, target, mask)
    rt = runtime_for(device, pred, target, mask)
    p = stage(pred, rt.device, torch.float32)
    t = stage(target, rt.device, torch.float32)
    m = _mask_u8(mask, rt.device)
    with torch.cuda.device(rt.device):
        state = torch.empty(4, dtype=torch.float64, device=rt.device)
        rt.silog_loss(p, t, m, state, lambd, bounds)
    return rt, state, p, t, m


def _backward(rt, p, t, m, state, coeff, lambd, bounds) -> torch.Tensor:
    with torch.cuda.device(rt.device):
        grad = torch.empty_like(p)
        rt.silog_loss_backward(p, t, m, state, coeff, grad, lambd, bounds)
    return grad


class _SiLogFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, mask, lambd, bounds, device):
        rt, state, p, t, m = _forward(pred, target, mask, lambd, bounds, device)
        ctx.save_for_backward(p, t, m, state)
        ctx.args = (rt, lambd, bounds, pred.dtype, pred.device)
        with torch.cuda.device(rt.device):
            return state[0].to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        p, t, m, state = ctx.saved_tensors
        rt, lambd, bounds, dtype, device = ctx.args
        with torch.cuda.device(rt.device):
            coeff = g.to(device=rt.device, dtype=torch.float32).reshape(1).contiguous()
        grad = _backward(rt, p, t, m, state, coeff, lambd, bounds)
        return grad.to(device=device, dtype=dtype), None, None, None, None, None


def _lambd(lambd) -> float:
    if isinstance(lambd, bool) or not isinstance(lambd, (int, float)) or lambd != lambd:
        raise ValueError(f"lambd={lambd!r}: a number")
    return float(lambd)


class SiLogLoss(torch.nn.Module):
    """metric_depth/util/loss.py:SiLogLoss with the reference's constructor and attribute, differentiable in the prediction."""

    def __init__(self, lambd=0.5, *, device="cuda"):
        super().__init__()
        _lambd(lambd)
        self.lambd = lambd
        self.device = device

    def _run(self, pred, target, mask, bounds) -> torch.Tensor:
        lambd = _lambd(self.lambd)   # the attribute is public, as in the reference
        if wants_grad(pred, target):
            return _SiLogFn.apply(pred, target, mask, lambd, bounds, self.device)
        rt, state, *_ = _forward(pred, target, mask, lambd, bounds, self.device)
        with torch.cuda.device(rt.device):
            return state[0].to(torch.float32)

    def forward(self, pred, target, valid_mask) -> torch.Tensor:
        """pred, target, valid_mask of one shape -> the 0-dim float32 loss on the device, sqrt(mean(dl^2) - lambd mean(dl)^2)
        over the kept pixels with dl = log(target) - log(pred); no host synchronisation. With gradients enabled and a prediction
        that requires one, the value carries a grad_fn whose backward gives pred.grad in the prediction's dtype and shape."""
        return self._run(pred, target, valid_mask, None)

    def forward_from_valid(self, pred, depth, valid_mask, min_depth, max_depth) -> torch.Tensor:
        """criterion(pred, depth, (valid_mask == 1) & (depth >= min_depth) & (depth <= max_depth)), the training step of
        metric_depth/train.py:133, with the mask composed per pixel in the same launch and never stored."""
        bounds = _bounds(min_depth, max_depth)
        if bounds is None:
            raise ValueError("min_depth and max_depth are required")
        return self._run(pred, depth, valid_mask, bounds)


def silog_loss(pred, target, valid_mask, lambd=0.5, *, min_depth=None, max_depth=None, device="cuda") -> Dict[str, float]:
    """The fp64 values of one launch, read with one synchronising copy: {'loss', 'n', 'sum', 'sum_sq'} (the loss, the kept
    pixels, and the sums of dl and dl^2 over them)."""
    rt, state, *_ = _forward(pred, target, valid_mask, _lambd(lambd), _bounds(min_depth, max_depth), device)
    loss, n, s1, s2 = state.cpu().tolist()
    return {"loss": loss, "n": int(n), "sum": s1, "sum_sq": s2}


def silog_loss_grad(pred, target, valid_mask, lambd=0.5, *, weight=1.0, min_depth=None, max_depth=None, device="cuda") -> torch.Tensor:
    """weight * d loss / d pred without autograd: float32 of pred's shape on the device (the forward's launch and one of
    vdn_silog_loss_backward). What SiLogLoss's backward computes, for tools and tests."""
    lambd, bounds = _lambd(lambd), _bounds(min_depth, max_depth)
    rt, state, p, t, m = _forward(pred, target, valid_mask, lambd, bounds, device)
    with torch.cuda.device(rt.device):
        coeff = torch.tensor([float(weight)], dtype=torch.float32, device=rt.device)
    return _backward(rt, p, t, m, state, coeff, lambd, bounds).view(pred.shape)
