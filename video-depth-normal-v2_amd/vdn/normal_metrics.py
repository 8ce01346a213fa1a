"""Angular error of predicted normals on the device (csrc/normal_metrics.hip): the numbers the field reports for normals,
which the reference does not compute. Its one measure is VideoNormalLoss (vdn.normals), one minus the mean cosine; this
module scores the same pixels in degrees.

The angle of a kept pixel with prediction a and target b is atan2(|a x b|, a . b) * 180 / pi in fp64 from the float32
components (not acos of a cosine, which loses half the digits near 0 and 180 degrees). NaN or inf in any component gives NaN;
otherwise a zero vector on either side gives 90, the angle whose cosine is the 0 that F.cosine_similarity's clamped norms
give the loss. With from_depth the target is a depth map and b = (-Ix, -Iy, 1) of the Sobel / 8 stencil on the reflect-padded
map, made per pixel and never stored (the direction of vdn.normals.normal_vector(depth), without its rounding to float32).

Kept pixels are those of VideoNormalLoss: the mask (None = all ones) after the 3 x 3 erosion, or the mask itself with
erode=False. A dropped pixel is skipped: NaN under it reaches nothing.

Per set of pixels (the batch, each item, each frame) the nine numbers `normal_metric_names`: the kept pixels n, the mean, the
median (numpy.median of the angles rounded to float32: exact, the mean of the two middle values for even n) and the root mean
square of the angle, and the shares of kept pixels under 5, 7.5, 11.25, 22.5 and 30 degrees (strict). A set without a kept
pixel has n = 0 and NaN elsewhere; a set with a NaN angle has NaN in every column but n, and the other sets are untouched.
Sums are fp64 in a fixed order: two runs give the same bits.

These are scores, not criteria: nothing records a gradient, and a prediction or target that requires one is detached.
Tensors are staged as in vdn.normals (float32, masks "non-zero = keep", a CUDA tensor of the right type used in place)."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from ._device import runtime_for as _runtime_for, stage
from .normals import _check_loss_shapes

normal_metric_names = ["n", "mean", "median", "rmse", "a5", "a7_5", "a11_25", "a22_5", "a30"]


def _staged(prediction, target, mask, from_depth: bool, device):
    """The shape checks (every ValueError before the device is touched), then the runtime and the float32 prediction
    [F, 3, H, W], target [F, 3, H, W] or [F, H, W] and uint8 mask [F, H, W] or None the kernels read."""
    if not isinstance(target, (torch.Tensor, np.ndarray)):
        raise ValueError("gt_depth must be a tensor [B, T, H, W] or [B, T, 1, H, W]" if from_depth
                         else "target must be a tensor [B, T, 3, H, W]")
    if mask is not None and not isinstance(mask, (torch.Tensor, np.ndarray)):
        raise ValueError("mask must be a tensor [B, T, H, W] or None")
    B, T, H, W = _check_loss_shapes(prediction, target, mask, from_depth)
    rt = _runtime_for(device, prediction, target, mask)
    F = B * T
    detach = lambda x: x.detach() if isinstance(x, torch.Tensor) else x
    p = stage(detach(prediction), rt.device, torch.float32).view(F, 3, H, W)
    t = stage(detach(target), rt.device, torch.float32).view((F, H, W) if from_depth else (F, 3, H, W))
    m = None if mask is None else stage(mask, rt.device, torch.uint8).view(F, H, W)
    return rt, (B, T, H, W), p, t, m


def angular_error_map(prediction, target, mask=None, *, from_depth=False, erode=True, device="cuda") -> torch.Tensor:
    """prediction [B, T, 3, H, W]; target [B, T, 3, H, W], or with from_depth a depth map [B, T, H, W] or [B, T, 1, H, W]; mask
    [B, T, H, W] or None -> float32 [B, T, H, W] on the device: the angle in degrees rounded to float32 once, NaN at a dropped
    pixel."""
    rt, (B, T, H, W), p, t, m = _staged(prediction, target, mask, bool(from_depth), device)
    with torch.cuda.device(rt.device):
        out = torch.empty((B * T, H, W), dtype=torch.float32, device=rt.device)
        rt.normal_angle_map(p, t, m, bool(erode), out)
    return out.view(B, T, H, W)


def _rows(prediction, target, mask, from_depth, erode, device):
    rt, (B, T, H, W), p, t, m = _staged(prediction, target, mask, bool(from_depth), device)
    with torch.cuda.device(rt.device):
        rows = torch.empty((1 + B + B * T, 9), dtype=torch.float64, device=rt.device)
        rt.normal_angle_stats(p, t, m, bool(erode), B, T, rows)
    return rows, B, T


def angular_error(prediction, target, mask=None, *, from_depth=False, erode=True, device="cuda") -> Dict[str, torch.Tensor]:
    """The nine `normal_metric_names` of the batch, of each item and of each frame -> {"batch": [9], "items": [B, 9], "frames":
    [B, T, 9]}, float64 tensors on the device (views of one tensor of the call's own). No host synchronisation. Arguments as
    angular_error_map."""
    rows, B, T = _rows(prediction, target, mask, from_depth, erode, device)
    return {"batch": rows[0], "items": rows[1:1 + B], "frames": rows[1 + B:].view(B, T, 9)}


def angular_error_values(prediction, target, mask=None, *, from_depth=False, erode=True, device="cuda") -> Dict[str, list]:
    """angular_error as Python lists (one synchronising copy), for tools: {"batch": [9 floats], "items": B lists, "frames": B
    lists of T lists}."""
    rows, B, T = _rows(prediction, target, mask, from_depth, erode, device)
    host = rows.cpu()
    return {"batch": host[0].tolist(), "items": host[1:1 + B].tolist(), "frames": host[1 + B:].view(B, T, 9).tolist()}
