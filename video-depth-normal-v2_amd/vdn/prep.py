"""Batch preparation on the device: what the reference's scripts/train*.py and scripts/evaluate*.py do to a batch between
the loader and the model, computed by the kernels of csrc/prep.hip on tensors that stay in HBM. In those scripts, delete the
definitions of preprocess_rgb_sequences, preprocess_rgb_viz_sequences and preprocess_depth_sequences and write

    from vdn.prep import preprocess_rgb_sequences, preprocess_rgb_viz_sequences, preprocess_depth_sequences, inverse_depth

with `gt_depths = inverse_depth(gt_depths)` for `gt_depths = 1. / torch.clamp(gt_depths, min=1e-8)`.

The results have the bits of the torch composition (include/vdn.h, vdn_prep_rgb and vdn_prep_depth; the sign of a zero
excepted). The reference's `.view(B, S, C, INPUT_SIZE, INPUT_SIZE)` forces square frames of one size; any H, W is taken here.
Masks are "non-zero = keep": bool, uint8 and float tensors all do, and None keeps every pixel. A dropped pixel never enters
the minimum and maximum of the normalisation.

Tensors are taken as float32; a CUDA tensor of the right type is used in place (made contiguous if it is a view), anything
else is copied to `device` once, and results stay on the device. Nothing here synchronises with the host. A wrong rank or a
shape mismatch raises ValueError before the device is touched; a CPU device raises VdnError."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _abi as abi
from ._device import runtime_for, stage

_EPS = float(np.float32(1e-8))


def trip_elements(wide: bool) -> int:
    """The elements of one item (one frame, for rgb) that one trip of the grid covers (vdn_prep_trip): a longer item sends every
    lane round its stride loop again. wide: the four-floats-per-lane path."""
    return int(abi.lib.vdn_prep_trip(int(wide)))


def _shape(t, name: str, rank: int, channels: Optional[int] = None) -> tuple:
    if not isinstance(t, torch.Tensor) or t.dim() != rank or (channels is not None and t.shape[2] != channels):
        want = "[B, S, H, W]" if rank == 4 else f"[B, S, {channels}, H, W]"
        raise ValueError(f"{name} must be {want}, got {tuple(getattr(t, 'shape', ()))}")
    if t.numel() == 0:
        raise ValueError(f"{name} is empty")
    return tuple(t.shape)


def _rgb(rgb_batch, normalize: bool, device) -> torch.Tensor:
    B, S, _, H, W = _shape(rgb_batch, "rgb_batch", 5, 3)
    rt = runtime_for(device, rgb_batch)
    x = stage(rgb_batch, rt.device, torch.float32).view(B * S, 3, H, W)
    with torch.cuda.device(rt.device):
        out = torch.empty_like(x)
        rt.prep_rgb(x, out, normalize)
    return out.view(B, S, 3, H, W)


def preprocess_rgb_sequences(rgb_batch, *, device="cuda") -> torch.Tensor:
    """rgb_batch [B, S, 3, H, W] -> float32 of the same shape: clamp to [0, 1], then (x - mean) / std with timm's
    IMAGENET_DEFAULT_MEAN / IMAGENET_DEFAULT_STD, as torchvision's Normalize computes it (sub_, then div_)."""
    return _rgb(rgb_batch, True, device)


def preprocess_rgb_viz_sequences(rgb_batch, *, device="cuda") -> torch.Tensor:
    """rgb_batch [B, S, 3, H, W] -> float32 of the same shape: the clamp to [0, 1] alone."""
    return _rgb(rgb_batch, False, device)


def _depth(x, masks, shape4: tuple, reciprocal: bool, clamp0: bool, normalize: bool, device, minmax: bool = False):
    """x and masks (or None) hold B * S * H * W elements in [B, S, H, W] order -> float32 [B, S, H, W] (and lo / hi [B, 2])."""
    B = shape4[0]
    rt = runtime_for(device, x, masks)
    d = stage(x, rt.device, torch.float32).view(B, -1)
    m = None if masks is None or not normalize else stage(masks, rt.device, torch.uint8).view(B, -1)
    with torch.cuda.device(rt.device):
        out = torch.empty_like(d)
        mm = torch.empty((B, 2), dtype=torch.float32, device=rt.device) if minmax else None
        rt.prep_depth(d, m, out, reciprocal, clamp0, normalize, mm)
    return (out.view(shape4), mm) if minmax else out.view(shape4)


def _check_masks(masks, shape: tuple, name: str = "masks"):
    if masks is not None and (not isinstance(masks, torch.Tensor) or tuple(masks.shape) != tuple(shape)):
        raise ValueError(f"{name} shape {tuple(getattr(masks, 'shape', ()))} is not {tuple(shape)}")


def preprocess_depth_sequences(depth_batch, masks, norm=True, *, device="cuda") -> torch.Tensor:
    """depth_batch [B, S, 1, H, W], masks [B, S, 1, H, W] or None -> float32 [B, S, H, W]: clamp at 0 and, with `norm`,
    batch_wise_min_max_norm under the masks. Without `norm` the masks are not read."""
    B, S, _, H, W = _shape(depth_batch, "depth_batch", 5, 1)
    _check_masks(masks, (B, S, 1, H, W))
    return _depth(depth_batch, masks, (B, S, H, W), False, True, bool(norm), device)


def batch_wise_min_max_norm(x, masks, *, device="cuda", return_minmax: bool = False):
    """x [B, S, H, W], masks [B, S, H, W] or None -> float32 [B, S, H, W]: per item (x - lo) / max(hi - lo, 1e-8) clamped to
    [0, 1], lo and hi the item's minimum and maximum over its kept pixels; an item with no kept pixel gives zeros.
    return_minmax: also the float32 [B, 2] of (lo, hi) on the device (+inf, -inf for an item with no kept pixel)."""
    shape = _shape(x, "x", 4)
    _check_masks(masks, shape)
    return _depth(x, masks, shape, False, False, True, device, return_minmax)


def inverse_depth(gt_depths, min=1e-8, *, device="cuda") -> torch.Tensor:
    """1. / torch.clamp(gt_depths, min=1e-8) in float32, any shape -> the same shape. The bound is the kernel's constant:
    another `min` raises ValueError."""
    if not isinstance(gt_depths, torch.Tensor) or gt_depths.numel() == 0:
        raise ValueError(f"gt_depths must be a non-empty tensor, got {tuple(getattr(gt_depths, 'shape', ()))}")
    if float(np.float32(min)) != _EPS:
        raise ValueError(f"min must be 1e-8 (the scripts' bound), got {min!r}")
    return _depth(gt_depths, None, (1, gt_depths.numel()), True, False, False, device).view(gt_depths.shape)


def preprocess_inverse_depth_sequences(gt_depths, masks, norm=True, *, device="cuda") -> torch.Tensor:
    """preprocess_depth_sequences(inverse_depth(gt_depths), masks, norm) in one pass, as create_sample_visualizations composes
    them: gt_depths [B, S, 1, H, W], masks [B, S, 1, H, W] or None -> float32 [B, S, H, W]. The inverse depth is recomputed
    per pixel in both launches and never stored."""
    B, S, _, H, W = _shape(gt_depths, "gt_depths", 5, 1)
    _check_masks(masks, (B, S, 1, H, W))
    return _depth(gt_depths, masks, (B, S, H, W), True, True, bool(norm), device)
