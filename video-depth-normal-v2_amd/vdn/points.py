"""The point cloud of a metric depth map on the device: the last step of metric_depth/depth_to_pointcloud.py (lines 99-104),
one launch of vdn_depth_to_points (csrc/points.hip) on tensors that stay in HBM.

    for the pixel at (row, col) of an h x w map with depth z (float32, widened) and colour rgb (uint8), in float64:
    x = (col - w / 2) / fx,  y = (row - h / 2) / fy,  point = (x z, y z, z),  colour = rgb / 255

The script's `Image.fromarray(pred).resize((width, height), Image.NEAREST)` in front of these (line 96) is the identity:
infer_image(image, height) already returns a (height, width) map, so no resize is made here. Writing the .ply file (open3d) is
the caller's: copy the two tensors to the host and hand them to o3d.utility.Vector3dVector as the script does.

The values are the script's float64 numbers, bit for bit: every one is a subtraction, a division and a product of float64
values, correctly rounded on the device as on the host."""
from __future__ import annotations

from typing import Tuple

import torch

from ._device import runtime_for, stage


def depth_to_points(depth, rgb_u8, fx: float, fy: float, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """depth float32 [h, w] (metres) and rgb_u8 uint8 [h, w, 3] (RGB) -> (points, colors), float64 [h*w, 3] each, on the device:
    points = ((col - w / 2) / fx * z, (row - h / 2) / fy * z, z), colors = rgb / 255.0. A CUDA tensor of the right type is used
    in place, anything else is copied to `device` once. fx, fy: the focal lengths in pixels (the script's default is 470.4)."""
    if not isinstance(depth, torch.Tensor) or depth.dim() != 2 or depth.numel() == 0:
        raise ValueError(f"depth must be [h, w], got {tuple(getattr(depth, 'shape', ()))}")
    h, w = depth.shape
    if not isinstance(rgb_u8, torch.Tensor) or tuple(rgb_u8.shape) != (h, w, 3) or rgb_u8.dtype != torch.uint8:
        raise ValueError(f"rgb_u8 must be uint8 [{h}, {w}, 3], got {getattr(rgb_u8, 'dtype', None)} "
                         f"{tuple(getattr(rgb_u8, 'shape', ()))}")
    fx, fy = float(fx), float(fy)
    if not (fx > 0 or fx < 0) or not (fy > 0 or fy < 0):
        raise ValueError(f"fx={fx!r}, fy={fy!r}: a focal length is zero or NaN")
    rt = runtime_for(device, depth, rgb_u8)
    depth = stage(depth, rt.device, torch.float32)
    rgb_u8 = stage(rgb_u8, rt.device, torch.uint8)
    points = torch.empty((h * w, 3), dtype=torch.float64, device=rt.device)
    colors = torch.empty((h * w, 3), dtype=torch.float64, device=rt.device)
    with torch.cuda.device(rt.device):
        rt.depth_to_points(depth, rgb_u8, fx, fy, points, colors)
    return points, colors
