"""The colourised depth the reference's front ends write to disk, made on the device (csrc/vis.hip): what run.py:59-71,
run_video.py:75-89 and metric_depth/run.py:67-78 do per frame on the host (min/max of the frame, matplotlib palette, BGR,
optionally [raw | 50 white columns | depth]) and what save_video of utils/dc_utils.py:72-86 does per clip (one min/max, the
inferno palette, RGB). The result is bit for bit the reference's uint8 array; only that array crosses to the host.

Three cases the reference leaves to an undefined float -> uint8 cast are defined here (include/vdn.h, vdn_colorize): a
constant map (max == min) gives palette index 0 everywhere, a depth outside a caller-supplied [min, max] clamps to index 0 /
255, and a NaN depth gives index 0.

matplotlib is not needed: the palettes are literals (vdn/_palettes.py, written by tools/make_vis_palettes.py).

colorize_normals is the picture of a normal map, which the reference does not have: each unit vector's x, y, z as the red,
green and blue byte (csrc/normal_metrics.hip)."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from ._device import runtime as _runtime, runtime_for as _runtime_for, stage
from ._palettes import PALETTES
from .runtime import Runtime

_LUTS: Dict[tuple, torch.Tensor] = {}


def _check(palette: str, order: str, scope: str, grayscale: bool, gray_channels: int):
    if palette not in PALETTES:
        raise ValueError(f"palette must be one of {sorted(PALETTES)}, got {palette!r}")
    if order not in ("bgr", "rgb"):
        raise ValueError(f"order must be 'bgr' or 'rgb', got {order!r}")
    if scope not in ("frame", "clip"):
        raise ValueError(f"scope must be 'frame' or 'clip', got {scope!r}")
    if gray_channels not in (1, 3):
        raise ValueError(f"gray_channels must be 1 or 3, got {gray_channels!r}")


def lut(palette: str, order: str, grayscale: bool, gray_channels: int, device: torch.device) -> torch.Tensor:
    """u8 [256, ch] on `device`: the palette in the channel order asked for, or the grey ramp i -> (i,) * gray_channels."""
    key = ("gray", gray_channels, device) if grayscale else (palette, order, device)
    t = _LUTS.get(key)
    if t is None:
        if grayscale:
            t = torch.arange(256, dtype=torch.uint8)[:, None].repeat(1, gray_channels)
        else:
            t = torch.tensor(PALETTES[palette], dtype=torch.uint8).reshape(256, 3)
            if order == "bgr":
                t = t.flip(1)
        t = _LUTS[key] = t.contiguous().to(device)
    return t


def _minmax(rt: Runtime, depth: torch.Tensor, scope: str) -> torch.Tensor:
    groups = depth.shape[0] if scope == "frame" else 1
    out = torch.empty((groups, 2), dtype=torch.float32, device=depth.device)
    rt.minmax(depth, groups, out)
    return out


def _colorize(rt: Runtime, depth: torch.Tensor, palette: str, order: str, scope: str, grayscale: bool, gray_channels: int,
              raw: Optional[torch.Tensor], margin: int, minmax: Optional[torch.Tensor]) -> torch.Tensor:
    N, H, W = depth.shape
    table = lut(palette, order, grayscale, gray_channels, depth.device)
    ch = table.shape[1]
    if minmax is None:
        minmax = _minmax(rt, depth, scope)
    else:
        minmax = minmax.to(device=depth.device, dtype=torch.float32).reshape(-1, 2).contiguous()
        if minmax.shape[0] not in (1, N):
            raise ValueError(f"minmax must be [2] or [{N}, 2], got {tuple(minmax.shape)}")
    if raw is None:
        out = torch.empty((N, H, W, ch), dtype=torch.uint8, device=depth.device)
    else:
        if ch != 3:
            raise ValueError("a raw frame beside the depth needs three channels (gray_channels=3)")
        if margin < 0:
            raise ValueError(f"margin must be >= 0, got {margin}")
        if raw.dtype != torch.uint8 or tuple(raw.shape[-3:]) != (H, W, 3) or raw.numel() != N * H * W * 3:
            raise ValueError(f"raw must be uint8 [{N}, {H}, {W}, 3], got {raw.dtype} {tuple(raw.shape)}")
        raw = raw.to(depth.device).reshape(N, H, W, 3).contiguous()
        out = torch.empty((N, H, 2 * W + margin, 3), dtype=torch.uint8, device=depth.device)
    rt.colorize(depth, minmax, table, out, raw, margin)
    return out


def _depth3(depth) -> torch.Tensor:
    if not isinstance(depth, torch.Tensor):
        raise TypeError(f"expected a torch tensor, got {type(depth).__name__}")
    if depth.dim() not in (2, 3) or depth.numel() == 0:
        raise ValueError(f"depth must be a non-empty [N, H, W] or [H, W], got {tuple(depth.shape)}")
    _runtime(depth.device)   # raises for a CPU tensor
    d = depth if depth.dim() == 3 else depth[None]
    return d.to(torch.float32).contiguous()


def minmax(depth: torch.Tensor, scope: str = "frame") -> torch.Tensor:
    """{min, max} of a CUDA f32 depth [N, H, W] (or [H, W]) as a device tensor: [N, 2] for scope='frame', [1, 2] for 'clip'.
    numpy semantics: a NaN in a frame (clip) makes both of its values NaN."""
    if scope not in ("frame", "clip"):
        raise ValueError(f"scope must be 'frame' or 'clip', got {scope!r}")
    d = _depth3(depth)
    with torch.cuda.device(d.device):
        return _minmax(_runtime(d.device), d, scope)


def colorize(depth: torch.Tensor, palette: str = "Spectral_r", order: str = "bgr", scope: str = "frame", grayscale: bool = False,
             gray_channels: int = 3, raw: Optional[torch.Tensor] = None, margin: int = 50,
             minmax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CUDA f32 depth [N, H, W] or [H, W] -> CUDA u8 [N, H, W, ch] (or [H, W, ch]); with raw u8 [N, H, W, 3] the width is
    2W + margin: raw | margin white pixels | depth (cv2.hconcat of run.py:70-71).

    palette  'Spectral_r' (run.py, run_video.py), 'Spectral' (metric_depth/run.py) or 'inferno' (save_video); order is the
             channel order of the result. grayscale=True ignores both: ch = gray_channels (3: np.repeat of run.py:63;
             1: depth_norm of dc_utils.py:80).
    scope    'frame': each frame's own min/max (the per-frame scripts); 'clip': one for all frames (save_video).
    minmax   a [2] or [N, 2] tensor to use instead; depths outside it clamp.
    Any depth map serves: the drivers', the refiners', the depth + normal model's."""
    _check(palette, order, scope, grayscale, gray_channels)
    d = _depth3(depth)
    with torch.cuda.device(d.device):
        out = _colorize(_runtime(d.device), d, palette, order, scope, grayscale, gray_channels, raw, margin, minmax)
    return out if depth.dim() == 3 else out[0]


def colorize_normals(normals: torch.Tensor, *, from_depth: bool = False, order: str = "rgb", device="cuda") -> torch.Tensor:
    """normals [N, 3, H, W] or [B, T, 3, H, W] of any length -> uint8 [N, H, W, 3] or [B, T, H, W, 3] on the device: each
    component of the unit vector as the byte floor(((a_c / |a|) * 0.5 + 0.5) * 255 + 0.5), in fp64; x, y, z are red, green and
    blue in that order, or reversed for order='bgr'. A zero-length or non-finite vector gives 128, 128, 128 (grey).

    from_depth=True takes a depth clip [N, H, W], [B, T, H, W] or [B, T, 1, H, W] instead and paints the normal (-Ix, -Iy, 1) of
    the Sobel / 8 stencil on the reflect-padded map, made per pixel and never stored: the picture of
    vdn.normals.normal_vector(depth) without that tensor or its rounding to float32 (H, W >= 2). A tensor that is not on a GPU
    is copied to `device` once."""
    if order not in ("bgr", "rgb"):
        raise ValueError(f"order must be 'bgr' or 'rgb', got {order!r}")
    if not isinstance(normals, torch.Tensor):
        raise ValueError(f"expected a torch tensor, got {type(normals).__name__}")
    shape = tuple(normals.shape)
    if from_depth:
        if len(shape) == 5 and shape[2] == 1:
            shape = shape[:2] + shape[3:]
        if len(shape) not in (3, 4):
            raise ValueError(f"depth must be [N, H, W], [B, T, H, W] or [B, T, 1, H, W], got {tuple(normals.shape)}")
        if shape[-2] < 2 or shape[-1] < 2:
            raise ValueError(f"H and W must be at least 2 (the reflect pad of the Sobel stencil), got {shape[-2]} x {shape[-1]}")
        lead = shape[:-2]
    else:
        if len(shape) not in (4, 5) or shape[-3] != 3:
            raise ValueError(f"normals must be [N, 3, H, W] or [B, T, 3, H, W], got {shape}")
        lead = shape[:-3]
    H, W = shape[-2:]
    N = 1
    for n in lead:
        N *= n
    if N * H * W == 0:
        raise ValueError("empty input")
    rt = _runtime_for(device, normals)
    x = stage(normals.detach(), rt.device, torch.float32).view((N, H, W) if from_depth else (N, 3, H, W))
    with torch.cuda.device(rt.device):
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=rt.device)
        rt.normal_colorize(x, out, order == "bgr")
    return out.view(*lead, H, W, 3)
