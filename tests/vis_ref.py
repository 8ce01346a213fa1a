"""The reference front ends' depth colourisation in plain numpy: the yardstick of vdn.vis (csrc/vis.hip).

The reference's scripts cannot be imported as functions (they are __main__ bodies, and utils/dc_utils.py imports imageio),
so their call sites are restated here line for line. The palettes come from tests/golden/vis_palettes.npz, written by
tools/make_vis_palettes.py with the reference's own expressions; neither matplotlib nor the reference is imported."""
from __future__ import annotations

import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vis_palettes.npz")


def tables():
    """{'Spectral_r', 'Spectral', 'inferno'} -> uint8 [256, 3], RGB as matplotlib has them."""
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


def run_frame(depth, raw, pred_only, grayscale, table, margin_width=50):
    """run.py:59-73, run_video.py:75-89, metric_depth/run.py:66-81 for one frame. depth f32 [h, w] as infer_image returns
    it, raw u8 [h, w, 3] BGR, table u8 [256, 3] RGB = (cmap(arange(256, uint8))[:, :3] * 255).astype(uint8), i.e. the
    reference's `(cmap(depth)[:, :, :3] * 255)[:, :, ::-1].astype(np.uint8)` with the per-pixel cmap call taken as the
    lookup it is. Returns the array handed to cv2.imwrite / VideoWriter.write."""
    assert depth.dtype == np.float32
    depth = (depth - depth.min()) / (depth.max() - depth.min()) * 255.0
    depth = depth.astype(np.uint8)
    if grayscale:
        depth = np.repeat(depth[..., np.newaxis], 3, axis=-1)
    else:
        depth = table[depth][:, :, ::-1]
    if pred_only:
        return np.ascontiguousarray(depth)
    split_region = np.ones((raw.shape[0], margin_width, 3), dtype=np.uint8) * 255
    return np.concatenate([raw, split_region, depth], axis=1)   # cv2.hconcat


def save_video_frames(depths, grayscale, table):
    """utils/dc_utils.py:72-81 (save_video, is_depths=True): the frames it appends to the writer, stacked. depths f32
    [N, h, w], table u8 [256, 3] = (np.array(cmap.colors) * 255).astype(uint8). [N, h, w, 3] RGB, or [N, h, w] grey."""
    assert depths.dtype == np.float32
    d_min, d_max = depths.min(), depths.max()
    out = []
    for i in range(depths.shape[0]):
        depth = depths[i]
        depth_norm = ((depth - d_min) / (d_max - d_min) * 255).astype(np.uint8)
        out.append(table[depth_norm] if not grayscale else depth_norm)
    return np.stack(out)
