"""The clip-level encoder tap cache of the windowed drivers, written once for `VideoDepthAnything.infer_video_depth` (RGB
frames) and the depth refiners' `refine_video_depth` (depth frames): both cut a clip into 32-slot windows by
`util.window_table`, 10 of whose slots repeat earlier input frames, and both run a per-frame encoder in front of a temporal head.

The reference runs the encoder on all 32 slots of every window (video_depth.py:96-103), but 10 of the 32 are copies of earlier
input frames (Appendix B of SURVEY.md: slot 0 = frame 0, slot 1 = the previous window's keyframe, slots 2..9 = the previous
window's last 8), and the encoder is per-frame: here every DISTINCT frame goes through the encoder once (its 4 final-normed taps
stay in HBM, 22 MB per 518x518 ViT-L frame), and a window's head reads its 32 slots from that cache — 256 instead of 384 encoder
passes for a 256-frame clip, same numbers. Every encoder batch holds INFER_LEN frames, the clip's ragged tail filled up with
copies of its last frame (never more encoder passes than the reference's 32 per window): vdn_gemm picks its kernel by the row
count, so a frame encoded in a batch of 2 is 1e-5 away from the same frame in `forward`'s batch of 32, and a clip's depth would
depend on how its length splits."""
from __future__ import annotations

import os
from typing import Callable, List, Sequence

import torch

from . import util


def tap_bytes_per_frame(rt, embed_dim: int, H: int, W: int) -> int:
    """Bytes of encoder taps one frame keeps in the cache: 4 taps x P tokens x C channels x 16-bit planes."""
    return 4 * (H // 14) * (W // 14) * embed_dim * 2 * (2 if rt.split else 1)


def cache_budget_bytes() -> float:
    """Bytes a clip-level cache may take: VDN_TAP_CACHE_GB, default 96. A driver whose cache does not fit runs its own
    `forward` window by window."""
    return float(os.environ.get("VDN_TAP_CACHE_GB", "96")) * 2 ** 30


def tap_cache_plan(rt, embed_dim: int, H: int, W: int, table, windows: Sequence[int]):
    """-> (the distinct frames the windows `windows` of `table` show, sorted; does their cache fit the budget VDN_TAP_CACHE_GB,
    default 96). A driver whose cache does not fit encodes window by window (its own `forward`)."""
    need = sorted({f for w in windows for f in table[w]})
    batches = -(-len(need) // util.INFER_LEN)
    return need, batches * util.INFER_LEN * tap_bytes_per_frame(rt, embed_dim, H, W) <= cache_budget_bytes()


def cached_window_depths(rt, enc, head, embed_dim: int, net_batch: Callable[[List[int]], torch.Tensor], H: int, W: int, table,
                         windows: Sequence[int], need: List[int]):
    """Yields the temporal head's rectified depth [32, H, W] of each of the windows `windows` of `table`, a view of the head's
    output buffer. `net_batch(frames)` returns the network input [32, 3, H, W] (contiguous, on the device) of the 32 clip frames
    listed; it is called once per encoder batch of the distinct frames `need` (tap_cache_plan)."""
    T = util.INFER_LEN
    batches = -(-len(need) // T)
    ph, pw = H // 14, W // 14
    P, C = ph * pw, embed_dim
    slot = {f: i for i, f in enumerate(need)}        # cache row block of frame f
    cache = [rt.hbuf(f"clip_tap{j}", (batches * T * P, C)) for j in range(4)]
    for c0 in range(0, len(need), T):   # encoder batches of 32 distinct frames
        fr = need[c0:c0 + T]
        fr = fr + fr[-1:] * (T - len(fr))
        enc.run(net_batch(fr), tap_out=[t.narrow0(c0 * P, T * P) for t in cache])
    for w in windows:
        rows = [slot[f] for f in table[w]]
        if rows == list(range(rows[0], rows[0] + T)):          # one contiguous run: read the cache in place
            taps = [t.narrow0(rows[0] * P, T * P) for t in cache]
        else:                                                   # copy the (typically 3) runs of slots into a window buffer
            taps = [rt.hbuf(f"win_tap{j}", (T * P, C)) for j in range(4)]
            i = 0
            while i < T:
                k = i
                while k + 1 < T and rows[k + 1] == rows[k] + 1:
                    k += 1
                for src, dst in zip(cache, taps):
                    dst.hi[i * P:(k + 1) * P].copy_(src.hi[rows[i] * P:(rows[k] + 1) * P])
                    if dst.lo is not None:
                        dst.lo[i * P:(k + 1) * P].copy_(src.lo[rows[i] * P:(rows[k] + 1) * P])
                i = k + 1
        yield head.run(taps, T, ph, pw, T=T, relu=True).reshape(T, H, W)
