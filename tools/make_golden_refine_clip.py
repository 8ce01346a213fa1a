#!/usr/bin/env python3
"""Generate the fixtures of the depth refiners' clip driver (`refine_video_depth`): RC5_vits, RC3_vits and RC2_vits in
tests/golden/, on top of tools/make_golden.py's shims and tools/make_golden_refiners.reference_model.

The reference's `infer_video_depth` of these models (models/video_depth_model_v5.py:194-283, the same text in v2 .. v4) cannot
run: it feeds an RGB window [1,32,3,H,W] into a `forward` that unpacks four dimensions. Its halves can: the
IMPORTED `forward` of the version, and the imported `compute_scale_and_shift` / `get_interpolate_frames` of utils/util.py. Only
the loop that joins them (v5:215-283) is restated here, on depth windows: pad the clip with copies of its last frame, 32-frame
windows every 22 frames, the previous window's inputs at KEYFRAMES into slots 0..9, `forward`, the resize to the frame size
(the identity: `forward` returns the input's size), then scale/shift on the two alignment frames, clamp at 0 and the 8-frame
cross-fade. The result is held to <= 1e-5 of tests/refine_clip_ref.restate, which the tests run without the reference.

With the plain synthetic draw the stitcher's clamp never acts, so for v3 and v5 the head's bias (final_res2.0.bias /
shift_head.0.bias) is shifted by minus the 20 % quantile of window 1's normalised output and stored in the fixture as
"sd/<key>", as R2_vits stores its final_res scalars. Conditions, on the reference's output alone: exact zeros among the frames
>= 32 make up 0.5 % .. 50 % (v3, v5); each ReLU of final_res clips 5 % .. 95 % (v2, as R2_vits).

Usage: python tools/make_golden_refine_clip.py [--only NAME ...]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import GOLD, ROOT, SEED, install_shims, load_synth  # noqa: E402
from make_golden_refiners import reference_model  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))

N_FRAMES = 50   # three windows of 32 / 28 / 6 distinct frames: the last one is mostly padding


def reference_clip(model, clip: torch.Tensor):
    """The loop v5:215-283 with the depth clip [N,H,W] in place of the transformed RGB frames -> (stitched f32 [N,H,W], the
    per-window outputs). The constants are the model file's own, the alignment and the cross-fade the imported functions."""
    from utils.util import compute_scale_and_shift, get_interpolate_frames
    k = type(model).infer_video_depth.__globals__
    T, OVERLAP, KEYFRAMES, INTERP = k["INFER_LEN"], k["OVERLAP"], k["KEYFRAMES"], k["INTERP_LEN"]
    n, fh, fw = clip.shape
    step = T - OVERLAP
    frames = [clip[i] for i in range(n)]
    frames += [frames[-1].clone()] * ((step - n % step) % step + (T - step))
    depth_list, windows, prev = [], [], None
    for start in range(0, n, step):
        cur = torch.stack(frames[start:start + T])[None]
        if prev is not None:
            cur[:, :OVERLAP] = prev[:, KEYFRAMES]
        with torch.no_grad():
            d = model.forward(cur)
        d = F.interpolate(d.to(cur.dtype).flatten(0, 1).unsqueeze(1), size=(fh, fw), mode="bilinear", align_corners=True)
        windows.append(d[:, 0].numpy())
        depth_list += [d[i][0].numpy() for i in range(d.shape[0])]
        prev = cur
    out, ref = [], []
    align = OVERLAP - INTERP
    kfs = KEYFRAMES[:align]
    for base in range(0, len(depth_list), T):
        if not out:
            out += depth_list[:T]
            ref = [depth_list[base + kf] for kf in kfs]
            continue
        scale, shift = compute_scale_and_shift(np.concatenate([depth_list[base + i] for i in range(len(kfs))]), np.concatenate(ref),
                                               np.concatenate(np.ones_like(ref) == 1))

        def fit(d):
            d = d * scale + shift
            d[d < 0] = 0
            return d

        out[-INTERP:] = get_interpolate_frames(out[-INTERP:], [fit(d) for d in depth_list[base + align:base + OVERLAP]])
        out += [fit(depth_list[base + i]) for i in range(OVERLAP, T)]
        ref = ref[:1] + [fit(depth_list[base + kf]) for kf in kfs[1:]]
    return np.stack(out[:n], axis=0).astype(np.float32), np.stack(windows)


def gen(version: int, H: int, W: int, name: str):
    import refine_clip_ref as RC
    import refiner_ref as R
    from vdn import synth, util
    enc = "vits"
    _, _, bias_key = RC.FIXTURES[name]
    model = reference_model(version, enc)
    sd, _ = load_synth(model)
    extra = {}
    if version == 2:   # the plain draw makes final_res a constant (tests/refiner_ref.R2_FINAL_RES, refine_clip_ref.RC2_FINAL_RES)
        sd = R.with_final_res(sd, RC.RC2_FINAL_RES)
        extra = {f"sd/{k}": np.asarray(v, np.float32) for k, v in RC.RC2_FINAL_RES.items()}
    clip = torch.from_numpy(synth.depth_clip(SEED, N_FRAMES, H, W))
    table = util.window_table(N_FRAMES)
    assert [len(set(w)) for w in table] == [32, 28, 6], [len(set(w)) for w in table]
    if bias_key is not None:   # move window 1's 20 % quantile to zero: the aligned later windows then reach below 0
        model.load_state_dict(sd, strict=True)
        with torch.no_grad():
            w1 = model.forward(clip[torch.tensor(table[1])][None])
        unit = float(model.max_depth) if version >= 4 else 1.0   # v2 / v3 return the normalised map
        q = float(torch.quantile((w1 / unit).flatten(), 0.2))
        sd = dict(sd)
        sd[bias_key] = sd[bias_key] - q
        extra[f"sd/{bias_key}"] = sd[bias_key].numpy().astype(np.float32)
        print(f"[{name}] {bias_key} shifted by {-q:+.5f} to {float(sd[bias_key].reshape(())):+.5f}")
    model.load_state_dict(sd, strict=True)
    t0 = time.time()
    ref, ref_windows = reference_clip(model, clip)
    traces = []
    mine, _ = RC.restate(sd, clip.numpy(), enc, version, traces)
    e = float(np.linalg.norm(mine.astype(np.float64) - ref) / np.linalg.norm(ref.astype(np.float64)))
    worst = float(np.abs(mine - ref).max() / np.abs(ref).max())
    print(f"[{name}] v{version} N={N_FRAMES} {H}x{W} {time.time() - t0:.1f}s out mean {ref.mean():.4f} max {ref.max():.4f} | "
          f"restatement rel err {e:.2e} worst pixel {worst:.2e}")
    assert e <= 1e-5, e   # rel-L2, the measure of tools/make_golden_refiners.py; the worst pixel is printed
    if version == 2:   # on every window, and on out[:RAW]: the frames of window 0 in front of the cross-fade, all the host test has raw
        z0 = float((ref[:RC.RAW] == 0).mean())
        print(f"[{name}] frames < {RC.RAW}: outputs exactly zero {z0:.3f}")
        assert np.array_equal(ref[:RC.RAW], ref_windows[0][:RC.RAW]) and RC.RELU_SHARE[0] <= z0 <= RC.RELU_SHARE[1], z0
        for w, t in enumerate(traces):
            clipped, zero = float((t["pre_relu1"] < 0).float().mean()), float((ref_windows[w] == 0).mean())
            print(f"[{name}] window {w}: clipped by the first ReLU {clipped:.3f}, outputs exactly zero {zero:.3f}")
            assert RC.RELU_SHARE[0] <= clipped <= RC.RELU_SHARE[1] and RC.RELU_SHARE[0] <= zero <= RC.RELU_SHARE[1], (clipped, zero)
    else:
        z = RC.zero_share(ref)
        print(f"[{name}] exact zeros among the frames >= 32: {z:.4f}")
        assert RC.ZERO_SHARE[0] <= z <= RC.ZERO_SHARE[1], z
    path = os.path.join(GOLD, f"{name}.npz")
    np.savez_compressed(path, meta=np.array([version, N_FRAMES, H, W, SEED]), out=ref, **extra)
    assert os.path.getsize(path) < 1_000_000, os.path.getsize(path)
    print(f"[{name}] {os.path.getsize(path)} bytes")


JOBS = {
    "RC5_vits": lambda: gen(5, 36, 52, "RC5_vits"),    # the network runs at 224 x 224: the tail resamples
    "RC3_vits": lambda: gen(3, 42, 56, "RC3_vits"),    # 3 x 4 patches, the network at the clip's size
    "RC2_vits": lambda: gen(2, 42, 56, "RC2_vits"),    # the final_res mix
}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    install_shims()
    torch.set_num_threads(8)
    for k, fn in JOBS.items():
        if a.only and k not in a.only:
            continue
        t0 = time.time()
        fn()
        print(f"== {k} done in {time.time() - t0:.1f}s")
