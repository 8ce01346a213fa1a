#!/usr/bin/env python3
"""Throughput of the depth + normal head (vdn.VideoDepthAnythingHeadV2) on one MI355X: B = 1, S = 32 frames, attention on
levels [2, 3], synthetic weights, features resident on the GPU; HIP events around `--iters` forward calls after warm-up.
Prints one JSON line: frames/s and the fraction of the 2.5 PF fp16 peak at 32.8 GFLOP per frame (the torch FLOP count
of the reference head at S = 32)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

GFLOP_PER_FRAME = 32.8
PEAK_TFLOPS = 2500.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    import vdn
    import dn_fixture as DF
    dev = torch.device("cuda:0")
    head = vdn.VideoDepthAnythingHeadV2(sequence_length=a.frames, attention_feature_levels=[2, 3])
    head.load_state_dict(DF.state_dict(head), strict=True)
    head = head.to(dev).eval()
    feats = [torch.from_numpy(f).to(dev) for f in DF.head_inputs(1, a.frames)]
    for _ in range(a.warmup):
        head(feats)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.iters):
        head(feats)
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / a.iters
    fps = a.frames / (ms / 1e3)
    print(json.dumps({"workload": "dn_head_b1_s32_l23", "ms_per_clip": round(ms, 3), "frames_per_s": round(fps, 1),
                      "peak_fraction": round(fps * GFLOP_PER_FRAME / (PEAK_TFLOPS * 1e3), 5),
                      "precision": head.precision or os.environ.get("VDN_PRECISION", "f16x3")}))


if __name__ == "__main__":
    main()
