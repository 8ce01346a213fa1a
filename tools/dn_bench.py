#!/usr/bin/env python3
"""Throughput of the depth + normal model's parts on one MI355X, B = 1, S = `--frames` frames, attention on levels [2, 3],
synthetic weights, inputs resident on the GPU; HIP events around `--iters` forward calls after warm-up. One JSON line.

  --trunk none (default)  the head alone (vdn.VideoDepthAnythingHeadV2) on resident features: frames/s and the fraction of
                          the 2.5 PF fp16 peak at 32.8 GFLOP per frame (the torch FLOP count of the reference head at S = 32)
  --trunk standin         vdn.VideoDepthEstimationModel on the injected stand-in trunks (vdn.synth.dn_trunk, torch ops)
  --trunk native          the same model on two vdn.HieraImageEncoder trunks, and one such trunk alone on the same frames"""
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


def timed(fn, warmup, iters):
    """ms per call: HIP events around `iters` calls after `warmup`."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--trunk", choices=("none", "standin", "native"), default="none")
    ap.add_argument("--encoder", default="hiera_base_224")
    a = ap.parse_args()
    import vdn
    import dn_fixture as DF
    dev = torch.device("cuda:0")
    if a.trunk == "none":
        head = vdn.VideoDepthAnythingHeadV2(sequence_length=a.frames, attention_feature_levels=[2, 3])
        head.load_state_dict(DF.state_dict(head), strict=True)
        head = head.to(dev).eval()
        feats = [torch.from_numpy(f).to(dev) for f in DF.head_inputs(1, a.frames)]
        ms = timed(lambda: head(feats), a.warmup, a.iters)
        fps = a.frames / (ms / 1e3)
        print(json.dumps({"workload": "dn_head_b1_s32_l23", "ms_per_clip": round(ms, 3), "frames_per_s": round(fps, 1),
                          "peak_fraction": round(fps * GFLOP_PER_FRAME / (PEAK_TFLOPS * 1e3), 5),
                          "precision": head.precision or os.environ.get("VDN_PRECISION", "f16x3")}))
        return
    from vdn import synth
    if a.trunk == "native":
        m = vdn.VideoDepthEstimationModel.with_native_trunks(a.frames, encoder=a.encoder, attention_feature_levels=[2, 3])
    else:
        m = vdn.VideoDepthEstimationModel(a.frames, attention_feature_levels=[2, 3], trunk=synth.dn_trunk(), img_trunk=synth.dn_trunk())
    sd = synth.fast_state_dict([(k, tuple(p.shape)) for k, p in m.named_parameters()], DF.SEED)   # timing only: torch's generator
    for k, b in m.named_buffers():
        v = synth.synth_buffer(DF.SEED, k, tuple(b.shape))
        sd[k] = torch.as_tensor(v) if v is not None else b.detach().clone()
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    depth, img = (torch.from_numpy(t).to(dev) for t in DF.wrapper_inputs(1, a.frames, 224, 224))
    ms = timed(lambda: m(depth, img), a.warmup, a.iters)
    out = {"workload": f"dn_model_b1_s{a.frames}_{a.trunk}", "ms_per_clip": round(ms, 3), "frames_per_s": round(a.frames / (ms / 1e3), 1),
           "precision": m.precision or os.environ.get("VDN_PRECISION", "f16x3")}
    if a.trunk == "native":
        x = img.reshape(a.frames, 3, 224, 224).contiguous()
        tms = timed(lambda: m.img_encoder(x), a.warmup, a.iters)
        out.update(encoder=a.encoder, trunk_ms=round(tms, 3), trunk_frames_per_s=round(a.frames / (tms / 1e3), 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
