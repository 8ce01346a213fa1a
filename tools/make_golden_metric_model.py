#!/usr/bin/env python3
"""Generate tests/golden/M*.npz and schema_M*.json: the metric-depth model (vdn.metric_depth) against the IMPORTED reference.

Runs only in the build container (the GPU box has no reference checkout). The reference keeps its metric DepthAnythingV2 class
commented out (metric_depth/depth_anything_v2/dpt.py:152-222) but ships both halves live, so this tool imports
    metric_depth/depth_anything_v2/dinov2.py:DINOv2      and      metric_depth/depth_anything_v2/dpt.py:DPTHead
under the three shims of tools/make_golden.py and composes, here, the three statements the commented class and every caller
spell out (dpt.py:178-185; metric_depth/train.py:88,131,165-166, run.py:38,60, depth_to_pointcloud.py:66,93):

    features = pretrained.get_intermediate_layers(x, idx[encoder], return_class_token=True)
    depth    = depth_head(features, patch_h, patch_w) * max_depth
    return depth.squeeze(1)

No reference source is copied: the fixtures hold numbers and key lists only.

Weights are the project's synthetic ones (load_synth), with one change. Plain synthetic weights give logits of std ~0.4, where
a sigmoid is almost a straight line and a ReLU or a clamp in its place would differ by little. So the final 1x1 convolution
(depth_head.scratch.output_conv2.2) has its weight multiplied by GAIN and its bias set so that the median logit is 0; the gain
starts at 4 and doubles until the map meets SATURATION below. That layer's weights go into the fixture and the test overlays
them on common.synth_sd's.

Usage: python tools/make_golden_metric_model.py [--only NAME ...]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G   # noqa: E402  (install_shims, load_synth, samples, stats, make_inputs; puts the package on sys.path)

LAST = "depth_head.scratch.output_conv2.2"
TAPS = {"vits": [2, 5, 8, 11], "vitb": [2, 5, 8, 11], "vitl": [4, 11, 17, 23], "vitg": [9, 19, 29, 39]}   # dpt.py:164-169
# at least this share of the depth map below 0.05 max_depth, above 0.95 max_depth, and inside 0.2 .. 0.8 max_depth
SATURATION = (0.01, 0.01, 0.20)


def saturation(depth, max_depth):
    """(share below 0.05, share above 0.95, share in 0.2 .. 0.8) of depth / max_depth; tests/test_metric_model_host.py re-checks it."""
    s = np.asarray(depth, np.float64) / max_depth
    return float((s < 0.05).mean()), float((s > 0.95).mean()), float(((s > 0.2) & (s < 0.8)).mean())


def meets(sat):
    return all(v >= need for v, need in zip(sat, SATURATION))


class Composed(torch.nn.Module):
    """The two live reference modules under the attribute names of the commented class: the state-dict keys of an upstream
    metric checkpoint."""

    def __init__(self, enc, features, out_channels, use_bn=False, use_clstoken=False):
        super().__init__()
        from depth_anything_v2.dinov2 import DINOv2
        from depth_anything_v2.dpt import DPTHead
        self.pretrained = DINOv2(model_name=enc)
        self.depth_head = DPTHead(self.pretrained.embed_dim, features, use_bn, out_channels=out_channels, use_clstoken=use_clstoken)


def gen_M(enc, H, W, B, max_depth, sub, name, schema, flags=None, heavy=False, full_logits=False):
    import vdn
    cfg = vdn.MODEL_CONFIGS[enc]
    torch.manual_seed(0)
    model = Composed(enc, cfg["features"], cfg["out_channels"], **(flags or {})).eval()
    assert "metric_depth" in sys.modules["depth_anything_v2.dpt"].__file__, "the main copy's depth_anything_v2 was imported"
    sd, shapes = G.load_synth(model, heavy=heavy)
    with open(os.path.join(G.GOLD, f"schema_{schema}_{enc}.json"), "w") as f:
        json.dump({"params": [[k, list(s)] for k, s in shapes],
                   "buffers": [[k, list(v.shape)] for k, v in model.named_buffers()]}, f)
    x = G.make_inputs(B, H, W)
    ph, pw = H // 14, W // 14
    last = model.depth_head.scratch.output_conv2[2]
    got = {}
    last.register_forward_hook(lambda m, i, o: got.update(logits=o.detach().clone()))
    sc = model.depth_head.scratch
    sc.refinenet1.register_forward_hook(lambda m, i, o: got.update(path1=o.detach().permute(0, 2, 3, 1).contiguous()))
    sc.output_conv1.register_forward_hook(lambda m, i, o: got.update(oc1=o.detach().permute(0, 2, 3, 1).contiguous()))

    def run():
        with torch.no_grad():   # the three statements
            features = model.pretrained.get_intermediate_layers(x, TAPS[enc], return_class_token=True)
            depth = model.depth_head(features, ph, pw) * max_depth
            return features, depth.squeeze(1)

    t0 = time.time()
    _, _ = run()
    w0, b0 = last.weight.detach().clone(), float(last.bias.detach())
    base = got["logits"].double() - b0   # w0 . features, before any gain
    gain = 4.0
    while True:
        with torch.no_grad():
            last.weight.copy_(w0 * gain)
            last.bias.fill_(float(-gain * base.median()))
        features, depth = run()
        sat = saturation(depth.numpy(), max_depth)
        print(f"[M {name}] gain {gain:g}: below 0.05 {sat[0]:.3%}, above 0.95 {sat[1]:.3%}, in 0.2..0.8 {sat[2]:.3%}")
        if meets(sat):
            break
        gain *= 2.0
        assert gain <= 64.0, "no gain up to 64 meets the saturation condition"
    logits = got["logits"][:, 0]
    assert torch.equal(depth, torch.sigmoid(logits) * max_depth)
    print(f"[M {name}] {enc} {H}x{W} B={B} ref {time.time() - t0:.1f}s logits mean {logits.mean():.3f} std {logits.std():.3f} "
          f"min {logits.min():.2f} max {logits.max():.2f}")
    ls = 1 if full_logits else sub
    out = {"meta": np.array([B, H, W, sub, ls, G.SEED]), "max_depth": np.array(max_depth, np.float64), "gain": np.array(gain),
           "last_weight": last.weight.detach().numpy().copy(), "last_bias": last.bias.detach().numpy().copy(),
           "saturation": np.array(sat),
           "logits": logits[:, ::ls, ::ls].numpy().copy(), "logits_stats": G.stats(logits),
           "depth": depth[:, ::sub, ::sub].numpy().copy(), "depth_stats": G.stats(depth)}
    for i, (pt, ct) in enumerate(features):
        out[f"tap{i}_stats"] = G.stats(pt)
        out[f"tap{i}_samp"] = G.samples(pt)[1]
    for k in ("path1", "oc1"):
        out[f"{k}_stats"] = G.stats(got[k])
        out[f"{k}_samp"] = G.samples(got[k], 1024)[1]
    path = os.path.join(G.GOLD, f"{name}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    print(f"[M {name}] {os.path.getsize(path) / 1024:.0f} KiB")


JOBS = {
    # 19 x 25 patches: not square, tile tails of the fused tail in both directions, two frames
    "M_vits_266x350": lambda: gen_M("vits", 266, 350, 2, 20.0, 2, "M_vits_266x350", "M", full_logits=True),
    # both constructor flags, BatchNorm statistics from synth_buffer, another max_depth
    "Mf_vits_266": lambda: gen_M("vits", 266, 266, 1, 80.0, 1, "Mf_vits_266", "Mf", flags=dict(use_bn=True, use_clstoken=True)),
    # ViT-L at the size where the fused tail follows the low-resolution output_conv1, checkpoint-like weights
    "M_vitl_518_heavy": lambda: gen_M("vitl", 518, 518, 1, 20.0, 4, "M_vitl_518_heavy", "M", heavy=True),
}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    G.install_shims()
    sys.path.insert(0, os.path.join(G.REF, "metric_depth"))   # depth_anything_v2 = the metric copy, in front of the main one
    os.makedirs(G.GOLD, exist_ok=True)
    torch.set_num_threads(8)
    for k, fn in JOBS.items():
        if a.only and k not in a.only:
            continue
        t0 = time.time()
        fn()
        print(f"== {k} done in {time.time() - t0:.1f}s")
