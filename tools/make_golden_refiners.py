#!/usr/bin/env python3
"""Generate the depth-refiner fixtures R2_vits, R3_vits (models/video_depth_model_v2 / _v3) and R5r_vits (v5 with
pe='rope') in tests/golden/ by running the IMPORTED reference on the CPU, on top of tools/make_golden.py's shims.
Each is checked against its CPU restatement (tests/refiner_ref.py, oracle/ref_cpu.py; <= 1e-5) before it is written.

Usage: python tools/make_golden_refiners.py [--only NAME ...]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import GOLD, REF, ROOT, SEED, install_shims, load_synth, relerr  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))


def reference_model(version: int, enc: str, **flags):
    """models/__init__.py pulls in encoder wrappers this path never uses: load the one module file directly."""
    from oracle import ref_cpu as O
    spec = importlib.util.spec_from_file_location(f"ref_video_depth_model_v{version}",
                                                  os.path.join(REF, "models", f"video_depth_model_v{version}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    return mod.VideoDepthAnything(**dict(O.MODEL_CONFIGS[enc], **flags)).eval()


def write_schema(model, shapes, name: str):
    with open(os.path.join(GOLD, f"schema_{name}.json"), "w") as f:
        json.dump({"params": [[k, list(s)] for k, s in shapes],
                   "buffers": [[k, list(v.shape)] for k, v in model.named_buffers()]}, f)


def share(mask) -> float:
    return float(mask.float().mean())


def gen(version: int, enc: str, S: int, H: int, W: int, name: str, tag: str, **flags):
    import refiner_ref as R
    from oracle import ref_cpu as O
    from vdn import synth
    model = reference_model(version, enc, **flags)
    sd, shapes = load_synth(model)
    write_schema(model, shapes, f"{tag}_{enc}")
    extra = {}
    if version == 2:   # the plain draw makes final_res a constant (tests/refiner_ref.R2_FINAL_RES)
        sd = R.with_final_res(sd)
        model.load_state_dict(sd, strict=True)
        extra = {f"sd/{k}": np.asarray(v, np.float32) for k, v in R.R2_FINAL_RES.items()}
    x = torch.from_numpy(synth.depth_clip(SEED, S, H, W))[None]
    t0 = time.time()
    with torch.no_grad():
        ref = model(x)
    tr = {}
    with torch.no_grad():
        if version in (2, 3):
            mine = R.refiner23_forward(sd, x, enc, version=version, trace=tr)
        else:
            mine = O.depth_refiner_forward(sd, x, enc, version=version, trace=tr)
    e = relerr(mine, ref)
    print(f"[{name}] v{version} S={S} {H}x{W} ref {time.time() - t0:.1f}s out mean {ref.mean():.4f} std {ref.std():.4f} "
          f"min {ref.min():.4f} net_depth mean {tr['net_depth'].mean():.4f} | restatement rel err {e:.2e}")
    assert e <= 1e-5, e
    if version == 2:   # conditions on the reference alone: both ReLUs of final_res are partly active
        clipped, zero = share(tr["pre_relu1"] < 0), share(ref == 0)
        print(f"[{name}] clipped by the first ReLU {clipped:.3f}, outputs exactly zero {zero:.3f}")
        assert 0.05 <= clipped <= 0.95 and 0.05 <= zero <= 0.95, (clipped, zero)
    out = {"meta": np.array([version, S, H, W, SEED]), "out": ref[0].numpy(), "net_depth": tr["net_depth"][0].numpy(), **extra}
    if "median" in tr:
        out.update(median=tr["median"].numpy(), scale=tr["scale"].numpy())
    path = os.path.join(GOLD, f"{name}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1_000_000, os.path.getsize(path)


JOBS = {
    # 9 x 12 patches, n = 21 168 pixels per frame (not a multiple of 1024): the shape of R4_vits
    "R2_vits": lambda: gen(2, "vits", 3, 126, 168, "R2_vits", "R2"),
    "R3_vits": lambda: gen(3, "vits", 3, 126, 168, "R3_vits", "R3"),
    # pe = 'rope' through a refiner: the shape of R5_vits
    "R5r_vits": lambda: gen(5, "vits", 4, 90, 121, "R5r_vits", "R5r", pe="rope"),
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
