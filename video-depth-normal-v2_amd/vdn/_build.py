"""Build libvdn_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIBDIR, "libvdn_hip.so")
SOURCES = ["gemm_big_f16.hip", "gemm_big_bf16.hip", "gemm_small_f16.hip", "gemm_small_bf16.hip", "gemm_x8.hip", "gemm.hip", "attn.hip",
           "norm.hip", "spatial.hip", "tail.hip", "pack.hip", "stitch.hip", "refine.hip",
           "dn_head.hip", "hiera.hip", "lane_attn.hip", "eval.hip", "vis.hip", "normals.hip", "normals_grad.hip", "normal_metrics.hip", "loss.hip",
           "loss_grad.hip", "ssim.hip", "prep.hip", "metric.hip", "points.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]


def _newer(src_list, target):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in src_list)


def build_library(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(LIBDIR, exist_ok=True)
    hdrs = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hpp", ".inc"))]
    hdrs.append(os.path.join(os.path.dirname(PKG), "include", "vdn.h"))
    objs, jobs = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(LIBDIR, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or _newer([src] + hdrs, obj):
            jobs.append([HIPCC] + FLAGS + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print("[vdn build]", " ".join(cmd), file=sys.stderr, flush=True)
        subprocess.run(cmd, check=True)

    if jobs:
        with ThreadPoolExecutor(max_workers=6) as ex:
            list(ex.map(run, jobs))
    if jobs or force or _newer(objs, LIB):
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv))
