#!/usr/bin/env python3
"""Measurements behind profiles/metric_model.md (GPU box), three parts, each printed as markdown lines:

  tail    vdn_depth_tail_act(VDN_OUT_SIGMOID) and vdn_depth_tail(relu=1) of this tree at the ViT-L size of tools/tail_bench.py
          (B = 8, 296^2 -> 518^2, C = 128), and with --parent-lib the same vdn_depth_tail of an earlier build (a checkout of the
          parent commit built under .abtest/, tools/ab_prev.sh), called through ctypes on the same buffers. The variants alternate
          inside every repeat; a repeat is the mean of `--launches` back-to-back launches between two device events. The ReLU
          outputs of the two builds are compared bit for bit.
  model   frames/s of vdn.metric_depth's DepthAnythingV2(vitl) at 518 x 518, B = 1 and B = 8, a batch frame by frame (the
          default) and in one pass (set_batch_invariant(False)), with vdn.DepthAnythingV2 (which
          also runs the memory block) beside it for orientation. Synthetic weights (synth.fast_state_dict).
  points  vdn.points.depth_to_points at 518 x 686 against the numpy statements of depth_to_pointcloud.py:99-104 on the host,
          the device-to-host copy of the depth map included on the numpy side.

Usage: python tools/metric_model_bench.py [--parent-lib PATH] [--parts tail model points] [--repeats 5] [--launches 20]"""
import argparse
import ctypes
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
import numpy as np   # noqa: E402
import torch         # noqa: E402


def event_us(fn, launches):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / launches


def spread(v):
    return f"{min(v):.1f} .. {max(v):.1f} (median {sorted(v)[len(v) // 2]:.1f})"


def part_tail(a):
    from vdn import _abi as abi, pack
    from vdn.runtime import Runtime
    rt = Runtime(torch.device("cuda:0"), torch.float16, split=True)
    B, IH, C, OH = 8, 296, 128, 518
    x = torch.randn(B * IH * IH, C, device="cuda")
    w = pack.conv3x3_taps(torch.randn(32, C, 3, 3, device="cuda") / math.sqrt(9 * C), rt.prec)
    b2, w1 = torch.randn(32, device="cuda") * 0.1, torch.randn(32, device="cuda") * 0.3
    d = {k: torch.empty(B, OH, OH, device="cuda") for k in ("relu", "sigmoid", "parent")}
    st = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

    def old_entry(lib, out):
        return lambda: lib.vdn_depth_tail(abi.F16, x.data_ptr(), B, IH, IH, C, w.hi.data_ptr(), w.lo.data_ptr(), w.hi.shape[1],
                                          b2.data_ptr(), w1.data_ptr(), ctypes.c_float(0.2), out.data_ptr(), OH, OH, 1, st())

    # all three through ctypes with the same arguments: the host path per launch is the same
    variants = {"relu": old_entry(abi.lib, d["relu"]),
                "sigmoid": lambda: abi.lib.vdn_depth_tail_act(abi.F16, x.data_ptr(), B, IH, IH, C, w.hi.data_ptr(), w.lo.data_ptr(),
                                                              w.hi.shape[1], b2.data_ptr(), w1.data_ptr(), ctypes.c_float(0.2),
                                                              d["sigmoid"].data_ptr(), OH, OH, abi.OUT_SIGMOID, ctypes.c_float(20.0), st())}
    if a.parent_lib:
        plib = ctypes.CDLL(a.parent_lib)
        plib.vdn_depth_tail.restype = ctypes.c_int
        plib.vdn_depth_tail.argtypes = abi.EXPORTS["vdn_depth_tail"][1]
        variants["parent"] = old_entry(plib, d["parent"])
    for fn in variants.values():   # warm-up: code objects loaded, clocks up
        for _ in range(5):
            assert fn() in (0, None)
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for r in range(a.repeats):
        order = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for k in order:
            us[k].append(event_us(variants[k], a.launches))
    fl = 2.0 * B * OH * OH * 32 * 9 * C
    print(f"### Tail: B = {B}, {IH}^2 -> {OH}^2, C = {C}; {a.repeats} repeats of {a.launches} launches, variants alternating; us per launch\n")
    print("| variant | min .. max (median) us | TF/s algorithmic at the median |")
    print("|---|---|---|")
    names = {"relu": "vdn_depth_tail(relu=1), this tree", "sigmoid": "vdn_depth_tail_act(VDN_OUT_SIGMOID), this tree",
             "parent": "vdn_depth_tail(relu=1), parent commit"}
    for k, v in us.items():
        print(f"| {names[k]} | {spread(v)} | {fl / sorted(v)[len(v) // 2] / 1e6:.0f} |")
    print("\nper repeat: " + "; ".join(f"{k} " + " ".join(f"{t:.1f}" for t in v) for k, v in us.items()))
    if a.parent_lib:
        print(f"\nReLU output of this tree equals the parent build's bit for bit: {torch.equal(d['relu'], d['parent'])}")
    m = lambda k: sorted(us[k])[len(us[k]) // 2]   # noqa: E731
    print(f"\nsigmoid over ReLU at the medians: {m('sigmoid') - m('relu'):+.1f} us ({(m('sigmoid') / m('relu') - 1) * 100:+.2f} %)")


def _load(model, seed=1234):
    from vdn import synth
    sd = model.state_dict()
    sd.update(synth.fast_state_dict([(k, tuple(v.shape)) for k, v in model.named_parameters()], seed))
    model.load_state_dict(sd, strict=True)
    return model.to("cuda").eval()


def part_model(a):
    import vdn
    from vdn.metric_depth.depth_anything_v2.dpt import DepthAnythingV2 as Metric
    models = {"vdn.metric_depth DepthAnythingV2(vitl, max_depth=20): a batch frame by frame (default)":
                  _load(Metric(**vdn.MODEL_CONFIGS["vitl"], max_depth=20.0)),
              "the same after set_batch_invariant(False): the batch in one pass (a frame's bits then follow its batch)":
                  _load(Metric(**vdn.MODEL_CONFIGS["vitl"], max_depth=20.0)).set_batch_invariant(False),
              "vdn.DepthAnythingV2(vitl) (with the memory block; orientation only)": _load(vdn.DepthAnythingV2(**vdn.MODEL_CONFIGS["vitl"]))}
    print(f"### Model: ViT-L, 518 x 518, f16x3, synthetic weights; {a.repeats} repeats of {a.steps} forwards; frames/s\n")
    print("| model | B | ms per forward, min .. max (median) | frames/s at the median |")
    print("|---|---|---|---|")
    for B in (1, 8):
        x = torch.randn(B, 3, 518, 518, device="cuda")
        res = {k: [] for k in models}
        for m in models.values():
            if hasattr(m, "clear_memory"):
                m.clear_memory()
            for _ in range(8):   # warm-up; the relative model's bank fills to its 6 frames
                m.forward(x)
        torch.cuda.synchronize()
        for r in range(a.repeats):
            for k in (list(models) if r % 2 == 0 else list(models)[::-1]):
                res[k].append(event_us(lambda: models[k].forward(x), a.steps) / 1e3)
        for k, v in res.items():
            med = sorted(v)[len(v) // 2]
            print(f"| {k} | {B} | {min(v):.2f} .. {max(v):.2f} ({med:.2f}) | {B * 1e3 / med:.1f} |")


def part_points(a):
    from vdn.points import depth_to_points
    h, w, fx, fy = 518, 686, 470.4, 470.4
    depth = torch.rand(h, w, device="cuda") * 20.0
    rgb = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda")
    rgb_host = rgb.cpu().numpy()
    for _ in range(5):
        depth_to_points(depth, rgb, fx, fy)
    dev = [event_us(lambda: depth_to_points(depth, rgb, fx, fy), a.launches) for _ in range(a.repeats)]

    def host():
        z = depth.cpu().numpy()   # what infer_image returns to the script
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        x = (x - w / 2) / fx
        y = (y - h / 2) / fy
        points = np.stack((np.multiply(x, z), np.multiply(y, z), z), axis=-1).reshape(-1, 3)
        colors = np.array(rgb_host).reshape(-1, 3) / 255.0
        return points, colors

    host()
    hs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        pts, col = host()
        hs.append((time.perf_counter() - t0) * 1e6)
    p, c = depth_to_points(depth, rgb, fx, fy)
    same = np.array_equal(p.cpu().numpy(), pts) and np.array_equal(c.cpu().numpy(), col)
    by = h * w * (4 + 3 + 48 + 48)
    med = sorted(dev)[len(dev) // 2]
    print(f"### Points: {h} x {w}; {a.repeats} repeats; us per call\n")
    print("| path | min .. max (median) us |")
    print("|---|---|")
    print(f"| vdn.points.depth_to_points (two output allocations + one launch, results stay on the device) | {spread(dev)} |")
    print(f"| numpy on the host, depth copied from the device first | {spread(hs)} |")
    print(f"\n{by / 1e6:.1f} MB moved per call: {by / med / 1e6:.2f} TB/s at the median (call time, allocations included). "
          f"Device result equals numpy's bit for bit: {same}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parts", nargs="*", default=["tail", "model", "points"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    print(f"device: {torch.cuda.get_device_name(0)}\n")
    for p in a.parts:
        {"tail": part_tail, "model": part_model, "points": part_points}[p](a)
        print()
