#!/usr/bin/env python3
"""Time the batch preparation (vdn.prep) and count what one loop body costs (vdn.steps) on one MI355X; writes profiles/prep.md.

At [4, 16, ., 224, 224] (the scripts' size) and [2, 32, ., 518, 518], with seeded inputs resident on the GPU (nothing is read
from the reference), for each function of vdn.prep:
  * the function itself (its launches and the allocation of its result);
  * the same composition in torch float32 ops on the same device, written here as the scripts write it (clamp, sub_, div_;
    where / min / max / sub / clamp / div / clamp / any / where; 1. / clamp);
  * a device-to-device copy of the bytes the function must move;
and whether the two results are equal at that size (torch.equal; a report, the tests are the gate).
Each timed call works on the next of `sets` copies of the inputs, enough that together they exceed the 256 MiB Infinity Cache
twice over, so a call reads from HBM. A sample is the time of `--batch` calls between two device events, divided by the batch;
the figure is the median (min .. max) of `--iters` samples after `--warmup` calls. Event figures include launch overhead.

Then, for one validate_step on a stub model at the scripts' size: the library entry-point calls, the torch operator calls
(counted by a TorchDispatchMode; each is at least one launch) and the host synchronisations (Tensor.item / .cpu / .tolist),
beside the scripts' loop body written with the torch composition and `value.item()` per key."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

from normal_bench import HBM_MEASURED, sample_us  # noqa: E402

SHAPES = [(4, 16, 224, 224), (2, 32, 518, 518)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---------------------------------------------------------------------------------- the scripts' composition in torch ops
def t_rgb(x, normalize=True):
    B, S, C, H, W = x.shape
    y = x.view(B * S, C, H, W).clamp(0, 1)
    if normalize:
        mean = torch.as_tensor(MEAN, dtype=y.dtype, device=y.device).view(-1, 1, 1)
        std = torch.as_tensor(STD, dtype=y.dtype, device=y.device).view(-1, 1, 1)
        y = y.clone().sub_(mean).div_(std)
    return y.view(B, S, C, H, W)


def t_norm(x, masks):
    B = x.shape[0]
    lo = torch.where(masks, x, torch.full_like(x, float("inf"))).view(B, -1).min(dim=1, keepdim=True)[0].view(B, 1, 1, 1)
    hi = torch.where(masks, x, torch.full_like(x, float("-inf"))).view(B, -1).max(dim=1, keepdim=True)[0].view(B, 1, 1, 1)
    out = ((x - lo) / torch.clamp(hi - lo, min=1e-8)).clamp(0.0, 1.0)
    valid = masks.any(dim=(-1, -2, -3)).view(B, 1, 1, 1)
    return torch.where(valid, out, torch.zeros_like(out))


def t_pre(x, masks, norm):
    d = x.clamp(min=0).squeeze(2)
    return t_norm(d, masks.squeeze(2)) if norm else d


def t_inv(x):
    return 1. / torch.clamp(x, min=1e-8)


# ---------------------------------------------------------------------------------- timing
def host_us(fn, calls=50):
    """Host time to issue one call, microseconds: a host clock around `calls` calls with no synchronisation inside."""
    import time
    for i in range(5):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(calls):
        fn(i)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / calls * 1e6


def bench_shape(shape, a, dev):
    from vdn import prep
    B, S, H, W = shape
    px = B * S * H * W
    g = torch.Generator(device=dev).manual_seed(3)
    sets = max(2, math.ceil(2 * 256 * 2 ** 20 / (13 * px)))
    rsets = max(2, math.ceil(2 * 256 * 2 ** 20 / (24 * px)))
    depth = [torch.empty(B, S, 1, H, W, device=dev).uniform_(-1.0, 20.0, generator=g) for _ in range(sets)]
    mask = [torch.rand(B, S, 1, H, W, device=dev, generator=g) < 0.7 for _ in range(sets)]
    rgb = [torch.empty(B, S, 3, H, W, device=dev).uniform_(-0.2, 1.2, generator=g) for _ in range(rsets)]
    d, m, r = (lambda i: depth[i % sets]), (lambda i: mask[i % sets]), (lambda i: rgb[i % rsets])
    #        name, elements, bytes per element, ours, torch composition
    rows = [("preprocess_rgb_sequences", 3 * px, 8, lambda i: prep.preprocess_rgb_sequences(r(i)), lambda i: t_rgb(r(i))),
            ("preprocess_rgb_viz_sequences", 3 * px, 8, lambda i: prep.preprocess_rgb_viz_sequences(r(i)), lambda i: t_rgb(r(i), False)),
            ("preprocess_depth_sequences, norm=False", px, 8, lambda i: prep.preprocess_depth_sequences(d(i), m(i), False),
             lambda i: t_pre(d(i), m(i), False)),
            ("preprocess_depth_sequences, norm=True", px, 13, lambda i: prep.preprocess_depth_sequences(d(i), m(i), True),
             lambda i: t_pre(d(i), m(i), True)),
            ("inverse_depth", px, 8, lambda i: prep.inverse_depth(d(i)), lambda i: t_inv(d(i))),
            ("preprocess_inverse_depth_sequences", px, 13, lambda i: prep.preprocess_inverse_depth_sequences(d(i), m(i), True),
             lambda i: t_pre(t_inv(d(i)), m(i), True))]
    S_ = lambda fn: sample_us(fn, a.warmup, a.iters, a.batch)
    out = []
    for name, n, bpe, ours, theirs in rows:
        nbytes = n * bpe
        t_ours, t_torch = S_(ours), S_(theirs)
        h_ours, h_torch = host_us(ours), host_us(theirs)
        src = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(max(2, math.ceil(2 * 256 * 2 ** 20 / nbytes)))]
        dst = torch.empty_like(src[0])
        t_copy = S_(lambda i: dst.copy_(src[i % len(src)]))
        got = ours(0)
        with OpCounter() as oc:
            want = theirs(0)
        same = bool(torch.equal(got, want.view(got.shape)))
        del src, dst
        out.append(dict(name=name, bytes=nbytes, bpe=bpe, ours=t_ours, torch=t_torch, copy=t_copy, equal=same, host=h_ours, host_torch=h_torch, ops=oc.n))
        print(f"{shape} {name}: ours {t_ours[0]:.1f} us (host {h_ours:.1f}), torch {t_torch[0]:.1f} us, copy {t_copy[0]:.1f} us, equal {same}", flush=True)
    return dict(shape=shape, px=px, sets=sets, rsets=rsets, rows=out)


# ---------------------------------------------------------------------------------- counting one loop body
class OpCounter(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def count_body(dev):
    from vdn import prep, steps
    from vdn.loss import VideoDepthLoss
    from vdn.normals import VideoNormalLoss, normal_vector
    from vdn.runtime import Runtime
    B, S, H, W = SHAPES[0]
    g = torch.Generator(device=dev).manual_seed(4)
    batch = {"rgb": torch.empty(B, S, 3, H, W, device=dev).uniform_(-0.2, 1.2, generator=g),
             "depth_anything_v2": torch.empty(B, S, 1, H, W, device=dev).uniform_(0.0, 10.0, generator=g),
             "depth": torch.empty(B, S, 1, H, W, device=dev).uniform_(0.5, 20.0, generator=g),
             "mask": torch.rand(B, S, 1, H, W, device=dev, generator=g) < 0.8}
    normals = torch.randn(B, S, 3, H, W, device=dev, generator=g)
    model = lambda depth, rgb: (0.75 * depth + 0.125, normals)
    dc, nc = VideoDepthLoss(), VideoNormalLoss()

    def ours():
        meter = steps.LossMeter()
        steps.validate_step(model, batch, dc, nc, meter=meter)

    def script():
        running = {}
        with torch.no_grad():
            rgbs = t_rgb(batch["rgb"])
            masks = batch["mask"]
            input_depths = t_pre(batch["depth_anything_v2"], masks, False)
            gt = t_inv(batch["depth"])
            gt_normals = normal_vector(gt)
            pd, pn = model(input_depths, rgbs)
            losses = dc(pd, gt.squeeze(2), masks.squeeze(2)) | nc(pn, gt_normals, masks.squeeze(2))
            for k, v in losses.items():
                running[k] = running.get(k, 0.0) + v.item()

    res = {}
    for name, fn in (("validate_step", ours), ("script body", script)):
        fn()                                                      # buffers and code objects exist before the count
        calls = {"entry": 0, "item": 0, "cpu": 0, "tolist": 0}
        saved = {k: getattr(torch.Tensor, k) for k in ("item", "cpu", "tolist")}
        launch = Runtime._launch

        def counted_launch(self, fn_, *args, **kw):
            calls["entry"] += 1
            return launch(self, fn_, *args, **kw)

        def wrap(k):
            def f(self, *args, **kw):
                calls[k] += 1
                return saved[k](self, *args, **kw)
            return f

        Runtime._launch = counted_launch
        for k in saved:
            setattr(torch.Tensor, k, wrap(k))
        try:
            with OpCounter() as oc:
                fn()
        finally:
            Runtime._launch = launch
            for k, v in saved.items():
                setattr(torch.Tensor, k, v)
        torch.cuda.synchronize()
        res[name] = dict(calls, ops=oc.n)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prep.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prep_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    results = [bench_shape(s, a, dev) for s in SHAPES]
    counts = count_body(dev)
    f3 = lambda v: f"{v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})"
    lines = [
        "# vdn.prep: the scripts' batch preparation on the device",
        "",
        f"Written by `tools/prep_bench.py` on {torch.cuda.get_device_name(0)}. Device events around {a.batch} calls, {a.warmup} warm-up calls,",
        f"median (min .. max) of {a.iters} samples, in microseconds per call; launch overhead and the allocation of the result are",
        "included. Every call works on the next of several copies of the inputs, which together exceed the Infinity Cache twice",
        "over. Bytes are the compulsory traffic (rgb, clamp, reciprocal: 4 read + 4 written per element; the masked normalisation:",
        f"4 + 1 read, 4 read again, 4 written per pixel); the share is of {HBM_MEASURED / 1e12:.2f} TB/s, a float4 copy measured on this part.",
        "The copy moves the same bytes (half read, half written). `equal`: torch.equal of the two results at this size. `host us to",
        "issue`: a host clock around 50 calls with no synchronisation inside, per call; a call cannot take less than that.",
        "",
    ]
    slower = []
    for r in results:
        B, S, H, W = r["shape"]
        lines += [f"## [{B}, {S}, ., {H}, {W}]: {r['px'] / 1e6:.2f} M pixels ({r['sets']} depth sets, {r['rsets']} rgb sets)", "",
                  "| function | MB | vdn.prep us | host us to issue | TB/s | of measured HBM rate | torch composition us | host us to issue | copy us | share of the copy's rate | equal |",
                  "|---|---:|---|---:|---:|---:|---|---:|---|---:|---|"]
        for x in r["rows"]:
            rate = x["bytes"] / x["ours"][0] / 1e6
            lines.append(f"| `{x['name']}` | {x['bytes'] / 1e6:.0f} | {f3(x['ours'])} | {x['host']:.1f} | {rate:.2f} | {rate * 1e12 / HBM_MEASURED:.0%} | "
                         f"{f3(x['torch'])} | {x['host_torch']:.1f} | {f3(x['copy'])} | {x['copy'][0] / x['ours'][0]:.0%} | {'yes' if x['equal'] else 'NO'} |")
            if x["ours"][0] > x["torch"][0]:
                why = (f"the call is bound by the host: issuing it takes {x['host']:.1f} us (the wrapper's device guard, argument checks and "
                       f"ctypes marshalling), longer than the copy of its bytes ({x['copy'][0]:.1f} us), and the {x['ops']} torch operator call(s) of "
                       f"this composition (views included) are issued in {x['host_torch']:.1f} us" if x["host"] > x["copy"][0] else
                       f"the composition is {x['ops']} torch operator call(s) (views included), one kernel over the same bytes where "
                       f"that is a single clamp, so equal is the best the function can do; it runs at {x['copy'][0] / x['ours'][0]:.0%} of the rate of the copy ({x['copy'][0]:.1f} us)")
                slower.append(f"`{x['name']}` at {list(r['shape'])}: {x['ours'][0]:.1f} us against {x['torch'][0]:.1f} us; {why}")
        lines.append("")
    lines += ["## Slower than the torch composition", ""]
    lines += [f"- {s}" for s in slower] if slower else ["None at either shape."]
    lines += ["", f"## One loop body at {list(SHAPES[0])}, stub model", "",
              "`validate_step` with both criteria and a `LossMeter`, beside the scripts' loop body with the torch composition, the same",
              "criteria and `value.item()` per key. Library calls are entry points of `libvdn_hip.so` (each one to a few launches,",
              "`include/vdn.h`); torch operator calls are counted by a TorchDispatchMode (views included; each kernel-backed one is at",
              "least one launch).", "",
              "| | library entry-point calls | torch operator calls | .item() | .cpu() | .tolist() |", "|---|---:|---:|---:|---:|---:|"]
    for k, v in counts.items():
        lines.append(f"| {k} | {v['entry']} | {v['ops']} | {v['item']} | {v['cpu']} | {v['tolist']} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
