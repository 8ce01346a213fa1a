#!/usr/bin/env python3
"""Time vdn.metric on one MI355X and record how far it sits from tests/metric_ref.py; writes profiles/metric_depth.md.

With seeded inputs resident on the GPU (nothing is read from the reference):
  * eval_depth_batch at the validation shape of metric_depth/train.py: one item, prediction 518 x 518, ground truth 768 x 1024,
    alone and followed by the one copy to the host that a caller reading the values makes;
  * SiLogLoss.forward_from_valid and its backward at the training shape [2, 518, 518];
each beside
  * the scripts' statements for the same step as a torch composition on the same device, written here as the scripts write
    them: F.interpolate(align_corners=True), the mask expression, `if valid_mask.sum() < 10`, the two boolean-indexed copies,
    the metric formulas and one .item() per metric; for the loss the mask expression, the indexed log difference and autograd;
  * a device-to-device copy of the bytes the function must move (4 + 4 + 1 per ground-truth pixel and the small prediction;
    the backward 4 more for the gradient).
Each timed call works on the next of `sets` copies of the inputs, enough that together they exceed the 256 MiB Infinity Cache
twice over, so a call reads from HBM. A sample is the time of `--batch` calls between two device events, divided by the batch;
the figure is the median (min .. max) of `--iters` samples after `--warmup` calls. Event figures include launch overhead and,
where a call synchronises, the wait.

Then the largest differences between the device and tests/metric_ref.py at these two shapes, and the float32 gap recorded in
tests/golden/metric_cases.npz."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from normal_bench import HBM_MEASURED, sample_us  # noqa: E402
from prep_bench import OpCounter, host_us  # noqa: E402

MIN_DEPTH, MAX_DEPTH = 0.001, 20.0
EVAL_PRED, EVAL_GT = (518, 518), (768, 1024)
TRAIN = (2, 518, 518)
CACHE2 = 2 * 256 * 2 ** 20


# ---------------------------------------------------------------------------------- the scripts' statements in torch ops
def t_metrics(pred, target):
    """The nine metrics of two 1-D tensors, one .item() each."""
    thresh = torch.max(target / pred, pred / target)
    n = len(thresh)
    d = [torch.sum(thresh < 1.25 ** k).float() / n for k in (1, 2, 3)]
    diff, diff_log = pred - target, torch.log(pred) - torch.log(target)
    sq, sq_log = torch.pow(diff, 2), torch.pow(diff_log, 2)
    vals = d + [torch.mean(torch.abs(diff) / target), torch.mean(sq / target), torch.sqrt(torch.mean(sq)), torch.sqrt(torch.mean(sq_log)),
                torch.mean(torch.abs(torch.log10(pred) - torch.log10(target))), torch.sqrt(sq_log.mean() - 0.5 * torch.pow(diff_log.mean(), 2))]
    return [v.item() for v in vals]


def t_validate(pred, depth, valid):
    """One pass of the validation loop's body for one item: pred [1, h, w], depth [H, W], valid [H, W]."""
    p = F.interpolate(pred[:, None], depth.shape[-2:], mode="bilinear", align_corners=True)[0, 0]
    vm = (valid == 1) & (depth >= MIN_DEPTH) & (depth <= MAX_DEPTH)
    if vm.sum() < 10:
        return None
    return t_metrics(p[vm], depth[vm])


def t_loss(pred, depth, valid, lambd=0.5):
    vm = ((valid == 1) & (depth >= MIN_DEPTH) & (depth <= MAX_DEPTH)).detach()
    dl = torch.log(depth[vm]) - torch.log(pred[vm])
    return torch.sqrt(torch.pow(dl, 2).mean() - lambd * torch.pow(dl.mean(), 2))


# ---------------------------------------------------------------------------------- timing
def copy_us(nbytes, S_, dev):
    src = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(max(2, math.ceil(CACHE2 / nbytes)))]
    dst = torch.empty_like(src[0])
    return S_(lambda i: dst.copy_(src[i % len(src)]))


def inputs(shape, pshape, sets, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    depth = [torch.empty(shape, device=dev).uniform_(0.05, 25.0, generator=g) for _ in range(sets)]
    pred = [torch.empty(shape[:1] + pshape, device=dev).uniform_(0.05, 25.0, generator=g) if pshape != shape[1:] else
            d * torch.exp(0.35 * torch.randn(shape, device=dev, generator=g)) for d in depth]
    valid = [torch.rand(shape, device=dev, generator=g) < 0.7 for _ in range(sets)]
    return pred, depth, valid


def differences(got_rows, want_rows):
    g, w = got_rows.cpu().numpy(), want_rows
    exact = bool(np.array_equal(g[:, :4], w[:, :4]))
    rel = float((np.abs(g[:, 4:] - w[:, 4:]) / np.abs(w[:, 4:])).max())
    return exact, rel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metric_depth.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("metric_bench.py measures on the GPU; none is visible")
    import metric_ref as R
    from vdn import metric
    dev = torch.device("cuda:0")
    S_ = lambda fn: sample_us(fn, a.warmup, a.iters, a.batch)
    kw = dict(min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
    rows = []

    # ---- the nine metrics at the validation shape
    px = EVAL_GT[0] * EVAL_GT[1]
    ebytes = 9 * px + 4 * EVAL_PRED[0] * EVAL_PRED[1]
    sets = max(2, math.ceil(CACHE2 / ebytes))
    pred, depth, valid = inputs((1,) + EVAL_GT, EVAL_PRED, sets, dev, 3)
    ours = lambda i: metric.eval_depth_batch(pred[i % sets], depth[i % sets], valid[i % sets], **kw)
    ours_read = lambda i: ours(i).cpu()
    theirs = lambda i: t_validate(pred[i % sets], depth[i % sets][0], valid[i % sets][0])
    with OpCounter() as oc:
        want = theirs(0)
    got = ours(0)[0].cpu().tolist()
    gap_torch = max(abs(g - w) / abs(w) for g, w in zip(got[1:], want))
    rows.append(dict(name="`eval_depth_batch`, 518 x 518 -> 768 x 1024", bytes=ebytes, bpp=ebytes / px, ours=S_(ours), host=host_us(ours),
                     theirs=S_(theirs), ops=oc.n, copy=copy_us(ebytes, S_, dev), note="no synchronisation"))
    rows.append(dict(name="... and `.cpu()` of the row", bytes=ebytes, bpp=ebytes / px, ours=S_(ours_read), host=None, theirs=rows[0]["theirs"],
                     ops=oc.n, copy=rows[0]["copy"], note="one synchronising copy, as the composition's nine .item()"))
    case = dict(pred=pred[0].cpu().numpy(), depth=depth[0].cpu().numpy(), mask=valid[0].cpu().numpy())
    exact_e, rel_e = differences(ours(0), R.eval_rows(case["pred"], case["depth"], case["mask"], MIN_DEPTH, MAX_DEPTH))
    del pred, depth, valid

    # ---- the loss and its backward at the training shape
    px_t = TRAIN[0] * TRAIN[1] * TRAIN[2]
    sets = max(2, math.ceil(CACHE2 / (9 * px_t)))
    pred, depth, valid = inputs(TRAIN, TRAIN[1:], sets, dev, 4)
    crit = metric.SiLogLoss()
    fwd = lambda i: crit.forward_from_valid(pred[i % sets], depth[i % sets], valid[i % sets], MIN_DEPTH, MAX_DEPTH)
    t_fwd = lambda i: t_loss(pred[i % sets], depth[i % sets], valid[i % sets])
    leaves = [p.clone().requires_grad_(True) for p in pred]

    def both(i):
        leaves[i % sets].grad = None
        crit.forward_from_valid(leaves[i % sets], depth[i % sets], valid[i % sets], MIN_DEPTH, MAX_DEPTH).backward()

    def t_both(i):
        leaves[i % sets].grad = None
        t_loss(leaves[i % sets], depth[i % sets], valid[i % sets]).backward()

    with OpCounter() as oc_f:
        want_loss = t_fwd(0).item()
    with OpCounter() as oc_b:
        t_both(0)
    want_grad = leaves[0].grad.clone()
    both(0)
    got_grad = leaves[0].grad.clone()
    rows.append(dict(name="`SiLogLoss.forward_from_valid`, [2, 518, 518]", bytes=9 * px_t, bpp=9.0, ours=S_(fwd), host=host_us(fwd),
                     theirs=S_(t_fwd), ops=oc_f.n, copy=copy_us(9 * px_t, S_, dev), note="no synchronisation on either side"))
    rows.append(dict(name="forward and backward, [2, 518, 518]", bytes=22 * px_t, bpp=22.0, ours=S_(both), host=host_us(both),
                     theirs=S_(t_both), ops=oc_b.n, copy=copy_us(22 * px_t, S_, dev), note="9 bytes forward, 9 + 4 backward"))
    p0, d0, m0 = (x[0].cpu().numpy() for x in (pred, depth, valid))
    keep = R.keep_mask(m0, d0, MIN_DEPTH, MAX_DEPTH)
    st = R.silog_ref(p0, d0, keep, 0.5)
    got_state = metric.silog_loss(pred[0], depth[0], valid[0], **kw)
    rel_l = abs(got_state["loss"] - st[0]) / abs(st[0])
    gref = R.silog_grad_ref(p0, d0, keep, 0.5).astype(np.float32)
    gg = got_grad.cpu().numpy()
    ulps = float((np.abs(gg.astype(np.float64) - gref.astype(np.float64))[keep] / np.spacing(np.abs(gref[keep])).astype(np.float64)).max())
    grad_vs_torch = float((got_grad - want_grad).abs().max() / want_grad.abs().max())
    loss_vs_torch = abs(float(fwd(0)) - want_loss) / abs(want_loss)
    fixture = np.load(os.path.join(ROOT, "tests", "golden", "metric_cases.npz"))

    f3 = lambda v: f"{v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})"
    lines = [
        "# vdn.metric: SiLogLoss and the nine depth metrics on the device",
        "",
        f"Written by `tools/metric_bench.py` on {torch.cuda.get_device_name(0)}. Device events around {a.batch} calls, {a.warmup} warm-up calls,",
        f"median (min .. max) of {a.iters} samples, in microseconds per call; launch overhead, the allocation of the result and, where a",
        "call synchronises, the wait are included. Every call works on the next of several copies of the inputs, which together",
        "exceed the Infinity Cache twice over. Bytes are the compulsory traffic: 4 + 4 + 1 per ground-truth pixel (prediction or its",
        "share of the small map, depth, mask), 4 more per pixel for the gradient the backward writes. The copy moves the same bytes",
        f"(half read, half written); the share of HBM is of {HBM_MEASURED / 1e12:.2f} TB/s, a float4 copy measured on this part. `host us to issue`:",
        "a host clock around 50 calls with no synchronisation inside, per call. The torch composition is the scripts' statements on",
        "the same device: `F.interpolate(align_corners=True)`, the mask expression, `valid_mask.sum() < 10`, two boolean-indexed",
        "copies, the formulas and one `.item()` per metric; for the loss the mask expression, the indexed log difference and autograd.",
        "",
        "| call | MB | bytes per pixel | vdn.metric us | host us to issue | TB/s | of measured HBM rate | torch composition us | torch operator calls | copy us | share of the copy's rate | |",
        "|---|---:|---:|---|---:|---:|---:|---|---:|---|---:|---|",
    ]
    slower = []
    for x in rows:
        rate = x["bytes"] / x["ours"][0] / 1e6
        host = "" if x["host"] is None else f"{x['host']:.1f}"
        lines.append(f"| {x['name']} | {x['bytes'] / 1e6:.1f} | {x['bpp']:.1f} | {f3(x['ours'])} | {host} | {rate:.2f} | {rate * 1e12 / HBM_MEASURED:.0%} | "
                     f"{f3(x['theirs'])} | {x['ops']} | {f3(x['copy'])} | {x['copy'][0] / x['ours'][0]:.0%} | {x['note']} |")
        if x["ours"][0] > x["theirs"][0]:
            issue = "" if x["host"] is None else f"issuing the call takes {x['host']:.1f} us on the host, "
            slower.append(f"{x['name']}: {x['ours'][0]:.1f} us against {x['theirs'][0]:.1f} us; {issue}the copy of its bytes takes "
                          f"{x['copy'][0]:.1f} us, and the composition's {x['ops']} torch operator calls are what it is compared with")
    lines += ["", "## Slower than the torch composition", ""]
    lines += [f"- {s}" for s in slower] if slower else ["None of the four."]
    lines += ["", "## What bounds the calls", "",
              "The bytes of one call take a few microseconds at the copy's rate, so a call is bound by its two launches and by the host",
              "time to issue it (the wrapper's device guard, argument checks, the allocation of the result and ctypes marshalling), not",
              "by memory: the share of the copy's rate above is what is left of it. The validation loop has one item per call; a batch",
              "of items costs the same two launches. Forward and backward together go through a torch.autograd.Function, whose round",
              f"trip through Python is most of their {rows[3]['host']:.0f} us to issue.",
              "", "## Differences", "",
              "| | |", "|---|---|",
              f"| n, d1, d2, d3 against tests/metric_ref.py, resampled 518 x 518 -> 768 x 1024 | {'equal bits' if exact_e else 'DIFFERENT'} |",
              f"| the six fp64 metrics against tests/metric_ref.py, same case, largest relative difference | {rel_e:.2e} |",
              f"| loss against tests/metric_ref.py, [2, 518, 518], relative | {rel_l:.2e} |",
              f"| gradient against float32(tests/metric_ref.py), largest difference at a kept pixel | {ulps:.2f} ulp |",
              f"| the nine metrics against the float32 torch composition on this device, largest relative difference | {gap_torch:.2e} |",
              f"| loss against the float32 torch composition, relative | {loss_vs_torch:.2e} |",
              f"| gradient against the float32 torch composition's autograd, largest difference over max abs gradient | {grad_vs_torch:.2e} |",
              f"| recorded in tests/golden/metric_cases.npz: the reference's float32 run against its float64 run on the CPU, largest relative gap | {float(fixture['f32_gap']):.2e} |",
              "",
              "The float32 composition resamples with fused multiply-adds and sums in float32; the device's continuous metrics are fp64",
              "from the float32 inputs on (include/vdn.h), so the last three rows above say how far the scripts' printed values sit",
              "from the contract, not how far the device sits from it."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
