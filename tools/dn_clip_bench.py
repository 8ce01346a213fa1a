#!/usr/bin/env python3
"""Time the depth + normal model's clip driver (`VideoDepthEstimationModel.infer_video`) on one MI355X and write a markdown
report (profiles/dn_clip.md is a run of this tool):

    python tools/dn_clip_bench.py --out profiles/dn_clip.md [--errors LOG]

Model: with_native_trunks(16, "hiera_base_224"), synthetic weights; clip: 256 frames at 224 x 224, overlap 4 (21 windows, 336
window slots over a padded clip of 256 frames). On the same seeded clip resident on the GPU:
  * cached:   `infer_video` (both trunks once per frame of the padded clip into the per-clip feature cache, the head per window
              from the cache, vdn_stitch_fit + vdn_dn_stitch_apply), frames/s by a host clock around a call that ends in the
              driver's own range check, which synchronises;
  * fallback: the same call with the cache budget forced to nothing (VDN_TAP_CACHE_GB=0): `forward` on every window's 16 frames
              through the same stitcher. This is what the code before the driver offers a user. The two alternate in one process;
  * split:    HIP events, median of --iters, around one batch of 16 frames through both trunks (with vdn_refine_pack), one
              window through the head (prologue .. vdn_dn_tail), and one window's fit + apply; times a clip's counts of each.
The two results are compared (rel-L2, worst pixel) before anything is timed. Reports, not gates; --errors adds the `[dn_clip ..]`
lines of a test log (tests/test_gpu_dn_clip.py -s) to the report."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_clip(n, hw, device):
    """A seeded clip: depths [n, hw, hw] in (0, 1) and normalised frames [n, 3, hw, hw], eight synthetic frames repeated with a
    slow per-frame gain on the depth."""
    from vdn import synth
    idx = torch.arange(n, device=device) % 8
    d = torch.from_numpy(synth.depth_clip(1234, 8, hw, hw, max_depth=1.0).astype(np.float32)).to(device)[idx]
    f = torch.from_numpy(synth.normalize_frames(synth.frames_u8(1234, 8, hw, hw)).astype(np.float32)).to(device)[idx]
    gain = 1.0 - 0.001 * torch.arange(n, device=device, dtype=torch.float32)
    return (d * gain[:, None, None]).contiguous(), f.contiguous()


def clock_fps(fns, n, warmup, iters):
    """Alternate the callables `fns` (each ends synchronised); -> per callable (median frames/s, best frames/s)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    times = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[i].append(time.perf_counter() - t0)
    return [(n / statistics.median(t), n / min(t)) for t in times]


def event_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--seq", type=int, default=16)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--encoder", default="hiera_base_224")
    ap.add_argument("--clips", type=int, default=3, help="timed clips per variant")
    ap.add_argument("--iters", type=int, default=10, help="timed repeats of each part of the split")
    ap.add_argument("--out", default=None)
    ap.add_argument("--errors", default=None)
    a = ap.parse_args()

    import vdn
    from vdn import synth, util
    assert torch.cuda.is_available(), "this tool times the MI355X; there is no CPU path"
    dev = torch.device("cuda")
    N, S, ov, hw = a.frames, a.seq, a.overlap, 224
    m = vdn.VideoDepthEstimationModel.with_native_trunks(S, a.encoder, use_residual=True, use_final_relu=True)
    sd = synth.fast_state_dict([(k, tuple(p.shape)) for k, p in m.named_parameters()], 1234)   # timing only: torch's generator
    for k, b in m.named_buffers():
        v = synth.synth_buffer(1234, k, tuple(b.shape))
        sd[k] = torch.as_tensor(v) if v is not None else b.detach().clone()
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    d, f = make_clip(N, hw, dev)
    table = util.dn_window_table(N, S, ov)
    windows, chunks = len(table), -(-(table[-1][0] + S) // S)

    def cached():
        os.environ.pop("VDN_TAP_CACHE_GB", None)
        return m.infer_video(d, f, overlap=ov)

    def fallback():
        os.environ["VDN_TAP_CACHE_GB"] = "0"
        try:
            return m.infer_video(d, f, overlap=ov)
        finally:
            os.environ.pop("VDN_TAP_CACHE_GB", None)

    (gd, gn), (wd, wn) = cached(), fallback()
    agree = []
    for g, w in ((gd, wd), (gn[:, :2], wn[:, :2])):
        g, w = g.double(), w.double()
        agree.append((float((g - w).norm() / w.norm()), float((g - w).abs().max() / w.abs().max())))
    del gd, gn, wd, wn
    (c_med, c_best), (f_med, f_best) = clock_fps([cached, fallback], N, 1, a.clips)
    print("frames/s cached", c_med, c_best, "fallback", f_med, f_best, flush=True)

    # the split: one trunk batch, one window of the head, one window of the stitcher
    e = m._engines()
    rt, eng = e["rt"], e["head"]
    feats = {}

    def trunks():
        feats["a"], feats["b"], feats["sizes"] = m._trunk_features(rt, d[:S], f[:S])

    t_med, t_best = event_ms(trunks, 2, a.iters)
    out_d, out_n = torch.empty((S, hw, hw), device=dev), torch.empty((S, 3, hw, hw), device=dev)

    def head():
        eng.run_model(feats["a"], feats["b"], 1, S, feats["sizes"], hw, hw, d[:S], True, out_d, out_n)

    h_med, h_best = event_ms(head, 2, a.iters)
    clip_d, clip_n = torch.rand((S, hw, hw), device=dev), torch.rand((S, 3, hw, hw), device=dev)
    coef = torch.empty(2, device=dev)

    def stitch():
        rt.stitch_fit(out_d[:ov], clip_d[:ov], coef)
        rt.dn_stitch_apply(out_d, out_n, coef, clip_d, clip_n, ov, S, True)

    s_med, s_best = event_ms(stitch, 2, a.iters)

    def apply_only():
        rt.dn_stitch_apply(out_d, out_n, coef, clip_d, clip_n, ov, S, True)

    a_med, a_best = event_ms(apply_only, 5, 5 * a.iters)
    # bytes vdn_dn_stitch_apply must move: depth, nx, ny read and depth, nx, ny, nz written for S frames, plus the overlap's read
    apply_bytes = (3 * S + 4 * S + 3 * ov) * hw * hw * 4

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    sum_c = chunks * t_med + windows * (h_med + s_med)
    sum_f = windows * (t_med + h_med + s_med)
    lines = ["# infer_video: the depth + normal model's whole-clip driver", "",
             f"`python tools/dn_clip_bench.py` on {torch.cuda.get_device_name(0)} (torch {torch.__version__}), "
             f"{'on top of commit ' + commit if commit else 'working tree without git metadata'}; "
             f"`with_native_trunks({S}, \"{a.encoder}\", use_residual=True, use_final_relu=True)`, synthetic weights, one GPU; a clip of "
             f"{N} frames at {hw} x {hw}, overlap {ov}: {windows} windows, {windows * S} window slots, {chunks * S} frames in the padded clip. "
             f"Frames/s by a host clock around a call that ends synchronised (the driver's range check): median (best) of {a.clips} "
             "clips per variant after one warm-up clip, the two variants alternating in one process.", "",
             "Cached = `infer_video`: both trunks once per frame of the padded clip into the per-clip feature cache, the head per "
             "window from the cache, `vdn_stitch_fit` + `vdn_dn_stitch_apply`. Fallback = the same call with `VDN_TAP_CACHE_GB=0`: "
             "`forward` on every window's frames (both trunks on every slot again) through the same stitcher, which is what the code "
             "before this driver offers. `agreement` is the cached clip against the fallback's, rel-L2 / worst pixel of max, for "
             "depth and for (nx, ny).", "",
             "| frames | windows | trunk passes cached / fallback | cached frames/s | fallback frames/s | cached / fallback | agreement depth | agreement normals |",
             "|---|---|---|---|---|---|---|---|",
             f"| {N} | {windows} | {chunks * S} / {windows * S} | {c_med:.1f} ({c_best:.1f}) | {f_med:.1f} ({f_best:.1f}) | {c_med / f_med:.2f} x | "
             f"{agree[0][0]:.1e} / {agree[0][1]:.1e} | {agree[1][0]:.1e} / {agree[1][1]:.1e} |", "",
             f"The split, HIP events, median (best) of {a.iters}: one batch of {S} frames through `vdn_refine_pack` and both trunks; one "
             "window through the head (`vdn_dn_prologue` .. `vdn_dn_tail`); one window's `vdn_stitch_fit` + `vdn_dn_stitch_apply`. The "
             "clip columns multiply by the counts above; their sum against the measured clip time shows what the parts leave out "
             "(the copies into the cache, launch gaps, the range check).", "",
             "| part | one call ms | per clip cached ms | per clip fallback ms |", "|---|---|---|---|",
             f"| trunks, {S} frames | {t_med:.2f} ({t_best:.2f}) | {chunks} x = {chunks * t_med:.1f} | {windows} x = {windows * t_med:.1f} |",
             f"| head, one window | {h_med:.2f} ({h_best:.2f}) | {windows} x = {windows * h_med:.1f} | {windows} x = {windows * h_med:.1f} |",
             f"| stitch, one window | {s_med:.3f} ({s_best:.3f}) | {windows} x = {windows * s_med:.1f} | {windows} x = {windows * s_med:.1f} |",
             f"| sum | | {sum_c:.1f} | {sum_f:.1f} |",
             f"| measured clip | | {1e3 * N / c_med:.1f} | {1e3 * N / f_med:.1f} |", "",
             f"`vdn_dn_stitch_apply` alone on one {S}-frame window (overlap {ov}, all {S} frames kept): {1e3 * a_med:.1f} us "
             f"({1e3 * a_best:.1f}), {apply_bytes / 1e6:.1f} MB of compulsory traffic = {apply_bytes / (a_med * 1e-3) / 1e9:.0f} GB/s."]
    if a.errors:
        lines += ["", "## Measured errors of tests/test_gpu_dn_clip.py", "",
                  "Against the restated loop (`forward` on every window's gathered frames, then the float64 host stitch of "
                  "tests/dn_clip_ref.py); bar 1e-3 on every line.", "", "```"]
        lines += [l.strip().lstrip(".") for l in open(a.errors) if "[dn_clip" in l]
        lines += ["```"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
