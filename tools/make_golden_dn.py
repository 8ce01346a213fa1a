#!/usr/bin/env python3
"""Generate the depth + normal model fixtures (tests/golden/dn_*.npz, schema_dn_wrapper.json) by running the IMPORTED
reference head and wrapper (models/video_depth_head_v2_sangyu.py, models/video_depth_model.py) on CPU.

Runs only where the reference tree is available. A stub `models` package (its __path__ pointed at the reference's
models/ directory) skips models/__init__.py, which pulls in transformers; the Hiera trunk, which the reference fetches
with torch.hub, is replaced in sys.modules by vdn.synth.dn_trunk (so is the unused v1 head / DINOv2 encoder, which
also fetch over the network). No reference source is copied: fixtures hold output numbers and key lists only.
Weights: vdn.synth.synth_state_dict + synth_buffer (non-trivial BatchNorm statistics); inputs: vdn.synth.

The output is bit-identical on every run (fixed zip timestamps). For each fixture the generator prints, and asserts,
how far skipping every attention stack moves the checked metrics: the tests' 1e-3 bar must be >= 10x below that.

Usage: python tools/make_golden_dn.py [REFERENCE_ROOT]
"""
from __future__ import annotations

import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

ROOT = MG.ROOT
GOLD = MG.GOLD
SEED = MG.SEED
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dn_fixture as DF  # noqa: E402  (the sampling / metric helpers the GPU tests use)

TOL = 1e-3


def install(ref_root: str):
    MG.install_shims()
    from vdn import synth
    models = types.ModuleType("models")
    models.__path__ = [os.path.join(ref_root, "models")]
    sys.modules["models"] = models
    hiera = types.ModuleType("models.hiera_image_encoder")
    hiera.HieraImageEncoder = lambda model_name=None, finetune=False: synth.dn_trunk()
    sys.modules["models.hiera_image_encoder"] = hiera
    for name, cls in (("models.dinov2_encoder", "DINOv2Encoder"), ("models.video_depth_head", "VideoDepthAnythingHead")):
        m = types.ModuleType(name)
        setattr(m, cls, None)
        sys.modules[name] = m
    import models.video_depth_head_v2_sangyu as H
    import models.video_depth_model as M
    return H, M


def save(path: str, **arrays):
    """np.savez_compressed with a fixed member timestamp: regenerating gives the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())
    size = os.path.getsize(path)
    assert size <= 1 << 20, (path, size)
    print(f"  wrote {os.path.relpath(path, ROOT)} ({size / 1024:.0f} KiB)")


def tap_head(head):
    """Wrap the head's _maybe_process to keep the processed level-2 / level-3 maps; returns (taps dict, skip switch)."""
    taps, state = {}, {"skip": False}
    orig = head._maybe_process

    def wrapped(lvl, feat):
        if state["skip"]:
            return feat
        out = orig(lvl, feat)
        taps[lvl] = out.detach().clone()
        taps[f"in{lvl}"] = feat.detach().clone()
        return out

    def conditioning(lvl):
        """Rel-L2 move of the processed map under a 1e-7 relative perturbation of its input: how much fp32 rounding noise
        the 16 blocks amplify (the level-3 stack at S = 32 turns 1e-7 into ~7e-4 with these weights). The tests allow
        3x this on the taps, never less than their 1e-3 bar."""
        x = taps[f"in{lvl}"]
        g = torch.Generator().manual_seed(lvl)
        with torch.no_grad():
            y = orig(lvl, x * (1 + 1e-7 * torch.randn(x.shape, generator=g)))
        return float((y - taps[lvl]).norm() / taps[lvl].norm())

    state["cond"] = conditioning

    head._maybe_process = wrapped
    return taps, state


def check_sensitivity(name, ref, skipped, keys):
    """Rel-L2 moves of the checked output metrics when the attention stacks are skipped: the most sensitive mean-removed
    one must move >= 10x TOL, every one >= 5x TOL (the stage taps, which move 7-10x in norm, are the finer check)."""
    moves = []
    for k in keys:
        r, s = DF.metrics(skipped, ref, k)[:2]
        print(f"  {name}:{k} skipping attention moves raw {r:.2e}, mean-removed {s:.2e}")
        moves.append(s)
    assert max(moves) >= 10 * TOL and min(moves) >= 5 * TOL, f"{name}: checked metrics too insensitive to attention {moves}"


def gen_head(H, name, S, seq_len, levels):
    print(f"[{name}] head S={S} sequence_length={seq_len} levels={levels}")
    torch.manual_seed(0)
    head = H.VideoDepthAnythingHeadV2(sequence_length=seq_len, attention_feature_levels=levels).eval()
    MG.load_synth(head)
    feats = [torch.from_numpy(f) for f in DF.head_inputs(1, S)]
    taps, state = tap_head(head)
    with torch.no_grad():
        out = head(feats)
        state["skip"] = True
        out_skip = head(feats)
    ref = DF.summarise_head(out)
    sk = DF.summarise_head(out_skip)
    for lvl in (2, 3):
        if lvl in levels:
            ref.update(DF.summarise_tap(taps[lvl], lvl))
            ref[f"tap{lvl}_cond"] = np.array(state["cond"](lvl))
            print(f"  tap{lvl} conditioning {float(ref[f'tap{lvl}_cond']):.2e}")
    check_sensitivity(name, DF.flatten(ref), DF.flatten(sk), ["out"])
    save(os.path.join(GOLD, f"{name}.npz"), meta=np.array([1, S, seq_len], np.int64), levels=np.array(levels, np.int64),
         **DF.flatten(ref))


def gen_wrapper(H, M, name, B, S, Hh, Ww, seq_len, levels, flags, pe="ape", schema=False):
    print(f"[{name}] wrapper B={B} S={S} {Hh}x{Ww} flags={flags} pe={pe}")
    torch.manual_seed(0)
    model = M.VideoDepthEstimationModel(seq_len, attention_feature_levels=levels, **flags).eval()
    if pe != "ape":
        model.head = H.VideoDepthAnythingHeadV2(sequence_length=seq_len, pe=pe, attention_feature_levels=levels)
        model.eval()   # the new head's BatchNorms too
    _, shapes = MG.load_synth(model)
    if schema:
        with open(os.path.join(GOLD, "schema_dn_wrapper.json"), "w") as f:
            json.dump({"params": [[k, list(s)] for k, s in shapes],
                       "buffers": [[k, list(v.shape)] for k, v in model.named_buffers()]}, f, indent=0)
        print(f"  wrote schema ({len(shapes)} parameters)")
    depth, img = (torch.from_numpy(t) for t in DF.wrapper_inputs(B, S, Hh, Ww))
    taps, state = tap_head(model.head)
    with torch.no_grad():
        d, n = model(depth, img)
        state["skip"] = True
        d_s, n_s = model(depth, img)
    d_in = depth if flags.get("use_residual") else None
    ref, sk = DF.summarise_wrapper(d, n, d_in), DF.summarise_wrapper(d_s, n_s, d_in)
    for lvl in (2, 3):
        if lvl in levels:
            ref.update(DF.summarise_tap(taps[lvl], lvl))
            ref[f"tap{lvl}_cond"] = np.array(state["cond"](lvl))
            print(f"  tap{lvl} conditioning {float(ref[f'tap{lvl}_cond']):.2e}")
    check_sensitivity(name, DF.flatten(ref), DF.flatten(sk), ["dres" if d_in is not None else "depth", "dx", "dy"])
    f = dict(flags)
    save(os.path.join(GOLD, f"{name}.npz"), meta=np.array([B, S, Hh, Ww, seq_len], np.int64), levels=np.array(levels, np.int64),
         flags=np.array([int(f.get("use_residual", False)), int(f.get("use_final_relu", False)),
                         int(f.get("use_depth_feature", True)), int(f.get("use_rgb_feature", True)), int(pe == "ape")], np.int64),
         **DF.flatten(ref))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else MG.REF
    H, M = install(ref_root)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    only = sys.argv[2:]
    if not only or "head" in only:
        gen_head(H, "dn_head_s4", 4, 8, [2, 3])
        gen_head(H, "dn_head_s32", 32, 32, [2, 3])
        gen_head(H, "dn_head_s2_all", 2, 8, [0, 1, 2, 3])
    gen_wrapper(H, M, "dn_model_b2", 2, 4, 240, 320, 8, [2, 3], dict(use_residual=True, use_final_relu=True), schema=True)
    gen_wrapper(H, M, "dn_model_nope", 1, 4, 224, 224, 4, [2, 3], dict(use_rgb_feature=False), pe="none")


if __name__ == "__main__":
    main()
