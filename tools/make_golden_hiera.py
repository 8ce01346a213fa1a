#!/usr/bin/env python3
"""Generate the Hiera trunk fixtures (tests/golden/hiera_*.npz, schema_hiera_*.json, dn_model_native.npz) on CPU.

The oracle is the `transformers` port of the hub model (transformers.models.hiera.HieraModel built from a HieraConfig:
nothing is downloaded), so this runs only where that package is installed; no test imports it. Weights come from
vdn.synth keyed by THIS package's names (the hub names vdn.HieraImageEncoder holds) and reach the oracle through the one
rename table of vdn/hiera_image_encoder.py, which a strict load therefore verifies. No source of the oracle is copied:
fixtures hold output numbers, index tables and key lists.

Checks made while generating (all asserted):
  * tests/hiera_ref.py, the from-scratch restatement the tests use, equals the oracle to 1e-5 on every stage map;
  * each of four faults (no query max-pool, no residual max-pool, a windowed block run as global, no unroll) moves the
    checked stage maps by >= 10x the tests' 1e-3 bar;
  * the unroll / reroll index tables pushed through the oracle's own unroll / reroll equal the restatement's.
dn_model_native.npz additionally needs the reference tree: the imported reference wrapper (as tools/make_golden_dn.py
imports it) with its HieraImageEncoder replaced by an adapter around the oracle.

Usage: python tools/make_golden_hiera.py [REFERENCE_ROOT] [trunk] [wrapper]
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_dn as MD  # noqa: E402

ROOT, GOLD, SEED = MG.ROOT, MG.GOLD, MG.SEED
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dn_fixture as DF  # noqa: E402
import hiera_ref as HR  # noqa: E402

TOL = 1e-3
N_MAP, N_TAP = 4096, 2048
SHORT = {"hiera_tiny_224": "tiny", "hiera_small_224": "small", "hiera_base_224": "base"}


def oracle(depths):
    from transformers import HieraConfig
    from transformers.models.hiera.modeling_hiera import HieraModel
    return HieraModel(HieraConfig(depths=list(depths)), add_pooling_layer=False).eval()


def load_oracle(tf, sd, depths, prefix="model."):
    """Fill the oracle from a hub-keyed state dict through the rename table; every oracle parameter must be hit."""
    from vdn.hiera_image_encoder import transformers_key
    new = {}
    for k, v in sd.items():
        if not k.startswith(prefix):
            continue
        t = transformers_key(k[len(prefix):], depths)
        if t is not None:
            new[t] = v
    missing = tf.load_state_dict(new, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys


def frames(n):
    from vdn import synth
    return torch.from_numpy(synth.normalize_frames(synth.frames_u8(SEED, n, 224, 224)))


def map_summary(name, t, n):
    """NHWC map or token stream [N, ..., C] -> dn_fixture.summarise on [N, C, positions]."""
    N, C = t.shape[0], t.shape[-1]
    return DF.summarise(name, t.reshape(N, -1, C).permute(0, 2, 1), n)


def index_tables(tf):
    """The oracle's own unroll / reroll on an arange: what the host-side tables of the package must equal."""
    from transformers.models.hiera.modeling_hiera import unroll
    out = {}
    ar = torch.arange(HR.TOKENS, dtype=torch.float32).reshape(1, HR.TOKENS, 1)
    out["unroll"] = unroll(ar, (224, 224), tf.config.patch_stride, tf.unroll_schedule).reshape(-1).long().numpy()
    for s in range(4):
        T = HR.TOKENS >> (2 * s)
        out[f"reroll{s}"] = tf.encoder.reroll(torch.arange(T, dtype=torch.float32).reshape(1, T, 1), s).reshape(-1).long().numpy()
    return out


def gen_trunk(model_name, F, schema=False):
    import vdn
    from vdn.hiera_image_encoder import DEPTHS
    name = f"hiera_{SHORT[model_name]}_f{F}"
    depths = DEPTHS[model_name]
    print(f"[{name}] {model_name} depths={depths} frames={F}")
    enc = vdn.HieraImageEncoder(model_name)
    if schema:
        write_schema(model_name, enc)
    sd = DF.state_dict(enc)
    tf = oracle(depths)
    load_oracle(tf, sd, depths)
    x = frames(F)
    with torch.no_grad():
        ref = list(tf(pixel_values=x, output_hidden_states=True).reshaped_hidden_states[1:])
        hub = {k[len("model."):]: v for k, v in sd.items()}
        maps, taps = HR.forward(hub, x, depths)
        for s, (a, b) in enumerate(zip(maps, ref)):
            assert a.shape == b.shape == (F, 56 >> s, 56 >> s, 96 << s), (a.shape, b.shape)
            err = float((a - b).norm() / b.norm())
            print(f"  stage {s}: restatement vs oracle rel-L2 {err:.2e}")
            assert err < 1e-5, (s, err)
        out = {}
        for s, m in enumerate(ref):
            out.update(map_summary(f"map{s}", m, N_MAP))
        for k, t in taps.items():
            out.update(map_summary(k, t, N_TAP))
        for fault in HR.FAULTS:
            fm, _ = HR.forward(hub, x, depths, fault=fault)
            moves = []
            for s, m in enumerate(fm):
                got = map_summary(f"map{s}", m, N_MAP)
                moves.append(DF.metrics(got, out, f"map{s}")[1])
            print(f"  fault {fault}: mean-removed rel-L2 moves of the four maps {['%.2e' % v for v in moves]}")
            assert max(moves) >= 10 * TOL, (fault, moves)
    tabs = index_tables(tf)
    assert np.array_equal(tabs["unroll"], HR.unroll_index(3).numpy())
    MD.save(os.path.join(GOLD, f"{name}.npz"), meta=np.array([F] + list(depths), np.int64), **out, **tabs)


class OracleTrunk(torch.nn.Module):
    """The reference's HieraImageEncoder with the hub model replaced by its `transformers` port."""

    def __init__(self, model_name="hiera_base_224", finetune=False):
        super().__init__()
        from vdn.hiera_image_encoder import DEPTHS
        self.depths = DEPTHS[model_name]
        self.model = oracle(self.depths)
        self.hub_sd, self.fault = None, None   # set by gen_wrapper: the restatement with a fault stands in for the oracle

    def forward(self, x):
        if self.fault is not None:
            return None, [m.contiguous() for m in HR.forward(self.hub_sd, x.float(), self.depths, fault=self.fault)[0]]
        return None, list(self.model(pixel_values=x, output_hidden_states=True).reshaped_hidden_states[1:])


def gen_wrapper(ref_root, name="dn_model_native", B=1, S=8, seq_len=8, levels=(2, 3)):
    import vdn
    print(f"[{name}] reference wrapper on oracle trunks, B={B} S={S}")
    oracle((1, 1, 1, 1))   # import transformers before the stub torchvision of the reference shims hides the real one from it
    H, M = MD.install(ref_root)
    M.HieraImageEncoder = OracleTrunk
    torch.manual_seed(0)
    model = M.VideoDepthEstimationModel(seq_len, attention_feature_levels=list(levels)).eval()
    ours = vdn.VideoDepthEstimationModel.with_native_trunks(seq_len, attention_feature_levels=list(levels))
    sd = DF.state_dict(ours)
    for t in ("encoder", "img_encoder"):
        load_oracle(getattr(model, t).model, sd, getattr(model, t).depths, prefix=t + ".model.")
    model.head.load_state_dict({k[len("head."):]: v for k, v in sd.items() if k.startswith("head.")}, strict=True)
    depth, img = (torch.from_numpy(t) for t in DF.wrapper_inputs(B, S, 224, 224))
    taps, state = MD.tap_head(model.head)
    with torch.no_grad():
        d, n = model(depth, img)
        state["skip"] = True
        d_s, n_s = model(depth, img)
    ref, sk = DF.summarise_wrapper(d, n), DF.summarise_wrapper(d_s, n_s)
    for lvl in levels:
        ref.update(DF.summarise_tap(taps[lvl], lvl))
        ref[f"tap{lvl}_cond"] = np.array(state["cond"](lvl))
        print(f"  tap{lvl} conditioning {float(ref[f'tap{lvl}_cond']):.2e}")
    for k in ("depth", "dx", "dy"):   # printed only: the head's own fixtures (tools/make_golden_dn.py) pin its attention stacks
        print(f"  {name}:{k} skipping the head's attention moves mean-removed {DF.metrics(sk, ref, k)[1]:.2e}")
    # what this fixture is for: the model's outputs must see the trunks. Each trunk fault, in both trunks, must move the most
    # sensitive checked output by >= 10x the tests' bar.
    state["skip"] = False
    for t in ("encoder", "img_encoder"):
        getattr(model, t).hub_sd = {k[len(t + ".model."):]: v for k, v in sd.items() if k.startswith(t + ".model.")}
    for fault in HR.FAULTS:
        for t in ("encoder", "img_encoder"):
            getattr(model, t).fault = fault
        with torch.no_grad():
            d_f, n_f = model(depth, img)
        fs = DF.summarise_wrapper(d_f, n_f)
        for lvl in levels:   # the processed level maps the test checks as well: the finer view of the trunks
            fs.update(DF.summarise_tap(taps[lvl], lvl))
        moves = [DF.metrics(fs, ref, k)[1] for k in ["depth", "dx", "dy"] + [f"tap{l}" for l in levels]]
        print(f"  {name}: trunk fault {fault} moves depth / dx / dy / taps (mean-removed) {['%.2e' % v for v in moves]}")
        assert max(moves) >= 10 * TOL, (fault, moves)
    MD.save(os.path.join(GOLD, f"{name}.npz"), meta=np.array([B, S, 224, 224, seq_len], np.int64), levels=np.array(levels, np.int64),
            flags=np.array([0, 0, 1, 1, 1], np.int64), **ref)


def main():
    args = sys.argv[1:]
    ref_root = args[0] if args and os.path.isdir(args[0]) else MG.REF
    only = [a for a in args if a in ("trunk", "wrapper")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    if not only or "trunk" in only:
        gen_trunk("hiera_tiny_224", 2, schema=True)
        write_schema("hiera_small_224")   # no trunk fixture of its own: a strict load of the oracle checks its names
        gen_trunk("hiera_base_224", 2, schema=True)
        gen_trunk("hiera_base_224", 8)
    if not only or "wrapper" in only:
        gen_wrapper(ref_root)


def write_schema(model_name, enc=None):
    """Keys and shapes of vdn.HieraImageEncoder(model_name), after a strict load of the oracle through the rename table has
    shown that every trunk parameter has an oracle parameter of the same shape."""
    import vdn
    from vdn.hiera_image_encoder import DEPTHS
    enc = enc or vdn.HieraImageEncoder(model_name)
    load_oracle(oracle(DEPTHS[model_name]), enc.state_dict(), DEPTHS[model_name])
    with open(os.path.join(GOLD, f"schema_hiera_{SHORT[model_name]}.json"), "w") as f:
        json.dump({"params": [[k, list(p.shape)] for k, p in enc.named_parameters()], "buffers": []}, f, indent=0)


if __name__ == "__main__":
    main()
