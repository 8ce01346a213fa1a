#!/usr/bin/env python3
"""Generate tests/golden/prep_cases.npz: what the reference's own batch-preparation functions give for the seeded cases of
tests/prep_ref.py (CASES, make_case), run on the CPU in float32.

The functions are taken from the eight scripts (scripts/train.py, train_v2.py .. train_v4.py, evaluate.py, evaluate_v2.py ..
evaluate_v4.py) at generation time: each file is parsed, the definitions of preprocess_rgb_sequences,
preprocess_rgb_viz_sequences and preprocess_depth_sequences (and the batch_wise_min_max_norm nested in the last) are compiled
out of its syntax tree and nothing else of the file is run. The names they use are supplied here:
  torch                    the installed one
  transforms               a stand-in with Lambda, Compose and Normalize; torchvision is not required. Normalize is written as
                           torchvision's: tensor.clone(), then sub_(mean[:, None, None]).div_(std[:, None, None]) on float32
  IMAGENET_DEFAULT_MEAN / IMAGENET_DEFAULT_STD   timm's two tuples (timm is not required)
  INPUT_SIZE               the case's side: the scripts' final .view forces square frames, so every case is square
The ground-truth line `1. / torch.clamp(gt_depths, min=1e-8)` is an expression inside the scripts' loops; it is written here
as the scripts write it.

The file is written only if (1) every script that defines a function gives the same array for every case, and (2) the numpy
restatement tests/prep_ref.py equals it under np.array_equal(..., equal_nan=True), which is numeric equality and does not
compare the sign of a zero. It holds seeds, shapes, flags, input checksums and the expected arrays, under 200 KB.

Usage: python tools/make_golden_prep.py
"""
from __future__ import annotations

import ast
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import GOLD, REF, ROOT  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))

SCRIPTS = ["train.py", "train_v2.py", "train_v3.py", "train_v4.py", "evaluate.py", "evaluate_v2.py", "evaluate_v3.py",
           "evaluate_v4.py"]
NAMES = ("preprocess_rgb_sequences", "preprocess_rgb_viz_sequences", "preprocess_depth_sequences")
NESTED = "batch_wise_min_max_norm"
MAX_BYTES = 200 * 1000


class _Transforms:
    class Lambda:
        def __init__(self, fn):
            self.fn = fn

        def __call__(self, x):
            return self.fn(x)

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

        def __call__(self, tensor):
            assert tensor.dtype == torch.float32
            tensor = tensor.clone()
            mean = torch.as_tensor(self.mean, dtype=tensor.dtype)
            std = torch.as_tensor(self.std, dtype=tensor.dtype)
            return tensor.sub_(mean.view(-1, 1, 1)).div_(std.view(-1, 1, 1))


def load_functions(path: str) -> dict:
    """The named definitions of one script, compiled alone -> {name: function} over a namespace whose INPUT_SIZE the caller
    sets through ns['INPUT_SIZE']."""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    for n in list(defs):
        if n.name == "preprocess_depth_sequences":
            nested = [m for m in n.body if isinstance(m, ast.FunctionDef) and m.name == NESTED]
            assert len(nested) == 1, f"{path}: no nested {NESTED}"
            defs.append(nested[0])
    ns = dict(torch=torch, transforms=_Transforms, INPUT_SIZE=None,
              IMAGENET_DEFAULT_MEAN=(0.485, 0.456, 0.406), IMAGENET_DEFAULT_STD=(0.229, 0.224, 0.225))
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    fns = {n.name: ns[n.name] for n in defs}
    fns["__ns__"] = ns
    return fns


def run_reference(fns: dict, c: dict, case: dict):
    """The case through one script's functions, or None when the script does not define what the case needs."""
    need = {"rgb": NAMES[0], "viz": NAMES[1], "bwn": NESTED, "inv": None}.get(c["op"], NAMES[2])
    if need is not None and need not in fns:
        return None
    fns["__ns__"]["INPUT_SIZE"] = c["shape"][-1]
    x = torch.from_numpy(case["x"].copy())
    m = None if case["mask"] is None else torch.from_numpy(case["mask"] != 0)   # torch.where takes a bool condition
    with torch.no_grad():
        if c["op"] in ("rgb", "viz"):
            out = fns[need](x)
        elif c["op"] == "pre":
            out = fns[need](x, m, c["norm"])
        elif c["op"] == "bwn":
            out = fns[need](x.squeeze(2), None if m is None else m.squeeze(2))
        elif c["op"] == "inv":
            out = 1. / torch.clamp(x, min=1e-8)
        else:
            out = fns[need](1. / torch.clamp(x, min=1e-8), m, c["norm"])
    assert out.dtype == torch.float32
    return out.numpy()


def main():
    import prep_ref as R
    scripts = {s: load_functions(os.path.join(REF, "scripts", s)) for s in SCRIPTS}
    for s, fns in scripts.items():
        print(f"{s}: {sorted(k for k in fns if k != '__ns__')}")
    assert all(NAMES[0] in f and NAMES[2] in f and NESTED in f for f in scripts.values())
    out = dict(op=[], seed=[], shape=[], mask=[], special=[], norm=[], checksum=[])
    for i, c in enumerate(R.CASES):
        assert c["shape"][-1] == c["shape"][-2], "the reference's view forces square frames"
        case = R.make_case(c)
        got = {s: run_reference(f, c, case) for s, f in scripts.items()}
        got = {s: g for s, g in got.items() if g is not None}
        assert len(got) >= 4, (c, sorted(got))
        first = next(iter(got.values()))
        for s, g in got.items():
            if not (g.shape == first.shape and np.array_equal(g, first, equal_nan=True)):
                raise SystemExit(f"REFUSED: case {i} {c}: {s} disagrees with the other scripts")
        mine = R.restate(c, case)
        if not (mine.shape == first.shape and mine.dtype == np.float32 and np.array_equal(mine, first, equal_nan=True)):
            bad = int((~((mine == first) | (np.isnan(mine) & np.isnan(first)))).sum()) if mine.shape == first.shape else -1
            raise SystemExit(f"REFUSED: case {i} {c}: tests/prep_ref.py differs from the reference at {bad} elements")
        print(f"case {i:2d} {c['op']:6s} {c['special']:14s} {c['shape']} mask={c['mask']:5s} norm={int(c['norm'])}: "
              f"{len(got)} scripts agree, restatement equal; nan={int(np.isnan(first).sum())}")
        for k in ("op", "seed", "mask", "special", "norm"):
            out[k].append(c[k])
        out["shape"].append(c["shape"])
        out["checksum"].append(R.checksum(case))
        out[f"exp{i}"] = first
    arrays = {k: np.asarray(v) for k, v in out.items()}
    path = os.path.join(GOLD, "prep_cases.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, size
    print(f"wrote {path}: {size} bytes, {len(R.CASES)} cases")


if __name__ == "__main__":
    main()
