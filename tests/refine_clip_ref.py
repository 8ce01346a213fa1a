"""CPU restatement of the depth refiners' windowed clip driver (`refine_video_depth`): the loop of the reference's
`infer_video_depth` (models/video_depth_model_v5.py:215-283, the same text in v2 .. v4) on DEPTH windows, built from pieces the
tests can run without the reference: `vdn.util.window_table`, the per-window forward restatements (oracle.ref_cpu.
depth_refiner_forward for v4 / v5, tests/refiner_ref.refiner23_forward for v2 / v3) and `vdn.util.stitch`.
tools/make_golden_refine_clip.py holds it to <= 1e-5 of the imported reference's halves before it writes a fixture; the
fixtures are RC5_vits, RC3_vits and RC2_vits."""
import os
from functools import lru_cache

import numpy as np
import torch

import refiner_ref as R
from common import GOLD, synth_sd

# fixture -> (version, schema of its synthetic state dict, the head bias the tool shifted so that the stitcher's clamp acts)
FIXTURES = {"RC5_vits": (5, "R5", "shift_head.0.bias"), "RC3_vits": (3, "R3", "final_res2.0.bias"), "RC2_vits": (2, "R2", None)}
ZERO_SHARE = (0.005, 0.5)   # exact zeros among the frames >= 32 of a v3 / v5 fixture: the clamp acts, and not everywhere
RELU_SHARE = (0.05, 0.95)   # v2: what each ReLU of final_res clips (the conditions of R2_vits)
RAW = 24                    # the frames in front of the first cross-fade are window 0's outputs as `forward` gave them
# RC2's final_res scalars: R2_FINAL_RES leaves the second ReLU 6 % / 3 % / 2 % of the three windows of this 50-frame clip (its
# later frames are brighter than R2's three), below the 5 % the condition asks. A first BatchNorm bias of 0 instead of -0.3
# lets more of the first ReLU through: it clips 31 % / 39 % / 41 %, the second 16 % / 8 % / 8 %. (A lower SECOND bias does it
# too, but halves the output's range, 0.53 -> 0.28, under the same absolute error of the network's depth.)
RC2_FINAL_RES = dict(R.R2_FINAL_RES, **{"final_res.1.bias": [0.0]})


def window_forward(sd, x, enc: str, version: int, trace=None):
    """One window x [1,32,H,W] through the version's forward restatement -> [1,32,H,W]."""
    from oracle import ref_cpu as O
    with torch.no_grad():
        if version in (2, 3):
            return R.refiner23_forward(sd, x, enc, version=version, trace=trace)
        return O.depth_refiner_forward(sd, x, enc, version=version, trace=trace)


def restate(sd, clip: np.ndarray, enc: str, version: int, traces=None):
    """clip f32 [N,H,W] -> (stitched f32 [N,H,W], the per-window outputs [windows,32,H,W]); `traces` collects one dict per
    window."""
    from vdn import util
    x = torch.from_numpy(np.ascontiguousarray(clip, dtype=np.float32))
    per_window = []
    for idxs in util.window_table(x.shape[0]):
        tr = {} if traces is not None else None
        per_window.append(window_forward(sd, x[torch.tensor(idxs)][None], enc, version, tr)[0].numpy())
        if traces is not None:
            traces.append(tr)
    frames = [w[i] for w in per_window for i in range(util.INFER_LEN)]
    return util.stitch(frames, x.shape[0]).astype(np.float32), np.stack(per_window)


@lru_cache(maxsize=None)
def fixture(name: str):
    """-> (npz, version, clip f32 [N,H,W], state dict the fixture was made with)."""
    from vdn import synth
    version, schema, _ = FIXTURES[name]
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    v, N, H, W, seed = [int(t) for t in g["meta"]]
    assert v == version
    sd = R.r2_state_dict(g, synth_sd(schema, "vits"))   # the "sd/<key>" entries replace the synthetic draw's
    return g, version, synth.depth_clip(seed, N, H, W), sd


def zero_share(out: np.ndarray, first: int = 32) -> float:
    return float((out[first:] == 0).mean())
