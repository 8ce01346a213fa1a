"""Depth + normal model fixtures (tests/golden/dn_*.npz, tools/make_golden_dn.py): inputs, weights and the summaries
both the generator and the tests compute. The full outputs are larger than a committed file may be, so a fixture holds
per-(frame, channel) means plus fixed strided samples; the tests compare samples raw and with their (frame, channel)
mean removed (the synthetic decoder is dominated by its biases: the mean-removed view is where attention shows)."""
import numpy as np
import torch

SEED = 1234
CHANNELS = [96, 192, 384, 768]
SIZES = [(56, 56), (28, 28), (14, 14), (7, 7)]
N_OUT, N_TAP = 16384, 8192


def head_inputs(B, S):
    """Four f32 [B, S, C, h, w] maps at strides 4..32 of a 224 x 224 frame."""
    from vdn import synth
    return [synth.normal(SEED, f"dn_head_feat{l}", (B, S, c, h, w)).astype(np.float32)
            for l, (c, (h, w)) in enumerate(zip(CHANNELS, SIZES))]


def wrapper_inputs(B, S, H, W):
    """Raw depth f32 [B, S, H, W] in (0, 1) and normalised frames f32 [B, S, 3, H, W]."""
    from vdn import synth
    d = synth.depth_clip(SEED, B * S, H, W, max_depth=1.0).reshape(B, S, H, W)
    img = synth.normalize_frames(synth.frames_u8(SEED, B * S, H, W)).reshape(B, S, 3, H, W)
    return d.astype(np.float32), img.astype(np.float32)


def state_dict(model):
    """Synthetic weights keyed by `model`'s own names (the reference's, tests/test_dn_host.py): what the generator loads."""
    from vdn import synth
    sd = {k: torch.from_numpy(synth.synth_param(SEED, k, tuple(p.shape))) for k, p in model.named_parameters()}
    for k, b in model.named_buffers():
        v = synth.synth_buffer(SEED, k, tuple(b.shape))
        sd[k] = torch.from_numpy(np.asarray(v)) if v is not None else b.detach().clone()
    return sd


def _idx(numel, n):
    n = min(n, numel)
    return (np.arange(n, dtype=np.int64) * 2654435761 + 12345) % numel


def summarise(name, t, n=N_OUT):
    """t [F, Cc, n_pix] -> {name_mean [F, Cc], name_idx, name_val} (float64 statistics, float32 values)."""
    t = torch.as_tensor(t).detach().float().cpu()
    F, Cc = t.shape[:2]
    flat = t.reshape(-1)
    idx = _idx(flat.numel(), n)
    return {f"{name}_mean": t.reshape(F, Cc, -1).double().mean(-1).numpy(), f"{name}_idx": idx,
            f"{name}_val": flat[torch.from_numpy(idx)].numpy(), f"{name}_per": np.array(t.shape[2], np.int64)}


def summarise_head(out):
    B, S, C, H, W = out.shape
    return summarise("out", out.reshape(B * S, C, H * W))


def summarise_wrapper(depth, normal, depth_in=None):
    """depth, dx, dy; with depth_in (use_residual) also dres = depth - depth_in, the head's own depth channel, which the
    input depth would otherwise drown."""
    B, S, H, W = depth.shape
    n = normal.reshape(B * S, 3, H * W)
    out = {**summarise("depth", depth.reshape(B * S, 1, H * W)), **summarise("dx", -n[:, 0:1]), **summarise("dy", -n[:, 1:2])}
    if depth_in is not None:
        res = torch.as_tensor(depth).cpu().double() - torch.as_tensor(depth_in).cpu().double()
        out.update(summarise("dres", res.reshape(B * S, 1, H * W)))
    return out


def summarise_tap(t, lvl):
    """The processed level map of the reference, [B, S, C, h, w] -> per frame [C, h*w]."""
    B, S, C, h, w = t.shape
    return summarise(f"tap{lvl}", t.reshape(B * S, C, h * w), N_TAP)


def tokens_as_maps(tok, F, C, hw):
    """Our token rows [(f hw + p), C] -> [F, C, hw] (the layout of summarise_tap)."""
    return tok.reshape(F, hw, C).permute(0, 2, 1)


def flatten(d):
    return dict(d)


def metrics(got, ref, name):
    """(raw rel-L2, mean-removed rel-L2, raw worst pixel, mean-removed worst pixel) of the samples `name` of two
    summaries taken at the same indices; mean-removed = each sample minus its own summary's (frame, channel) mean."""
    idx = np.asarray(ref[f"{name}_idx"])
    assert np.array_equal(np.asarray(got[f"{name}_idx"]), idx)
    fc = idx // int(np.asarray(ref[f"{name}_per"]).reshape(()))
    g, r = np.asarray(got[f"{name}_val"], np.float64), np.asarray(ref[f"{name}_val"], np.float64)
    gc = g - np.asarray(got[f"{name}_mean"], np.float64).reshape(-1)[fc]
    rc = r - np.asarray(ref[f"{name}_mean"], np.float64).reshape(-1)[fc]
    return _rel(g, r), _rel(gc, rc), _worst(g, r), _worst(gc, rc)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _worst(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))
