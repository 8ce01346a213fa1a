#!/usr/bin/env python3
"""Generate tests/golden/ssim_cases.npz: the IMPORTED reference's loss.loss.DepthShallowSSIMLoss, and its VideoDepthLoss with
ssim_loss_scale = 0.3 whole, on the CPU, value and autograd gradient, each run in float32 (the dtype the scripts run it in)
and in float64, for the seeded cases of CASES at the smallest sizes the library admits (min(H, W) > 160).

pytorch_msssim cannot be installed offline, so its MS_SSIM is restated here as an in-memory module (MS_SSIM below: the
library's algorithm as its documentation and paper give it, all five levels, for any weights) and the reference's own file
is imported on top of it. Parity with the library's file itself is therefore NOT pinned by this fixture; what is pinned is
the reference's code around it (the per-item maximum, the division, the flattening, the composite's alignment and sum).

The inputs are not stored: tests/ssim_ref.py's make_case builds them from integer hashes and exactly rounded operations, so
they are the same bits everywhere; their checksums are stored and the host test compares them. Stored per case: the value in
both precisions, the gradient at SAMPLES hashed positions plus the position of the item maxima in both precisions, the
rel-L2 and the value difference between the two precisions (the yardstick: tests/test_ssim_host.py allows the restatement four
times each), the same for the composite's total_loss and its dictionary; and once the eleven float32 taps. Data only.

Conditions asserted here; a seed that breaks one is to be replaced: every item has a unique maximum among its kept
predictions; 'plain' has its maximum in the prediction when alone; the case named 'gated' has exactly one frame with cs_f <= 0, alone and in the composite.

Usage: python tools/make_golden_ssim.py
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import GOLD, REF, ROOT  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))

#        name      seed  shape               keep    inverse frames   alpha  stable_scale  gain
CASES = (("plain", 11, (1, 2, 161, 164), 0.875, (), 0.5, 10, 1.5),
         ("gated", 12, (2, 2, 163, 161), 0.875, ((0, 1),), 0.5, 10, 1.0),
         ("sparse", 13, (1, 3, 161, 161), 0.5, (), 0.25, 0, 1.0))
SSIM_SCALE = 0.3
SAMPLES = 1024


class MS_SSIM(torch.nn.Module):
    """The library's module restated: Gaussian window 11, sigma 1.5, separable 'valid' filtering along H then W, the cs map
    and the ssim map per level, relu per level, 2 x 2 average pooling (padded by the size's parity) between levels, the
    product of the levels to the power of their weights."""

    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2, weights=None,
                 K=(0.01, 0.03)):
        super().__init__()
        c = torch.arange(win_size, dtype=torch.float) - win_size // 2
        g = torch.exp(-(c ** 2) / (2 * win_sigma ** 2))
        self.win = g / g.sum()
        self.size_average, self.data_range, self.K = size_average, data_range, K
        self.weights = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333] if weights is None else weights

    def _level(self, X, Y):
        win = self.win.to(X.dtype)
        n = win.numel()
        f = lambda z: Fn.conv2d(Fn.conv2d(z, win.view(1, 1, n, 1)), win.view(1, 1, 1, n))
        C1, C2 = (self.K[0] * self.data_range) ** 2, (self.K[1] * self.data_range) ** 2
        mu1, mu2 = f(X), f(Y)
        s1, s2, s12 = f(X * X) - mu1 * mu1, f(Y * Y) - mu2 * mu2, f(X * Y) - mu1 * mu2
        cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
        ssim_map = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs_map
        return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)

    def forward(self, X, Y):
        assert min(X.shape[-2:]) > (self.win.numel() - 1) * 2 ** 4, "image too small for four downsamplings"
        w = X.new_tensor(self.weights)
        vals = []
        for i in range(w.numel()):
            ssim, cs = self._level(X, Y)
            if i < w.numel() - 1:
                vals.append(torch.relu(cs))
                pad = [s % 2 for s in X.shape[2:]]
                X, Y = Fn.avg_pool2d(X, 2, padding=pad), Fn.avg_pool2d(Y, 2, padding=pad)
        vals.append(torch.relu(ssim))
        v = torch.prod(torch.stack(vals, 0) ** w.view(-1, 1, 1), dim=0)
        return v.mean() if self.size_average else v.mean(1)


def main():
    argparse.ArgumentParser(description=__doc__.splitlines()[0]).parse_args()
    sys.path.insert(0, REF)
    m = types.ModuleType("pytorch_msssim")
    m.MS_SSIM = MS_SSIM
    sys.modules["pytorch_msssim"] = m
    from loss.loss import DepthShallowSSIMLoss, VideoDepthLoss
    import ssim_ref as S

    out = {"window": MS_SSIM().win.numpy().copy(), "names": np.array([c[0] for c in CASES]),
           "seeds": np.array([c[1] for c in CASES]), "shapes": np.array([c[2] for c in CASES]),
           "keep": np.array([c[3] for c in CASES]), "alpha": np.array([c[5] for c in CASES], np.float64),
           "stable_scale": np.array([c[6] for c in CASES], np.float64), "ssim_scale": np.array(SSIM_SCALE),
           "gain": np.array([c[7] for c in CASES], np.float64)}
    assert out["window"].dtype == np.float32
    for name, seed, shape, keep, inverse, alpha, ss, gain in CASES:
        c = S.make_case(seed, shape, keep, inverse, gain)
        out[f"{name}_inverse"] = np.array(inverse, np.int64).reshape(-1, 2)
        out[f"{name}_checksum"] = np.array(S.checksum(c))
        n = c["pred"].size
        B = shape[0]
        for b in range(B):
            a, k = c["pred"][b].ravel(), c["mask"][b].ravel()
            assert (a[k] == a[k].max()).sum() == 1, f"{name}: item {b} has two kept predictions at the maximum: replace the seed"
        own = S.ssim_ref(c["pred"], c["target"], c["mask"])
        at = np.unique(np.concatenate(((S._hash01(seed + 77, SAMPLES) * n).astype(np.int64),
                                       own["index"] + np.arange(B) * (n // B))))
        out[f"{name}_at"] = at
        for what in ("alone", "whole"):
            res = {}
            for dt in (torch.float32, torch.float64):
                p = torch.from_numpy(c["pred"].copy()).to(dt).requires_grad_()
                t, k = torch.from_numpy(c["target"].copy()).to(dt), torch.from_numpy(c["mask"].copy())
                if what == "alone":
                    v = DepthShallowSSIMLoss()(p, t, k.to(dt))
                    d = {"ssim_loss": v}
                else:
                    # the reference casts its mask with .float(), which pins its per-frame statistics to float32: for the
                    # float64 run that one cast is redirected to double, nothing else
                    to_float = torch.Tensor.float
                    if dt == torch.float64:
                        torch.Tensor.float = lambda self: self.double()
                    try:
                        d = VideoDepthLoss(alpha=alpha, stable_scale=ss, ssim_loss_scale=SSIM_SCALE)(p, t, k)
                    finally:
                        torch.Tensor.float = to_float
                    v = d["total_loss"]
                    out[f"{name}_whole_keys"] = np.array(list(d))
                v.backward()
                assert torch.isfinite(p.grad).all()
                res[dt] = (float(v), p.grad.numpy().astype(np.float64).ravel(), np.array([float(x) for x in d.values()]))
            (v32, g32, d32), (v64, g64, d64) = res[torch.float32], res[torch.float64]
            rel = float(np.sqrt(((g32 - g64) ** 2).sum() / (g64 ** 2).sum()))
            print(f"{name} {what}: value f32 {v32:.9f} f64 {v64:.12f} diff {abs(v32 - v64):.2e}; gradient rel-L2 f32 vs f64 {rel:.2e}; "
                  f"|g| max {np.abs(g64).max():.3g} median {np.median(np.abs(g64)):.3g}")
            out[f"{name}_{what}_value"] = np.array([v32, v64])
            out[f"{name}_{what}_dict"] = np.stack((d32, d64))
            out[f"{name}_{what}_grad32"] = g32[at].astype(np.float32)
            out[f"{name}_{what}_grad64"] = g64[at]
            out[f"{name}_{what}_norm"] = np.array([np.sqrt((g32 ** 2).sum()), np.sqrt((g64 ** 2).sum())])
            out[f"{name}_{what}_yardstick"] = np.array([abs(v32 - v64), rel])
        print(f"{name}: restatement cs {own['cs'].ravel()}, holder {own['holder']}, gated {own['gated']}, "
              f"value vs the reference's float64 run {abs(own['loss'] - out[name + '_alone_value'][1]):.2e}")
        assert own["gated"] == len(inverse), f"{name}: {own['gated']} gated frames"
        assert name != "plain" or own["holder"][0] == 0, "plain: the prediction does not hold the maximum"
        fit = S.R.fit_ref(c["pred"], c["target"], c["mask"])
        assert S.ssim_ref(c["pred"], c["target"], c["mask"], fit)["gated"] == len(inverse), f"{name}: gating changes under the fit"
    path = os.path.join(GOLD, "ssim_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
