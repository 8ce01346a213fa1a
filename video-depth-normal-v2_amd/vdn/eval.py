"""Clip evaluation on the device: the reference's eval_depthcrafter.eval.eval_single_by_data and its seven metrics
(AbsRel, delta1, TGM, AbsDiff, RMSE, delta2, delta3 after a least-squares scale/shift alignment), computed by the kernels
of csrc/eval.hip on a clip that can stay in HBM. In scripts/evaluate*.py, replace

    from eval_depthcrafter.eval import eval_metrics, eval_single_by_data
by
    from vdn.eval import eval_metrics, eval_single_by_data
"""
from __future__ import annotations

from typing import List

import torch

from . import _abi as abi
from ._device import runtime as _runtime, runtime_for, stage   # _runtime: the name the GPU tests and tools fetch the runtime by

eval_metrics = [
    "abs_relative_difference",
    "delta1_acc",
    "temporal_gradient_matching_error",
    "abs_difference",
    "rmse_linear",
    "delta2_acc",
    "delta3_acc",
]

_DOMAINS = {"depth": abi.EVAL_DEPTH, "disp": abi.EVAL_DISP}


def _check_clip(pred_disp, gt_disp, seq_len, domain, mask) -> int:
    if domain not in _DOMAINS:
        raise ValueError(f"domain must be 'depth' or 'disp', got {domain!r}")
    if pred_disp.ndim != 3 or gt_disp.ndim != 3:
        raise ValueError(f"pred and gt must be [T, H, W], got {tuple(pred_disp.shape)} and {tuple(gt_disp.shape)}")
    seq_len = min(int(seq_len), pred_disp.shape[0])
    if gt_disp.shape[0] < seq_len:
        raise ValueError(f"gt has {gt_disp.shape[0]} frames, the prediction {seq_len} after truncation")
    if mask is not None and tuple(mask.shape) != tuple(gt_disp.shape):
        raise ValueError(f"mask shape {tuple(mask.shape)} is not gt's {tuple(gt_disp.shape)}")
    if seq_len == 0 or 0 in tuple(pred_disp.shape) or 0 in tuple(gt_disp.shape):
        raise ValueError("empty clip")
    return seq_len


def _clip_launches(rt, pred_disp, gt_disp, mask, seq_len: int, domain, lo: float, hi: float, tgm_over_time: bool, res):
    """The launches of one clip: res float64 [9] on the device <- coef[2] | the seven metrics."""
    dev = rt.device
    pred = stage(pred_disp[:seq_len], dev, torch.float32)
    gt = stage(gt_disp[:seq_len], dev, torch.float32)
    m = None if mask is None else stage(mask[:seq_len], dev, torch.uint8)
    if pred.shape[1:] != gt.shape[1:]:
        resized = torch.empty_like(gt)
        rt.resize_bilinear_hp(pred, resized)
        pred = resized
    rt.eval_fit(pred, gt, m, lo, hi, _DOMAINS[domain], res[:2])
    rt.eval_metrics(pred, gt, m, lo, hi, _DOMAINS[domain], abi.EVAL_TGM_FRAMES if tgm_over_time else abi.EVAL_TGM_ROWS,
                    res[:2], res[2:])


def eval_batch_by_data(pred, gt, device="cuda", seq_len=98, domain="depth", dataset_min_depth=1e-3, dataset_max_depth=70,
                       mask=None, *, tgm_over_time=False) -> torch.Tensor:
    """eval_single_by_data for every item of a batch, left on the device: pred [B, S, h, w], gt [B, S, H, W] and the optional
    mask [B, S, H, W] (numpy arrays or torch tensors) -> float64 [B, 7], row b the seven `eval_metrics` of item b with the bits
    eval_single_by_data(pred[b], gt[b], ..., mask=mask[b]) returns. Per item it makes that function's launches and nothing
    else; nothing is copied to the host and nothing synchronises. An item without a valid pixel gives a row of NaN."""
    if pred.ndim != 4 or gt.ndim != 4:
        raise ValueError(f"pred and gt must be [B, S, H, W], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if pred.shape[0] != gt.shape[0] or pred.shape[0] == 0:
        raise ValueError(f"pred has {pred.shape[0]} items, gt {gt.shape[0]}")
    if mask is not None and tuple(mask.shape) != tuple(gt.shape):
        raise ValueError(f"mask shape {tuple(mask.shape)} is not gt's {tuple(gt.shape)}")
    B = pred.shape[0]
    n = _check_clip(pred[0], gt[0], seq_len, domain, None if mask is None else mask[0])
    rt = runtime_for(device, pred, gt)
    with torch.cuda.device(rt.device):
        res = torch.empty((B, 9), dtype=torch.float64, device=rt.device)   # per item coef[2] | out[7]
        for b in range(B):
            _clip_launches(rt, pred[b], gt[b], None if mask is None else mask[b], n, domain, float(dataset_min_depth),
                           float(dataset_max_depth), tgm_over_time, res[b])
    return res[:, 2:]


def eval_single_by_data(pred_disp, gt_disp, device="cuda", seq_len=98, domain="depth", dataset_min_depth=1e-3,
                        dataset_max_depth=70, mask=None, *, tgm_over_time=False) -> List[float]:
    """The seven `eval_metrics` of a clip, with the reference's signature and semantics.

    pred_disp [T, h, w], gt_disp [T', H, W] and the optional mask [T', H, W] are numpy arrays or torch tensors. CUDA
    tensors are used where they are (the clip need not leave the device); anything else is copied to `device` once.
    Inputs are taken as float32: a float64 gt is rounded to float32 first, where the reference would compare and subtract
    it in float64. The mask is "non-zero = use".

    * Both clips are cut to min(seq_len, T) frames; ValueError if gt (or the mask) has fewer, if the mask's shape is not
      gt's, or for a domain other than 'depth' and 'disp'.
    * A prediction of another size is resized to (H, W), half-pixel bilinear. The reference does this with cv2.resize,
      which is not available to this project's tests: this step alone is parity-unpinned against cv2 (it is checked against
      F.interpolate(mode='bilinear', align_corners=False), the same geometry).
    * Frames without a valid pixel (gt in (min, max) and mask) are dropped.
    * TGM: by default what the reference computes. It hands [T, H, W] tensors to a function written for [B, S, H, W], so
      its "temporal" gradient runs along H inside each frame. tgm_over_time=True gives the metric as metric.py defines it:
      gradients between consecutive kept frames.
    * The three delta accuracies are float32 values, as in the reference. Their mean over the kept frames is summed in
      frame order; torch's CPU sum uses interleaved accumulators, so beyond four kept frames the reference's value can
      differ in the last float32 bit.
    * A clip without any valid pixel: the reference (observed on the CPU, numpy 2.2 / torch 2.10) raises nothing; lstsq
      on the empty system returns, every frame is dropped and all seven metrics are NaN. So here: seven NaN.
    * A kept frame whose TGM mask is empty makes TGM NaN, as in the reference.

    The result is read back with one synchronising copy of the seven values."""
    seq_len = _check_clip(pred_disp, gt_disp, seq_len, domain, mask)
    rt = runtime_for(device, pred_disp, gt_disp)
    with torch.cuda.device(rt.device):
        res = rt.buf("eval_out", (9,), torch.float64)   # coef[2] | out[7]
        _clip_launches(rt, pred_disp, gt_disp, mask, seq_len, domain, float(dataset_min_depth), float(dataset_max_depth),
                       tgm_over_time, res)
        return res[2:].cpu().tolist()
