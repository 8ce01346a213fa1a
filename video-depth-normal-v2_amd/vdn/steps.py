"""The bodies of the reference's validate() and evaluate() loops (scripts/train*.py, scripts/evaluate*.py) with nothing
crossing to the host inside them: the batch preparation of vdn.prep, the model, the criteria of vdn.loss and vdn.normals or
the clip metrics of vdn.eval, and meters that accumulate on the device. The scripts call value.item() per loss key and
pred_depths[b].cpu().numpy() per item, a synchronisation each; here the one copy is made by LossMeter.averages() or
MetricMeter.means() when the loop has ended.

    meter = LossMeter()
    for batch in val_loader:
        validate_step(model, batch, depth_criterion, normal_criterion, meter=meter)
    avg_losses = meter.averages()

`model` is any callable: model(input_depth, rgb) -> (depth, normals) as scripts/train.py and evaluate.py call it (with_rgb=True),
or model(input_depth) -> depth as the _v2 .. _v4 scripts do (with_rgb=False). Nothing here knows the engines.

The metric-depth branch (metric_depth/train.py:149-177) has the same loop around vdn.metric: metric_validate_step is its body,
DepthMetricMeter its `results` and `nsamples`.

    meter = DepthMetricMeter()
    for sample in valloader:
        metric_validate_step(model, sample, min_depth=args.min_depth, max_depth=args.max_depth, meter=meter)
    dist.reduce(meter.state(), dst=0)        # as the script reduces its ten tensors
    results = meter.means()"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import prep
from .eval import eval_batch_by_data
from .metric import KEYS as DEPTH_METRIC_KEYS, eval_depth_batch
from .normal_metrics import angular_error


def prepare_batch(batch, *, input_key="depth_anything_v2", normalize_input=False, device="cuda") -> Dict[str, torch.Tensor]:
    """The tensors validate() and evaluate() build from a loader's batch {'rgb' [B, S, 3, H, W], input_key [B, S, 1, H, W],
    'depth' [B, S, 1, H, W], 'mask' [B, S, 1, H, W]}, on the device:
      rgb          [B, S, 3, H, W]  preprocess_rgb_sequences(batch['rgb'])
      input_depth  [B, S, H, W]     preprocess_depth_sequences(batch[input_key], batch['mask'], normalize_input)
      gt           [B, S, H, W]     1. / clamp(batch['depth'], min=1e-8), the inverse depth
      mask         [B, S, H, W]     batch['mask'] in its own dtype
    A host tensor is copied to `device` once."""
    mask = batch["mask"]
    if not isinstance(mask, torch.Tensor) or mask.dim() != 5 or mask.shape[2] != 1:
        raise ValueError(f"batch['mask'] must be [B, S, 1, H, W], got {tuple(getattr(mask, 'shape', ()))}")
    depth = batch["depth"]
    if not isinstance(depth, torch.Tensor) or tuple(depth.shape) != tuple(mask.shape):
        raise ValueError(f"batch['depth'] must be [B, S, 1, H, W] = {tuple(mask.shape)}, got {tuple(getattr(depth, 'shape', ()))}")
    if not mask.is_cuda:
        mask = mask.to(device)
    gt = prep.inverse_depth(depth, device=device)
    return {"rgb": prep.preprocess_rgb_sequences(batch["rgb"], device=device),
            "input_depth": prep.preprocess_depth_sequences(batch[input_key], mask, normalize_input, device=device),
            "gt": gt.squeeze(2), "mask": mask.squeeze(2)}


def _predict(model, t, with_rgb: bool):
    if with_rgb:
        depth, normals = model(t["input_depth"], t["rgb"])
        return depth, normals
    return model(t["input_depth"]), None


class LossMeter:
    """running_losses of validate(), on the device: add() accumulates each key in float64 in call order, averages() divides by
    the number of batches and makes the one copy to the host."""

    def __init__(self):
        self.sums: Dict[str, torch.Tensor] = {}
        self.batches = 0

    def add(self, losses: Dict[str, torch.Tensor]):
        for k, v in losses.items():
            if torch.is_tensor(v):
                v = v.detach().to(torch.float64)
                self.sums[k] = v if k not in self.sums else self.sums[k] + v
        self.batches += 1

    def averages(self) -> Dict[str, float]:
        if not self.sums:
            return {}
        keys = list(self.sums)
        sums = torch.stack([self.sums[k].reshape(()) for k in keys])
        # a tensor divisor: torch turns a division by a Python number into a multiplication by its reciprocal, another rounding
        host = (sums / torch.full_like(sums, float(self.batches))).cpu()
        return dict(zip(keys, host.tolist()))


class MetricMeter:
    """metric_vals of evaluate(), on the device: add() takes the float64 [B, 7] rows of a batch, means() is np.nanmean per
    column over all rows (NaN for a column without a number), computed on the device and copied once. Rows are summed one
    by one in the order they came, as numpy sums the rows of a list."""

    def __init__(self):
        self.sum: Optional[torch.Tensor] = None
        self.count: Optional[torch.Tensor] = None
        self.rows = 0

    def add(self, rows: torch.Tensor):
        if rows.dim() != 2:
            raise ValueError(f"rows must be [B, K], got {tuple(rows.shape)}")
        rows = rows.detach().to(torch.float64)
        nan = torch.isnan(rows)
        clean = torch.where(nan, torch.zeros_like(rows), rows)
        count = (~nan).sum(0)
        if self.sum is None:
            self.sum, self.count = torch.zeros_like(clean[0]), torch.zeros_like(count)
        for b in range(rows.shape[0]):
            self.sum = self.sum + clean[b]
        self.count = self.count + count
        self.rows += rows.shape[0]

    def means(self) -> list:
        if self.sum is None:
            return []
        return (self.sum / self.count.to(torch.float64)).cpu().tolist()


@torch.no_grad()
def validate_step(model, batch, depth_criterion, normal_criterion=None, *, with_rgb=True, meter: Optional[LossMeter] = None,
                  input_key="depth_anything_v2", device="cuda") -> Dict[str, torch.Tensor]:
    """One pass of validate()'s loop body -> the loss dictionary of 0-dim device tensors (the depth criterion's entries, then
    the normal criterion's where one is given), also added to `meter`. The normal criterion scores the predicted normals
    against the normals of the inverse ground-truth depth under the same mask (normal_criterion.forward_from_depth, which
    makes normal_vector(gt) per pixel and never stores it), so it needs with_rgb=True. No host synchronisation."""
    if normal_criterion is not None and not with_rgb:
        raise ValueError("normal_criterion needs the model's normals: with_rgb=True")
    t = prepare_batch(batch, input_key=input_key, device=device)
    depth, normals = _predict(model, t, with_rgb)
    losses = dict(depth_criterion(depth, t["gt"], t["mask"]))
    if normal_criterion is not None:
        losses.update(normal_criterion.forward_from_depth(normals, t["gt"], t["mask"]))
    if meter is not None:
        meter.add(losses)
    return losses


@torch.no_grad()
def evaluate_step(model, batch, *, with_rgb=True, meter: Optional[MetricMeter] = None, domain="disp", dataset_max_depth=70,
                  input_key="depth_anything_v2", device="cuda") -> torch.Tensor:
    """One pass of evaluate()'s loop body -> float64 [B, 7] on the device: per item the seven vdn.eval.eval_metrics of the
    predicted clip against the inverse ground-truth depth with seq_len = S, as the scripts call eval_single_by_data (no mask),
    also added to `meter`. No host synchronisation."""
    t = prepare_batch(batch, input_key=input_key, device=device)
    depth, _ = _predict(model, t, with_rgb)
    rows = eval_batch_by_data(depth, t["gt"], device=device, seq_len=t["gt"].shape[1], domain=domain,
                              dataset_max_depth=dataset_max_depth)
    if meter is not None:
        meter.add(rows)
    return rows


@torch.no_grad()
def evaluate_normals_step(model, batch, *, meter: Optional[MetricMeter] = None, erode=True, input_key="depth_anything_v2",
                          device="cuda") -> torch.Tensor:
    """evaluate_step's body for the normals -> float64 [B, 9] on the device: per item the nine vdn.normal_metrics
    (normal_metric_names: n, mean, median, rmse and the shares under 5 .. 30 degrees) of the normals of model(input_depth, rgb)
    against the normals of the inverse ground-truth depth, made per pixel (from_depth), under the batch's mask (eroded as
    VideoNormalLoss erodes it, unless erode=False); also added to `meter`, a MetricMeter, whose means() are then the NaN-means
    of the columns over the items. An extension: the reference's scripts do not score normals in degrees. No host
    synchronisation."""
    t = prepare_batch(batch, input_key=input_key, device=device)
    _, normals = _predict(model, t, True)
    rows = angular_error(normals, t["gt"], t["mask"], from_depth=True, erode=erode, device=device)["items"]
    if meter is not None:
        meter.add(rows)
    return rows


class DepthMetricMeter:
    """`results` and `nsamples` of metric_depth/train.py:149-177, on the device: a float64 [10] of the sums of the nine
    metrics and the number of items counted. add() takes the [B, 10] rows of vdn.metric.eval_depth_batch (n, then the nine) and
    counts an item only where n >= 10, the script's `if valid_mask.sum() < 10: continue`, decided on the device by torch.where
    with no synchronisation; a skipped item's NaN reaches nothing. Rows are added one by one in the order they came.
    One difference from the script: it accumulates each metric's Python float into a float32 tensor, this meter in float64."""

    MIN_PIXELS = 10

    def __init__(self):
        self.sums: Optional[torch.Tensor] = None

    def add(self, rows: torch.Tensor):
        if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[1] != 1 + len(DEPTH_METRIC_KEYS):
            raise ValueError(f"rows must be [B, {1 + len(DEPTH_METRIC_KEYS)}], got {tuple(getattr(rows, 'shape', ()))}")
        rows = rows.detach().to(torch.float64)
        counted = rows[:, :1] >= self.MIN_PIXELS
        one = torch.ones_like(rows[:, :1])
        terms = torch.where(counted, torch.cat((rows[:, 1:], one), 1), torch.zeros_like(rows))   # the nine, then 1 per item
        if self.sums is None:
            self.sums = torch.zeros_like(terms[0])
        for b in range(terms.shape[0]):
            self.sums = self.sums + terms[b]

    def state(self) -> torch.Tensor:
        """float64 [10] on the device: the sums of d1 .. silog over the counted items, then their number. What a distributed
        run reduces; load_state() takes the reduced tensor back."""
        if self.sums is None:
            raise ValueError("nothing was added")
        return self.sums

    def load_state(self, sums: torch.Tensor):
        if not isinstance(sums, torch.Tensor) or tuple(sums.shape) != (1 + len(DEPTH_METRIC_KEYS),):
            raise ValueError(f"state must be [{1 + len(DEPTH_METRIC_KEYS)}], got {tuple(getattr(sums, 'shape', ()))}")
        self.sums = sums.detach().to(torch.float64)

    def means(self) -> Dict[str, float]:
        """{'d1': ..., 'silog': ...}: each sum over the number of counted items (NaN when none was), with the one copy to the
        host."""
        if self.sums is None:
            return {}
        host = (self.sums[:-1] / self.sums[-1]).cpu().tolist()
        return dict(zip(DEPTH_METRIC_KEYS, host))


@torch.no_grad()
def metric_validate_step(model, sample, *, min_depth, max_depth, meter: Optional[DepthMetricMeter] = None,
                         device="cuda") -> torch.Tensor:
    """One pass of the validation loop's body of metric_depth/train.py:160-177 for sample = {'image' [B, 3, h, w], 'depth'
    [B, H, W], 'valid_mask' [B, H, W]} and any callable model(image) -> [B, h', w'] -> float64 [B, 10] on the device: per item
    the kept pixels and the nine metrics of the prediction, resized to (H, W) with align_corners=True, under (valid_mask == 1)
    & (depth >= min_depth) & (depth <= max_depth) (vdn.metric.eval_depth_batch: the resized prediction and the mask are never
    stored), also added to `meter`. The script runs one item per pass; any B is taken here. No host synchronisation."""
    depth, valid = sample["depth"], sample["valid_mask"]
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
        raise ValueError(f"sample['depth'] must be [B, H, W], got {tuple(getattr(depth, 'shape', ()))}")
    if not isinstance(valid, torch.Tensor) or tuple(valid.shape) != tuple(depth.shape):
        raise ValueError(f"sample['valid_mask'] must be [B, H, W] = {tuple(depth.shape)}, got {tuple(getattr(valid, 'shape', ()))}")
    image = sample["image"]
    if not image.is_cuda:
        image = image.to(device)
    pred = model(image.float())
    rows = eval_depth_batch(pred, depth, valid, min_depth=min_depth, max_depth=max_depth, device=device)
    if meter is not None:
        meter.add(rows)
    return rows
