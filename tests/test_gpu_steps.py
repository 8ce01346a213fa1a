"""The loop bodies of vdn.steps on the device, with a stub model: prepare_batch against the four calls of vdn.prep,
validate_step + LossMeter against the criteria called directly and summed on the host as the scripts' validate() does, and
evaluate_step + MetricMeter against eval_single_by_data per item and np.nanmean, as the scripts' evaluate() does.

Bars. The steps make the launches of the direct calls on the same tensors, and the kernels are deterministic, so values are
compared by their bytes. LossMeter adds the float32 losses in float64 in call order and divides once, which is what
`running += value.item()` and `running / len(loader)` do on the host: the same bits. MetricMeter.means() sums the rows one by
one, as numpy sums the rows of a list; the issue allows it 1 ulp of float64.

No call inside a step may synchronise with the host: torch.Tensor.item, .cpu and .tolist are wrapped to count, and the count
must be zero until averages() / means() makes its one copy."""
from __future__ import annotations

import contextlib
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, S, H, W = 2, 3, 17, 13


class Stub(torch.nn.Module):
    """depth -> a * depth + b and a fixed normal field; model(depth, rgb) -> (depth, normals), model(depth) -> depth."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor(0.75))
        self.b = torch.nn.Parameter(torch.tensor(0.125))
        g = torch.Generator().manual_seed(5)
        self.register_buffer("normals", torch.randn(B, S, 3, H, W, generator=g))

    def forward(self, depth, rgb=None):
        out = self.a * depth + self.b
        if rgb is None:
            return out
        assert tuple(rgb.shape) == (B, S, 3, H, W) and rgb.dtype == torch.float32
        return out, self.normals


def make_batch(seed: int, on_device: bool = True, dead_item=None) -> dict:
    rng = np.random.default_rng(seed)
    batch = {"rgb": rng.uniform(-0.2, 1.2, (B, S, 3, H, W)).astype(np.float32),
             "depth_anything_v2": rng.uniform(-1.0, 10.0, (B, S, 1, H, W)).astype(np.float32),
             "depth": rng.uniform(0.5, 20.0, (B, S, 1, H, W)).astype(np.float32),
             "mask": rng.random((B, S, 1, H, W)) < 0.8}
    if dead_item is not None:
        batch["depth"][dead_item] = 1e-9            # inverse depth 1e8, outside (1e-3, 70): no valid pixel in the item
    return {k: torch.from_numpy(v).to(DEV) if on_device else torch.from_numpy(v) for k, v in batch.items()}


def same_bits(a, b):
    a, b = (x.detach().cpu().numpy() for x in (a, b))
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@contextlib.contextmanager
def count_syncs():
    """Counts the calls of torch.Tensor.item / .cpu / .tolist made while it is open."""
    calls = {"item": 0, "cpu": 0, "tolist": 0}
    saved = {k: getattr(torch.Tensor, k) for k in calls}

    def wrap(name):
        def counted(self, *a, **kw):
            calls[name] += 1
            return saved[name](self, *a, **kw)
        return counted

    for k in calls:
        setattr(torch.Tensor, k, wrap(k))
    try:
        yield calls
    finally:
        for k, v in saved.items():
            setattr(torch.Tensor, k, v)


@pytest.mark.parametrize("on_device", [True, False], ids=["device-batch", "host-batch"])
def test_prepare_batch_equals_the_prep_calls(on_device):
    from vdn import prep, steps
    batch = make_batch(1, on_device)
    with count_syncs() as calls:
        t = steps.prepare_batch(batch)
        tn = steps.prepare_batch(batch, normalize_input=True)
    assert sum(calls.values()) == 0
    assert set(t) == {"rgb", "input_depth", "gt", "mask"}
    assert all(v.is_cuda for v in t.values())
    same_bits(t["rgb"], prep.preprocess_rgb_sequences(batch["rgb"]))
    same_bits(t["input_depth"], prep.preprocess_depth_sequences(batch["depth_anything_v2"], batch["mask"], False))
    same_bits(tn["input_depth"], prep.preprocess_depth_sequences(batch["depth_anything_v2"], batch["mask"], True))
    same_bits(t["gt"], prep.inverse_depth(batch["depth"]).squeeze(2))
    same_bits(t["mask"], batch["mask"].squeeze(2))
    assert tuple(t["input_depth"].shape) == tuple(t["gt"].shape) == tuple(t["mask"].shape) == (B, S, H, W)
    other = dict(batch, other=batch["depth"])
    same_bits(steps.prepare_batch(other, input_key="other")["input_depth"],
              prep.preprocess_depth_sequences(batch["depth"], batch["mask"], False))


@pytest.mark.parametrize("with_rgb", [True, False], ids=["depth+normals", "depth-only"])
def test_validate_step_and_loss_meter(with_rgb):
    from vdn import prep, steps
    from vdn.loss import VideoDepthLoss
    from vdn.normals import VideoNormalLoss, normal_vector
    model = Stub().to(DEV).eval()
    depth_criterion = VideoDepthLoss()
    normal_criterion = VideoNormalLoss() if with_rgb else None
    batches = [make_batch(10 + i) for i in range(3)]
    meter = steps.LossMeter()
    with count_syncs() as calls:
        for batch in batches:
            losses = steps.validate_step(model, batch, depth_criterion, normal_criterion, with_rgb=with_rgb, meter=meter)
            assert all(v.is_cuda and v.dim() == 0 and not v.requires_grad for v in losses.values())
        assert sum(calls.values()) == 0, calls           # nothing crossed to the host inside the steps
        got = meter.averages()
        assert calls["cpu"] == 1 and calls["item"] == 0, calls  # the one copy
    keys = list(depth_criterion.keys) + (["normal_loss"] if with_rgb else [])
    assert list(got) == keys and list(losses) == keys
    # the scripts' loop body, with the prep functions and the criteria called directly and the sums kept on the host
    running = {}
    with torch.no_grad():
        for batch in batches:
            rgbs = prep.preprocess_rgb_sequences(batch["rgb"])
            masks = batch["mask"]
            input_depths = prep.preprocess_depth_sequences(batch["depth_anything_v2"], masks, False)
            gt_depths = prep.inverse_depth(batch["depth"])
            if with_rgb:
                gt_normals = normal_vector(gt_depths)
                pred_depths, pred_normals = model(input_depths, rgbs)
            else:
                pred_depths = model(input_depths)
            loss_dict = dict(depth_criterion(pred_depths, gt_depths.squeeze(2), masks.squeeze(2)))
            if with_rgb:
                from_depth = normal_criterion.forward_from_depth(pred_normals, gt_depths, masks.squeeze(2))
                stored = normal_criterion(pred_normals, gt_normals, masks.squeeze(2))
                # the step scores against normal_vector(gt) made per pixel in fp64 and never stored (train.py:306-312 stores
                # it in float32 first): the two agree to float32 rounding of the stored normals
                assert abs(from_depth["normal_loss"].item() - stored["normal_loss"].item()) < 1e-5
                loss_dict.update(from_depth)
            for k, v in loss_dict.items():
                running[k] = running.get(k, 0.0) + v.item()
    want = {k: v / len(batches) for k, v in running.items()}
    for k in keys:
        print(f"{k}: {got[k]!r} vs {want[k]!r}")
        assert struct.pack("<d", got[k]) == struct.pack("<d", want[k]), k


def test_evaluate_step_and_metric_meter():
    from vdn import steps
    from vdn.eval import eval_single_by_data
    model = Stub().to(DEV).eval()
    batches = [make_batch(20), make_batch(21, dead_item=1), make_batch(22)]
    meter = steps.MetricMeter()
    rows = []
    with count_syncs() as calls:
        for batch in batches:
            r = steps.evaluate_step(model, batch, meter=meter)
            assert r.is_cuda and r.dtype == torch.float64 and tuple(r.shape) == (B, 7)
            rows.append(r)
        assert sum(calls.values()) == 0, calls
        got = meter.means()
        assert calls["cpu"] == 1 and calls["item"] == 0, calls
    rows = torch.cat(rows).cpu().numpy()
    want_rows = []
    with torch.no_grad():
        for batch in batches:
            t = steps.prepare_batch(batch)
            pred_depths, _ = model(t["input_depth"], t["rgb"])
            for b in range(B):
                want_rows.append(eval_single_by_data(pred_depths[b], t["gt"][b], device=DEV, seq_len=S, domain="disp",
                                                     dataset_max_depth=70))
    want_rows = np.array(want_rows, np.float64)
    assert np.isnan(want_rows[3]).all() and not np.isnan(np.delete(want_rows, 3, 0)).any()    # the item with no valid pixel
    assert np.array_equal(rows, want_rows, equal_nan=True)
    ok = ~np.isnan(want_rows)
    assert rows[ok].tobytes() == want_rows[ok].tobytes()                                       # bit for bit
    want = np.nanmean(want_rows, axis=0)
    assert len(got) == 7 and meter.rows == 3 * B
    for g, w in zip(got, want):
        print(f"{g!r} vs {w!r}")
        assert abs(g - w) <= np.spacing(abs(w))
    same_bits(steps.evaluate_step(lambda d: model(d), batches[0], with_rgb=False), torch.from_numpy(rows[:B]).to(DEV))
    empty = steps.MetricMeter()
    empty.add(torch.full((2, 7), float("nan"), dtype=torch.float64, device=DEV))
    assert np.isnan(empty.means()).all()                                                       # np.nanmean of no number
