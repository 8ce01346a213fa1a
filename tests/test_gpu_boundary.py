"""The criteria's Python boundary on the device (vdn._device and runtime.checked_ptr): one Runtime per GPU whichever module asks,
a contract violation that launches nothing, and staging across two GPUs. 4 x 4 frames: no kernel shape matters here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CANARY = -12345.678


def _round():
    """One call each of vdn.normals, vdn.eval, vdn.vis, vdn.loss and vdn.metric on device tensors."""
    from vdn import eval as E, loss, metric, normals, vis
    g = torch.Generator().manual_seed(5)
    depth = (torch.rand(1, 2, 4, 4, generator=g) + 0.5).to(DEV)
    normals.normal_vector(depth[:, :1, None])                                           # [1, 1, 1, 4, 4]
    E.eval_single_by_data(depth[0] * 0.9, depth[0], seq_len=2, dataset_max_depth=70)    # [2, 4, 4]
    vis.colorize(depth[0, :1])                                                          # [1, 4, 4]
    loss.VideoDepthLoss()(depth * 1.1 + 0.05, depth, torch.ones_like(depth))            # [1, 2, 4, 4]
    metric.eval_depth_batch(depth[0, :1] * 1.1, depth[0, :1], torch.ones_like(depth[0, :1]), min_depth=0.1, max_depth=10.0)
    torch.cuda.synchronize()


def test_one_runtime_per_device_across_modules():
    from vdn import _device
    _round()
    mine = [rt for dev, rt in _device._RUNTIMES.items() if dev == DEV]
    assert len(mine) == 1 and list(_device._RUNTIMES).count(DEV) == 1
    assert all(dev.index is not None for dev in _device._RUNTIMES)
    size = mine[0].workspace_bytes()
    assert size > 0
    _round()
    assert _device.runtime(DEV) is mine[0] and mine[0].workspace_bytes() == size


def test_a_wrong_dtype_reaches_no_launch():
    """A float64 prediction handed straight to Runtime.depth_loss: VdnError, and the out it would have written keeps its canary."""
    from vdn import _device
    from vdn._abi import VdnError
    rt = _device.runtime(DEV)
    pred = torch.rand(1, 2, 4, 4, dtype=torch.float64, device=DEV) + 0.5
    target, mask = pred.float() * 1.1, torch.ones(1, 2, 4, 4, dtype=torch.uint8, device=DEV)
    out = torch.full((20,), CANARY, dtype=torch.float64, device=DEV)
    with pytest.raises(VdnError, match=r"depth_loss: prediction: expected .*torch.float32.* got torch.float64 \[1, 2, 4, 4\] on cuda:0"):
        rt.depth_loss(pred, target, mask, out)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    rt.depth_loss(pred.float(), target, mask, out)      # the conforming call does write it
    torch.cuda.synchronize()
    assert not bool((out == CANARY).any())


def test_an_out_one_element_short_reaches_no_launch():
    """refine_scale with an `out` of F * n - 1 elements: the C side would write F * n floats from the pointer."""
    from vdn import _device
    from vdn._abi import VdnError
    rt = _device.runtime(DEV)
    x = torch.rand(2, 4, 4, device=DEV) * 100.0 + 1.0
    med = torch.full((2,), 50.0, device=DEV)
    buf = torch.full((2 * 16 + 8,), CANARY, dtype=torch.float32, device=DEV)
    with pytest.raises(VdnError, match=r"refine_scale: out: expected .* of 32 elements on cuda:0, got torch.float32 \[31\] on cuda:0"):
        rt.refine_scale(x, med, 0.7, -0.2, 1.0, 65535.0, buf[:31])
    torch.cuda.synchronize()
    assert bool((buf == torch.tensor(CANARY, dtype=torch.float32)).all())
    rt.refine_scale(x, med, 0.7, -0.2, 1.0, 65535.0, buf[:32])
    torch.cuda.synchronize()
    canary = torch.tensor(CANARY, dtype=torch.float32, device=DEV)
    assert not bool((buf[:32] == canary).any()) and bool((buf[32:] == canary).all())


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_a_mask_on_another_gpu_is_staged_to_the_predictions():
    """Prediction on device 0, mask on device 1: the values of the call with everything on device 0, bit for bit."""
    from vdn import loss
    g = torch.Generator().manual_seed(6)
    target = (torch.rand(1, 2, 4, 4, generator=g) + 0.5).to(DEV)
    pred = target * 1.1 + 0.05
    mask = (torch.rand(1, 2, 4, 4, generator=g) > 0.2)
    want = loss.depth_loss(pred, target, mask.to(DEV))
    got = loss.depth_loss(pred, target, mask.to(torch.device("cuda", 1)))
    assert want.keys() == got.keys()
    for k, v in want.items():
        same = torch.equal(torch.as_tensor(v).view(-1).view(torch.uint8), torch.as_tensor(got[k]).view(-1).view(torch.uint8)) \
            if isinstance(v, torch.Tensor) else repr(v) == repr(got[k])
        assert same, (k, v, got[k])
