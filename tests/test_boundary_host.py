"""Host-side checks of the criteria's boundary: runtime.checked_ptr, the contract under which a tensor becomes a pointer, and
vdn._device, the staging rule and the gradient gate the criteria modules share. No GPU: the contract compares devices without a
CUDA call, and staging is exercised with a CPU or meta target device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from common import ROOT

CUDA0 = torch.device("cuda", 0)
CPU = torch.device("cpu")


def test_checked_ptr_returns_the_pointer_of_a_conforming_tensor():
    from vdn.runtime import checked_ptr
    t = torch.zeros(2, 3, 4)
    assert checked_ptr("w: x", t, CPU, torch.float32) == t.data_ptr()
    assert checked_ptr("w: x", t, CPU, torch.float32, (2, 3, 4)) == t.data_ptr()
    assert checked_ptr("w: x", t, CPU, torch.float32, (2, None, 4), count=24) == t.data_ptr()
    assert checked_ptr("w: x", t, CPU, torch.float32, 3) == t.data_ptr()                 # a rank: any [*, *, *]
    assert checked_ptr("w: x", t, CPU, (torch.uint8, torch.float32), count=24) == t.data_ptr()
    assert checked_ptr("w: x", t[1], CPU, torch.float32, (3, 4)) == t.data_ptr() + 48     # a contiguous view: its own pointer
    assert checked_ptr("w: x", None, CPU, torch.float32, (2, 3, 4), optional=True) is None


@pytest.mark.parametrize("case,tensor,kw,says", [
    ("dtype", torch.zeros(2, 3, dtype=torch.float64), dict(shape=(2, 3)), "torch.float64"),
    ("view", torch.zeros(3, 2).t(), dict(shape=(2, 3)), "not contiguous"),
    ("shape", torch.zeros(2, 3), dict(shape=(3, 2)), "[3, 2]"),
    ("rank", torch.zeros(6), dict(shape=(2, None)), "[2, *]"),
    ("rank alone", torch.zeros(2, 3), dict(shape=3), "[*, *, *]"),
    ("count", torch.zeros(2, 3), dict(count=7), "7 elements"),
    ("non-tensor", np.zeros((2, 3), np.float32), dict(shape=(2, 3)), "ndarray"),
    ("required", None, dict(shape=(2, 3)), "NoneType"),
])
def test_checked_ptr_refuses(case, tensor, kw, says):
    from vdn._abi import VdnError
    from vdn.runtime import checked_ptr
    with pytest.raises(VdnError, match="depth_loss: prediction") as e:
        checked_ptr("depth_loss: prediction", tensor, CPU, torch.float32, **kw)
    assert says in str(e.value) and "torch.float32" in str(e.value), str(e.value)


def test_checked_ptr_refuses_another_device_without_a_cuda_call():
    """A CPU tensor against cuda:0, and a meta tensor against the CPU: devices are compared, nothing is initialised."""
    from vdn._abi import VdnError
    from vdn.runtime import checked_ptr
    with pytest.raises(VdnError, match=r"refine_scale: out.*on cuda:0, got torch.float32 \[2, 3\] on cpu"):
        checked_ptr("refine_scale: out", torch.zeros(2, 3), CUDA0, torch.float32, (2, 3))
    with pytest.raises(VdnError, match="on cpu, got .* on meta"):
        checked_ptr("w: x", torch.zeros(2, 3, device="meta"), CPU, torch.float32)


def test_the_contract_survives_python_O():
    """`assert` is compiled away under -O; the contract raises. A fresh interpreter with -O sees the same VdnError."""
    code = ("import torch\n"
            "from vdn._abi import VdnError\n"
            "from vdn.runtime import checked_ptr\n"
            "assert False, 'asserts are off'\n"
            "try:\n"
            "    checked_ptr('depth_loss: prediction', torch.zeros(2, 3, dtype=torch.float64), torch.device('cpu'), torch.float32, (2, 3))\n"
            "except VdnError as e:\n"
            "    print('VdnError:', e)\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "video-depth-normal-v2_amd"))
    out = subprocess.run([sys.executable, "-O", "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("VdnError: depth_loss: prediction: expected a contiguous torch.float32 tensor [2, 3] on cpu"), out.stdout
    assert "got torch.float64 [2, 3] on cpu" in out.stdout


KEEP = np.array([[0, 1, 2], [0, 0, 3]])


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.float32, torch.int64], ids=str)
def test_stage_masks_are_non_zero_keeps(dtype):
    from vdn._device import stage
    want = torch.tensor(KEEP != 0)
    m = stage(torch.from_numpy(KEEP).to(dtype), CPU, torch.uint8)
    assert m.dtype == torch.uint8 and m.is_contiguous() and torch.equal(m != 0, want)
    if dtype != torch.uint8:
        assert torch.equal(m, want.to(torch.uint8))       # 0 / 1 bytes; a uint8 mask is used as it is
    else:
        assert m.data_ptr() == stage(m, CPU, torch.uint8).data_ptr()


def test_stage_takes_numpy_float64_and_views():
    from vdn._device import stage
    x = np.arange(6, dtype=np.float64).reshape(2, 3) / 3.0
    got = stage(x, CPU, torch.float32)
    assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, torch.from_numpy(x).float())
    assert stage(x[:, ::2], CPU, torch.float32).tolist() == torch.from_numpy(x[:, ::2].copy()).float().tolist()
    assert stage(x > 0.5, CPU, torch.uint8).tolist() == (x > 0.5).astype(np.uint8).tolist()
    view = torch.arange(6, dtype=torch.float32).reshape(2, 3).t()
    got = stage(view, CPU, torch.float32)
    assert got.is_contiguous() and torch.equal(got, view) and got.data_ptr() != view.data_ptr()
    same = torch.zeros(2, 3)
    assert stage(same, CPU, torch.float32) is same        # right place, right type: used in place
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        stage([[1.0, 2.0]], CPU, torch.float32)


def test_stage_moves_a_tensor_that_is_elsewhere_to_the_target_device():
    """The two-device rule with the devices a host has: a CPU tensor of the right type staged for `meta` arrives on meta, where
    the rule before kept a tensor wherever it lay; so does a bool mask, which is not reinterpreted where it lies."""
    from vdn._device import stage
    meta = torch.device("meta")
    for x, dtype in ((torch.zeros(2, 3), torch.float32), (torch.zeros(2, 3, dtype=torch.float64).t(), torch.float32),
                     (torch.zeros(2, 3, dtype=torch.bool), torch.uint8), (torch.zeros(2, 3, dtype=torch.uint8), torch.uint8)):
        got = stage(x, meta, dtype)
        assert got.device == meta and got.dtype == dtype and got.is_contiguous() and got.shape == x.shape


def test_one_refusal_for_every_module():
    from vdn import _device
    from vdn._abi import VdnError
    for device in ("cpu", torch.device("cpu")):
        with pytest.raises(VdnError, match="no CPU path"):
            _device.runtime(device)
    with pytest.raises(VdnError, match="no CPU path"):
        _device.runtime_for("cpu", None, np.zeros(3), torch.zeros(3))
    assert _device._RUNTIMES == {} or all(d.type == "cuda" for d in _device._RUNTIMES)


def test_gradient_gate():
    from vdn._device import wants_grad
    p, t = torch.zeros(3, requires_grad=True), torch.zeros(3)
    assert wants_grad(p, t) and not wants_grad(t, t) and not wants_grad(None, None)
    with torch.no_grad():
        assert not wants_grad(p, t) and not wants_grad(p, p)
    with pytest.raises(NotImplementedError, match="with respect to gt_depth is not computed; detach the gt_depth"):
        wants_grad(p, p, "gt_depth")
