"""What the criteria modules (normals, loss, metric, prep, points, eval, vis) share on the way to the device, each written once:
the per-device Runtime cache, the staging rule that turns an input into the tensor a kernel reads, and the gradient gate of the
differentiable criteria. runtime.checked_ptr states the contract of a staged tensor where it becomes a pointer."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import _abi as abi
from .runtime import Runtime

_RUNTIMES: Dict[torch.device, Runtime] = {}


def runtime(device) -> Runtime:
    """The one Runtime (and workspace arena) of a CUDA device, whichever module asks."""
    device = torch.device(device)
    if device.type != "cuda":
        raise abi.VdnError("the vdn criteria run on an MI355X ('cuda' device under ROCm); there is no CPU path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _RUNTIMES:
        _RUNTIMES[device] = Runtime(device)
    return _RUNTIMES[device]


def runtime_for(device, *tensors) -> Runtime:
    """The runtime of the first CUDA tensor among `tensors` (None and numpy arrays are passed over), otherwise of `device`."""
    return runtime(next((t.device for t in tensors if isinstance(t, torch.Tensor) and t.is_cuda), device))


def stage(x, device: torch.device, dtype: torch.dtype) -> torch.Tensor:
    """A torch tensor or numpy array as the contiguous tensor of `dtype` on `device` that a kernel reads. A tensor that is
    there already is used in place (a bool mask viewed as bytes, a view made contiguous); anything else, a tensor on another
    GPU included, is copied once. dtype uint8 is a mask, "non-zero = keep": one that is neither bool nor uint8 becomes != 0."""
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"expected a numpy array or a torch tensor, got {type(x).__name__}")
    if dtype == torch.uint8:
        if t.dtype == torch.bool and t.is_cuda and t.device == device:
            return t.contiguous().view(torch.uint8)
        if t.dtype != torch.uint8:
            t = t != 0
    return t.to(device=device, dtype=dtype).contiguous()


def wants_grad(prediction, target, name: str = "target") -> bool:
    """Does this call record a gradient: gradients enabled and a prediction that requires one. A target that requires one
    raises NotImplementedError (the reference would differentiate it and none of its scripts does)."""
    if not torch.is_grad_enabled():
        return False
    if isinstance(target, torch.Tensor) and target.requires_grad:
        raise NotImplementedError(f"the gradient with respect to {name} is not computed; detach the {name}")
    return isinstance(prediction, torch.Tensor) and prediction.requires_grad
