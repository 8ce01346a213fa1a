"""The module path metric_depth/run.py:8, train.py:20 and depth_to_pointcloud.py:21 import the model from:
`from depth_anything_v2.dpt import DepthAnythingV2` becomes `from vdn.metric_depth.depth_anything_v2.dpt import DepthAnythingV2`,
and this module offers the same class under the name of the main copy's file."""
from .dpt import DepthAnythingV2

__all__ = ["DepthAnythingV2"]
