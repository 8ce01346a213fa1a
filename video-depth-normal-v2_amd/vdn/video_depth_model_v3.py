"""Drop-in for models/video_depth_model_v3.py:128-206 (class name and state-dict keys kept)."""
from .refiner import _DepthRefiner65535


class VideoDepthAnything(_DepthRefiner65535):
    VERSION = 3
    HEAD = "head"
    SCALE_HEAD = "final_scale2"
    NET_HW = None
    FINISH = ("shift", "final_res2")
