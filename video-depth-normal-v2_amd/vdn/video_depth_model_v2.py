"""Drop-in for models/video_depth_model_v2.py:37-100 (class name and state-dict keys kept)."""
from .refiner import _DepthRefiner65535


class VideoDepthAnything(_DepthRefiner65535):
    VERSION = 2
    HEAD = "head"
    SCALE_HEAD = None
    NET_HW = None
    FINISH = ("mix", "final_res")
