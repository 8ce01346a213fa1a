"""vdn — MI355X-native per-frame depth inference behind the Depth-Anything-V2 / Video-Depth-Anything API.

Importing the model classes loads libvdn_hip.so (hand-written gfx950 kernels); there is no CPU path.
`from vdn import synth, util, modules` stay importable without the library (host logic only)."""

MODEL_CONFIGS = {
    "vits": {"encoder": "vits", "features": 64, "out_channels": [48, 96, 192, 384]},
    "vitb": {"encoder": "vitb", "features": 128, "out_channels": [96, 192, 384, 768]},
    "vitl": {"encoder": "vitl", "features": 256, "out_channels": [256, 512, 1024, 1024]},
    "vitg": {"encoder": "vitg", "features": 384, "out_channels": [1536, 1536, 1536, 1536]},   # DepthAnythingV2 only (run_video.py:32)
}


def __getattr__(name):
    if name == "DepthAnythingV2":
        from .depth_anything_v2 import DepthAnythingV2
        return DepthAnythingV2
    if name == "VideoDepthAnything":
        from .video_depth import VideoDepthAnything
        return VideoDepthAnything
    if name == "VideoDepthAnythingHeadV2":
        from .video_depth_head_v2_sangyu import VideoDepthAnythingHeadV2
        return VideoDepthAnythingHeadV2
    if name == "HieraImageEncoder":
        from .hiera_image_encoder import HieraImageEncoder
        return HieraImageEncoder
    if name == "VideoDepthEstimationModel":
        from .video_depth_model import VideoDepthEstimationModel
        return VideoDepthEstimationModel
    if name == "eval":   # clip evaluation metrics on the device (vdn/eval.py)
        import importlib
        return importlib.import_module(".eval", __name__)
    if name == "vis":    # the front ends' colourised depth output on the device (vdn/vis.py)
        import importlib
        return importlib.import_module(".vis", __name__)
    if name == "normals":  # normal_vector and VideoNormalLoss on the device (vdn/normals.py)
        import importlib
        return importlib.import_module(".normals", __name__)
    if name == "normal_metrics":  # angular-error statistics of predicted normals on the device (vdn/normal_metrics.py)
        import importlib
        return importlib.import_module(".normal_metrics", __name__)
    if name == "loss":   # VideoDepthLoss on the device (vdn/loss.py)
        import importlib
        return importlib.import_module(".loss", __name__)
    if name == "prep":   # the scripts' batch preparation on the device (vdn/prep.py)
        import importlib
        return importlib.import_module(".prep", __name__)
    if name == "metric":  # SiLogLoss and eval_depth's nine metrics of the metric-depth branch on the device (vdn/metric.py)
        import importlib
        return importlib.import_module(".metric", __name__)
    if name == "metric_depth":  # the metric-depth model, DepthAnythingV2(max_depth), under the reference's module path (vdn/metric_depth/)
        import importlib
        return importlib.import_module(".metric_depth", __name__)
    if name == "points":  # the point cloud of a metric depth map on the device (vdn/points.py)
        import importlib
        return importlib.import_module(".points", __name__)
    if name == "steps":  # the bodies of the scripts' validate and evaluate loops, without host synchronisation (vdn/steps.py)
        import importlib
        return importlib.import_module(".steps", __name__)
    raise AttributeError(name)
