"""metric_depth/ of the reference: DepthAnythingV2(max_depth) on the device, under the reference's module path
(vdn.metric_depth.depth_anything_v2.dpt). Its criterion and scores are vdn.metric, its validation loop's body
vdn.steps.metric_validate_step, its point cloud vdn.points. Importing the model loads libvdn_hip.so."""


def __getattr__(name):
    if name == "DepthAnythingV2":
        from .depth_anything_v2.dpt import DepthAnythingV2
        return DepthAnythingV2
    raise AttributeError(name)
