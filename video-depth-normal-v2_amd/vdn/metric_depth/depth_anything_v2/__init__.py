"""metric_depth/depth_anything_v2 of the reference: the metric-depth model (dpt.py)."""
