#!/usr/bin/env python3
"""Time vdn_frame_median at [32, 518 x 518] with device events: the median of 30 timed calls after 10 warm-up calls
(profiles/video_kernel_edges.md). Another build of the library is timed with VDN_LIB=<its libvdn_hip.so>, one process each."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-depth-normal-v2_amd"))

import torch  # noqa: E402


def main():
    from vdn.runtime import Runtime
    rt = Runtime(torch.device("cuda:0"), torch.float16)
    x = (torch.rand(32, 518 * 518, generator=torch.Generator().manual_seed(1)) * 60000.0 + 100.0).cuda()
    med = torch.empty(32, device="cuda")
    for _ in range(10):
        rt.frame_median(x, med)
    torch.cuda.synchronize()
    ts = []
    for _ in range(30):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        rt.frame_median(x, med)
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1000.0)
    ts.sort()
    print(f"vdn_frame_median [32, 518 x 518]: median {statistics.median(ts):.1f} us, min {ts[0]:.1f}, quartiles {ts[7]:.1f} .. {ts[22]:.1f}, "
          f"max {ts[-1]:.1f} (library: {os.environ.get('VDN_LIB', 'this tree')}; sum of medians {float(med.sum()):.3f})")


if __name__ == "__main__":
    main()
