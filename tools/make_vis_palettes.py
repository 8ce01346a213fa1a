"""Write the three palettes of vdn.vis from matplotlib, once: video-depth-normal-v2_amd/vdn/_palettes.py (uint8 literals; the
package never imports matplotlib) and tests/golden/vis_palettes.npz (what tests/vis_ref.py reads).

    python tools/make_vis_palettes.py

The expressions are the reference's own, truncation included (an entry of 93.99999 is 93):
  Spectral_r  run.py:50,65 / run_video.py:43,81     (cmap(uint8)[:, :3] * 255).astype(uint8), reversed to BGR by the caller
  Spectral    metric_depth/run.py:53,72              the same expression
  inferno     utils/dc_utils.py:75,80                (np.array(cmap.colors) * 255).astype(uint8), RGB
Generated with matplotlib 3.10.8; tests/test_vis_host.py compares against whatever matplotlib is importable."""
from __future__ import annotations

import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("Spectral_r", "Spectral", "inferno")


def tables():
    import matplotlib
    idx = np.arange(256, dtype=np.uint8)
    out = {n: (matplotlib.colormaps.get_cmap(n)(idx)[:, :3] * 255).astype(np.uint8) for n in ("Spectral_r", "Spectral")}
    out["inferno"] = (np.array(matplotlib.colormaps.get_cmap("inferno").colors) * 255).astype(np.uint8)
    for n, t in out.items():
        assert t.shape == (256, 3) and t.dtype == np.uint8, (n, t.shape, t.dtype)
    return out, matplotlib.__version__


def main():
    tabs, version = tables()
    np.savez(os.path.join(ROOT, "tests", "golden", "vis_palettes.npz"), **tabs)
    lines = ['"""The palettes of vdn.vis as uint8 [256][3] RGB literals, written by tools/make_vis_palettes.py (matplotlib '
             f'{version}).\nTruncation is part of each table; do not edit by hand."""', "", "PALETTES = {"]
    for n in NAMES:
        lines.append(f'    "{n}": (')
        flat = tabs[n].reshape(-1)
        for i in range(0, 768, 24):   # 8 entries per line
            lines.append("        " + " ".join(f"{v}," for v in flat[i:i + 24]))
        lines.append("    ),")
    lines.append("}")
    with open(os.path.join(ROOT, "video-depth-normal-v2_amd", "vdn", "_palettes.py"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
