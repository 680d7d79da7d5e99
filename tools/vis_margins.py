"""Writes profiles/vis_margins.txt: the float32 SSIM model's worst deviation from the float64 model over the GPU test's
cases (tests/vis_ref.py), the tolerance the kernel is held to (4 x that), and what each mutation of the definition deviates
by under the same criterion - the smallest must sit well above the tolerance.  CPU only.
    python tools/vis_margins.py [profiles/vis_margins.txt]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from myslam_amd import _hip, ops       # noqa: E402
from tests import vis_ref as vr        # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vis_margins.txt")
    th, tw = _hip.SSIM_TILE_H, _hip.SSIM_TILE_W
    m = vr.margins(th, tw, ops.load_plasma_lut())
    shapes = ", ".join(f"{h}x{w}" for h, w in vr.ssim_shapes(th, tw))
    lines = [f"SSIM acceptance margins (tests/vis_ref.py; tile {th} x {tw}; shapes {shapes}; C in {vr.CHANNELS};",
             f"inputs {', '.join(vr.INPUT_KINDS)}).  Deviation = the larger of max |map - float64 map| and |mean - float64 mean|,",
             "worst over all cases.", "",
             f"float32 model (kernel's operation order) vs float64 model   {m['model_error']:.3e}",
             f"tolerance of the GPU test ({vr.TOL_FACTOR:g} x the line above)              {m['tolerance']:.3e}", "",
             "mutation of the definition                                  deviation    / tolerance"]
    for name, dev in m["ssim_mutations"].items():
        lines.append(f"  {name:<57} {dev:.3e}    {dev / m['tolerance']:8.1f}")
    small = min(m["ssim_mutations"].values())
    lines += [f"smallest mutation deviation                                 {small:.3e}    {small / m['tolerance']:8.1f}", "",
              "Panel (criterion: bit equality with the float32 model), bytes changed over the panel cases:"]
    for name, n in m["panel_mutations"].items():
        lines.append(f"  {name:<57} {n}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
