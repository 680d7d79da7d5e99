#!/usr/bin/env python3
"""Generate tests/golden/viewer_reference.npz by running the REFERENCE's src/tools/visualizer_util.py (build container only).

The reference's module is loaded in place, with a stand-in for open3d that records what the module hands it: the points
and the colour of the point clouds create_camera_actor builds, and the extrinsic draw_trajectory gives the view control.
Only those inputs and outputs are stored, no reference code:
  scales [2], actor_points [2,1200,3], color_est [3], color_gt [3]    create_camera_actor (visualizer_util.py:36-61)
  init_poses [3,4,4], extrinsics [3,4,4], point_size, back_face        draw_trajectory (visualizer_util.py:178-198)
"""
import os
import sys
import types
from types import SimpleNamespace

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "viewer_reference.npz")
sys.dont_write_bytecode = True

seen = SimpleNamespace(extrinsic=None, options=SimpleNamespace())


class PointCloud:
    def __init__(self, points=None):
        self.points = np.asarray(points)

    def paint_uniform_color(self, color):
        self.color = color


class ViewControl:
    def set_constant_z_near(self, z):
        pass

    def set_constant_z_far(self, z):
        pass

    def convert_to_pinhole_camera_parameters(self):
        return SimpleNamespace(extrinsic=None)

    def convert_from_pinhole_camera_parameters(self, param):
        seen.extrinsic = np.array(param.extrinsic)


class Visualizer:
    def register_animation_callback(self, cb):
        pass

    def create_window(self, **kw):
        pass

    def get_render_option(self):
        return seen.options

    def get_view_control(self):
        return ViewControl()

    def run(self):
        pass

    def destroy_window(self):
        pass


def main():
    o3d = types.ModuleType("open3d")
    o3d.geometry = SimpleNamespace(PointCloud=PointCloud)
    o3d.utility = SimpleNamespace(Vector3dVector=np.asarray)
    o3d.visualization = SimpleNamespace(Visualizer=Visualizer)
    sys.modules["open3d"] = o3d
    sys.path.insert(0, REF)
    from src.tools import visualizer_util as ref
    scales = np.array([0.005, 0.2])
    actors = [ref.create_camera_actor(0, False, s) for s in scales]
    gt = ref.create_camera_actor(0, True, scales[0])
    rng = np.random.default_rng(0)
    init = np.tile(np.eye(4), (3, 1, 1))
    for k in (1, 2):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        init[k, :3, :3] = q * np.sign(np.linalg.det(q))
        init[k, :3, 3] = rng.uniform(-2, 2, size=3)
    ext = []
    for k in range(3):
        ref.draw_trajectory(None, "unused", init[k].copy(), 0.2, False, 0, None, None)
        ext.append(seen.extrinsic)
    np.savez(OUT, scales=scales, actor_points=np.stack([a.points for a in actors]), color_est=np.array(actors[0].color),
             color_gt=np.array(gt.color), init_poses=init, extrinsics=np.stack(ext),
             point_size=np.array(seen.options.point_size), back_face=np.array(seen.options.mesh_show_back_face))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
