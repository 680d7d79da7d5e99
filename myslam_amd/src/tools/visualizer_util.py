"""The offline viewer's frontend without a window (reference src/tools/visualizer_util.py): the state the reference's
animation callback keeps - the current mesh, one estimated and one ground-truth camera actor, the two trajectories -
drawn by ops.render_view on the GPU instead of open3d's GL loop, so it runs on a node without a display.

What the reference's window shows and this draws: the mesh unlit with its vertex colours (the PLYs carry no normals),
back faces hidden (mesh_show_back_face = False), camera actors and trajectories as point clouds 4 pixels wide, estimated
in red, ground truth in green, on open3d's white background.  Deviations:
  * no process and no queue: update_* change the state at once, start / join / terminate do nothing; render() draws it;
  * the intrinsics are ours: the reference takes whatever open3d's view control starts with, which is a vertical field
    of view of 60 degrees (open3d's default) with the principal point at the centre; so fy = fx = (H / 2) / tan(30 deg),
    cx = W / 2 - 0.5, cy = H / 2 - 0.5 for the 1080 x 1920 window;
  * the near plane is the caller's `near` when positive, else the rasteriser's ESLAM_RASTER_Z_NEAR (open3d falls back to one
    derived from the scene's bounding box); the far plane is the reference's 1000;
  * update_pose negates the z column on a copy, where the reference writes into the caller's array;
  * save_rendering: the reference captures whatever the GL loop showed at each of its ticks; capture(i) writes the state
    at sequence index i to tmp_rendering/{i:06d}.jpg - deterministic."""
import math
import os
import shutil

import numpy as np
import torch

from ... import _hip
from ... import ops
from ..utils.Mesher import read_ply, read_ply_with_normals

WINDOW_H, WINDOW_W = 1080, 1920
FOV_Y_DEG = 60.0
POINT_SIZE = 4
Z_FAR = 1000.0
BACKGROUND = (255, 255, 255)
RED, GREEN = (255, 0, 0), (0, 255, 0)
GT_KEY = 100000


def normalize(x):
    return x / np.linalg.norm(x)


def camera_actor_points(scale=0.005):
    """visualizer_util.py:36-55: float64 [1200,3], the 12 segments of the camera glyph with 100 points each (the image
    rectangle and its diagonals, the four edges to the centre, the roof that marks `up`), in the camera's frame."""
    cam_points = scale * np.array([[0, 0, 0], [-1, -1, 1.5], [1, -1, 1.5], [1, 1, 1.5], [-1, 1, 1.5], [-0.5, 1, 1.5],
                                   [0.5, 1, 1.5], [0, 1.2, 1.5]], dtype=np.float64)
    cam_lines = np.array([[1, 2], [2, 3], [3, 4], [4, 1], [1, 3], [2, 4], [1, 0], [0, 2], [3, 0], [0, 4], [5, 7], [7, 6]])
    t = np.linspace(0., 1., 100)
    begin, end = cam_points[cam_lines[:, 0]], cam_points[cam_lines[:, 1]]
    pts = begin[:, None, :] * (1. - t)[None, :, None] + end[:, None, :] * t[None, :, None]
    return pts.reshape(-1, 3)


def viewing_pose(init_pose):
    """visualizer_util.py:189-198: the viewer's camera-to-world matrix [4,4] float64 - 4 m back along the initial pose's z
    column, the y and z columns negated (the reference hands its inverse to open3d as the extrinsic)."""
    c = np.array(init_pose, dtype=np.float64)
    c[:3, 3] += 4.0 * normalize(c[:3, 2])
    c[:3, 2] *= -1
    c[:3, 1] *= -1
    return c


def window_intrinsics(H, W):
    f = (H / 2.0) / math.tan(math.radians(FOV_Y_DEG / 2.0))
    return (f, f, W / 2.0 - 0.5, H / 2.0 - 0.5)


class SLAMFrontend:
    def __init__(self, output, init_pose, cam_scale=1, save_rendering=False, near=0, estimate_c2w_list=None,
                 gt_c2w_list=None, size=(WINDOW_H, WINDOW_W), device=None, shaded=False, ambient=0.3):
        """size: the image's (H, W); the reference's window everywhere but in tests.  shaded (ours): meshes whose PLY carries
        vertex normals are lit by a headlight (ops.render_view(shade=True, ambient=ambient)); the reference's window is unlit."""
        self.shaded, self.ambient = bool(shaded), float(ambient)
        self.output = output
        self.cam_scale = cam_scale
        self.save_rendering = save_rendering
        self.z_near = float(near) if near > 0 else _hip.RASTER_Z_NEAR
        self.estimate_c2w_list = None if estimate_c2w_list is None else np.asarray(estimate_c2w_list)
        self.gt_c2w_list = None if gt_c2w_list is None else np.asarray(gt_c2w_list)
        self.H, self.W = int(size[0]), int(size[1])
        self.K = window_intrinsics(self.H, self.W)
        self.view = viewing_pose(init_pose)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.reset()
        self.mesh = None
        self.traj = {False: None, True: None}
        if save_rendering:
            shutil.rmtree(os.path.join(output, 'tmp_rendering'), ignore_errors=True)

    def _gpu(self, a, dtype=torch.float32):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device, dtype)

    def update_pose(self, index, pose, gt=False):
        if isinstance(pose, torch.Tensor):
            pose = pose.cpu().numpy()
        pose = np.array(pose, dtype=np.float64)
        pose[:3, 2] *= -1
        pts = camera_actor_points(self.cam_scale) @ pose[:3, :3].T + pose[:3, 3]
        self.cameras[index + GT_KEY if gt else index] = (self._gpu(pts), pose)

    def update_mesh(self, path):
        v, f, c, nrm = read_ply_with_normals(path) if self.shaded else read_ply(path) + (None,)
        col = None if c is None else self._gpu(np.floor(np.clip(c, 0.0, 1.0) * 255.0 + 0.5), torch.uint8)
        if self.shaded and nrm is None:
            print(f'WARNING: {path} has no vertex normals (run with meshing.normals); drawn unlit')
        self.mesh = (self._gpu(v), self._gpu(f, torch.int32), col, None if nrm is None else self._gpu(nrm))

    def update_cam_trajectory(self, c2w_list, gt):
        i = c2w_list
        pts = (self.gt_c2w_list if gt else self.estimate_c2w_list)[:i, :3, 3]
        pts = pts[np.isfinite(pts).all(-1)].reshape(-1, 3)
        self.traj[bool(gt)] = self._gpu(pts)

    def reset(self):
        self.cameras = {}

    def start(self):
        return self

    def join(self):
        pass

    def terminate(self):
        pass

    def render(self):
        """uint8 [H,W,3] on the GPU: the current state from the viewing pose, one ops.render_view call."""
        meshes = [self.mesh] if self.mesh is not None else []
        points = [(pts, RED if key < GT_KEY else GREEN, POINT_SIZE) for key, (pts, _) in sorted(self.cameras.items())]
        points += [(pts, GREEN if gt else RED, POINT_SIZE) for gt, pts in sorted(self.traj.items()) if pts is not None]
        points = [(p, torch.tensor(c, dtype=torch.uint8), s) for p, c, s in points]
        return ops.render_view(meshes, points, self.view[None], self.K, self.H, self.W, background=BACKGROUND,
                               z_near=self.z_near, z_far=Z_FAR, cull_backfaces=True, chunk=1, shade=self.shaded,
                               ambient=self.ambient)[0]

    def capture(self, index):
        """Writes render() to <output>/tmp_rendering/{index:06d}.jpg (visualizer_util.py:171-176); returns the path."""
        from PIL import Image
        d = os.path.join(self.output, 'tmp_rendering')
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f'{index:06d}.jpg')
        Image.fromarray(self.render().cpu().numpy()).save(path, quality=95)
        return path
