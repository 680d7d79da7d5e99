"""The offline viewer, as the reference's visualizer.py drives it, without a window:

    python -m myslam_amd.visualizer configs/Replica/room0.yaml [--output D] [--save_rendering] [--top_view] [--no_gt_traj]
                                    [--every K] [--size H W] [--shaded [--ambient A]]

Replays a finished run from its output folder: the newest checkpoint's estimated and ground-truth trajectories
(translations divided by the config's `scale`), and for every frame i the mesh mesh/{i:05d}_mesh_culled.ply when the
run wrote one, the two current cameras, and the trajectories up to i, refreshed every 10th frame.  The state is drawn on
the GPU (src/tools/visualizer_util.py, ops.render_view).  With --save_rendering every K-th sequence index i (--every, ours;
default 1) is written to <output>/tmp_rendering/{i:06d}.jpg; without it only the final state is written, to
<output>/vis.jpg (the reference shows a window instead).  The images are deterministic: the reference captures whatever
its GL loop showed between sleeps.  --size (ours) is the image's height and width, the reference's 1080 x 1920 window
by default.  --shaded (ours): meshes whose PLY carries vertex normals (a run with meshing.normals) are lit by a headlight at
the viewing camera, k = ambient + (1 - ambient) max(0, n . l) with --ambient A (default 0.3); a mesh without normals is drawn
unlit with one warning line.  No video is encoded: the reference's ffmpeg command line is printed for the user to run.

--top_view: the reference asks trimesh for the newest mesh's minimum-volume oriented box (oriented_bounds, ordered=False)
and views along that box's z axis, whichever axis that search ended on.  Here the box is the one of
eval_recon.get_cam_position's candidate search (the deviation from trimesh is documented there), and the view is along
its axis of smallest extent - a room's height - with the other two axes in ascending order of extent as x and y."""
import argparse
import glob
import os

import numpy as np

from . import checkpoint
from .run import default_config_for
from .src import config
from .src.tools.visualizer_util import SLAMFrontend, WINDOW_H, WINDOW_W


def top_view_pose(meshfile_or_vertices):
    """The init_pose of --top_view, float64 [4,4]: the mesh's oriented box as a frame whose z column is the axis of
    smallest extent (columns: middle, largest, smallest extent; right-handed), at the box's centre."""
    from .src.tools.eval_recon import get_cam_position
    _, transform = get_cam_position(meshfile_or_vertices)
    pose = np.eye(4)
    pose[:3, :3] = transform[:3, [1, 2, 0]]
    pose[:3, 3] = transform[:3, 3]
    pose[2, 3] -= 0.4                                    # (get_cam_position lifts its sampling box by 0.4)
    return pose


def main(argv=None):
    parser = argparse.ArgumentParser(description='Arguments to visualize the SLAM process.')
    parser.add_argument('config', type=str, help='Path to config file.')
    parser.add_argument('--output', type=str,
                        help='output folder, this have higher priority, can overwrite the one inconfig file')
    parser.add_argument('--save_rendering', action='store_true', help='save the renderings to `tmp_rendering` in output folder')
    parser.add_argument('--top_view', action='store_true',
                        help='Setting the camera to top view. Otherwise, the camera is at the first frame\'s pose.')
    parser.add_argument('--no_gt_traj', action='store_true', help='not visualize gt trajectory')
    parser.add_argument('--every', type=int, default=1, metavar='K', help='render every K-th sequence index')
    parser.add_argument('--size', type=int, nargs=2, default=(WINDOW_H, WINDOW_W), metavar=('H', 'W'), help='image size')
    parser.add_argument('--shaded', action='store_true', help='light meshes that carry vertex normals (headlight Lambert)')
    parser.add_argument('--ambient', type=float, default=0.3, metavar='A', help='ambient share of the shading, in [0, 1]')
    args = parser.parse_args(argv)
    if not 0.0 <= args.ambient <= 1.0:
        parser.error('--ambient must lie in [0, 1]')
    if args.every < 1:
        parser.error('--every must be at least 1')
    cfg = config.load_config(args.config, default_config_for(args.config))
    scale = cfg['scale']
    output = cfg['data']['output'] if args.output is None else args.output
    ckptsdir = f'{output}/ckpts'
    ckpts = [os.path.join(ckptsdir, f) for f in sorted(os.listdir(ckptsdir)) if 'tar' in f] if os.path.exists(ckptsdir) else []
    if not ckpts:
        raise FileNotFoundError(f'no checkpoint under {ckptsdir}')
    ckpt_path = ckpts[-1]
    print('Get ckpt :', ckpt_path)
    ckpt = checkpoint.load(ckpt_path)
    estimate_c2w_list = ckpt['estimate_c2w_list'].clone()
    gt_c2w_list = ckpt['gt_c2w_list'].clone()
    N = ckpt['idx']
    estimate_c2w_list[:, :3, 3] /= scale
    gt_c2w_list[:, :3, 3] /= scale
    estimate_c2w_list = estimate_c2w_list.cpu().numpy()
    gt_c2w_list = gt_c2w_list.cpu().numpy()

    meshfiles = sorted(glob.glob(f'{output}/mesh/*.ply'))
    if not meshfiles:
        raise FileNotFoundError(f'no mesh under {output}/mesh')
    init_pose = top_view_pose(meshfiles[-1]) if args.top_view else gt_c2w_list[0].copy()
    frontend = SLAMFrontend(output, init_pose=init_pose, cam_scale=0.2, save_rendering=args.save_rendering, near=0,
                            estimate_c2w_list=estimate_c2w_list, gt_c2w_list=gt_c2w_list, size=tuple(args.size),
                            shaded=args.shaded, ambient=args.ambient)
    frontend.start()
    written = []
    for i in range(0, N + 1):
        meshfile = f'{output}/mesh/{i:05d}_mesh_culled.ply'
        if os.path.isfile(meshfile):
            frontend.update_mesh(meshfile)
        frontend.update_pose(1, estimate_c2w_list[i], gt=False)
        if not args.no_gt_traj:
            frontend.update_pose(1, gt_c2w_list[i], gt=True)
        if i % 10 == 0:
            frontend.update_cam_trajectory(i, gt=False)
            if not args.no_gt_traj:
                frontend.update_cam_trajectory(i, gt=True)
        if args.save_rendering and i % args.every == 0:
            written.append(frontend.capture(i))
    frontend.terminate()
    if args.save_rendering:
        print(f'{len(written)} images under {output}/tmp_rendering; for a video:')
        print(f"/usr/bin/ffmpeg -f image2 -r 30 -pattern_type glob -i '{output}/tmp_rendering/*.jpg' -y {output}/vis.mp4")
    else:
        from PIL import Image
        Image.fromarray(frontend.render().cpu().numpy()).save(f'{output}/vis.jpg')
        print(f'the final state: {output}/vis.jpg')
    return written


if __name__ == '__main__':
    main()
