"""A classical TSDF mesh of an RGB-D sequence, from ground-truth or estimated poses: the frames fused into a dense volume
(ops.TSDFVolume, eslam_tsdf_integrate), marching cubes over the observed voxels, a coloured PLY.  The ground-truth stand-in
for datasets that ship no mesh (TUM, ScanNet) and the baseline a neural-SLAM mesh is compared with; the reference has no
such tool (its only fusion is the hull of src/utils/Mesher.py:63-128).

    python -m myslam_amd.src.tools.tsdf_fuse configs/Replica/room0.yaml --output fused.ply [--voxel 0.02] [--trunc 0.08]
                                             [--every 5] [--poses gt|<checkpoint>]

The volume covers cfg['mapping']['marching_cubes_bound'] (else cfg['mapping']['bound']) times cfg['scale'].  --poses gt
uses the reader's poses, a checkpoint path its estimate_c2w_list (whose length is then the frame count).  Rule, kernel and
the deviations from open3d: DESIGN.md section 17.
"""
import argparse

import numpy as np
import torch

from ... import checkpoint, ops
from ..utils.Mesher import write_ply
from .cull_mesh import load_config


def fuse_frames(frames, K, H, W, bound, voxel, trunc, every=1, color=True, device='cuda:0'):
    """(vertices float32 [V,3], faces int32 [F,3], colours float32 [V,3] or None) as numpy arrays: every `every`-th of
    `frames` ((idx, colour, depth, c2w) tuples, as the dataset readers and synthscene.make_sequence yield them; depth
    [H,W]) fused over `bound` ([3,2]) at `voxel` with truncation `trunc`, K = (fx, fy, cx, cy)."""
    every = max(1, int(every))
    H, W = int(H), int(W)

    def picked():
        for n, fr in enumerate(frames):
            if n % every:
                continue
            idx, colour, depth, c2w = fr
            depth = torch.as_tensor(depth)
            if tuple(depth.shape) != (H, W):
                raise RuntimeError(f"fuse_frames: frame {idx} has depth {tuple(depth.shape)}, expected ({H}, {W})")
            yield idx, colour, depth, torch.as_tensor(c2w)

    with torch.no_grad():
        vol = ops.TSDFVolume(bound, voxel, trunc, color=color, device=device)
        vol.integrate(picked(), K)
        verts, faces, colours = vol.extract_mesh()
        return (verts.cpu().numpy(), faces.cpu().numpy(), None if colours is None else colours.cpu().numpy())


def fuse(cfg, args, device, output, voxel=0.02, trunc=None, every=1, estimate_c2w_list=None):
    """Fuse the sequence of `cfg` (datasets.get_dataset(cfg, args, scale, device)) and write `output` (PLY).  With
    estimate_c2w_list, its length is the frame count and its poses replace the reader's.  Returns the arrays written."""
    from ..utils.datasets import get_dataset
    scale = cfg.get('scale', 1)
    frame_reader = get_dataset(cfg, args, scale, device=device)
    H, W, fx, fy, cx, cy = (cfg['cam'][k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
    mapping = cfg['mapping']
    bound = np.array(mapping.get('marching_cubes_bound', mapping.get('bound')), dtype=np.float64) * scale
    trunc = 4.0 * voxel if trunc is None else trunc
    n_imgs = len(estimate_c2w_list) if estimate_c2w_list is not None else len(frame_reader)

    def frames():
        for i in range(n_imgs):
            idx, color, depth, c2w = frame_reader[i]
            if estimate_c2w_list is not None:
                c2w = estimate_c2w_list[i]
            yield idx, color, depth, c2w

    out = fuse_frames(frames(), (fx, fy, cx, cy), H, W, bound, voxel, trunc, every=every, device=device)
    write_ply(output, *out)
    return out


def main(argv=None):
    parser = argparse.ArgumentParser(description='Arguments to fuse a sequence into a TSDF mesh.')
    parser.add_argument('config', type=str, help='path to the config file')
    parser.add_argument('--output', type=str, required=True, help='path of the PLY to write')
    parser.add_argument('--voxel', type=float, default=0.02, help='voxel size in scene units')
    parser.add_argument('--trunc', type=float, default=None, help='truncation distance (default: 4 voxels)')
    parser.add_argument('--every', type=int, default=1, help='use every n-th frame')
    parser.add_argument('--poses', type=str, default='gt', help="'gt' or the path of a checkpoint (its estimate_c2w_list)")
    args = parser.parse_args(argv)
    args.input_folder = None
    est = None
    if args.poses != 'gt':
        ckpt = checkpoint.load(args.poses)
        est = ckpt['estimate_c2w_list'][:int(ckpt['idx']) + 1]
    fuse(load_config(args.config, 'configs/ESLAM.yaml'), args, 'cuda', args.output, args.voxel, args.trunc, args.every, est)


if __name__ == '__main__':
    main()
