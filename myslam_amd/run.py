"""Run the system on a dataset from its YAML config, as the reference's run.py does:

    python -m myslam_amd.run configs/Replica/room0.yaml [--input_folder D] [--output D] [--graph] [--render_eval N] [--clean_mesh N]

The config is read over the file its `inherit_from` names and over the defaults file: configs/ESLAM.yaml from the
working directory, as the reference has it, else the nearest ESLAM.yaml in a directory above the config.  --graph replays
every optimisation iteration as a captured hipGraph (slam_graph.GraphedSlam).  --render_eval N sets the config's
render_eval.every: after the run every N-th frame is rendered at its estimated pose and PSNR, SSIM and depth L1 are written
to <output>/render_eval.json.  --clean_mesh N sets meshing.clean_min_faces: every culled mesh is written once more as
<stem>_culled_clean.ply without the connected components of fewer than N faces."""
import argparse
import os

from .src import config
from .src.ESLAM import ESLAM


def default_config_for(path):
    """configs/ESLAM.yaml as the reference names it, else the nearest ESLAM.yaml in a directory above `path`."""
    if os.path.exists('configs/ESLAM.yaml'):
        return 'configs/ESLAM.yaml'
    d = os.path.dirname(os.path.abspath(path))
    while True:
        cand = os.path.join(d, 'ESLAM.yaml')
        if os.path.exists(cand):
            return cand
        up = os.path.dirname(d)
        if up == d:
            raise FileNotFoundError(f"no defaults file: configs/ESLAM.yaml does not exist here and no ESLAM.yaml lies above {path}")
        d = up


def main(argv=None):
    parser = argparse.ArgumentParser(description='Arguments for running ESLAM.')
    parser.add_argument('config', type=str, help='Path to config file.')
    parser.add_argument('--input_folder', type=str,
                        help='input folder, this have higher priority, can overwrite the one in config file')
    parser.add_argument('--output', type=str,
                        help='output folder, this have higher priority, can overwrite the one in config file')
    parser.add_argument('--graph', action='store_true', help='replay the iterations as captured hipGraphs')
    parser.add_argument('--render_eval', type=int, metavar='N',
                        help='render every N-th frame at its estimated pose after the run; PSNR, SSIM, depth L1 to render_eval.json')
    parser.add_argument('--clean_mesh', type=int, metavar='N',
                        help='also write every culled mesh without its connected components of fewer than N faces')
    parser.add_argument('--mesh_normals', action='store_true',
                        help='write unit vertex normals (+grad sdf of the learned field) into every mesh file')
    args = parser.parse_args(argv)
    cfg = config.load_config(args.config, default_config_for(args.config))
    if args.render_eval is not None:
        cfg['render_eval'] = dict(every=args.render_eval)
    if args.clean_mesh is not None:
        cfg['meshing']['clean_min_faces'] = args.clean_mesh
    if args.mesh_normals:
        cfg['meshing']['normals'] = True
    eslam = ESLAM(cfg, args)
    eslam.run()
    return eslam


if __name__ == '__main__':
    main()
