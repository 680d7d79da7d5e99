"""The system: a dataset, a config and the tracking + mapping loop, with the files the reference's ESLAM / Mapper / Logger
leave behind (reference src/ESLAM.py:45-125, src/Mapper.py:437-455, src/utils/Logger.py:41-47).

    cfg = config.load_config('configs/Replica/room0.yaml', 'configs/ESLAM.yaml')
    ESLAM(cfg, args).run()            # args: input_folder, output (None = the config's), graph (optional)

What it sets up is what the reference's constructor sets up: the output directory with ckpts/ and mesh/, the scale, the
camera after update_cam, the bound, the frame reader, the mesher.  What differs is how it runs: one process that tracks
and maps in the lock-step order the reference's two processes synchronise to (slam.Slam, or slam_graph.GraphedSlam with
args.graph), fed by datasets.FrameStream, which prepares the frames on the device.  Slam.run's schedule is kept as it is:
unlike the reference's mapper, the last frame is not mapped unless the schedule maps it, and frame n_img - 2 is not
added as a keyframe.  The visualisers are not built.

Written under <output>/:
    ckpts/NNNNN.tar            checkpoint.save, every mapping.ckpt_freq frames (mapped frames only, as the reference's
                               mapper logs) and at the last frame; frame 0 skipped with mapping.no_log_on_first_frame
    mesh/NNNNN_mesh.ply        every mapping.mesh_freq frames, with its culled copy NNNNN_mesh_culled.ply; frame 0
                               skipped with mapping.no_mesh_on_first_frame
    mesh/final_mesh.ply        (final_mesh_eval_rec.ply with meshing.eval_rec) and its culled copy, at the end
    ate.json                   eval_ate.evaluate of the estimated against the dataset's trajectory
"""
import json
import os

import torch

from .. import checkpoint, eval_ate
from ..scene import scene_from_config
from ..slam import Slam, SlamConfig
from .tools.cull_mesh import cull_mesh
from .utils.datasets import FrameStream, get_dataset
from .utils.Mesher import Mesher


class ESLAM:
    def __init__(self, cfg, args):
        self.cfg, self.args = cfg, args
        self.verbose = cfg.get('verbose', False)
        self.device = torch.device(cfg.get('device', 'cuda:0'))
        self.dataset = cfg['dataset']
        self.truncation = cfg['model']['truncation']
        self.graph = bool(getattr(args, 'graph', False))

        out = getattr(args, 'output', None)
        self.output = cfg['data']['output'] if out is None else out
        self.ckptsdir = os.path.join(self.output, 'ckpts')
        os.makedirs(self.output, exist_ok=True)
        os.makedirs(self.ckptsdir, exist_ok=True)
        os.makedirs(os.path.join(self.output, 'mesh'), exist_ok=True)

        self.scale = cfg['scale']
        self.scene = scene_from_config(cfg)                              # update_cam, load_bound, the planes' shapes
        sc = self.scene
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy
        self.bound = sc.bound

        self.frame_reader = get_dataset(cfg, args, self.scale, device=self.device)
        self.n_img = len(self.frame_reader)
        self.slam_config = SlamConfig.from_config(cfg)
        self.mesher = Mesher(cfg, args, self)

        m = cfg['mapping']
        self.ckpt_freq, self.mesh_freq = int(m['ckpt_freq']), int(m['mesh_freq'])
        self.no_log_on_first_frame = bool(m.get('no_log_on_first_frame', False))
        self.no_mesh_on_first_frame = bool(m.get('no_mesh_on_first_frame', False))
        self.eval_rec = bool(cfg['meshing']['eval_rec'])
        self.slam = None
        self.stats = None
        self.ate = None
        self.print_output_desc()

    def print_output_desc(self):
        print(f"INFO: The output folder is {self.output}")
        print(f"INFO: The mesh can be found under {self.output}/mesh/")
        print(f"INFO: The checkpoint can be found under {self.output}/ckpts/")

    # ------------------------------------------------------------------------------------------------------------
    def _log(self, s, idx):
        """Logger.log: ckpts/NNNNN.tar."""
        path = os.path.join(self.ckptsdir, f'{idx:05d}.tar')
        checkpoint.save(path, s.decoders, s.gt_c2w_list, s.estimate_c2w_list, s.keyframe_list, idx)
        if self.verbose:
            print('Saved checkpoints at', path)

    def _mesh(self, s, mesh_out_file, n_poses):
        """Mapper.py:444-446 / :454-455: the mesh, then its copy culled to what the frames see from the estimated poses."""
        with s._precision():
            self.mesher.get_mesh(mesh_out_file, s.all_planes, s.decoders, s.keyframe_dict, self.device)
        if os.path.exists(mesh_out_file):                                # (no surface: get_mesh says so and writes nothing)
            est = torch.stack([c.detach().cpu() for c in s.estimate_c2w_list[:n_poses]], 0)
            cull_mesh(mesh_out_file, self.cfg, self.args, self.device, estimate_c2w_list=est)

    def _on_frame(self, s, idx):
        """Mapper.py:437-446 for a frame the mapper has seen (its loop runs at mapped frames and at the last one)."""
        last = idx == self.n_img - 1
        mapped = idx % s.cfg.every_frame == 0
        if not (mapped or last):
            return
        if (not (idx == 0 and self.no_log_on_first_frame) and idx % self.ckpt_freq == 0) or last:
            self._log(s, idx)
        if idx % self.mesh_freq == 0 and not (idx == 0 and self.no_mesh_on_first_frame):
            self._mesh(s, os.path.join(self.output, 'mesh', f'{idx:05d}_mesh.ply'), idx + 1)

    def run(self):
        """Track and map the whole sequence; returns the loop's stats."""
        if self.n_img == 0:
            raise RuntimeError(f"no frames found under {self.frame_reader.input_folder}")
        seed = int(self.cfg.get('seed', 0))
        torch.manual_seed(seed)
        if self.graph:
            from ..slam_graph import GraphedSlam
            s = GraphedSlam(self.scene, self.slam_config, device=self.device, seed=seed)
        else:
            s = Slam(self.scene, self.slam_config, device=self.device, seed=seed)
        self.slam = s
        frames = FrameStream(self.frame_reader, self.device, prefetch=2)
        s.run(frames, on_frame=self._on_frame)

        name = 'final_mesh_eval_rec.ply' if self.eval_rec else 'final_mesh.ply'
        self._mesh(s, os.path.join(self.output, 'mesh', name), self.n_img)            # Mapper.py:448-455

        est = [c.cpu().numpy() for c in s.estimate_c2w_list]
        gt = [c.cpu().numpy() for c in s.gt_c2w_list]
        for m in est + gt:
            m[:3, 3] /= self.scale                                       # back to the dataset's length unit
        self.ate = eval_ate.evaluate(est, gt)
        with open(os.path.join(self.output, 'ate.json'), 'w') as f:
            json.dump(dict(self.ate, n_frames=len(est)), f, indent=1)
            f.write('\n')
        self.stats = s.stats
        print(f"ATE rmse {self.ate['rmse'] * 100:.2f} cm over {len(est)} frames; {s.stats}")
        return self.stats
