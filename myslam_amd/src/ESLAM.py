"""The system: a dataset, a config and the tracking + mapping loop, with the files the reference's ESLAM / Mapper / Logger
leave behind (reference src/ESLAM.py:45-125, src/Mapper.py:437-455, src/utils/Logger.py:41-47).

    cfg = config.load_config('configs/Replica/room0.yaml', 'configs/ESLAM.yaml')
    ESLAM(cfg, args).run()            # args: input_folder, output (None = the config's), graph (optional)

What it sets up is what the reference's constructor sets up: the output directory with ckpts/ and mesh/, the scale, the
camera after update_cam, the bound, the frame reader, the mesher.  What differs is how it runs: one process that tracks
and maps in the lock-step order the reference's two processes synchronise to (slam.Slam, or slam_graph.GraphedSlam with
args.graph), fed by datasets.FrameStream, which prepares the frames on the device.  Slam.run's schedule is kept as it is:
unlike the reference's mapper, the last frame is not mapped unless the schedule maps it, and frame n_img - 2 is not
added as a keyframe.  The in-loop frame visualisers (utils/Frame_Visualizer.py) hang on the loop's
on_iter hook when the config has tracking.vis_freq / mapping.vis_freq; the offline viewer (visualizer.py) is not built.

Written under <output>/:
    ckpts/NNNNN.tar            checkpoint.save, every mapping.ckpt_freq frames (mapped frames only, as the reference's
                               mapper logs) and at the last frame; frame 0 skipped with mapping.no_log_on_first_frame
    mesh/NNNNN_mesh.ply        every mapping.mesh_freq frames, with its culled copy NNNNN_mesh_culled.ply; frame 0
                               skipped with mapping.no_mesh_on_first_frame
    mesh/final_mesh.ply        (final_mesh_eval_rec.ply with meshing.eval_rec) and its culled copy, at the end
    mesh/*_culled_clean.ply    with meshing.clean_min_faces: N > 0 (ours; absent or 0 = off): every culled mesh once more
                               without the connected components of fewer than N faces (tools/clean_mesh.py)
    ate.json                   eval_ate.evaluate of the estimated against the dataset's trajectory
    tracking_vis/NNNNN_IIII.jpg, mapping_vis/NNNNN_IIII.jpg
                               the visualisers' panels: frame NNNNN, iteration IIII, every vis_freq frames and
                               vis_inside_freq iterations; frame 0 skipped with no_vis_on_first_frame (Tracker.py:276-302,
                               Mapper.py:308-310)
    (with meshing.normals: true - ours; absent or false = off - every mesh file above carries unit vertex normals nx, ny, nz:
    +grad sdf of the learned field at the file's own vertices, Mesher.vertex_normals; vertices, faces and colours unchanged)
    render_eval.json           with the top-level key render_eval: {every: N} (ours, like mixed_precision; absent or 0 = off):
                               PSNR, SSIM and depth L1 of every N-th frame rendered at its estimated pose, and their means
"""
import json
import os

import torch

from .. import checkpoint, eval_ate
from ..scene import scene_from_config
from ..slam import Slam, SlamConfig
from .tools.clean_mesh import clean_mesh, clean_path
from .tools.cull_mesh import cull_mesh, culled_path
from .utils.datasets import FrameStream, get_dataset
from .utils.Frame_Visualizer import Frame_Visualizer
from .utils.Mesher import Mesher, read_ply, write_ply


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
        self.clean_min_faces = int(cfg['meshing'].get('clean_min_faces', 0) or 0)
        self.mesh_normals = bool(cfg['meshing'].get('normals', False))
        self.render_eval_every = int((cfg.get('render_eval') or {}).get('every', 0) or 0)
        self.render_eval = None
        self.visualizers = {}
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
            self.mesher.get_mesh(mesh_out_file, s.all_planes, s.decoders, s.keyframe_dict, self.device,
                                 normals=self.mesh_normals)
        if os.path.exists(mesh_out_file):                                # (no surface: get_mesh says so and writes nothing)
            est = torch.stack([c.detach().cpu() for c in s.estimate_c2w_list[:n_poses]], 0)
            cull_mesh(mesh_out_file, self.cfg, self.args, self.device, estimate_c2w_list=est)
            self._add_normals(s, culled_path(mesh_out_file))
            if self.clean_min_faces > 0:
                clean_mesh(culled_path(mesh_out_file), device=self.device, min_faces=self.clean_min_faces)
                self._add_normals(s, clean_path(culled_path(mesh_out_file)))

    def _add_normals(self, s, path):
        """meshing.normals: the file rewritten with the field's normals at its own vertices (culling and clean-up move no
        vertex, so nothing is threaded through them: one launch per file)."""
        if not self.mesh_normals or not os.path.exists(path):
            return
        v, f, c = read_ply(path)
        write_ply(path, v, f, c, self.mesher.vertex_normals(v, s.all_planes, s.decoders))

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

    def _install_visualizers(self, s):
        """A Frame_Visualizer per stage whose section has vis_freq and vis_inside_freq (a missing key = off, as in a config
        written before them), and the on_iter hook that dispatches to them.  The hook is left unset when no call could pass
        a gate: frame 0 is the only multiple of a vis_freq >= n_img, and no_vis_on_first_frame skips it."""
        fires = False
        for stage in ('tracking', 'mapping'):
            sec = self.cfg[stage]
            freq, inside = sec.get('vis_freq'), sec.get('vis_inside_freq')
            if freq is None or inside is None or int(freq) <= 0 or int(inside) <= 0:
                continue
            vis = Frame_Visualizer(freq=int(freq), inside_freq=int(inside), vis_dir=os.path.join(self.output, f'{stage}_vis'),
                                   renderer=s.be.renderer, truncation=self.truncation, verbose=self.verbose, device=self.device)
            skip_first = bool(sec.get('no_vis_on_first_frame', False))
            self.visualizers[stage] = (vis, skip_first)
            fires = fires or not (skip_first and int(freq) >= self.n_img)
        if not fires:
            return

        def on_iter(stage, idx, it, gt_depth, gt_color, pose):
            entry = self.visualizers.get(stage)
            if entry is None or (idx == 0 and entry[1]):
                return
            with s._precision():
                entry[0].save_imgs(idx, it, gt_depth, gt_color, pose, s.all_planes, s.decoders)
        s.on_iter = on_iter

    def _render_eval(self, s):
        """render_eval.json: every N-th frame of the sequence, read again, rendered at its estimated pose."""
        rows = []
        for idx, gt_color, gt_depth, _ in FrameStream(self.frame_reader, self.device, prefetch=2):
            if idx % self.render_eval_every != 0 or idx >= len(s.estimate_c2w_list):
                continue
            r = s.render_report(gt_color, gt_depth, s.estimate_c2w_list[idx])
            rows.append(dict(idx=int(idx), psnr=r['psnr'], ssim=r['ssim'], depth_l1=r['depth_l1'] / self.scale))
        n = max(len(rows), 1)
        self.render_eval = dict(every=self.render_eval_every, frames=rows,
                                **{k: sum(r[k] for r in rows) / n for k in ('psnr', 'ssim', 'depth_l1')})
        with open(os.path.join(self.output, 'render_eval.json'), 'w') as f:
            json.dump(self.render_eval, f, indent=1)
            f.write('\n')

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
        self._install_visualizers(s)
        frames = FrameStream(self.frame_reader, self.device, prefetch=2)
        s.run(frames, on_frame=self._on_frame)

        name = 'final_mesh_eval_rec.ply' if self.eval_rec else 'final_mesh.ply'
        self._mesh(s, os.path.join(self.output, 'mesh', name), self.n_img)            # Mapper.py:448-455
        if self.render_eval_every > 0:
            self._render_eval(s)

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
        if self.render_eval is not None:
            q = self.render_eval
            print(f"Render: PSNR {q['psnr']:.2f} dB, SSIM {q['ssim']:.4f}, depth L1 {q['depth_l1'] * 100:.2f} cm over "
                  f"{len(q['frames'])} frames (every {q['every']})")
        return self.stats
