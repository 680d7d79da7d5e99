"""The reference's mesh culling (src/tools/cull_mesh.py) without trimesh: the visibility test of every vertex in every
frame runs in one HIP launch per chunk of frames (ops.cull_vertices), the mesh is read and written as PLY
(Mesher.read_ply / write_ply).  Bound onto the reference's Mapper with one line (its src/Mapper.py:35):

    from myslam_amd.src.tools.cull_mesh import cull_mesh

Rule (cull_mesh.py:61-112): a vertex is seen when one frame sees it (the test of eslam_cull_vertices, with the depth test
when cfg['meshing']['eval_rec']); faces whose three vertices were never seen are dropped, then the vertices no face
references; both keep their order, vertex colours follow their vertices.
The reference ends with trimesh's process(), which also removes non-finite vertices and merges vertices at equal
positions.  By default that step is skipped: the marching-cubes output of Mesher.get_mesh is already welded (one vertex per
crossing edge).  merge_vertices=True (--merge_vertices) applies it (tools/clean_mesh.py, steps (a) and (d)), for meshes
that come with one vertex per face corner.
"""
import argparse
import os

import numpy as np
import torch

from ... import ops
from ..utils.Mesher import read_ply, write_ply


def compact(vertices, faces, colors, seen):
    """(vertices, faces, colours) after dropping the faces none of whose vertices is seen and then the unreferenced
    vertices, order kept (cull_mesh.py:106-108).  numpy in, numpy out; seen bool [V]."""
    seen = np.asarray(seen, dtype=bool)
    faces = np.asarray(faces).reshape(-1, 3)
    keep_f = seen[faces].any(axis=1)
    f = faces[keep_f]
    used = np.zeros(len(vertices), dtype=bool)
    used[f.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return (np.asarray(vertices)[used], remap[f].astype(np.int64),
            None if colors is None else np.asarray(colors)[used])


def cull_mesh_arrays(vertices, faces, colors, frames, H, W, fx, fy, cx, cy, truncation, eval_rec, device="cuda:0",
                     chunk=32, merge_vertices=False):
    """In-memory cull_mesh: frames are (idx, colour, depth, c2w) tuples, as the dataset readers and
    synthscene.make_sequence yield them.  Returns (vertices, faces, colours) as numpy arrays.  merge_vertices: the
    reference's closing process() on the culled mesh (non-finite vertices removed, equal positions merged)."""
    dev = torch.device(device)
    v = torch.as_tensor(np.ascontiguousarray(vertices, dtype=np.float32)).to(dev)
    seen = ops.cull_vertices(v, ((fr[2], fr[3]) for fr in frames), (fx, fy, cx, cy), H, W, truncation, eval_rec, chunk)
    out = compact(vertices, faces, colors, seen.cpu().numpy())
    if merge_vertices:
        from .clean_mesh import clean_mesh_arrays
        out = clean_mesh_arrays(*out, merge_vertices=True, device=device)[:3]
    return out


def _update(dst, src):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _update(dst[k], v)
        else:
            dst[k] = v


def load_config(path, default_path=None):
    """The reference's src/config.py:load_config: a YAML file over the one its `inherit_from` names (recursively), else
    over default_path when that file exists."""
    import yaml
    with open(path) as f:
        cfg_special = yaml.full_load(f)
    inherit = cfg_special.get('inherit_from')
    cfg = {}
    if inherit is not None:
        cfg = load_config(inherit, default_path)
    elif default_path is not None and os.path.exists(default_path):
        with open(default_path) as f:
            cfg = yaml.full_load(f)
    _update(cfg, cfg_special)
    return cfg


def culled_path(mesh_file):
    """<stem>_culled.<ext> (cull_mesh.py:111-112)."""
    ext = mesh_file.split('.')[-1]
    return mesh_file[:-len(ext) - 1] + '_culled.' + ext


def cull_mesh(mesh_file, cfg, args, device, estimate_c2w_list=None, merge_vertices=False):
    """cull_mesh.py:36-113: cull the mesh to what the frames see, written next to it as <stem>_culled.<ext> (PLY).
    Frames come from datasets.get_dataset(cfg, args, 1, device); with estimate_c2w_list, its length is the frame count
    and its poses replace the reader's.  merge_vertices: see cull_mesh_arrays."""
    from ..utils.datasets import get_dataset
    frame_reader = get_dataset(cfg, args, 1, device=device)
    eval_rec = cfg['meshing']['eval_rec']
    truncation = cfg['model']['truncation']
    H, W, fx, fy, cx, cy = (cfg['cam'][k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
    n_imgs = len(estimate_c2w_list) if estimate_c2w_list is not None else len(frame_reader)

    def frames():
        for i in range(n_imgs):
            idx, color, depth, c2w = frame_reader[i]
            if estimate_c2w_list is not None:
                c2w = estimate_c2w_list[i]
            yield idx, color, torch.as_tensor(depth), torch.as_tensor(c2w)

    vertices, faces, colors = read_ply(mesh_file)
    out = cull_mesh_arrays(vertices, faces, colors, frames(), H, W, fx, fy, cx, cy, truncation, eval_rec, device,
                           merge_vertices=merge_vertices)
    write_ply(culled_path(mesh_file), *out)


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Arguments to cull the mesh.')
    parser.add_argument('config', type=str, help='path to the config file')
    parser.add_argument('--input_mesh', type=str, help='path to the mesh to be culled')
    parser.add_argument('--merge_vertices', action='store_true',
                        help="end as the reference's process() does: remove non-finite vertices, merge equal positions")
    args = parser.parse_args()
    args.input_folder = None
    cull_mesh(args.input_mesh, load_config(args.config, 'configs/ESLAM.yaml'), args, 'cuda', merge_vertices=args.merge_vertices)
