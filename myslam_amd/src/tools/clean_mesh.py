"""Mesh clean-up without trimesh, open3d or scipy: merge the vertices at equal positions, find the connected components,
drop the small ones.  The three graph steps run in HIP (ops.weld_vertices, ops.mesh_components,
ops.component_face_counts); the remap, the filter decision and the compaction are torch ops around them.

    python -m myslam_amd.src.tools.clean_mesh --input_mesh M.ply [--min_faces N] [--min_fraction X] [--keep_largest]
                                              [--no_merge] [--drop_degenerate]

writes <stem>_clean.ply next to the input and prints the numbers.  Steps, in this order:
  (a) weld        with merge_vertices: faces that touch a vertex with a NaN or infinite coordinate go, the others' indices
                  are replaced by their representatives (the smallest index at the same position, so a merged vertex keeps
                  the representative's colour).  drop_degenerate then removes faces with two equal corners; off by default,
                  as trimesh's process(validate=False) keeps them.
  (b) components  of the remapped faces, and every component's face count.
  (c) filter      a face stays when its component has at least min_faces faces, at least min_fraction x the largest count,
                  and with keep_largest is the component with most faces (ties go to the smaller label).
  (d) compaction  kept faces and the vertices they reference keep their order.
Steps (a) and (d) alone are what trimesh's process() does at the end of the reference's cull_mesh (src/tools/cull_mesh.py:109);
the filter is NICE-SLAM's remove_small_geometry.
Deviations: positions merge when they are EQUAL as float32 (-0 == +0), where trimesh rounds to 1e-8 first; components are
joined through shared VERTICES, where trimesh uses shared edges, so two pieces touching at one vertex are one component.
The vertex order is ours (the survivors' original order), not trimesh's.
"""
import argparse

import numpy as np
import torch

from ... import ops
from ..utils.Mesher import read_ply, write_ply


def weld_faces(faces, rep, drop_degenerate=False):
    """Step (a) on the host: faces int64 [F,3] -> the faces that survive, their indices replaced by rep's (int [V], -1 =
    a non-finite vertex); rep None = no merge.  Order kept."""
    f = faces
    if rep is not None:
        f = rep.to(torch.int64)[faces]
        f = f[(f >= 0).all(dim=1)]
    if drop_degenerate:
        f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    return f


def passing_labels(face_count, min_faces=0, min_fraction=0.0, keep_largest=False):
    """Step (c)'s decision: bool [V], true at the labels of the components that stay.  face_count int [V]: a component's
    face count at its label, 0 elsewhere."""
    fc = face_count.to(torch.int64)
    largest = int(fc.max()) if fc.numel() else 0
    ok = (fc > 0) & (fc >= int(min_faces)) & (fc.to(torch.float64) >= float(min_fraction) * largest)
    if keep_largest and largest > 0:
        first = int(torch.nonzero(fc == largest)[0])          # ties: the smaller label
        only = torch.zeros_like(ok)
        only[first] = True
        ok &= only
    return ok


def compact_faces(n_verts, faces):
    """Step (d): (used bool [n_verts], faces renumbered over the used vertices); both keep their order."""
    used = torch.zeros(n_verts, dtype=torch.bool, device=faces.device)
    used[faces.reshape(-1)] = True
    remap = torch.cumsum(used.to(torch.int64), 0) - 1
    return used, remap[faces]


def clean_tensors(verts, faces, weld, components, counts, merge_vertices=True, min_faces=0, min_fraction=0.0,
                  keep_largest=False, drop_degenerate=False):
    """The pipeline on tensors of one device, the three graph steps handed in: weld(verts) -> rep [V],
    components(faces, V) -> labels [V], counts(faces, labels) -> face_count [V] (ops.weld_vertices, ops.mesh_components,
    ops.component_face_counts on the GPU; any model of them elsewhere).  verts float32 [V,3], faces int64 [F,3].
    Returns (used bool [V], faces int64 [F',3] over the used vertices, info)."""
    V = verts.shape[0]
    rep = weld(verts).to(torch.int64) if merge_vertices else None
    f = weld_faces(faces, rep, drop_degenerate)
    labels = components(f, V).to(torch.int64)
    face_count = counts(f, labels).to(torch.int64)
    ok = passing_labels(face_count, min_faces, min_fraction, keep_largest)
    f = f[ok[labels[f[:, 0]]]]
    used, f = compact_faces(V, f)
    sizes = face_count[face_count > 0]
    info = dict(
        vertices_merged=0 if rep is None else int(((rep >= 0) & (rep != torch.arange(V, device=rep.device))).sum()),
        nonfinite_vertices=0 if rep is None else int((rep < 0).sum()),
        components=int(sizes.numel()),
        components_kept=int(ok.sum()),
        face_counts=torch.sort(sizes, descending=True).values.tolist())
    return used, f, info


def clean_mesh_arrays(vertices, faces, colors, merge_vertices=True, min_faces=0, min_fraction=0.0, keep_largest=False,
                      drop_degenerate=False, device="cuda:0"):
    """In-memory clean-up of a mesh given as numpy arrays (vertices [V,3], faces [F,3], colours [V,*] or None): returns
    (vertices, faces, colours, info) with the rows that stay, in their order.  An index outside [0, V) raises ValueError."""
    dev = torch.device(device)
    vertices = np.asarray(vertices)
    v = torch.as_tensor(np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)).to(dev)
    f = torch.as_tensor(np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)).to(dev)
    if f.shape[0]:
        lo, hi = (int(x) for x in f.aminmax())
        if lo < 0 or hi >= v.shape[0]:
            raise ValueError(f"faces: indices span [{lo}, {hi}], the mesh has {v.shape[0]} vertices")
    used, f, info = clean_tensors(v, f, ops.weld_vertices, ops.mesh_components, ops.component_face_counts, merge_vertices,
                                  min_faces, min_fraction, keep_largest, drop_degenerate)
    used = used.cpu().numpy()
    return (vertices.reshape(-1, 3)[used], f.cpu().numpy(), None if colors is None else np.asarray(colors)[used], info)


def clean_path(mesh_file):
    """<stem>_clean.<ext>."""
    ext = mesh_file.split('.')[-1]
    return mesh_file[:-len(ext) - 1] + '_clean.' + ext


def clean_mesh(mesh_file, out_file=None, device="cuda:0", **options):
    """Clean the PLY mesh_file into out_file (<stem>_clean.<ext> by default); options as clean_mesh_arrays.  Returns info."""
    vertices, faces, colors = read_ply(mesh_file)
    v, f, c, info = clean_mesh_arrays(vertices, faces, colors, device=device, **options)
    write_ply(out_file or clean_path(mesh_file), v, f, c)
    return info


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Merge equal vertices and drop small connected components of a mesh.')
    parser.add_argument('--input_mesh', type=str, required=True, help='path to the mesh to be cleaned (PLY)')
    parser.add_argument('--min_faces', type=int, default=0, help='drop components with fewer faces')
    parser.add_argument('--min_fraction', type=float, default=0.0, help='drop components below this fraction of the largest')
    parser.add_argument('--keep_largest', action='store_true', help='keep only the component with most faces')
    parser.add_argument('--no_merge', action='store_true', help='do not merge vertices at equal positions')
    parser.add_argument('--drop_degenerate', action='store_true', help='drop faces with two equal corners after the merge')
    a = parser.parse_args()
    print(clean_mesh(a.input_mesh, merge_vertices=not a.no_merge, min_faces=a.min_faces, min_fraction=a.min_fraction,
                     keep_largest=a.keep_largest, drop_degenerate=a.drop_degenerate))
