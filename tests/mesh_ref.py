"""Plain numpy marching cubes with the table and ordering rules of eslam_mesh.hip (tests only; the product never imports
it).  The table is parsed from the committed header, so the GPU and this reference read the same table."""
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "myslam_amd", "csrc", "eslam_mc_tables.h")


def load_tables(path=HEADER):
    """(ntri [256] int, tri [256, 3 * max_tris] int, max_tris) from eslam_mc_tables.h."""
    text = open(path).read()
    max_tris = int(re.search(r"#define MC_MAX_TRIS (\d+)", text).group(1))
    body = lambda name: text.split(name, 1)[1].split("= {", 1)[1].split("};", 1)[0]
    ntri = np.array([int(v) for v in re.findall(r"-?\d+", body("MC_NTRI[256]"))], dtype=np.int64)
    tri = np.array([int(v) for v in re.findall(r"-?\d+", body("MC_TRI[256]"))], dtype=np.int64).reshape(256, 3 * max_tris)
    assert ntri.shape == (256,)
    return ntri, tri, max_tris


def edge_owner(e):
    """(owner offset (dx, dy, dz) from the cube's lower corner, axis) of cube edge e."""
    axis, j = divmod(e, 4)
    a, b = j & 1, j >> 1
    off = [(0, a, b), (a, 0, b), (a, b, 0)][axis]
    return off, axis


def crossings(vol, level):
    """bool [nx,ny,nz,3]: edge (point, axis) crosses the level."""
    below = vol < level
    ex = np.zeros(vol.shape + (3,), dtype=bool)
    ex[:-1, :, :, 0] = below[:-1] != below[1:]
    ex[:, :-1, :, 1] = below[:, :-1] != below[:, 1:]
    ex[:, :, :-1, 2] = below[:, :, :-1] != below[:, :, 1:]
    return ex


def marching_cubes(vol, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """(verts float32 [V,3], faces int32 [F,3]) in the order of eslam_mc_emit."""
    vol = np.asarray(vol, dtype=np.float32)
    level = np.float32(level)
    nx, ny, nz = vol.shape
    ntri, tri, _ = load_tables()
    ex = crossings(vol, level)
    flat = ex.reshape(-1)
    vid = np.full(flat.shape, -1, dtype=np.int64)
    vid[flat] = np.arange(int(flat.sum()))
    vid = vid.reshape(nx, ny, nz, 3)
    # vertices
    pi, pj, pk, ax = np.nonzero(ex)                     # C order: point linear index, then axis
    idx = np.stack([pi, pj, pk], 1).astype(np.float64)
    lo = vol[pi, pj, pk].astype(np.float64)
    step = np.eye(3, dtype=np.int64)[ax]
    hi = vol[pi + step[:, 0], pj + step[:, 1], pk + step[:, 2]].astype(np.float64)
    t = (np.float64(level) - lo) / (hi - lo)
    idx[np.arange(len(ax)), ax] += t
    verts = (np.asarray(origin, dtype=np.float64) + idx * np.asarray(spacing, dtype=np.float64)).astype(np.float32)
    # faces
    if min(nx, ny, nz) < 2:
        return verts, np.zeros((0, 3), dtype=np.int32)
    b = (vol < level).astype(np.int64)
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, (k >> 2) & 1
        case |= b[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] << k
    ci, cj, ck = np.nonzero(ntri[case] > 0)             # cubes in linear-index order
    cs = case[ci, cj, ck]
    counts = ntri[cs]
    rep = np.repeat(np.arange(len(cs)), counts)
    tri_no = np.arange(len(rep)) - np.repeat(np.cumsum(counts) - counts, counts)
    faces = np.zeros((len(rep), 3), dtype=np.int64)
    for c3 in range(3):
        edges = tri[cs[rep], 3 * tri_no + c3]
        for e in range(12):
            sel = edges == e
            (dx, dy, dz), axis = edge_owner(e)
            faces[sel, c3] = vid[ci[rep[sel]] + dx, cj[rep[sel]] + dy, ck[rep[sel]] + dz, axis]
    assert (faces >= 0).all()
    return verts, faces.astype(np.int32)
