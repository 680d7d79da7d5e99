"""numpy model of the mesh clean-up (myslam_amd/csrc/eslam_meshclean.hip, myslam_amd/src/tools/clean_mesh.py): the vertex
merge, the connected components through shared vertices, their face counts, and the host pipeline on top of them.  No
scipy, no GPU.  Written from the rules in include/eslam_hip.h, not from the kernels: np.unique and label propagation where
the kernels use a hash table and a union-find."""
import numpy as np


def weld(verts):
    """int32 [V]: the smallest index at the same position (float equality, -0 == +0), -1 for a non-finite vertex."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    rep = np.full(len(v), -1, dtype=np.int32)
    idx = np.nonzero(np.isfinite(v).all(axis=1))[0]
    if len(idx):
        bits = (v[idx] + np.float32(0.0)).view(np.uint32)            # -0 + 0 = +0; denormals stay
        _, first, inv = np.unique(bits, axis=0, return_index=True, return_inverse=True)
        rep[idx] = idx[first[np.asarray(inv).reshape(-1)]]
    return rep


def components(faces, n_verts, rounds=None):
    """int32 [n_verts]: the smallest vertex index of every vertex's component (faces joined through shared vertices).
    Rounds of: every face hooks its three vertices and their labels under the smallest of the three labels, then
    pointer-jumping to a fixed point; until a round changes nothing.  rounds: a list that receives the round count."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lab = np.arange(n_verts, dtype=np.int64)
    n = 0
    while len(f):
        n += 1
        before = lab.copy()
        l = lab[f]
        m = np.repeat(l.min(axis=1), 3)
        np.minimum.at(lab, l.reshape(-1), m)
        np.minimum.at(lab, f.reshape(-1), m)
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        if np.array_equal(lab, before):
            break
    if rounds is not None:
        rounds.append(n)
    return lab.astype(np.int32)


def face_counts(faces, labels):
    """int32 [V]: at every component's label its number of faces (by the first corner), 0 elsewhere."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    labels = np.asarray(labels, dtype=np.int64)
    return np.bincount(labels[f[:, 0]], minlength=len(labels)).astype(np.int32)


def clean(vertices, faces, colors, merge_vertices=True, min_faces=0, min_fraction=0.0, keep_largest=False,
          drop_degenerate=False):
    """The pipeline of clean_mesh.clean_mesh_arrays in numpy: (vertices, faces int64, colours, info)."""
    vertices = np.asarray(vertices).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(vertices)
    merged = nonfinite = 0
    if merge_vertices:
        rep = weld(vertices).astype(np.int64)
        nonfinite = int((rep < 0).sum())
        merged = int(((rep >= 0) & (rep != np.arange(V))).sum())
        f = rep[f]
        f = f[(f >= 0).all(axis=1)]
    if drop_degenerate:
        f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    lab = components(f, V).astype(np.int64)
    fc = face_counts(f, lab).astype(np.int64)
    largest = int(fc.max()) if V else 0
    ok = (fc > 0) & (fc >= min_faces) & (fc.astype(np.float64) >= float(min_fraction) * largest)
    if keep_largest and largest > 0:
        first = int(np.nonzero(fc == largest)[0][0])
        only = np.zeros(V, dtype=bool)
        only[first] = True
        ok &= only
    f = f[ok[lab[f[:, 0]]]]
    used = np.zeros(V, dtype=bool)
    used[f.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    info = dict(vertices_merged=merged, nonfinite_vertices=nonfinite, components=int((fc > 0).sum()),
                components_kept=int(ok.sum()), face_counts=sorted(fc[fc > 0].tolist(), reverse=True))
    return vertices[used], remap[f].astype(np.int64), None if colors is None else np.asarray(colors)[used], info


# ---------------------------------------------------------------------------------------------------------------------
# small meshes the tests share
# ---------------------------------------------------------------------------------------------------------------------
def strip(n_faces, first=0):
    """A triangle strip of n_faces faces over the n_faces + 2 vertices first .. first + n_faces + 1."""
    k = np.arange(n_faces, dtype=np.int64) + first
    return np.stack([k, k + 1, k + 2], axis=1)


def permuted(faces, n_verts, rng):
    """The same mesh with its vertex indices and its face order randomly permuted: (faces, perm) with new = perm[old]."""
    perm = rng.permutation(n_verts)
    f = perm[np.asarray(faces, dtype=np.int64)]
    return f[rng.permutation(len(f))], perm


def blobs(rng, n_blobs=37, n_loose=50, lo=2, hi=470):
    """n_blobs disjoint strips of lo .. hi faces (both sizes present) and n_loose loose vertices, permuted:
    (faces, n_verts, sizes)."""
    sizes = np.concatenate([[lo, hi], rng.integers(lo, hi + 1, n_blobs - 2)])
    parts, first = [], 0
    for s in sizes:
        parts.append(strip(int(s), first))
        first += int(s) + 2
    n_verts = first + n_loose
    f, _ = permuted(np.concatenate(parts), n_verts, rng)
    return f, n_verts, sizes


def grid_mesh(n):
    """(vertices float32 [(n + 1)^2, 3], faces [2 n^2, 3]) of an n x n grid of quads, two triangles each."""
    y, x = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack([x.reshape(-1) * 0.125, y.reshape(-1) * 0.25 - 3.0, (x * y).reshape(-1) * 0.0625], axis=1).astype(np.float32)
    i = (y[:-1, :-1] * (n + 1) + x[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 1, i + n + 2], axis=1), np.stack([i, i + n + 2, i + n + 1], axis=1)])
    return v, f.astype(np.int64)


def soup(vertices, faces, rng=None):
    """One vertex per face corner (V = 3 F), the corners in shuffled order when rng is given: (vertices, faces)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    order = np.arange(3 * len(f)) if rng is None else rng.permutation(3 * len(f))
    v = np.empty((3 * len(f), 3), dtype=np.asarray(vertices).dtype)
    v[order] = np.asarray(vertices)[f.reshape(-1)]
    return v, order.reshape(-1, 3)
