"""numpy models of the point-to-mesh distance (csrc/eslam_meshdist.hip; include/eslam_hip.h, eslam_tri_*), no GPU:

  closest_f32 / model_query   the per-pair function in float32, operation by operation in the header's order (numpy's
                              float32 ufuncs round once per operation and never fuse), and the brute-force minimum over all
                              faces, equal d2 to the smaller face index: what the kernel must give bit for bit;
  truth_f64                   float64, by a different route: project onto the plane, inside by three edge-side tests,
                              otherwise the nearest of the three segments.  Shares no region logic with the model;
  segments_f64                float64 distance to the three edge segments alone (the truth for zero-area faces);
  icosphere                   the subdivided icosahedron.
"""
import numpy as np

F32 = np.float32


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _norm1(u):
    return (np.abs(u[..., 0]) + np.abs(u[..., 1])) + np.abs(u[..., 2])


def _ok(s):
    return (s > 0) & (s < np.inf)


def _segment_f32(o, e, q, bd2, bp):
    ee = _dot(e, e)
    t = np.where(_ok(ee), np.fmin(np.fmax(_dot(q - o, e) / ee, F32(0)), F32(1)), F32(0)).astype(F32)
    p = o + e * t[..., None]
    d = q - p
    d2 = _dot(d, d)
    take = d2 < bd2
    return np.where(take, d2, bd2), np.where(take[..., None], p, bp)


def closest_f32(a, b, c, q, drop_edges=False):
    """(float32 [...,3], region 0..6): the closest point of triangle (a, b, c) to q by the header's rule; all arguments float32
    and broadcastable.  drop_edges=True is a mutant for the tests: the three edge regions fall through to the interior
    formula, taken unguarded."""
    a, b, c, q = (np.asarray(x, dtype=F32) for x in (a, b, c, q))
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap = q - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = ap - ab
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = ap - ac
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        in_a = (d1 <= 0) & (d2 <= 0)
        in_b = (d3 >= 0) & (d4 <= d3)
        in_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        in_c = (d6 >= 0) & (d5 <= d6)
        in_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        in_bc = (va <= 0) & (e43 >= 0) & (e56 >= 0)
        if drop_edges:
            in_ab = in_ac = in_bc = np.zeros_like(in_a)
        region = np.select([in_a, in_b, in_ab, in_c, in_ac, in_bc], [0, 1, 2, 3, 4, 5], default=6)
        s_ab, s_ac, s_bc, s_in = d1 - d3, d2 - d6, e43 + e56, (va + vb) + vc
        r = F32(1) / s_in
        v, w = vb * r, vc * r
        full = lambda x: np.broadcast_to(x, ap.shape)
        cand = [full(a), full(b), a + ab * (d1 / s_ab)[..., None], full(c),
                a + ac * (d2 / s_ac)[..., None], b + (c - b) * (e43 / s_bc)[..., None],
                (a + ab * v[..., None]) + ac * w[..., None]]
        p = np.zeros_like(cand[0])
        for k, cand_k in enumerate(cand):
            p = np.where((region == k)[..., None], cand_k, p)
        nab, nac = _norm1(ab), _norm1(ac)
        m = (_norm1(ap) + nab) + nac
        tol = (F32(1e-6) * (nab * nac)) * (m * m)
        clear = ((va > tol) & (vb > tol) & (vc > tol)) | bool(drop_edges)
        bad = (((region == 2) & ~_ok(s_ab)) | ((region == 4) & ~_ok(s_ac)) | ((region == 5) & ~_ok(s_bc)) |
               ((region == 6) & ~(clear & _ok(s_in))))
        if bad.any():
            bd2 = np.full(region.shape, np.inf, dtype=F32)
            sp = cand[0]
            bd2, sp = _segment_f32(a, ab, q, bd2, sp)
            bd2, sp = _segment_f32(a, ac, q, bd2, sp)
            bd2, sp = _segment_f32(b, c - b, q, bd2, sp)
            p = np.where(bad[..., None], sp, p)
    return p.astype(F32), region


def pair_d2_f32(q, p):
    d = np.asarray(q, dtype=F32) - p
    with np.errstate(all="ignore"):
        return _dot(d, d)


def model_query(verts, faces, queries, max_dist=None, pair=None, ties="smaller", chunk=256):
    """(dist float32 [Q], face int32 [Q], closest float32 [Q,3]): the brute-force minimum of the per-pair function over
    all faces with finite vertices; equal d2 to the smaller (ties='larger': a mutant) face index; (inf, -1, NaN) for a
    non-finite query, no face, or dist >= max_dist.  pair(a, b, c, q) -> closest replaces closest_f32 (mutants)."""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    q = np.asarray(queries, dtype=F32).reshape(-1, 3)
    nq = q.shape[0]
    dist = np.full(nq, np.inf, dtype=F32)
    face = np.full(nq, -1, dtype=np.int32)
    near = np.full((nq, 3), np.nan, dtype=F32)
    if f.shape[0]:
        keep = np.isfinite(v[f]).all(axis=(1, 2))
        ids = np.nonzero(keep)[0]
        a, b, c = v[f[ids, 0]], v[f[ids, 1]], v[f[ids, 2]]
    else:
        ids = np.zeros(0, dtype=np.int64)
    if nq == 0 or len(ids) == 0:
        return dist, face, near
    for lo in range(0, nq, chunk):
        qq = q[lo:lo + chunk, None, :]
        p = pair(a[None], b[None], c[None], qq) if pair is not None else closest_f32(a[None], b[None], c[None], qq)[0]
        d2 = pair_d2_f32(qq, p)
        d2 = np.where(np.isnan(d2), np.inf, d2).astype(F32)
        m = d2.min(axis=1)
        hit = d2 == m[:, None]
        j = hit.argmax(axis=1) if ties == "smaller" else hit.shape[1] - 1 - hit[:, ::-1].argmax(axis=1)
        rows = np.arange(len(m))
        d = np.sqrt(m).astype(F32)
        ok = np.isfinite(q[lo:lo + chunk]).all(axis=1) & np.isfinite(m)
        if max_dist is not None:
            ok &= d < F32(max_dist)
        dist[lo:lo + chunk] = np.where(ok, d, F32(np.inf))
        face[lo:lo + chunk] = np.where(ok, ids[j], -1)
        near[lo:lo + chunk] = np.where(ok[:, None], p[rows, j], F32(np.nan))
    return dist, face, near


# ---------------------------------------------------------------------------------------------------------
# float64, another route
# ---------------------------------------------------------------------------------------------------------
def _seg_dist_f64(o, e, q):
    ee = (e * e).sum(-1)
    with np.errstate(all="ignore"):
        t = np.where(ee > 0, ((q - o) * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    return np.linalg.norm(q - (o + e * t[..., None]), axis=-1)


def segments_f64(a, b, c, q):
    """float64 [...]: the distance from q to the nearest of the segments ab, ac, bc."""
    a, b, c, q = (np.asarray(x, dtype=np.float64) for x in (a, b, c, q))
    return np.minimum(np.minimum(_seg_dist_f64(a, b - a, q), _seg_dist_f64(a, c - a, q)), _seg_dist_f64(b, c - b, q))


def pair_truth_f64(a, b, c, q):
    """float64 [...]: the distance from q to triangle abc: inside the three edge planes it is the distance to the
    plane, otherwise (and for a zero-area triangle) the distance to the nearest edge segment."""
    a, b, c, q = (np.asarray(x, dtype=np.float64) for x in (a, b, c, q))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    flat = nn > 0
    h = ((q - a) * n).sum(-1) / np.where(flat, nn, 1.0)              # signed height in units of |n|^2
    p = q - n * h[..., None]
    inside = flat
    for o, e in ((a, b - a), (b, c - b), (c, a - c)):
        inside = inside & ((np.cross(e, p - o) * n).sum(-1) >= 0)
    return np.where(inside, np.abs(h) * np.sqrt(nn), segments_f64(a, b, c, q))


def truth_f64(verts, faces, queries, chunk=256):
    """float64 [Q]: the distance from every query to the mesh (inf without a finite face)."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    out = np.full(q.shape[0], np.inf)
    if f.shape[0] == 0:
        return out
    f = f[np.isfinite(v[f]).all(axis=(1, 2))]
    if f.shape[0] == 0:
        return out
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    for lo in range(0, q.shape[0], chunk):
        out[lo:lo + chunk] = pair_truth_f64(a, b, c, q[lo:lo + chunk, None, :]).min(axis=1)
    return out


# ---------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------
def soup(n_faces, n_queries, seed, size=0.15, shift=0.0):
    """A seeded triangle soup in the unit cube (corners within `size` of a random centre) and uniform queries in a
    slightly larger cube, float32, both moved by `shift` on every axis (the shift applied in float64, then rounded)."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(size, 1.0 - size, (n_faces, 1, 3))
    verts = (centre + rng.uniform(-size, size, (n_faces, 3, 3))).reshape(-1, 3) + shift
    faces = np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)
    queries = rng.uniform(-0.1, 1.1, (n_queries, 3)) + shift
    return verts.astype(F32), faces, queries.astype(F32)


def icosphere(subdivisions, radius=1.0):
    """(verts float64 [V,3], faces int32 [F,3]): an icosahedron subdivided `subdivisions` times (20 * 4^s faces), every
    vertex at `radius` from the origin, faces counter-clockwise seen from outside."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for i, j, k in f:
            a, b, c = midpoint(i, j), midpoint(j, k), midpoint(k, i)
            nf += [(i, a, c), (j, b, a), (k, c, b), (a, b, c)]
        f = nf
    return np.stack(v) * radius, np.asarray(f, dtype=np.int32)
