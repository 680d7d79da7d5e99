"""A float64 numpy depth rasteriser written from the formulas of eslam_raster_depth in include/eslam_hip.h: the same edge
functions, fill rule and near / far rule, none of the kernel's code.  Beside the depth image it returns, per pixel,

  edge   the pixel centre lies within `edge_tol` pixels of an edge of any triangle whose edge_tol-dilated interior contains
         it: there float32 rounding may decide coverage either way.  The distance in pixels to edge k is
         |E_k| / hypot(m.x / fx, m.y / fy), m = v_i x v_j (E_k is affine in the pixel coordinates with that gradient);
  cond   c = |n . d| / (|n| |d|) of the winning triangle: the cosine between the ray and the surface normal, by which
         an error of the plane's position is divided on its way into the depth.

A triangle with a vertex at or behind the near plane gets the box of its part beyond half of z_near (nothing nearer can
be a hit).  Triangles with a small pixel box are evaluated in numpy batches (by box size class), larger ones one by one.  Also the
analytic test meshes (icosphere, box) and the scenes shared by tests/test_raster_host.py and tests/test_gpu_raster.py.
"""
import numpy as np

BOX_SLACK = 0.01
EDGE_TOL = 1e-3
H = W = 500
FOCAL = 300.0
K = (FOCAL, FOCAL, H / 2.0 - 0.5, W / 2.0 - 0.5)
Z_NEAR, Z_FAR = 0.01, 20.0


def _block(sel, x0, y0, x1, y1, bw, bh, m, n, nv0, K, z_near, z_far, W, depth, cond, edge, edge_tol):
    """Triangles `sel` against the bw x bh pixels from their (x0, y0): updates depth / cond / edge (flat [H*W])."""
    fx, fy, cx, cy = K
    xs = x0[sel][:, None, None] + np.arange(bw)[None, None, :]
    ys = y0[sel][:, None, None] + np.arange(bh)[None, :, None]
    valid = (xs <= x1[sel][:, None, None]) & (ys <= y1[sel][:, None, None])
    dx, dy = (xs - cx) / fx, (ys - cy) / fy
    E = [m[k][sel, 0][:, None, None] * dx + m[k][sel, 1][:, None, None] * dy + m[k][sel, 2][:, None, None] for k in range(3)]
    ns = n[sel]
    nd = ns[:, 0][:, None, None] * dx + ns[:, 1][:, None, None] * dy + ns[:, 2][:, None, None]
    inside = ((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = nv0[sel][:, None, None] / nd
        hit = valid & inside & (nd != 0) & (z >= z_near) & (z <= z_far)
        sgn = np.sign(nd)
        near_all, near_any = np.ones(z.shape, bool), np.zeros(z.shape, bool)
        for k in range(3):
            g = np.hypot(m[k][sel, 0] / fx, m[k][sel, 1] / fy)[:, None, None]
            s = np.where(g > 0, E[k] * sgn / np.where(g > 0, g, 1.0), np.inf * np.sign(E[k] * sgn))
            near_all &= s >= -edge_tol
            near_any |= np.abs(s) <= edge_tol
    idx = (ys * W + xs + np.zeros_like(dx, dtype=np.int64)).astype(np.int64)
    em = valid & (nd != 0) & near_all & near_any
    edge[idx[em]] = True
    if hit.any():
        zi, ii = z[hit], idx[hit]
        c = (np.abs(nd) / (np.linalg.norm(ns, axis=1)[:, None, None] * np.sqrt(dx * dx + dy * dy + 1.0)))[hit]
        np.minimum.at(depth, ii, zi)
        win = zi == depth[ii]
        cond[ii[win]] = c[win]


def _clipped_box(tri, zc, K, H, W):
    """Pixel box (inclusive, inside the image) of the part of the camera-space triangle `tri` [3,3] with z >= zc: the
    polygon cut by the plane z = zc, its corners projected.  zc below z_near keeps it conservative for every hit."""
    fx, fy, cx, cy = K
    poly = []
    for k in range(3):
        a, b = tri[k], tri[(k + 1) % 3]
        if a[2] >= zc:
            poly.append(a)
        if (a[2] >= zc) != (b[2] >= zc):
            poly.append(a + (b - a) * ((zc - a[2]) / (b[2] - a[2])))
    p = np.array(poly)
    px, py = fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy
    return (int(np.ceil(np.clip(px.min() - BOX_SLACK, 0, W))), int(np.ceil(np.clip(py.min() - BOX_SLACK, 0, H))),
            int(np.floor(np.clip(px.max() + BOX_SLACK, -1, W - 1))), int(np.floor(np.clip(py.max() + BOX_SLACK, -1, H - 1))))


def rasterize(verts, faces, c2w, K=K, H=H, W=W, z_near=Z_NEAR, z_far=Z_FAR, edge_tol=EDGE_TOL):
    """(depth [H,W] float64 with 0 where nothing is hit, edge [H,W] bool, cond [H,W] float64 with 0 where nothing is hit)."""
    fx, fy, cx, cy = K
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    w2c = np.linalg.inv(np.asarray(c2w, dtype=np.float64))
    vc = v @ w2c[:3, :3].T + w2c[:3, 3]
    depth = np.full(H * W, np.inf)
    cond = np.zeros(H * W)
    edge = np.zeros(H * W, dtype=bool)
    if len(f):
        v0, v1, v2 = vc[f[:, 0]], vc[f[:, 1]], vc[f[:, 2]]
        n = np.cross(v1 - v0, v2 - v0)
        nv0 = (n * v0).sum(1)
        m = [np.cross(v1, v2), np.cross(v2, v0), np.cross(v0, v1)]
        zs = np.stack([v0[:, 2], v1[:, 2], v2[:, 2]], 1)
        zmin, zmax = zs.min(1), zs.max(1)
        keep = (n != 0).any(1) & (zmax >= z_near) & (zmin <= z_far)
        whole = zmin <= z_near
        with np.errstate(divide="ignore", invalid="ignore"):
            px = fx * np.stack([v0[:, 0], v1[:, 0], v2[:, 0]], 1) / zs + cx
            py = fy * np.stack([v0[:, 1], v1[:, 1], v2[:, 1]], 1) / zs + cy
        big = 1e9
        px, py = np.nan_to_num(px, nan=0.0, posinf=big, neginf=-big), np.nan_to_num(py, nan=0.0, posinf=big, neginf=-big)
        x0 = np.ceil(np.clip(px.min(1) - BOX_SLACK, 0, W)).astype(np.int64)
        x1 = np.floor(np.clip(px.max(1) + BOX_SLACK, -1, W - 1)).astype(np.int64)
        y0 = np.ceil(np.clip(py.min(1) - BOX_SLACK, 0, H)).astype(np.int64)
        y1 = np.floor(np.clip(py.max(1) + BOX_SLACK, -1, H - 1)).astype(np.int64)
        for t in np.nonzero(keep & whole)[0]:
            x0[t], y0[t], x1[t], y1[t] = _clipped_box(np.stack([v0[t], v1[t], v2[t]]), 0.5 * z_near, K, H, W)
        keep &= (x0 <= x1) & (y0 <= y1)
        side = np.maximum(x1 - x0, y1 - y0) + 1
        args = (m, n, nv0, K, z_near, z_far, W, depth, cond, edge, edge_tol)
        lo = 0
        for cls in (2, 4, 8, 16):
            sel = np.nonzero(keep & (side > lo) & (side <= cls))[0]
            step = max(1, (1 << 22) // (cls * cls))
            for a in range(0, len(sel), step):
                _block(sel[a:a + step], x0, y0, x1, y1, cls, cls, *args)
            lo = cls
        for t in np.nonzero(keep & (side > lo))[0]:
            _block(np.array([t]), x0, y0, x1, y1, int(x1[t] - x0[t] + 1), int(y1[t] - y0[t] + 1), *args)
    hitm = np.isfinite(depth)
    depth = np.where(hitm, depth, 0.0)
    return depth.reshape(H, W), edge.reshape(H, W), np.where(hitm, cond, 0.0).reshape(H, W)


# ----------------------------------------------------------------------------------------------
# meshes
# ----------------------------------------------------------------------------------------------
def icosphere(subdivisions, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """(verts float32 [V,3], faces int32 [20 * 4^s, 3]) of a subdivided icosahedron, vertices on the sphere."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
                  [8, 6, 7], [9, 8, 1]], dtype=np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(subdivisions):
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
        e.sort(axis=1)
        ue, inv = np.unique(e, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        mid = v[ue[:, 0]] + v[ue[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        nf = len(f)
        a, b, c = (len(v) + inv[k * nf:(k + 1) * nf] for k in range(3))      # midpoints of edges 01, 12, 20
        v = np.concatenate([v, mid], 0)
        f = np.concatenate([np.stack([f[:, 0], a, c], 1), np.stack([f[:, 1], b, a], 1), np.stack([f[:, 2], c, b], 1),
                            np.stack([a, b, c], 1)], 0)
    return (v * radius + np.asarray(centre)).astype(np.float32), f.astype(np.int32)


def icosphere_sag(verts, faces, radius, centre=(0.0, 0.0, 0.0)):
    """(face sag, edge sag) of a sphere's tessellation.  Face sag: R minus the smallest distance of a face's plane from the
    centre - how far the deepest point of a flat face (the foot of the centre's perpendicular) lies inside the sphere,
    exactly.  Edge sag: R (1 - cos(theta / 2)) for the angle theta the longest edge spans at the centre - the same for the
    middle of a chord; a face's interior lies deeper than its edges, so this one undercounts."""
    v = np.asarray(verts, dtype=np.float64) - np.asarray(centre)
    f = np.asarray(faces)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    h = np.abs((n * v[f[:, 0]]).sum(1)) / np.linalg.norm(n, axis=1)
    e = np.concatenate([v[f[:, 0]] - v[f[:, 1]], v[f[:, 1]] - v[f[:, 2]], v[f[:, 2]] - v[f[:, 0]]], 0)
    theta = 2.0 * np.arcsin(np.linalg.norm(e, axis=1).max() / (2.0 * radius))
    return radius - h.min(), radius * (1.0 - np.cos(theta / 2.0))


def box_mesh(lo, hi):
    """(verts float32 [8,3], faces int32 [12,3]) of the axis-aligned box [lo, hi]."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)])
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))])
    return v.astype(np.float32), f.astype(np.int32)


def merge(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    return np.concatenate(vs, 0), np.concatenate(fs, 0).astype(np.int32)


def look_at(origin, target, up=(0.0, 0.0, -1.0)):
    """c2w [4,4] float64, camera looking along +z from origin to target (the reference's viewmatrix)."""
    z = np.asarray(target, dtype=np.float64) - np.asarray(origin, dtype=np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, dtype=np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c = np.eye(4)
    c[:3, 0], c[:3, 1], c[:3, 2], c[:3, 3] = x, y, z, origin
    return c


# ----------------------------------------------------------------------------------------------
# the scenes of the GPU parity tests
# ----------------------------------------------------------------------------------------------
ROOM_LO, ROOM_HI = (-2.0, -1.5, -1.2), (2.0, 1.5, 1.2)
BALL_C, BALL_R = (0.6, 0.3, -0.4), 0.5


def scene_room():
    return box_mesh(ROOM_LO, ROOM_HI)


def scene_a():
    """A 12-triangle room plus a 20 480-face icosphere inside it."""
    return merge(scene_room(), icosphere(5, BALL_R, BALL_C))


def scene_b():
    """A 327 680-face icosphere of radius 0.6: seen from 1.4 m its triangles are about a pixel."""
    return icosphere(7, 0.6)


def views_a():
    """Three random interior views (seeded), and one from 5 cm off the x = lo wall looking along it: the wall's and its
    neighbours' triangles cross the camera plane."""
    rng = np.random.default_rng(7)
    out = []
    lo, hi = np.asarray(ROOM_LO), np.asarray(ROOM_HI)
    while len(out) < 3:
        o = lo + (hi - lo) * (0.15 + 0.7 * rng.uniform(size=3))
        if np.linalg.norm(o - np.asarray(BALL_C)) < BALL_R + 0.2:
            continue
        out.append(look_at(o, lo + (hi - lo) * rng.uniform(size=3)))
    out.append(look_at((ROOM_LO[0] + 0.05, 0.3, 0.1), (ROOM_LO[0] + 0.05, 5.0, 0.35)))
    return np.stack(out)


def views_b():
    return np.stack([look_at((1.4, 0.0, 0.0), (0.0, 0.0, 0.0)), look_at((0.5, -1.1, 0.7), (0.05, 0.1, 0.0))])
