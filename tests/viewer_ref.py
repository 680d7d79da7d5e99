"""A float64 numpy colour renderer written from the formulas of eslam_viewer_* in include/eslam_hip.h - mesh fragments
with the edge functions as barycentrics, the rounding rule, the back-face rule, point squares, the (depth, colour) key
order - none of the kernels' code, and the criteria the GPU images are held to (tests/test_gpu_viewer.py); the same
criteria are shown to reject mutated definitions without a GPU (tests/test_viewer_ref.py).

Like raster_ref.rasterize it returns an edge mask: the pixels within EDGE_TOL of an edge of a triangle whose dilated
interior contains them, the pixels of a triangle whose facing is too close to edge-on for the back-face rule to be
decided safely, the pixels where a second candidate with another colour lies within DEPTH_TIE (relative) of the winning
depth, and the squares of points whose u - size / 2 or v - size / 2 lies within POINT_TOL of an integer or whose depth is
within DEPTH_TIE of the near or far plane.  Also a float32 operation-by-operation model of the point path, which the GPU
must match bit for bit."""
import functools

import numpy as np

from tests import raster_ref as rr

EDGE_TOL = rr.EDGE_TOL
EDGE_SHARE_CAP = 0.01            # of the pixels (the depth test's cap) / of the points
DEPTH_TIE = 1e-5                 # float32 depths of the two paths differ by a few 1e-7 relative (test_gpu_raster's PARITY_BOUND)
FACING_TOL = 1e-5                # |cos| between a triangle's normal and the direction to it below which culling is not decided
POINT_TOL = 1e-3
GREY = (200, 200, 200)
BACKGROUND = (255, 255, 255)
H, W, K = rr.H, rr.W, rr.K
Z_NEAR, Z_FAR = rr.Z_NEAR, rr.Z_FAR


def pack(rgb):
    """uint64 colour words of uint8 [...,3]: R in the lowest byte, alpha 255."""
    c = np.asarray(rgb).astype(np.uint64)
    return c[..., 0] | (c[..., 1] << np.uint64(8)) | (c[..., 2] << np.uint64(16)) | np.uint64(0xff000000)


def unpack(word):
    w = np.asarray(word).astype(np.uint64)
    return np.stack([(w >> np.uint64(s)) & np.uint64(255) for s in (0, 8, 16)], -1).astype(np.uint8)


def color_field(verts, k=(1.7, 2.3, 3.1)):
    """A smooth colour per vertex with jumps, uint8 [V,4]: channel a = 255 frac(position . k rolled by a); alpha 7 (ignored)."""
    v = np.asarray(verts, dtype=np.float64)
    k = np.asarray(k)
    c = np.stack([np.floor(255.0 * np.mod(v @ np.roll(k, a), 1.0)) for a in range(3)], 1)
    return np.concatenate([c, np.full((len(v), 1), 7.0)], 1).astype(np.uint8)


# ----------------------------------------------------------------------------------------------
# fragments
# ----------------------------------------------------------------------------------------------
def _to_u8(c, rounding):
    c = np.clip(c, 0.0, 255.0)
    return (np.floor(c + 0.5) if rounding == "nearest" else np.floor(c)).astype(np.uint8)


def _mesh_block(sel, x0, y0, x1, y1, bw, bh, m, n, nv0, cols, amb, vc3, K, z_near, z_far, W, edge, edge_tol, bary, rounding):
    """Triangles `sel` against the bw x bh pixels from their (x0, y0): (pixel index, z, rgb) of the hits; updates edge."""
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
    em = valid & (nd != 0) & near_all & (near_any | amb[sel][:, None, None])
    edge[idx[em]] = True
    if not hit.any():
        return np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 3), np.uint8)
    t_of = np.broadcast_to(np.arange(len(sel))[:, None, None], hit.shape)[hit]
    Eh = np.stack([E[k][hit] for k in range(3)], 1)
    if bary == "screen":            # (a mutation: affine in the image plane, wrong under perspective)
        P = vc3[sel][t_of]                                                   # [M,3 vertices,3]
        ok = (P[:, :, 2] > 0).all(1)
        px, py = fx * P[:, :, 0] / P[:, :, 2] + cx, fy * P[:, :, 1] / P[:, :, 2] + cy
        X, Y = np.broadcast_to(xs, hit.shape)[hit].astype(np.float64), np.broadcast_to(ys, hit.shape)[hit].astype(np.float64)
        A = [(px[:, (k + 1) % 3] - X) * (py[:, (k + 2) % 3] - Y) - (px[:, (k + 2) % 3] - X) * (py[:, (k + 1) % 3] - Y) for k in range(3)]
        Eh = np.where(ok[:, None], np.stack(A, 1), Eh)
    S = Eh.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.where((S != 0)[:, None], Eh / np.where(S != 0, S, 1.0)[:, None], np.array([1.0, 0.0, 0.0]))
    c = (b[:, :, None] * cols[sel][t_of]).sum(1)                             # [M,3 channels]
    return idx[hit], z[hit], _to_u8(c, rounding)


def mesh_fragments(verts, faces, colors, c2w, K=K, H=H, W=W, z_near=Z_NEAR, z_far=Z_FAR, cull=True, edge_tol=EDGE_TOL,
                   bary="edge", rounding="nearest", cull_sign=1.0):
    """(pixel index int64 [M], z float64 [M], rgb uint8 [M,3], edge bool [H*W]) of one mesh from one camera."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[((f >= 0) & (f < len(v))).all(1)]
    col = np.full((len(v), 3), GREY, dtype=np.float64) if colors is None else np.asarray(colors)[:, :3].astype(np.float64)
    w2c = np.linalg.inv(np.asarray(c2w, dtype=np.float64))
    vc = v @ w2c[:3, :3].T + w2c[:3, 3]
    edge = np.zeros(H * W, dtype=bool)
    out = [(np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 3), np.uint8))]
    if len(f):
        v0, v1, v2 = vc[f[:, 0]], vc[f[:, 1]], vc[f[:, 2]]
        n = np.cross(v1 - v0, v2 - v0)
        nv0 = (n * v0).sum(1)
        m = [np.cross(v1, v2), np.cross(v2, v0), np.cross(v0, v1)]
        zs = np.stack([v0[:, 2], v1[:, 2], v2[:, 2]], 1)
        zmin, zmax = zs.min(1), zs.max(1)
        keep = (n != 0).any(1) & (zmax >= z_near) & (zmin <= z_far)
        with np.errstate(divide="ignore", invalid="ignore"):
            facing = nv0 / (np.linalg.norm(n, axis=1) * np.linalg.norm(v0, axis=1))
        amb = np.zeros(len(f), dtype=bool)
        if cull:
            amb = np.abs(np.nan_to_num(facing)) <= FACING_TOL
            keep &= (cull_sign * nv0 < 0) | amb          # an undecided one stays in: its pixels go into the mask
        whole = zmin <= z_near
        with np.errstate(divide="ignore", invalid="ignore"):
            px = K[0] * np.stack([v0[:, 0], v1[:, 0], v2[:, 0]], 1) / zs + K[2]
            py = K[1] * np.stack([v0[:, 1], v1[:, 1], v2[:, 1]], 1) / zs + K[3]
        big = 1e9
        px, py = np.nan_to_num(px, nan=0.0, posinf=big, neginf=-big), np.nan_to_num(py, nan=0.0, posinf=big, neginf=-big)
        x0 = np.ceil(np.clip(px.min(1) - rr.BOX_SLACK, 0, W)).astype(np.int64)
        x1 = np.floor(np.clip(px.max(1) + rr.BOX_SLACK, -1, W - 1)).astype(np.int64)
        y0 = np.ceil(np.clip(py.min(1) - rr.BOX_SLACK, 0, H)).astype(np.int64)
        y1 = np.floor(np.clip(py.max(1) + rr.BOX_SLACK, -1, H - 1)).astype(np.int64)
        for t in np.nonzero(keep & whole)[0]:
            x0[t], y0[t], x1[t], y1[t] = rr._clipped_box(np.stack([v0[t], v1[t], v2[t]]), 0.5 * z_near, K, H, W)
        keep &= (x0 <= x1) & (y0 <= y1)
        side = np.maximum(x1 - x0, y1 - y0) + 1
        cols = np.stack([col[f[:, 0]], col[f[:, 1]], col[f[:, 2]]], 1)       # [F,3 vertices,3 channels]
        vc3 = np.stack([v0, v1, v2], 1)
        args = (m, n, nv0, cols, amb, vc3, K, z_near, z_far, W, edge, edge_tol, bary, rounding)
        lo = 0
        for cls in (2, 4, 8, 16):
            sel = np.nonzero(keep & (side > lo) & (side <= cls))[0]
            step = max(1, (1 << 20) // (cls * cls))
            for a in range(0, len(sel), step):
                out.append(_mesh_block(sel[a:a + step], x0, y0, x1, y1, cls, cls, *args))
            lo = cls
        for t in np.nonzero(keep & (side > lo))[0]:
            out.append(_mesh_block(np.array([t]), x0, y0, x1, y1, int(x1[t] - x0[t] + 1), int(y1[t] - y0[t] + 1), *args))
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out]), edge


def _square(x0, y0, size, H, W):
    """Pixel indices [N, size*size] of the squares from (x0, y0), and which of them lie in the image."""
    o = np.arange(size)
    xs = x0[:, None, None] + o[None, None, :]
    ys = y0[:, None, None] + o[None, :, None]
    ok = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    return (ys * W + xs).reshape(len(x0), -1), ok.reshape(len(x0), -1)


def point_fragments(xyz, rgb, size, c2w, K=K, H=H, W=W, z_near=Z_NEAR, z_far=Z_FAR, snap="ceil"):
    """(pixel index [M], z [M], rgb uint8 [M,3], edge bool [H*W], undecided bool [N]) of one point set in float64."""
    fx, fy, cx, cy = K
    p = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    col = np.broadcast_to(np.asarray(rgb, dtype=np.uint8).reshape(-1, np.asarray(rgb).shape[-1])[:, :3], (len(p), 3))
    w2c = np.linalg.inv(np.asarray(c2w, dtype=np.float64))
    c = p @ w2c[:3, :3].T + w2c[:3, 3]
    z = c[:, 2]
    live = (z >= z_near) & (z <= z_far)
    near_plane = (np.abs(z - z_near) <= DEPTH_TIE * z_near) | (np.abs(z - z_far) <= DEPTH_TIE * z_far)
    zs = np.where(live | near_plane, z, 1.0)
    a, b = fx * c[:, 0] / zs + cx - 0.5 * size, fy * c[:, 1] / zs + cy - 0.5 * size
    # (a square wholly off the image takes no part: only a corner that can reach a pixel is undecided near an integer)
    reach = (a >= -size - 1.0) & (a <= W + 1.0) & (b >= -size - 1.0) & (b <= H + 1.0)
    snapped = reach & ((np.abs(a - np.round(a)) <= POINT_TOL) | (np.abs(b - np.round(b)) <= POINT_TOL))
    a, b = np.clip(a, -float(size), float(W)), np.clip(b, -float(size), float(H))
    rnd = np.ceil if snap == "ceil" else np.round
    x0, y0 = rnd(a).astype(np.int64), rnd(b).astype(np.int64)
    und = (near_plane & reach) | (live & snapped)
    edge = np.zeros(H * W, dtype=bool)
    u_ix = np.nonzero(und)[0]
    if len(u_ix):                                        # both squares the point may take: one pixel more on every side
        ii, ok = _square(np.floor(a[u_ix]).astype(np.int64) - 1, np.floor(b[u_ix]).astype(np.int64) - 1, size + 2, H, W)
        edge[ii[ok]] = True
    l_ix = np.nonzero(live)[0]
    ii, ok = _square(x0[l_ix], y0[l_ix], size, H, W)
    n_of = np.broadcast_to(l_ix[:, None], ii.shape)[ok]
    return ii[ok], z[n_of], col[n_of], edge, und


def composite(idx, z, rgb, n_pix, key="depth"):
    """The winner of each pixel among the fragments: smallest (z, colour word), or with key='colour' (a mutation) smallest
    (colour word, z).  (hit bool [n_pix], z [n_pix], rgb uint8 [n_pix,3], tie bool [n_pix]): tie marks the pixels where a
    fragment of another colour lies within DEPTH_TIE (relative) of the winning depth."""
    hit, zo, co, tie = np.zeros(n_pix, bool), np.zeros(n_pix), np.zeros((n_pix, 3), np.uint8), np.zeros(n_pix, bool)
    if len(idx) == 0:
        return hit, zo, co, tie
    word = pack(rgb)
    order = np.lexsort((word, z, idx)) if key == "depth" else np.lexsort((z, word, idx))
    i_s, z_s, w_s = idx[order], z[order], word[order]
    first = np.r_[True, i_s[1:] != i_s[:-1]]
    g = np.cumsum(first) - 1
    win = np.nonzero(first)[0]
    hit[i_s[win]] = True
    zo[i_s[win]] = z_s[win]
    co[i_s[win]] = rgb[order][win]
    zmin = np.minimum.reduceat(z_s, win)                 # (the nearest of the group, whatever the key order)
    close = (z_s - zmin[g] <= DEPTH_TIE * zmin[g]) & (w_s != w_s[win][g])
    tie[i_s[close]] = True
    return hit, zo, co, tie


def render(meshes, points, c2w, K=K, H=H, W=W, background=BACKGROUND, z_near=Z_NEAR, z_far=Z_FAR, cull=True, key="depth",
           snap="ceil", **mesh_mut):
    """The float64 model of ops.render_view for one camera: dict(rgb uint8 [H,W,3], depth float64 [H,W] (0 = background),
    hit bool [H,W], edge bool [H,W], undecided = list of bool [N] per point set)."""
    fr, edge, und = [], np.zeros(H * W, bool), []
    for v, f, c in meshes:
        i, z, rgb, e = mesh_fragments(v, f, c, c2w, K, H, W, z_near, z_far, cull, **mesh_mut)
        fr.append((i, z, rgb))
        edge |= e
    for xyz, rgb, size in points:
        i, z, col, e, u = point_fragments(xyz, rgb, size, c2w, K, H, W, z_near, z_far, snap)
        fr.append((i, z, col))
        edge |= e
        und.append(u)
    if fr:
        hit, z, rgb, tie = composite(np.concatenate([a[0] for a in fr]), np.concatenate([a[1] for a in fr]),
                                     np.concatenate([a[2] for a in fr]), H * W, key)
    else:
        hit, z, rgb, tie = composite(np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 3), np.uint8), H * W, key)
    rgb = np.where(hit[:, None], rgb, np.asarray(background, dtype=np.uint8))
    return dict(rgb=rgb.reshape(H, W, 3), depth=z.reshape(H, W), hit=hit.reshape(H, W), edge=(edge | tie).reshape(H, W),
                undecided=und)


# ----------------------------------------------------------------------------------------------
# the float32 model of the point path, operation by operation (eslam_viewer_points)
# ----------------------------------------------------------------------------------------------
EMPTY_KEY = np.uint64(0xffffffffffffffff)


def point_keys32(keys, xyz, rgb, size, w2c_rows, K, H, W, z_near=Z_NEAR, z_far=Z_FAR):
    """Min-combines into keys (uint64 [H*W]) the keys of the points: w2c_rows float32 [12] as the library gets them."""
    f32 = np.float32
    m = np.asarray(w2c_rows, dtype=f32).reshape(12)
    p = np.asarray(xyz, dtype=f32).reshape(-1, 3)
    col = np.asarray(rgb, dtype=np.uint8)
    col = np.broadcast_to(col.reshape(-1, col.shape[-1])[:, :3], (len(p), 3))
    fx, fy, cx, cy = (f32(k) for k in K)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    x = m[0] * px + m[1] * py + m[2] * pz + m[3]
    y = m[4] * px + m[5] * py + m[6] * pz + m[7]
    z = m[8] * px + m[9] * py + m[10] * pz + m[11]
    assert x.dtype == f32 and z.dtype == f32
    live = np.nonzero((z >= f32(z_near)) & (z <= f32(z_far)))[0]
    x, y, z, col = x[live], y[live], z[live], col[live]
    with np.errstate(over="ignore", invalid="ignore"):
        u, v = fx * x / z + cx, fy * y / z + cy
        half = f32(0.5) * f32(size)
        a = np.minimum(np.fmax(u - half, f32(-size)), f32(W))
        b = np.minimum(np.fmax(v - half, f32(-size)), f32(H))
    assert a.dtype == f32
    x0, y0 = np.ceil(a).astype(np.int64), np.ceil(b).astype(np.int64)
    ii, ok = _square(x0, y0, size, H, W)
    k = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | pack(col)
    np.minimum.at(keys, ii[ok], np.broadcast_to(k[:, None], ii.shape)[ok])
    return keys


def resolve_keys(keys, H, W, background=BACKGROUND):
    """(rgb uint8 [H,W,3], depth float32 [H,W]) of a key buffer."""
    hit = keys != EMPTY_KEY
    rgb = np.where(hit[:, None], unpack(keys & np.uint64(0xffffffff)), np.asarray(background, dtype=np.uint8))
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0))
    return rgb.reshape(H, W, 3), depth.reshape(H, W).astype(np.float32)


# ----------------------------------------------------------------------------------------------
# the criteria
# ----------------------------------------------------------------------------------------------
def _shifts(a, fill):
    """[9,H,W,...]: a and its 8 neighbours' values at each pixel (fill outside the image)."""
    pad = [(1, 1), (1, 1)] + [(0, 0)] * (a.ndim - 2)
    p = np.pad(a, pad, constant_values=fill)
    return np.stack([p[1 + dy:1 + dy + a.shape[0], 1 + dx:1 + dx + a.shape[1]] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])


def check_image(rgb, hit, ref, label, background=BACKGROUND, tol=1, edge_cap=EDGE_SHARE_CAP):
    """The parity rules of one view: rgb uint8 [H,W,3] and hit bool [H,W] (depth > 0) of the renderer under test against
    render()'s dict.  The mask's share is asserted first.  Outside the mask: the same coverage, every channel within `tol`
    (1: a float32 barycentric is good to about 1e-6, 3e-4 of a step of 255, so the rounding can fall one step the other way
    and no further; 0 for points, whose colours are not interpolated).  Inside: the reference at the pixel or at one of its
    8 neighbours (within tol), or background.  Returns the share of the pixels outside the mask that are one step off."""
    edge = ref["edge"]
    if edge_cap is not None:                                                  # (points: the cap is on the points, the caller's duty)
        assert edge.mean() <= edge_cap, (label, edge.mean())                  # the condition on the input comes first
    clear = ~edge
    bg = np.asarray(background, dtype=np.int64)
    d = np.abs(rgb.astype(np.int64) - ref["rgb"].astype(np.int64)).max(-1)
    cov = int((hit != ref["hit"])[clear].sum())
    worst = int(d[clear].max()) if clear.any() else 0
    is_bg = ~hit & (rgb.astype(np.int64) == bg).all(-1)
    refs, hits = _shifts(ref["rgb"].astype(np.int64), -1000), _shifts(ref["hit"], False)
    match = ((np.abs(rgb.astype(np.int64)[None] - refs).max(-1) <= tol) & (hits == hit[None])).any(0)
    bad_edge = int((edge & ~match & ~is_bg).sum())
    off = float((d[clear] > 0).mean()) if clear.any() else 0.0
    print(f"{label}: largest channel difference outside the mask {worst} ({100 * off:.4f} % of those pixels differ; "
          f"{100 * edge.mean():.4f} % of the pixels in the mask), coverage differs at {cov}, mask pixels unmatched {bad_edge}, "
          f"hit {100 * hit.mean():.1f} %")
    assert cov == 0, (label, cov)
    assert worst <= tol, (label, worst)
    assert not ((~hit & ~is_bg)[clear]).any(), label
    assert bad_edge == 0, (label, bad_edge)
    return off


# ----------------------------------------------------------------------------------------------
# the scenes of the parity tests: raster_ref's meshes and views with color_field
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    v, f = {"A": rr.scene_a, "B": rr.scene_b, "room": rr.scene_room, "ball": lambda: rr.icosphere(5, rr.BALL_R, rr.BALL_C)}[name]()
    return v, f, color_field(v)


def views(name):
    return rr.views_b() if name == "B" else rr.views_a()


@functools.lru_cache(maxsize=None)
def mesh_ref(name, k, cull):
    """render() of scene `name` from its view k: computed once a session, shared by the tests, not to be written to."""
    return render([scene(name)], [], views(name)[k], cull=cull)


POINTS_SEED = 3


def points_a(seed=POINTS_SEED, n=2000):
    """n random points around scene A's room for its view 0: most inside the room, some behind the camera, some nearer
    than z_near, some whose square straddles each border of the image.  (xyz float32 [n,3], rgb uint8 [n,4])."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(rr.ROOM_LO), np.asarray(rr.ROOM_HI)
    p = lo + (hi - lo) * rng.uniform(-0.1, 1.1, size=(n, 3))
    c2w = rr.views_a()[0]
    fx, fy, cx, cy = K
    # the last 200: placed in the camera frame - 40 nearer than z_near (beyond and behind), 160 on the four borders
    zc = np.concatenate([rng.uniform(-0.02, 0.009, 40), rng.uniform(0.3, 3.0, 160)])
    u = rng.uniform(0, W, 200)
    v = rng.uniform(0, H, 200)
    u[40:80], u[80:120] = rng.uniform(-9, 9, 40), W + rng.uniform(-9, 9, 40)
    v[120:160], v[160:200] = rng.uniform(-9, 9, 40), H + rng.uniform(-9, 9, 40)
    cam = np.stack([(u - cx) / fx * zc, (v - cy) / fy * zc, zc], 1)
    p[-200:] = cam @ c2w[:3, :3].T + c2w[:3, 3]
    return p.astype(np.float32), rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
