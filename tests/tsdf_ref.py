"""Plain numpy models of TSDF fusion (tests only; the product never imports it):

  integrate             the per-voxel rule of eslam_tsdf_integrate (include/eslam_hip.h).  dtype=np.float32 mirrors the
                        kernel operation for operation (same order, no contraction) and must give its bits;
                        dtype=np.float64 is the yardstick: the same rule on the same float32 inputs, in double.
  marching_cubes_masked marching cubes over the voxels with weight > 0, on tests/mesh_ref.py's tables and ordering.
  room_distance         the analytic room's distance to its surface (box walls and spheres).
  shared_input          the input every TSDF test uses: 8 frames of the toy scene's analytic room.
"""
import functools
import math

import numpy as np
import torch

from tests import mesh_ref

VOXEL, TRUNC = 0.04, 0.2


def volume_dims(bound, voxel):
    """(dims, origin float32 [3]) of ops.TSDFVolume(bound, voxel, ...)."""
    b = np.asarray(bound, dtype=np.float64).reshape(3, 2)
    dims = tuple(int(math.ceil(float(b[k, 1] - b[k, 0]) / float(voxel))) for k in range(3))
    return dims, b[:, 0].astype(np.float32)


def w2c_rows(c2ws):
    """float32 [n,12]: the 3x4 rows of the float64 inverse of each c2w with its columns 1 and 2 negated."""
    c = np.asarray(c2ws, dtype=np.float64).reshape(-1, 4, 4).copy()
    c[:, :3, 1] *= -1.0
    c[:, :3, 2] *= -1.0
    return np.linalg.inv(c)[:, :3, :].astype(np.float32).reshape(-1, 12)


class Volume:
    def __init__(self, dims, origin, voxel, trunc, color=True, dtype=np.float32):
        self.dims, self.dtype = tuple(dims), dtype
        # the inputs are the kernel's float32 values in either model
        self.origin = np.asarray(origin, dtype=np.float32).astype(dtype)
        self.voxel, self.trunc = dtype(np.float32(voxel)), dtype(np.float32(trunc))
        self.tsdf = np.zeros(self.dims, dtype=dtype)
        self.weight = np.zeros(self.dims, dtype=dtype)
        self.color = np.zeros(self.dims + (3,), dtype=dtype) if color else None
        self.pixels = []                       # per frame: int32 [nx,ny,nz], the pixel iv * W + iu that updated the voxel, -1 = none

    def integrate(self, depths, colors, w2c, K):
        """depths [n,H,W] float32, colors [n,H,W,3] float32 or None, w2c float32 [n,12], K = (fx, fy, cx, cy)."""
        T = self.dtype
        fx, fy, cx, cy = (T(np.float32(k)) for k in K)
        one, half = T(1), T(0.5)
        nx, ny, nz = self.dims
        ax = [self.origin[a] + (np.arange(n).astype(T) + half) * self.voxel for a, n in enumerate(self.dims)]
        px, py, pz = ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :]
        depths = np.asarray(depths, dtype=np.float32)
        H, W = depths.shape[1:]
        with np.errstate(all="ignore"):
            for k in range(depths.shape[0]):
                m = np.asarray(w2c[k], dtype=np.float32).astype(T)
                c = [((m[4 * r] * px + m[4 * r + 1] * py) + m[4 * r + 2] * pz) + m[4 * r + 3] for r in range(3)]
                ok = c[2] > 0
                u = (fx * c[0]) / c[2] + cx
                v = (fy * c[1]) / c[2] + cy
                iu, iv = np.floor(u + half), np.floor(v + half)
                ok = ok & (iu >= 0) & (iu < W) & (iv >= 0) & (iv < H)
                ju, jv = np.where(ok, iu, 0).astype(np.int64), np.where(ok, iv, 0).astype(np.int64)
                d = depths[k][jv, ju].astype(T)
                ok = ok & (d > 0)
                xn, yn = (iu - cx) / fx, (iv - cy) / fy
                ln = np.sqrt((one + xn * xn) + yn * yn)
                sdf = (d - c[2]) * ln
                ok = ok & (sdf > -self.trunc)
                t = np.minimum(one, sdf / self.trunc)
                w1 = self.weight + one
                self.tsdf = np.where(ok, (self.tsdf * self.weight + t) / w1, self.tsdf)
                if self.color is not None:
                    cin = np.asarray(colors[k], dtype=np.float32)[jv, ju].astype(T)
                    self.color = np.where(ok[..., None], (self.color * self.weight[..., None] + cin) / w1[..., None], self.color)
                self.weight = np.where(ok, w1, self.weight)
                self.pixels.append(np.where(ok, jv * W + ju, -1).astype(np.int32))
        assert self.tsdf.dtype == T and self.weight.dtype == T
        return self

    def mesh(self, level=0.0):
        """(verts float32, faces int32) as ops.TSDFVolume.extract_mesh places them."""
        o = self.origin.astype(np.float32).astype(np.float64) + 0.5 * float(np.float32(self.voxel))
        return marching_cubes_masked(self.tsdf.astype(np.float32), self.weight, level, o, (float(np.float32(self.voxel)),) * 3)


def marching_cubes_masked(vol, weight, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """mesh_ref.marching_cubes restricted to the observed part: a cube emits its faces only when all eight corners have
    weight > 0, an edge its vertex only when it crosses the level and one of the cubes around it is fully valid."""
    vol = np.asarray(vol, dtype=np.float32)
    level = np.float32(level)
    nx, ny, nz = vol.shape
    ntri, tri, _ = mesh_ref.load_tables()
    valid = np.asarray(weight) > 0
    if min(nx, ny, nz) < 2:
        return np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32)
    cube_ok = np.ones((nx - 1, ny - 1, nz - 1), dtype=bool)
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, (k >> 2) & 1
        cube_ok &= valid[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
    P = np.zeros((nx + 1, ny + 1, nz + 1), dtype=bool)            # cube (i, j, k) at P[i + 1, j + 1, k + 1]
    P[1:nx, 1:ny, 1:nz] = cube_ok
    ex = mesh_ref.crossings(vol, level)
    A, B = slice(1, None), slice(0, -1)                            # the cube at the point's index / one lower
    ex[..., 0] &= P[A, A, A] | P[A, B, A] | P[A, A, B] | P[A, B, B]
    ex[..., 1] &= P[A, A, A] | P[B, A, A] | P[A, A, B] | P[B, A, B]
    ex[..., 2] &= P[A, A, A] | P[B, A, A] | P[A, B, A] | P[B, B, A]
    flat = ex.reshape(-1)
    vid = np.full(flat.shape, -1, dtype=np.int64)
    vid[flat] = np.arange(int(flat.sum()))
    vid = vid.reshape(nx, ny, nz, 3)
    pi, pj, pk, ax = np.nonzero(ex)
    idx = np.stack([pi, pj, pk], 1).astype(np.float64)
    lo = vol[pi, pj, pk].astype(np.float64)
    step = np.eye(3, dtype=np.int64)[ax]
    hi = vol[pi + step[:, 0], pj + step[:, 1], pk + step[:, 2]].astype(np.float64)
    t = (np.float64(level) - lo) / (hi - lo)
    idx[np.arange(len(ax)), ax] += t
    verts = (np.asarray(origin, dtype=np.float64) + idx * np.asarray(spacing, dtype=np.float64)).astype(np.float32)
    b = (vol < level).astype(np.int64)
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, (k >> 2) & 1
        case |= b[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] << k
    case = np.where(cube_ok, case, 0)
    ci, cj, ck = np.nonzero(ntri[case] > 0)
    cs = case[ci, cj, ck]
    counts = ntri[cs]
    rep = np.repeat(np.arange(len(cs)), counts)
    tri_no = np.arange(len(rep)) - np.repeat(np.cumsum(counts) - counts, counts)
    faces = np.zeros((len(rep), 3), dtype=np.int64)
    for c3 in range(3):
        edges = tri[cs[rep], 3 * tri_no + c3]
        for e in range(12):
            sel = edges == e
            (dx, dy, dz), axis = mesh_ref.edge_owner(e)
            faces[sel, c3] = vid[ci[rep[sel]] + dx, cj[rep[sel]] + dy, ck[rep[sel]] + dz, axis]
    assert (faces >= 0).all()
    return verts, faces.astype(np.int32)


def face_cubes(vol, weight, level):
    """int64 [F,3]: the cube (lower corner index) of every face of marching_cubes_masked, in face order."""
    vol = np.asarray(vol, dtype=np.float32)
    nx, ny, nz = vol.shape
    ntri = mesh_ref.load_tables()[0]
    valid = np.asarray(weight) > 0
    b = (vol < np.float32(level)).astype(np.int64)
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    ok = np.ones(case.shape, dtype=bool)
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, (k >> 2) & 1
        case |= b[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] << k
        ok &= valid[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
    case = np.where(ok, case, 0)
    ci, cj, ck = np.nonzero(ntri[case] > 0)
    return np.repeat(np.stack([ci, cj, ck], 1), ntri[case[ci, cj, ck]], axis=0)


def room_distance(room, pts):
    """float64 [N]: the distance of pts [N,3] to the surface of synthscene.AnalyticRoom (inside the box, outside the
    spheres: the smallest of the distances to the six walls and to the spheres; exact there)."""
    p = np.asarray(pts, dtype=np.float64)
    lo, hi = room.lo.numpy(), room.hi.numpy()
    sd = np.minimum((p - lo).min(axis=1), (hi - p).min(axis=1))
    for c, r in room.spheres:
        sd = np.minimum(sd, np.linalg.norm(p - c.numpy(), axis=1) - r)
    return np.abs(sd)


def room_albedo(room, pts):
    """float64 [N,3]: AnalyticRoom.cast's colour at the surface point nearest to each of pts [N,3] (the point projected
    onto the nearest wall or sphere, with that object's index)."""
    p = np.asarray(pts, dtype=np.float64)
    lo, hi = room.lo.numpy(), room.hi.numpy()
    dl, dh = p - lo, hi - p
    best = np.minimum(dl.min(axis=1), dh.min(axis=1))
    q = p.copy()
    al, ah = dl.argmin(axis=1), dh.argmin(axis=1)
    use_lo = dl.min(axis=1) <= dh.min(axis=1)
    rows = np.arange(len(p))
    q[rows[use_lo], al[use_lo]] = lo[al[use_lo]]
    q[rows[~use_lo], ah[~use_lo]] = hi[ah[~use_lo]]
    obj = np.zeros(len(p))
    for k, (c, r) in enumerate(room.spheres):
        c = c.numpy()
        dist = np.linalg.norm(p - c, axis=1)
        sel = np.abs(dist - r) < np.abs(best)
        q[sel] = c + (p[sel] - c) * (r / dist[sel])[:, None]
        obj[sel] = k + 1
        best = np.where(sel, dist - r, best)
    ph = np.array([0.0, 2.1, 4.2])
    k1 = np.array([[2.1, 0.7, 1.3], [0.9, 2.3, 0.5], [1.1, 0.6, 2.6]])
    return np.clip(0.5 + 0.35 * np.sin(q @ k1.T + ph + obj[:, None] * 1.7), 0, 1)


@functools.lru_cache(maxsize=None)
def shared_input():
    """The input all TSDF tests share: the toy scene's analytic room, frames 0, 30, ..., 210 of trajectory(240), each
    rendered with 2 % depth holes (seed = frame index); a volume over the scene bound at voxel 0.04, truncation 0.2.
    Returns a namespace: sc, room, frames [(k, colour, depth, c2w)] (CPU tensors), K, depths, colors, w2c (numpy),
    dims, origin."""
    from types import SimpleNamespace
    from myslam_amd import scene, synthscene
    sc = scene.make_scene("toy")
    room = synthscene.AnalyticRoom(sc.bound)
    poses = synthscene.trajectory(240, sc.bound)
    frames = []
    for k in range(0, 240, 30):
        depth, color = synthscene.render_frame(room, sc, poses[k], "cpu", hole_frac=0.02, seed=k)
        frames.append((k, color, depth, poses[k]))
    dims, origin = volume_dims(sc.bound.numpy(), VOXEL)
    return SimpleNamespace(sc=sc, room=room, frames=frames, K=(sc.fx, sc.fy, sc.cx, sc.cy),
                           depths=np.stack([f[2].numpy() for f in frames]), colors=np.stack([f[1].numpy() for f in frames]),
                           w2c=w2c_rows(torch.stack([f[3] for f in frames]).numpy()), dims=dims, origin=origin)


@functools.lru_cache(maxsize=None)
def shared_model(dtype_name):
    """The float32 / float64 model's volume of the shared input (computed once, left unchanged by the tests)."""
    s = shared_input()
    dtype = {"float32": np.float32, "float64": np.float64}[dtype_name]
    return Volume(s.dims, s.origin, VOXEL, TRUNC, color=True, dtype=dtype).integrate(s.depths, s.colors, s.w2c, s.K)


@functools.lru_cache(maxsize=None)
def shared_mesh(dtype_name):
    return shared_model(dtype_name).mesh()


def sphere_field(shape=(23, 17, 70), seed=0, invalid=0.2):
    """(vol float32, weight float32) of the masked marching-cubes tests: a sphere's distance field and a random mask."""
    nx, ny, nz = shape
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).astype(np.float64)
    c = np.array([nx * 0.47, ny * 0.52, nz * 0.4])
    vol = (np.linalg.norm((g - c) * np.array([1.0, 1.0, 0.3]), axis=-1) - 0.38 * min(nx, ny)).astype(np.float32)
    rng = np.random.default_rng(seed)
    weight = (rng.random(shape) >= invalid).astype(np.float32) * rng.integers(1, 5, shape).astype(np.float32)
    return vol, weight
