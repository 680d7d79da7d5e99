"""Pins tests/tsdf_ref.py, the numpy models the GPU TSDF tests are held to (no GPU): the per-voxel rule by hand on a plane,
the float32 mirror against the float64 yardstick, the float64 model's mesh against the analytic room, and the masked
marching cubes against tests/mesh_ref.py."""
import numpy as np

from tests import mesh_ref, tsdf_ref as R

WEIGHT_CAP = 1e-3            # share of voxels on which the float32 and float64 models may disagree on `weight`


def test_plane_by_hand():
    """A fronto-parallel plane at depth 1.5 seen by one camera at the origin (looking along +z, x right, y down)."""
    dims, origin, voxel, trunc = (20, 20, 30), (-1.0, -1.0, -0.5), 0.1, 0.3
    fx = fy = 40.0
    cx, cy, W, H = 31.5, 23.5, 64, 48
    w2c = np.eye(4)[:3].reshape(1, 12).astype(np.float32)
    depth = np.full((1, H, W), 1.5, dtype=np.float32)

    def pixel(i, j, k):
        p = np.float32(origin) .astype(np.float64) + (np.array([i, j, k]) + 0.5) * np.float64(np.float32(voxel))
        return p, int(np.floor(fx * p[0] / p[2] + cx + 0.5)), int(np.floor(fy * p[1] / p[2] + cy + 0.5))

    _, hu, hv = pixel(12, 9, 14)
    depth[0, hv, hu] = 0.0                                            # a depth hole under one chosen voxel
    vol = R.Volume(dims, origin, voxel, trunc, color=False, dtype=np.float64).integrate(depth, None, w2c, (fx, fy, cx, cy))
    for i, j, k in [(10, 10, 12), (7, 12, 19), (11, 8, 21), (13, 13, 22), (9, 9, 7), (12, 9, 13)]:
        p, iu, iv = pixel(i, j, k)
        assert 0 <= iu < W and 0 <= iv < H and (iu, iv) != (hu, hv)
        m = np.sqrt(1.0 + ((iu - cx) / fx) ** 2 + ((iv - cy) / fy) ** 2)
        want = min(1.0, (1.5 - p[2]) * m / np.float64(np.float32(trunc)))
        assert want > -1.0 and vol.weight[i, j, k] == 1.0
        assert abs(vol.tsdf[i, j, k] - want) <= 1e-12, (i, j, k, vol.tsdf[i, j, k], want)
    assert vol.tsdf[10, 10, 12] == 1.0 and -1.0 < vol.tsdf[13, 13, 22] < 0.0          # clamped in front, negative behind
    assert (vol.weight[:, :, :5] == 0).all()                          # z < 0: behind the camera
    assert vol.weight[0, 10, 5] == 0 and vol.weight[10, 0, 5] == 0    # z = 0.05, |x| or |y| = 0.95: outside the image
    assert vol.weight[12, 9, 14] == 0                                 # on the hole
    assert (vol.weight[:, :, 24:] == 0).all()                         # z >= 1.95: (1.5 - z) m <= -0.45 < -trunc
    assert vol.weight[10, 10, 22] == 1 and vol.weight[10, 10, 23] == 0                # z = 1.75 in, z = 1.85 out
    assert vol.weight.max() == 1.0 and vol.weight.sum() > 1000


def test_float32_mirror_against_the_float64_yardstick():
    """Measured on the shared input (102 x 78 x 66 voxels, 8 frames, 41.5 % of the voxels observed): the two models
    disagree on `weight` for 0.0223 % of the voxels (pixel-boundary flips of floor(u + 0.5) and of sdf > -trunc); where the
    weights and the chosen pixels agree, max |tsdf32 - tsdf64| = 1.9e-6 and max |colour32 - colour64| = 3.0e-8."""
    m32, m64 = R.shared_model("float32"), R.shared_model("float64")
    assert m32.tsdf.dtype == np.float32 and m32.weight.dtype == np.float32 and m32.color.dtype == np.float32
    share = float((m32.weight != m64.weight).mean())
    same = m32.weight == m64.weight
    for a, b in zip(m32.pixels, m64.pixels):
        same &= a == b
    dt = float(np.abs(m32.tsdf[same] - m64.tsdf[same]).max())
    dc = float(np.abs(m32.color[same] - m64.color[same]).max())
    print(f"\nweight disagreement {share * 100:.4f} %, observed {(m64.weight > 0).mean() * 100:.1f} %, max dtsdf {dt:.2e}, "
          f"max dcolour {dc:.2e}")
    assert share <= WEIGHT_CAP
    assert (m64.weight > 0).mean() > 0.3 and m64.weight.max() >= 2
    assert dt <= 1e-5 and dc <= 1e-5


def far_share(room, verts):
    """(median distance, share beyond voxel / 2) of mesh vertices to the analytic room's surface."""
    d = R.room_distance(room, verts)
    return float(np.median(d)), float((d > R.VOXEL / 2).mean())


def test_float64_mesh_lies_on_the_analytic_room():
    """The float64 model's masked mesh of the shared input: V = 24084, F = 44537; distance of the vertices to the analytic
    surface: median 0.129 mm, 99th percentile 1.09 cm, 0.345 % beyond voxel / 2, 0.042 % beyond one voxel (depth
    discontinuities at the spheres' silhouettes).  (The float32 model's mesh: V = 24091, F = 44545, 0.340 % beyond
    voxel / 2.)  Twice the float64 share beyond voxel / 2 is the bound the GPU mesh is held to."""
    s = R.shared_input()
    v, f = R.shared_mesh("float64")
    d = R.room_distance(s.room, v)
    med, far = far_share(s.room, v)
    print(f"\nV = {len(v)}, F = {len(f)}: median {med * 1e3:.3f} mm, p99 {np.percentile(d, 99) * 100:.2f} cm, "
          f"{far * 100:.3f} % beyond voxel/2, {(d > R.VOXEL).mean() * 100:.3f} % beyond one voxel")
    assert len(v) > 20000 and len(f) > 40000
    assert med <= R.VOXEL / 20
    assert 0 < far <= 0.01                                   # the figure the GPU bound is built on stays a small share
    assert np.array_equal(np.unique(f), np.arange(len(v)))   # no unreferenced vertex
    v32, _ = R.shared_mesh("float32")
    assert far_share(s.room, v32)[1] <= 2 * far


def test_masked_marching_cubes_all_valid_equals_mesh_ref():
    vol, _ = R.sphere_field()
    for shape_vol in (vol, vol[:9, :8, :11].copy()):
        v0, f0 = mesh_ref.marching_cubes(shape_vol, 0.0, (0.5, -1.0, 2.0), (0.1, 0.2, 0.3))
        v1, f1 = R.marching_cubes_masked(shape_vol, np.ones_like(shape_vol), 0.0, (0.5, -1.0, 2.0), (0.1, 0.2, 0.3))
        assert len(f0) > 0 and np.array_equal(f0, f1) and np.array_equal(v0.view(np.int32), v1.view(np.int32))


def test_masked_marching_cubes_on_a_random_mask():
    """23 x 17 x 70 sphere field, 20 % of the voxels invalid: every face lies in a fully valid cube, every vertex is
    referenced, and the faces are exactly the unmasked mesh's faces of the fully valid cubes, in order."""
    vol, weight = R.sphere_field()
    assert abs((weight == 0).mean() - 0.2) < 0.02
    v, f = R.marching_cubes_masked(vol, weight, 0.0)
    v0, f0 = mesh_ref.marching_cubes(vol, 0.0)
    assert 0 < len(f) < len(f0)
    assert np.array_equal(np.unique(f), np.arange(len(v)))

    def cubes(verts, faces):                                 # a face's cube from its geometry: the floor of its vertices' minimum
        return np.floor(verts[faces].astype(np.float64).min(axis=1)).astype(np.int64)

    valid = weight > 0
    cube_ok = np.ones(tuple(n - 1 for n in vol.shape), dtype=bool)
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, (k >> 2) & 1
        cube_ok &= valid[dx:vol.shape[0] - 1 + dx, dy:vol.shape[1] - 1 + dy, dz:vol.shape[2] - 1 + dz]
    c = cubes(v, f)
    assert cube_ok[c[:, 0], c[:, 1], c[:, 2]].all()
    assert np.array_equal(c, R.face_cubes(vol, weight, 0.0))
    c0 = cubes(v0, f0)
    keep = cube_ok[c0[:, 0], c0[:, 1], c0[:, 2]]
    assert keep.sum() == len(f)                              # no face lost from a fully valid cube
    assert np.array_equal(v[f].view(np.int32), v0[f0[keep]].view(np.int32))
