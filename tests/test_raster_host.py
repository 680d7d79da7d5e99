"""The 2D metric's host side, no GPU: the float64 reference rasteriser (tests/raster_ref.py) on cases with known answers,
the condition the GPU parity scenes must meet (few pixels within 1e-3 px of an edge), the camera box of get_cam_position,
and check_proj against a literal transcription of the reference's steps."""
import numpy as np
import pytest
import torch

from tests import raster_ref as rr

EDGE_SHARE_CAP = 0.01


def _ray_norm():
    fx, fy, cx, cy = rr.K
    xs, ys = np.meshgrid(np.arange(rr.W), np.arange(rr.H))
    return np.sqrt(((xs - cx) / fx) ** 2 + ((ys - cy) / fy) ** 2 + 1.0)


def test_reference_wall_at_known_distance():
    # a wall z = 2.5 in front of the camera, larger than the view: every pixel reads 2.5; and cond = 1 / |d|
    v = np.array([[-9, -9, 2.5], [9, -9, 2.5], [9, 9, 2.5], [-9, 9, 2.5]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    d, edge, c = rr.rasterize(v, f, np.eye(4))
    assert np.abs(d - 2.5).max() <= 1e-12
    assert np.abs(c - 1.0 / _ray_norm()).max() <= 1e-12
    # the shared diagonal passes through no pixel centre's 1e-3 neighbourhood except where it does: but it leaves no hole
    assert (d > 0).all()
    # moved: camera at z = 1 looking along +z sees it at 1.5; beyond z_far nothing
    c2w = np.eye(4)
    c2w[2, 3] = 1.0
    assert np.abs(rr.rasterize(v, f, c2w)[0] - 1.5).max() <= 1e-12
    assert (rr.rasterize(v, f, np.eye(4), z_far=2.0)[0] == 0).all()
    # looking away: nothing
    assert (rr.rasterize(v, f, rr.look_at((0, 0, 0), (0, 0, -1), up=(0, 1, 0)))[0] == 0).all()


def test_reference_sphere_from_its_centre():
    R = 2.0
    v, f = rr.icosphere(5, R)
    assert len(f) == 20480
    d, edge, _ = rr.rasterize(v, f, np.eye(4))
    face_sag, edge_sag = rr.icosphere_sag(v, f, R)
    err = R / _ray_norm() - d
    print(f"sphere: max depth error {err.max():.3e} min {err.min():.3e}, face sag {face_sag:.3e}, edge sag {edge_sag:.3e}")
    # Flat faces lie inside the sphere: the depth is at most R / |d| and short of it by at most the sag over |d|.  The bound
    # is the faces' exact sag R - min plane distance (5.70e-4 here).  The sag of the longest edge's middle,
    # R (1 - cos(theta / 2)) = 4.27e-4, is exceeded by a correct render (5.40e-4): face centres lie deeper than edges.
    assert (d > 0).all()
    assert err.min() >= -1e-6 and err.max() <= face_sag + 1e-6       # (the float32 vertices are off the sphere by 1e-7)
    assert edge_sag < err.max()


def test_reference_triangle_straddling_the_camera_plane():
    # a floor y = 0.2 from z = -5 (behind the camera) to z = +5: a pixel of row j sees it at z = 0.2 fy / (j - cy), beyond z_near only
    v = np.array([[-50, 0.2, -5], [50, 0.2, -5], [0, 0.2, 5]], dtype=np.float32)
    f = np.array([[0, 1, 2]], dtype=np.int32)
    d, _, _ = rr.rasterize(v, f, np.eye(4))
    fx, fy, cx, cy = rr.K
    rows = np.arange(rr.H)
    with np.errstate(divide="ignore"):
        expect = float(np.float32(0.2)) * fy / (rows - cy)
    col = rr.W // 2
    for j in rows:
        inside = 0 < expect[j] <= 5.0 - 1e-9 and abs(((col - cx) / fx) * expect[j]) < 50 * (5 - expect[j]) / 10
        if inside:
            assert abs(d[j, col] - expect[j]) <= 1e-9 * expect[j], j
        elif expect[j] < 0 or expect[j] > 5.0 + 1e-9:
            assert d[j, col] == 0, j
    assert (d[: rr.H // 2] == 0).all() and (d[rr.H // 2 + 100:, col] > 0).all()
    # with a near plane at 1 m the rows that see the floor nearer than that are empty
    d1, _, _ = rr.rasterize(v, f, np.eye(4), z_near=1.0)
    assert ((d1 == 0) | (d1 >= 1.0)).all() and (d1 > 0).any() and ((d > 0) & (d < 1.0) & (d1 == 0)).any()


@pytest.mark.parametrize("scene", ["A", "B"])
def test_parity_scenes_have_few_edge_pixels(scene):
    """A condition on the inputs of tests/test_gpu_raster.py: at most 1 % of a view's pixels lie within 1e-3 px of an edge."""
    mesh, views = (rr.scene_a(), rr.views_a()) if scene == "A" else (rr.scene_b(), rr.views_b())
    assert len(mesh[1]) == (12 + 20480 if scene == "A" else 327680)
    for k, c2w in enumerate(views):
        d, edge, c = rr.rasterize(*mesh, c2w)
        print(f"scene {scene} view {k}: edge share {100 * edge.mean():.4f} %, hit {100 * (d > 0).mean():.1f} %")
        assert edge.mean() <= EDGE_SHARE_CAP
        assert (d > 0).mean() > 0.2


def _rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] *= -1
    return q


def test_get_cam_position_recovers_a_rotated_cuboid():
    from myslam_amd.src.tools import eval_recon as ev
    ext = np.array([2.5, 4.0, 7.0])
    corners = np.array([[(k >> a) & 1 for a in range(3)] for k in range(8)], dtype=np.float64) - 0.5
    for seed in range(3):
        R, t = _rotation(seed), np.array([0.3, -1.2, 0.8])
        v = (corners * ext) @ R.T + t
        extents, transform = ev.get_cam_position(v)
        assert np.allclose(extents, ext * np.array([0.3, 0.7, 0.7]), rtol=1e-4, atol=0)
        assert np.allclose(transform[:3, 3], t + np.array([0, 0, 0.4]), atol=1e-6)
        A = transform[:3, :3]
        assert np.allclose(A.T @ A, np.eye(3), atol=1e-9) and np.linalg.det(A) > 0
        # the box axes are the cuboid's, up to sign, in ascending order of extent
        assert np.allclose(np.abs(A.T @ R), np.eye(3), atol=1e-6)


def test_get_cam_position_box_contains_the_cloud():
    from myslam_amd.src.tools import eval_recon as ev
    rng = np.random.default_rng(3)
    v = rng.normal(size=(5000, 3)) * np.array([3.0, 1.0, 0.4]) @ _rotation(5).T + np.array([1.0, 2.0, -0.5])
    extents, transform = ev.get_cam_position(torch.from_numpy(v))
    full = extents / np.array([0.3, 0.7, 0.7])
    assert (np.diff(full) >= 0).all()
    centre = transform[:3, 3] - np.array([0, 0, 0.4])
    local = (v - centre) @ transform[:3, :3]
    assert (np.abs(local) <= 0.5 * full + 1e-9).all()
    # and tightly: some point touches each pair of faces
    assert np.allclose(local.max(0) - local.min(0), full, rtol=1e-9)
    # no larger than the world-aligned and the PCA-aligned boxes, which are candidates
    w = (v.max(0) - v.min(0)).prod()
    p = v @ np.linalg.eigh(np.cov(v.T))[1]
    assert full.prod() <= min(w, (p.max(0) - p.min(0)).prod()) * (1 + 1e-9)
    assert len(ev.box_candidates(np.cov(v.T))) == 2 * 3 * ev.BOX_ANGLES


def _check_proj_reference(points, W, H, fx, fy, cx, cy, c2w):
    """The steps of the reference's check_proj (eval_recon.py:59-85) written out one at a time in numpy, each in the
    precision the reference has there: float64 up to the inverse, float32 from the cast of w2c on."""
    flipped = np.array(c2w, dtype=np.float64)
    flipped[:3, 1] = -flipped[:3, 1]                           # columns 1 and 2 negated
    flipped[:3, 2] = -flipped[:3, 2]
    w2c = np.linalg.inv(flipped).astype(np.float32)            # float64 inverse, then float32
    p = np.asarray(points).astype(np.float32)
    in_view = 0
    for q in p:
        cam = w2c @ np.array([q[0], q[1], q[2], 1.0], dtype=np.float32)
        x, y, zc = -cam[0], cam[1], cam[2]                     # x mirrored
        a = np.float32(fx) * x + np.float32(0.0) * y + np.float32(cx) * zc      # K (x, y, z)
        b = np.float32(0.0) * x + np.float32(fy) * y + np.float32(cy) * zc
        z = zc + np.float32(1e-5)
        u, v = a / z, b / z
        in_view += bool(0 <= -z and 0 < u < W and 0 < v < H)
    return in_view > 0


def test_check_proj_matches_the_reference_steps():
    from myslam_amd.src.tools import eval_recon as ev
    W = H = 500
    fx = fy = 300.0
    cx = cy = 249.5
    origin = np.array([0.5, -0.2, 0.3])
    c2w = np.eye(4)
    c2w[:3, :] = ev.viewmatrix(np.array([1.0, 0.4, -0.1]), [0, 0, -1], origin)
    R = c2w[:3, :3]
    # check_proj's camera has x mirrored: u = fx (-(-x)) ... derive the pixel of a camera-frame point from the steps:
    # c = (x, -y, -z) after the column flips, then c.x *= -1: u = (-fx x + cx (-z)) / (-z) = fx x / z + cx,
    # v = (fy (-y) + cy (-z)) / (-z) = fy y / z + cy: the pinhole image of the +z-looking camera
    def world(u, v, z):
        return origin + R @ np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
    cases = {
        "centre in front": (world(249.5, 249.5, 2.0), True),
        "behind": (world(249.5, 249.5, -2.0), False),
        "just inside left": (world(0.5, 250.0, 1.0), True),
        "just outside left": (world(-0.5, 250.0, 1.0), False),
        "just inside right": (world(499.5, 250.0, 1.0), True),
        "just outside right": (world(500.5, 250.0, 1.0), False),
        "just inside top": (world(250.0, 0.5, 3.0), True),
        "just outside top": (world(250.0, -0.5, 3.0), False),
        "just inside bottom": (world(250.0, 499.5, 3.0), True),
        "just outside bottom": (world(250.0, 500.5, 3.0), False),
    }
    for name, (p, expect) in cases.items():
        pts = p[None, :].astype(np.float64)
        assert bool(_check_proj_reference(pts, W, H, fx, fy, cx, cy, c2w)) is expect, name
        assert ev.check_proj(pts, W, H, fx, fy, cx, cy, c2w) is expect, name
    # any(): a cloud of outsiders with one insider
    outs = np.stack([p for p, e in cases.values() if not e])
    assert ev.check_proj(outs, W, H, fx, fy, cx, cy, c2w) is False
    assert ev.check_proj(np.concatenate([outs, cases["just inside top"][0][None]]), W, H, fx, fy, cx, cy, c2w) is True
    # random clouds and views: the two agree
    rng = np.random.default_rng(0)
    agree = seen = 0
    for k in range(40):
        o = rng.uniform(-1, 1, size=3)
        c = np.eye(4)
        c[:3, :] = ev.viewmatrix(rng.uniform(-1, 1, size=3), [0, 0, -1], o)
        pts = rng.normal(size=(3, 3)) * 2.0
        a, b = bool(_check_proj_reference(pts, W, H, fx, fy, cx, cy, c)), ev.check_proj(pts, W, H, fx, fy, cx, cy, c)
        agree += a == b
        seen += a
    assert agree == 40 and 0 < seen < 40


def test_viewmatrix_is_the_references():
    from myslam_amd.src.tools import eval_recon as ev
    m = ev.viewmatrix(np.array([0.0, 2.0, 0.0]), [0, 0, -1], np.array([1.0, 2.0, 3.0]))
    assert m.shape == (3, 4)
    assert np.allclose(m[:, 2], [0, 1, 0]) and np.allclose(m[:, 3], [1, 2, 3])
    assert np.allclose(m[:, 0], np.cross([0, 0, -1], [0, 1, 0])) and np.allclose(m[:, 1], np.cross(m[:, 2], m[:, 0]))
