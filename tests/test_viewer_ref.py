"""The viewer's reference model and criteria without a GPU (tests/viewer_ref.py): the conditions the GPU tests rely on
(the masks stay under their caps for the chosen scenes, views and seed; the float32 point model agrees with the float64
one outside the mask), the frontend's geometry against values recorded from the reference (tests/golden/
viewer_reference.npz, written by tests/golden/make_viewer_golden.py), and that the criteria reject mutated definitions."""
import os

import numpy as np
import pytest

from tests import raster_ref as rr
from tests import viewer_ref as vr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viewer_reference.npz")
# a small camera for the mutation checks: the views of scene A at a quarter of the size
HS = WS = 125
KS = (75.0, 75.0, 62.0, 62.0)


@pytest.mark.parametrize("scene", ["A", "B"])
def test_mesh_masks_stay_under_the_cap(scene):
    for k in range(len(vr.views(scene))):
        for cull in (True, False):
            r = vr.mesh_ref(scene, k, cull)
            assert r["edge"].mean() <= vr.EDGE_SHARE_CAP, (scene, k, cull, r["edge"].mean())
            assert r["hit"].mean() > 0.2
            vr.check_image(r["rgb"], r["hit"], r, f"scene {scene} view {k} cull {cull} against itself")
    # culling changes the picture where the camera sees a back face first: inside the ball nothing is left of it
    inside = rr.look_at(rr.BALL_C, (2.0, 1.5, 1.2))
    ball = vr.scene("ball")
    assert vr.render([ball], [], inside, cull=False)["hit"].all() and not vr.render([ball], [], inside, cull=True)["hit"].any()


def test_colour_is_perspective_correct():
    """A quad at a slant whose colour is linear in world x: the model's colour at a pixel is that linear function at the
    point the pixel's ray hits, not at the point an interpolation in the image plane would name."""
    v = np.array([[-1, -1, 1], [1, -1, 5], [1, 1, 5], [-1, 1, 1]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    c = np.array([[0, 0, 0, 0], [250, 0, 0, 0], [250, 0, 0, 0], [0, 0, 0, 0]], dtype=np.uint8)
    r = vr.render([(v, f, c)], [], np.eye(4), K=KS, H=HS, W=WS, cull=False)
    xs = np.arange(WS)
    dx = (xs - KS[2]) / KS[0]
    z = 3.0 / (1.0 - 2.0 * dx)                           # the plane z = 3 + 2 x along the row through the centre
    want = 125.0 * (dx * z + 1.0)
    row = HS // 2
    ok = r["hit"][row] & ~r["edge"][row]
    assert ok.sum() > 30 and np.abs(r["rgb"][row, ok, 0] - want[ok]).max() <= 0.5 + 1e-9
    assert np.abs(r["depth"][row, ok] - z[ok]).max() <= 1e-12


@pytest.mark.parametrize("size", [1, 4, 16])
def test_point_models_agree_and_the_seed_keeps_the_mask_small(size):
    from myslam_amd import ops
    import torch
    xyz, rgba = vr.points_a()
    c2w = rr.views_a()[0]
    for rgb in (rgba, rgba[7]):
        r = vr.render([], [(xyz, rgb, size)], c2w)
        und = r["undecided"][0]
        assert und.mean() <= vr.EDGE_SHARE_CAP, und.mean()
        rows = ops._w2c_rows(c2w[None], torch.device("cpu")).numpy()[0]
        keys = vr.point_keys32(np.full(vr.H * vr.W, vr.EMPTY_KEY), xyz, rgb, size, rows, vr.K, vr.H, vr.W)
        img, depth = vr.resolve_keys(keys, vr.H, vr.W)
        vr.check_image(img, depth > 0, r, f"float32 point model, size {size}", tol=0, edge_cap=None)
        clear = ~r["edge"]
        assert np.abs(depth - r["depth"])[clear].max() <= 1e-5
    # the set does what it is for: points behind the camera and nearer than z_near, squares cut by each border
    w2c = np.linalg.inv(c2w)
    cam = xyz.astype(np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
    assert (cam[:, 2] < 0).sum() >= 20 and ((cam[:, 2] > 0) & (cam[:, 2] < vr.Z_NEAR)).sum() >= 5
    live = cam[:, 2] >= vr.Z_NEAR
    u, v = vr.K[0] * cam[live, 0] / cam[live, 2] + vr.K[2], vr.K[1] * cam[live, 1] / cam[live, 2] + vr.K[3]
    for t, n in ((u, vr.W), (v, vr.H)):
        assert (np.abs(t) < 1.5).sum() >= 3 and (np.abs(t - n) < 1.5).sum() >= 3


def test_camera_actor_and_colours_against_the_reference():
    from myslam_amd.src.tools import visualizer_util as vu
    g = np.load(GOLDEN)
    for s, want in zip(g["scales"], g["actor_points"]):
        got = vu.camera_actor_points(float(s))
        assert got.shape == (1200, 3) and got.dtype == np.float64 and np.array_equal(got, want)
    assert tuple(np.round(g["color_est"] * 255).astype(int)) == vu.RED and tuple(np.round(g["color_gt"] * 255).astype(int)) == vu.GREEN
    assert int(g["point_size"]) == vu.POINT_SIZE and not bool(g["back_face"])
    assert (vu.WINDOW_H, vu.WINDOW_W) == (1080, 1920)
    fx, fy, cx, cy = vu.window_intrinsics(1080, 1920)
    assert fx == fy and abs(np.degrees(2 * np.arctan(540.0 / fy)) - 60.0) <= 1e-12 and (cx, cy) == (959.5, 539.5)


def test_viewing_pose_against_the_reference():
    from myslam_amd.src.tools import visualizer_util as vu
    g = np.load(GOLDEN)
    for init, ext in zip(g["init_poses"], g["extrinsics"]):
        keep = init.copy()
        c2w = vu.viewing_pose(init)
        assert np.array_equal(init, keep)                                  # (the caller's matrix is left alone)
        assert np.abs(np.linalg.inv(c2w) - ext).max() <= 1e-12
        # 4 m behind the initial camera, looking back along its z column
        assert np.abs(c2w[:3, 3] - (init[:3, 3] + 4.0 * init[:3, 2])).max() <= 1e-12
        assert np.abs(c2w[:3, 2] + init[:3, 2]).max() == 0.0


def test_frontend_state_without_a_gpu():
    """update_pose negates the z column on a copy and places the glyph; the trajectories drop non-finite rows."""
    import torch
    from myslam_amd.src.tools import visualizer_util as vu
    est = np.tile(np.eye(4), (5, 1, 1))
    est[:, :3, 3] = np.arange(15).reshape(5, 3)
    gt = est.copy()
    gt[2, :3, 3] = np.nan
    fe = vu.SLAMFrontend("unused", np.eye(4), cam_scale=0.2, estimate_c2w_list=est, gt_c2w_list=gt, size=(30, 40), device="cpu")
    assert (fe.H, fe.W) == (30, 40) and fe.z_near > 0
    pose = est[1].copy()
    fe.update_pose(1, torch.from_numpy(pose), gt=False)
    fe.update_pose(1, pose, gt=True)
    assert np.array_equal(pose, est[1]) and sorted(fe.cameras) == [1, 1 + vu.GT_KEY]
    pts = fe.cameras[1][0].numpy()
    flipped = pose.copy()
    flipped[:3, 2] *= -1
    want = vu.camera_actor_points(0.2) @ flipped[:3, :3].T + flipped[:3, 3]
    assert np.abs(pts - want).max() <= 1e-6 and pts[:, 2].min() < pose[2, 3] - 0.25     # the glyph opens towards -z
    fe.update_cam_trajectory(4, gt=False)
    fe.update_cam_trajectory(4, gt=True)
    assert fe.traj[False].shape == (4, 3) and fe.traj[True].shape == (3, 3)
    fe.reset()
    assert fe.cameras == {} and fe.start() is fe


# ----------------------------------------------------------------------------------------------
# the criteria reject mutated definitions
# ----------------------------------------------------------------------------------------------
def _small(meshes, points, k=0, **kw):
    return vr.render(meshes, points, rr.views_a()[k], K=KS, H=HS, W=WS, **kw)


def _rejected(mutant, ref, label, **kw):
    with pytest.raises(AssertionError):
        vr.check_image(mutant["rgb"], mutant["hit"], ref, label, **kw)


def test_criteria_reject_mutations():
    a = vr.scene("A")
    ref = _small([a], [])
    vr.check_image(ref["rgb"], ref["hit"], ref, "the model against itself")
    _rejected(_small([a], [], bary="screen"), ref, "barycentrics in the image plane")
    _rejected(_small([a], [], cull_sign=-1.0), ref, "flipped back-face rule")
    # truncation moves an interpolated channel by at most one step, which the bound of 1 allows; a mesh of one colour
    # shows it: c = 200 (b0 + b1 + b2) lies within 200 x 3e-7 of 200, to nearest that is 200 exactly, truncated it is 199
    # wherever the sum falls below 1
    grey = (a[0], a[1], None)
    ref_g = _small([grey], [])
    assert (ref_g["rgb"][ref_g["hit"]] == 200).all()
    vr.check_image(ref_g["rgb"], ref_g["hit"], ref_g, "the grey model against itself", tol=0)
    _rejected(_small([grey], [], rounding="trunc"), ref_g, "truncating conversion", tol=0)
    # points: squares placed by round instead of ceil; the key with the colour above the depth
    xyz, rgba = vr.points_a()
    pts = [(xyz, rgba, 4)]
    ref_p = _small([a], pts)
    vr.check_image(ref_p["rgb"], ref_p["hit"], ref_p, "mesh and points against itself", edge_cap=None)
    _rejected(_small([a], pts, snap="round"), ref_p, "round instead of ceil", edge_cap=None)
    _rejected(_small([a], pts, key="colour"), ref_p, "colour above depth in the key", edge_cap=None)


def test_key_order_at_equal_depth():
    """Two points at one depth on one pixel: the smaller colour word wins (R is the lowest byte, so B decides first)."""
    xyz = np.array([[0, 0, 2], [0, 0, 2]], dtype=np.float32)
    rgb = np.array([[255, 0, 1, 9], [0, 255, 0, 9]], dtype=np.uint8)
    r = vr.render([], [(xyz, rgb, 1)], np.eye(4), K=KS, H=HS, W=WS)
    assert r["hit"].sum() == 1 and tuple(r["rgb"][r["hit"]][0]) == (0, 255, 0)
    keys = vr.point_keys32(np.full(HS * WS, vr.EMPTY_KEY), xyz, rgb, 1, np.eye(4)[:3].reshape(12), KS, HS, WS)
    img, depth = vr.resolve_keys(keys, HS, WS)
    assert (depth > 0).sum() == 1 and tuple(img[depth > 0][0]) == (0, 255, 0) and depth.max() == 2.0
