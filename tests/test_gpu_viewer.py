"""The offline viewer on the GPU: ops.render_view (eslam_viewer_*) against the float64 model and the criteria of
tests/viewer_ref.py, the float32 point model bit for bit, both triangle paths, composition through the key buffer,
shapes that catch index errors, and python -m myslam_amd.visualizer end to end on a tiny run.

The bound on a channel outside the edge mask is derived, not measured: a float32 barycentric is good to about 1e-6, which
is 3e-4 of a step of 255, so the rounding can fall one step the other way and no further.  A mesh of one colour must give
that colour exactly.  Measured on an MI355X (printed by every run): see DESIGN.md section 20."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import raster_ref as rr
from tests import viewer_ref as vr

pytestmark = pytest.mark.gpu

H, W, K = vr.H, vr.W, vr.K
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _render(meshes, points, views, K=K, H=H, W=W, **kw):
    from myslam_amd import ops
    return ops.render_view([(_t(v), _t(f), _t(c)) for v, f, c in meshes], [(_t(p), _t(c), s) for p, c, s in points],
                           views, K, H, W, **kw)


# ----------------------------------------------------------------------------------------------
# mesh colour parity
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("scene", ["A", "B"])
def test_mesh_colour_parity_with_the_reference(scene, cull):
    from myslam_amd import ops
    mesh, views = vr.scene(scene), vr.views(scene)
    img, depth = _render([mesh], [], views, cull_backfaces=cull, return_depth=True)
    assert img.shape == (len(views), H, W, 3) and img.dtype == torch.uint8 and depth.shape == (len(views), H, W)
    if not cull:                                          # the depth rasteriser's bits
        assert torch.equal(depth, ops.render_mesh_depth(_t(mesh[0]), _t(mesh[1]), views, K, H, W))
    img, depth = img.cpu().numpy(), depth.cpu().numpy()
    off = [vr.check_image(img[k], depth[k] > 0, vr.mesh_ref(scene, k, cull), f"scene {scene} view {k} cull {cull}")
           for k in range(len(views))]
    print(f"scene {scene} cull {cull}: share of pixels one step off, per view: {['%.5f' % o for o in off]}")


def test_a_mesh_of_one_colour_is_exact():
    """c = 200 (b0 + b1 + b2) lies within 200 x 3e-7 of 200: to nearest that is 200, in every pixel; no colours = grey."""
    v, f, _ = vr.scene("A")
    view = vr.views("A")[:1]
    img, depth = _render([(v, f, None)], [], view, return_depth=True)
    ref = vr.render([(v, f, None)], [], view[0])
    vr.check_image(img[0].cpu().numpy(), depth[0].cpu().numpy() > 0, ref, "grey scene A", tol=0)
    assert (img[0][depth[0] > 0] == 200).all()
    col = np.tile(np.array([[10, 250, 99, 0]], dtype=np.uint8), (len(v), 1))
    img2 = _render([(v, f, col)], [], view)
    assert (img2[0][depth[0] > 0] == torch.tensor([10, 250, 99], dtype=torch.uint8, device=_dev())).all()


@pytest.mark.parametrize("scene", ["room", "ball"])
def test_both_paths_and_any_threshold(scene):
    """The 12-triangle room alone is all queued tiles, the dense sphere mostly lanes; forced the other way round the images
    and depths are the same, bit for bit."""
    mesh = vr.scene(scene)
    views = vr.views("A")[[0, 3]] if scene == "room" else np.stack([rr.look_at((-1.0, -1.0, 0.5), rr.BALL_C),
                                                                    rr.look_at(rr.BALL_C, (2.0, 1.5, 1.2))])
    for cull in (True, False):
        base, base_d = _render([mesh], [], views, cull_backfaces=cull, return_depth=True)
        assert cull or (base_d > 0).any()
        for area in (1, 16, 4096, 1 << 30):
            other, other_d = _render([mesh], [], views, cull_backfaces=cull, large_area=area, return_depth=True)
            assert torch.equal(base, other) and torch.equal(base_d, other_d), (scene, cull, area)
    # from inside the ball every face is a back face
    if scene == "ball":
        img, d = _render([mesh], [], views[1:], return_depth=True)
        assert not (d > 0).any() and (img == 255).all()


# ----------------------------------------------------------------------------------------------
# points
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 4, 16])
def test_points_against_both_models(size):
    from myslam_amd import ops
    xyz, rgba = vr.points_a()
    c2w = rr.views_a()[0]
    rows = ops._w2c_rows(c2w[None], torch.device("cpu")).numpy()[0]
    for rgb in (rgba, rgba[7], rgba[:, :3]):
        img, depth = _render([], [(xyz, rgb, size)], c2w[None], return_depth=True)
        img, depth = img[0].cpu().numpy(), depth[0].cpu().numpy()
        want, want_d = vr.resolve_keys(vr.point_keys32(np.full(H * W, vr.EMPTY_KEY), xyz, rgb, size, rows, K, H, W), H, W)
        assert np.array_equal(img, want) and np.array_equal(depth.view(np.uint32), want_d.view(np.uint32))
        ref = vr.render([], [(xyz, rgb, size)], c2w)
        assert ref["undecided"][0].mean() <= vr.EDGE_SHARE_CAP
        vr.check_image(img, depth > 0, ref, f"points, size {size}", tol=0, edge_cap=None)
        assert 0.001 * size * size < (depth > 0).mean() < 0.5


# ----------------------------------------------------------------------------------------------
# composition
# ----------------------------------------------------------------------------------------------
def test_composition_of_meshes_and_points():
    a, room, ball = vr.scene("A"), vr.scene("room"), vr.scene("ball")
    xyz, rgba = vr.points_a()
    views = vr.views("A")[:2]
    pts = [(xyz, rgba, 4), (xyz[:500] + np.float32(0.01), rgba[3], 2)]
    img, depth = _render([a], pts, views, return_depth=True)
    for k in range(2):
        ref = vr.render([a], pts, views[k])
        vr.check_image(img[k].cpu().numpy(), depth[k].cpu().numpy() > 0, ref, f"scene A and points, view {k}", edge_cap=None)
        only_mesh = vr.mesh_ref("A", k, True)
        front = ref["hit"] & (ref["depth"] < only_mesh["depth"] - 1e-3)
        assert front.sum() > 200                          # points in front of the surfaces; the rest of them lie behind
    # two meshes in two calls = merged into one; any order of the lists; run to run
    v, f = rr.merge((room[0], room[1]), (ball[0], ball[1]))
    assert np.array_equal(v, a[0]) and np.array_equal(f, a[1])
    two, two_d = _render([room, ball], pts, views, return_depth=True)
    assert torch.equal(two, img) and torch.equal(two_d, depth)
    rev, rev_d = _render([ball, room], pts[::-1], views, return_depth=True)
    assert torch.equal(rev, img) and torch.equal(rev_d, depth)
    again, again_d = _render([a], pts, views, return_depth=True)
    assert torch.equal(again, img) and torch.equal(again_d, depth)


def test_a_point_at_a_surface_depth_goes_by_the_colour_word():
    """A wall at z = 2 exactly (n = (0, 0, A), n . v0 = 2 A, n . d = A: z = 2 in float32 too) and a point on it: equal depth
    bits, the smaller colour word wins - blue is its highest byte after alpha."""
    wall = np.array([[-3, -3, 2], [-3, 3, 2], [3, 3, 2], [3, -3, 2]], dtype=np.float32)    # faces the camera at the origin
    wf = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    wc = np.tile(np.array([[90, 90, 90]], dtype=np.uint8), (4, 1))
    p = np.array([[0.1, 0.1, 2.0]], dtype=np.float32)
    eye = np.eye(4)[None]
    for rgb, wins in (((255, 255, 89), True), ((0, 0, 91), False), ((89, 90, 90), True), ((91, 90, 90), False)):
        img, d = _render([(wall, wf, wc)], [(p, np.array(rgb, dtype=np.uint8), 4)], eye, return_depth=True)
        assert (d[0] == 2.0).all()
        n = int((img[0] == torch.tensor(rgb, dtype=torch.uint8, device=_dev())).all(-1).sum())
        assert n == (16 if wins else 0), (rgb, n)
        assert int((img[0] == 90).all(-1).sum()) == H * W - n


# ----------------------------------------------------------------------------------------------
# shapes that catch index errors
# ----------------------------------------------------------------------------------------------
HS, WS, KS = 37, 53, (40.0, 38.0, 25.7, 18.2)


def test_odd_image_views_and_chunks():
    a = vr.scene("A")
    xyz, rgba = vr.points_a()
    views = np.concatenate([vr.views("A"), vr.views("A")[:1]])
    pts = [(xyz, rgba, 3)]
    img, depth = _render([a], pts, views, KS, HS, WS, chunk=2, return_depth=True)
    assert img.shape == (5, HS, WS, 3) and depth.shape == (5, HS, WS)
    assert torch.equal(img[0], img[4])
    for k in range(5):
        one, one_d = _render([a], pts, views[k:k + 1], KS, HS, WS, return_depth=True)
        assert torch.equal(one[0], img[k]) and torch.equal(one_d[0], depth[k])
    assert torch.equal(_render([a], pts, views, KS, HS, WS, chunk=8), img)
    # the mesh alone against the model; view 3 looks along a wall 5 cm away: its triangles cross the near plane
    mesh, mesh_d = _render([a], [], views[:4], KS, HS, WS, chunk=3, return_depth=True)
    for k in range(4):
        ref = vr.render([a], [], views[k], K=KS, H=HS, W=WS)
        vr.check_image(mesh[k].cpu().numpy(), mesh_d[k].cpu().numpy() > 0, ref, f"37 x 53, view {k}")


def test_empty_and_degenerate_input():
    v, f, c = vr.scene("room")
    xyz, rgba = vr.points_a()
    views = vr.views("A")[:2]
    white = torch.full((2, HS, WS, 3), 255, dtype=torch.uint8, device=_dev())
    none_f, none_p = np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32)
    assert torch.equal(_render([], [], views, KS, HS, WS), white)
    img, d = _render([(v, none_f, c)], [(none_p, rgba[:0], 4)], views, KS, HS, WS, return_depth=True, background=(1, 2, 3))
    assert (img == torch.tensor([1, 2, 3], dtype=torch.uint8, device=_dev())).all() and not d.any()
    out, out_d = _render([(v, f, c)], [(xyz, rgba, 4)], np.zeros((0, 4, 4)), KS, HS, WS, return_depth=True)
    assert out.shape == (0, HS, WS, 3) and out_d.shape == (0, HS, WS)
    # a face with an index outside the vertex array is skipped
    base = _render([(v, f, c)], [], views, KS, HS, WS, cull_backfaces=False)
    bad = np.concatenate([f[:5], np.array([[0, 1, len(v)], [-1, 2, 3]], dtype=np.int32), f[5:]])
    assert torch.equal(_render([(v, bad, c)], [], views, KS, HS, WS, cull_backfaces=False), base)
    # three or four colour columns
    assert torch.equal(_render([(v, f, c[:, :3])], [], views, KS, HS, WS, cull_backfaces=False), base)
    assert not torch.equal(base, white)


def test_bad_arguments_raise():
    from myslam_amd import ops
    v, f, c = vr.scene("room")
    xyz, rgba = vr.points_a()
    views = vr.views("A")[:1]
    with pytest.raises(RuntimeError, match="bad sizes"):
        _render([(v, f, c)], [], views, KS, 0, WS)
    with pytest.raises(RuntimeError, match="bad sizes"):
        _render([(v, f, c)], [], views, KS, HS, 16385)
    for size in (0, 17):
        with pytest.raises(RuntimeError, match="point size"):
            _render([], [(xyz, rgba, size)], views, KS, HS, WS)
    with pytest.raises(RuntimeError, match="z_near"):
        _render([(v, f, c)], [], views, KS, HS, WS, z_near=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_view([(torch.from_numpy(v), torch.from_numpy(f), None)], [], views, KS, HS, WS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_view([(_t(v), torch.from_numpy(f), None)], [], views, KS, HS, WS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_view([], [(torch.from_numpy(xyz), _t(rgba), 4)], views, KS, HS, WS)
    with pytest.raises(RuntimeError, match="colours"):
        _render([(v, f, c[:3])], [], views, KS, HS, WS)


# ----------------------------------------------------------------------------------------------
# end to end: a tiny run, then the viewer in a fresh process
# ----------------------------------------------------------------------------------------------
def _viewer(cfg_path, *flags):
    p = subprocess.run([sys.executable, "-m", "myslam_amd.visualizer", str(cfg_path), *flags], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def _near(img, uv, rgb_test, r=6):
    u, v = int(round(uv[0])), int(round(uv[1]))
    win = img[max(v - r, 0):v + r + 1, max(u - r, 0):u + r + 1].astype(np.int64)
    return int(rgb_test(win[..., 0], win[..., 1], win[..., 2]).sum())


def test_visualizer_end_to_end(tmp_path):
    import yaml
    from PIL import Image
    from types import SimpleNamespace
    from myslam_amd import checkpoint
    from myslam_amd.src.ESLAM import ESLAM
    from myslam_amd.src.tools import visualizer_util as vu
    from tests.test_gpu_frames import _toy_cfg, _write_toy_sequence
    n_frames = 9
    _write_toy_sequence(tmp_path / "seq", n_frames)
    out = tmp_path / "out"
    cfg = _toy_cfg(tmp_path / "seq", out)
    cfg["mapping"]["mesh_freq"] = 4
    ESLAM(cfg, SimpleNamespace(input_folder=None, output=None)).run()
    assert (out / "mesh" / "00004_mesh_culled.ply").exists() and (out / "mesh" / "00008_mesh_culled.ply").exists()
    with open(tmp_path / "ESLAM.yaml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    with open(tmp_path / "toy.yaml", "w") as fh:
        yaml.safe_dump(dict(data=dict(output=str(out))), fh)
    # the run tracks to within a fraction of a pixel of this view, where one camera would hide the other: a copy of the newest
    # checkpoint with the ground truth moved 0.6 m to the viewer's right (about 17 pixels) shows each where it belongs
    ck = checkpoint.load(sorted((out / "ckpts").glob("*.tar"))[-1])
    assert ck["idx"] == 8
    ck["gt_c2w_list"] = ck["gt_c2w_list"].clone()
    ck["gt_c2w_list"][:, :3, 3] += 0.6 * ck["gt_c2w_list"][0, :3, 0]
    torch.save(ck, out / "ckpts" / "00008_shifted.tar")
    hs, ws = 135, 240
    stdout = _viewer(tmp_path / "toy.yaml", "--save_rendering", "--every", "4", "--size", str(hs), str(ws))
    assert "00008_shifted.tar" in stdout and "ffmpeg" in stdout
    names = sorted(os.listdir(out / "tmp_rendering"))
    assert names == ["000000.jpg", "000004.jpg", "000008.jpg"]
    imgs = {int(n[:6]): np.asarray(Image.open(out / "tmp_rendering" / n)) for n in names}
    for im in imgs.values():
        assert im.shape == (hs, ws, 3) and im.dtype == np.uint8
    white = lambda im: (im.astype(np.int64).min(-1) >= 240).mean()             # noqa: E731
    # no mesh before frame 4: background and the two cameras.  With one it is not all background: the room is at least 2.4 m
    # across and at most 8 m away, 35 pixels at this focal length of 117 - upwards of 1000 of the 32 400 pixels, 3 %
    assert white(imgs[0]) > 0.95
    assert white(imgs[4]) < white(imgs[0]) - 0.02 and white(imgs[8]) < white(imgs[0]) - 0.02
    # red at the projection of the current estimated camera and green at the ground truth's, not the other way round
    est, gt = ck["estimate_c2w_list"].numpy().astype(np.float64), ck["gt_c2w_list"].numpy().astype(np.float64)
    w2c = np.linalg.inv(vu.viewing_pose(gt[0]))
    fx, fy, cx, cy = vu.window_intrinsics(hs, ws)
    red = lambda r, g, b: (r > 170) & (g < 110) & (b < 110)                    # noqa: E731  (JPEG softens the 4 px dots)
    green = lambda r, g, b: (g > 170) & (r < 110) & (b < 110)                  # noqa: E731
    for i, im in imgs.items():
        for poses, test, other in ((est, red, green), (gt, green, red)):
            c = w2c[:3, :3] @ poses[i, :3, 3] + w2c[:3, 3]
            assert c[2] > 0
            uv = (fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy)
            assert _near(im, uv, test, r=6) >= 8 > _near(im, uv, other, r=6), (i, uv)
    # no ground truth: no green anywhere; the top view runs and shows the mesh
    _viewer(tmp_path / "toy.yaml", "--save_rendering", "--every", "8", "--size", str(hs), str(ws), "--no_gt_traj", "--top_view")
    names = sorted(os.listdir(out / "tmp_rendering"))
    assert names == ["000000.jpg", "000008.jpg"]                            # (the folder is started afresh)
    top = np.asarray(Image.open(out / "tmp_rendering" / "000008.jpg")).astype(np.int64)
    assert top.shape == (hs, ws, 3) and int(green(top[..., 0], top[..., 1], top[..., 2]).sum()) == 0
    assert int(red(top[..., 0], top[..., 1], top[..., 2]).sum()) >= 8 and white(top) < 0.98
