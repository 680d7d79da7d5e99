"""TSDF fusion on the GPU (eslam_tsdf_integrate, eslam_mc_count_masked, eslam_tsdf_sample_color, ops.TSDFVolume and its
callers) against the numpy models of tests/tsdf_ref.py and the analytic room.  The float32 model mirrors the kernel
operation for operation, so volumes are compared bit for bit; the float64 model and the room are the yardsticks."""
import functools

import numpy as np
import pytest
import torch

from tests import tsdf_ref as R
from tests.test_tsdf_ref import WEIGHT_CAP, far_share

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _shared_volume():
    """The GPU volume of the shared input (read-only for the tests)."""
    from myslam_amd import ops
    s = R.shared_input()
    vol = ops.TSDFVolume(s.sc.bound, R.VOXEL, R.TRUNC, device=_dev()).integrate(s.frames, s.K)
    assert vol.dims == s.dims and np.array_equal(np.float32(vol.origin), s.origin)
    return vol


@functools.lru_cache(maxsize=None)
def _shared_gpu_mesh():
    return _shared_volume().extract_mesh()


# ----------------------------------------------------------------------------------------------
# parity on the shared input
# ----------------------------------------------------------------------------------------------
def test_parity_with_the_float32_model_is_bitwise():
    vol, m32 = _shared_volume(), R.shared_model("float32")
    w = vol.weight.cpu().numpy()
    print(f"\nweight differs on {(w != m32.weight).sum()} voxels, tsdf bits on {(_bits(vol.tsdf) != _bits(m32.tsdf)).sum()}, "
          f"colour bits on {(_bits(vol.color) != _bits(m32.color)).sum()}")
    assert np.array_equal(w, m32.weight)
    assert _same_bits(vol.tsdf, m32.tsdf)
    assert _same_bits(vol.color, m32.color)


def test_parity_with_the_float64_model():
    vol, m32, m64 = _shared_volume(), R.shared_model("float32"), R.shared_model("float64")
    w = vol.weight.cpu().numpy()
    share = float((w != m64.weight).mean())
    same = w == m64.weight
    for a, b in zip(m32.pixels, m64.pixels):          # the GPU's chosen pixels are the float32 model's (bitwise parity above)
        same &= a == b
    d = np.abs(vol.tsdf.cpu().numpy().astype(np.float64)[same] - m64.tsdf[same])
    print(f"\nweight disagreement with float64 {share * 100:.4f} %, max |dtsdf| {d.max():.2e} over {same.mean() * 100:.2f} % of voxels")
    assert share <= WEIGHT_CAP
    assert same.mean() > 0.99 and d.max() <= 1e-5


# ----------------------------------------------------------------------------------------------
# shapes where it can go wrong: a 37 x 21 x 70 volume inside the room
# ----------------------------------------------------------------------------------------------
SMALL_DIMS, SMALL_LO, SMALL_VOXEL, SMALL_TRUNC = (37, 21, 70), (-0.2, -0.2, -1.0), 0.03, 0.12


def _small_bound():
    lo = np.array(SMALL_LO)
    return np.stack([lo, lo + (np.array(SMALL_DIMS) - 0.5) * SMALL_VOXEL], 1)


@functools.lru_cache(maxsize=None)
def _small_frames():
    """5 frames: frames 0, 10 and 20 of the trajectory (cameras inside the volume, which lies partly outside every frustum
    and holds a part of one sphere that all three see), one of all-zero depth, and one camera outside the volume that looks
    away from it."""
    from myslam_amd import synthscene
    s = R.shared_input()
    poses = synthscene.trajectory(21, s.sc.bound)
    f = [s.frames[0]]
    for k in (10, 20):
        depth, color = synthscene.render_frame(s.room, s.sc, poses[k], "cpu", hole_frac=0.02, seed=k)
        f.append((k, color, depth, poses[k]))
    away = f[0][3].clone()
    away[0, 3] = 1.0                                    # frame 0 looks along +x; the volume ends at x = 0.91
    zero = (f[1][0], f[1][1], torch.zeros_like(f[1][2]), f[1][3])
    return [f[0], zero, f[1], (99, f[0][1], f[0][2], away), f[2]]


def _small_model(frames, color=True):
    s = R.shared_input()
    dims, origin = R.volume_dims(_small_bound(), SMALL_VOXEL)
    assert dims == SMALL_DIMS
    return R.Volume(dims, origin, SMALL_VOXEL, SMALL_TRUNC, color=color, dtype=np.float32).integrate(
        np.stack([fr[2].numpy() for fr in frames]), np.stack([fr[1].numpy() for fr in frames]),
        R.w2c_rows(torch.stack([fr[3] for fr in frames]).numpy()), s.K)


def _small_gpu(frames, chunk=32, color=True):
    from myslam_amd import ops
    s = R.shared_input()
    vol = ops.TSDFVolume(_small_bound(), SMALL_VOXEL, SMALL_TRUNC, color=color, device=_dev())
    assert vol.dims == SMALL_DIMS
    return vol.integrate(frames, s.K, chunk=chunk)


def test_small_volume_ragged_chunks_and_frames_that_change_nothing():
    frames = _small_frames()
    m = _small_model(frames)
    vol = _small_gpu(frames, chunk=2)
    observed = float((m.weight > 0).mean())
    print(f"\nobserved {observed * 100:.1f} % of the 37 x 21 x 70 volume, weight up to {m.weight.max():.0f}")
    assert 0.05 < observed < 0.95 and m.weight.max() == 3            # partly outside every frustum, overlapping frames
    assert np.array_equal(vol.weight.cpu().numpy(), m.weight) and _same_bits(vol.tsdf, m.tsdf) and _same_bits(vol.color, m.color)
    # the camera that looks away and the frame of all-zero depth change nothing, alone or together
    alone = _small_model([frames[3]])
    assert alone.weight.max() == 0 and _small_model([frames[1]]).weight.max() == 0
    before = [t.clone() for t in (vol.tsdf, vol.weight, vol.color)]
    s = R.shared_input()
    vol.integrate([frames[3]], s.K)
    vol.integrate([frames[1]], s.K)
    vol.integrate([frames[1], frames[3]], s.K)
    for a, b in zip(before, (vol.tsdf, vol.weight, vol.color)):
        assert _same_bits(a, b)
    fresh = _small_gpu([frames[3], frames[1]])
    assert float(fresh.weight.abs().max()) == 0 and float(fresh.tsdf.abs().max()) == 0


def test_chunking_determinism_and_frame_order():
    frames = _small_frames()
    ref = _small_gpu(frames, chunk=32)
    for vol in (_small_gpu(frames, chunk=1), _small_gpu(frames, chunk=2), _small_gpu(frames, chunk=32)):
        assert _same_bits(vol.tsdf, ref.tsdf) and _same_bits(vol.weight, ref.weight) and _same_bits(vol.color, ref.color)
    rev = _small_gpu(frames[::-1])
    assert torch.equal(rev.weight, ref.weight)
    assert not torch.equal(rev.tsdf, ref.tsdf)                         # the running average is ordered
    assert float((rev.tsdf - ref.tsdf).abs().max()) < 1e-5


def test_without_colour():
    frames = _small_frames()
    ref, vol = _small_gpu(frames), _small_gpu(frames, color=False)
    assert vol.color is None
    assert _same_bits(vol.tsdf, ref.tsdf) and _same_bits(vol.weight, ref.weight)
    v, f, c = vol.extract_mesh()
    v0, f0, c0 = ref.extract_mesh()
    assert c is None and c0 is not None and c0.shape == v0.shape
    assert len(f) > 0 and torch.equal(v, v0) and torch.equal(f, f0)


def test_construction_reports_the_bytes_it_cannot_get():
    from myslam_amd import ops
    with pytest.raises(RuntimeError, match=r"need 4\d{15} bytes"):       # 1e5^3 voxels of 4 bytes: 4e15 (x 2 arrays)
        ops.TSDFVolume([[0, 1000.0], [0, 1000.0], [0, 500.0]], 0.01, 0.04, color=False, device=_dev())


# ----------------------------------------------------------------------------------------------
# masked marching cubes
# ----------------------------------------------------------------------------------------------
def test_masked_marching_cubes_against_the_model():
    from myslam_amd import ops
    vol, weight = R.sphere_field()
    origin, spacing = (0.5, -1.0, 2.0), (0.1, 0.2, 0.3)
    g = torch.from_numpy(vol).to(_dev())
    for w in (np.ones_like(vol), weight):
        v, f = ops.marching_cubes_masked(g, torch.from_numpy(w).to(_dev()), 0.0, origin, spacing)
        v0, f0 = R.marching_cubes_masked(vol, w, 0.0, origin, spacing)
        assert len(f0) > 0 and np.array_equal(f.cpu().numpy(), f0)
        assert np.abs(v.cpu().numpy() - v0).max() <= 1e-6 * np.abs(v0).max()
    va, fa = ops.marching_cubes_masked(g, torch.ones_like(g), 0.0, origin, spacing)
    vb, fb = ops.marching_cubes(g, 0.0, origin, spacing)
    assert torch.equal(va, vb) and torch.equal(fa, fb)
    # no fully valid cube (every second voxel along z unobserved): empty arrays, no error
    none = torch.ones_like(g)
    none[:, :, ::2] = 0
    v, f = ops.marching_cubes_masked(g, none, 0.0, origin, spacing)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and f.dtype == torch.int32


# ----------------------------------------------------------------------------------------------
# the fused mesh of the shared input
# ----------------------------------------------------------------------------------------------
def _depth_share(verts, faces):
    """Share of frame 0's valid depth pixels that the mesh, rendered from frame 0's pose, reproduces to within a voxel."""
    from myslam_amd import ops
    s = R.shared_input()
    c2w = s.frames[0][3].clone().double()
    c2w[:3, 1] *= -1.0
    c2w[:3, 2] *= -1.0
    img = ops.render_mesh_depth(torch.as_tensor(verts).to(_dev()), torch.as_tensor(faces).to(_dev()), c2w[None], s.K,
                                s.sc.H, s.sc.W)[0].cpu()
    gt = s.frames[0][2]
    ok = gt > 0
    return float((((img - gt).abs() <= R.VOXEL) & (img > 0))[ok].float().mean())


def test_fused_mesh_of_the_shared_input():
    """Measured on an MI355X (printed by every run): V = 24091, F = 44545, faces equal to the float32 model's; vertices to
    the analytic surface: median 0.129 mm (float64 model 0.129 mm), 0.340 % beyond voxel / 2 (model 0.345 %, bound twice
    that); rendered from frame 0's pose, the float64 model's mesh reproduces 92.76 % of frame 0's valid depth pixels to
    within one voxel - the rest is what 8 frames 45 degrees apart leave unobserved of that view's surfaces - and the GPU's
    mesh 92.76 % (bound: the model's share less 1 % absolute); the vertex colours' median distance from the room's albedo
    is 0.0010 (bound 0.05)."""
    s = R.shared_input()
    v, f, c = _shared_gpu_mesh()
    v32, f32 = R.shared_mesh("float32")
    v64, f64 = R.shared_mesh("float64")
    vn = v.cpu().numpy()
    assert np.array_equal(f.cpu().numpy(), f32)
    assert np.abs(vn - v32).max() <= 1e-6 * np.abs(v32).max()
    med64, far64 = far_share(s.room, v64)
    med, far = far_share(s.room, vn)
    share64, share = _depth_share(v64, f64), _depth_share(vn, f.cpu().numpy())
    dc = np.abs(c.cpu().numpy().astype(np.float64) - R.room_albedo(s.room, vn)).max(axis=1)
    print(f"\nV = {len(vn)}, F = {len(f)}: median {med * 1e3:.3f} mm (model {med64 * 1e3:.3f}), beyond voxel/2 {far * 100:.3f} % "
          f"(model {far64 * 100:.3f} %); depth share {share * 100:.2f} % (model {share64 * 100:.2f} %); colour median {np.median(dc):.4f}")
    assert med <= R.VOXEL / 20 and far <= 2 * far64
    assert share64 > 0.9 and share >= share64 - 0.01
    assert np.median(dc) <= 0.05


# ----------------------------------------------------------------------------------------------
# hull
# ----------------------------------------------------------------------------------------------
def test_hull_from_fused_keyframes():
    from myslam_amd import ops
    from myslam_amd.src.utils import Mesher as M
    from tests.test_gpu_mesh import _mesher
    s = R.shared_input()
    dev = _dev()
    kfs = [{"est_c2w": c2w.to(dev), "depth": depth.to(dev), "color": color.to(dev), "idx": idx}
           for idx, color, depth, c2w in s.frames[:4]]
    m = _mesher(s.sc)
    hull = M.get_bound_from_frames_tsdf(m, kfs, voxel=R.VOXEL)
    vol = ops.TSDFVolume(m.marching_cubes_bound, R.VOXEL, 0.04, color=False, device=dev)
    vol.integrate(s.frames[:4], s.K)
    verts = vol.extract_mesh()[0]
    assert verts.shape[0] > 1000
    cams = torch.stack([kf["est_c2w"][:3, 3] for kf in kfs])
    assert bool(hull.contains(verts).all()) and bool(hull.contains(cams).all())
    assert tuple(hull.halfspaces.shape) == (M.N_DIRECTIONS, 4)
    # at the reference's voxel (4 / 512) the construction still holds the cameras and its own vertices
    fine = M.get_bound_from_frames_tsdf(m, kfs)
    assert bool(fine.contains(cams).all())
    # the default hull is untouched: bit-identical to its definition
    old = M.get_bound_from_frames(m, kfs)
    again = M.halfspaces_from_points(M.keyframe_points(m, kfs), m.mesh_bound_scale)
    assert torch.equal(old.halfspaces, again)


# ----------------------------------------------------------------------------------------------
# tool
# ----------------------------------------------------------------------------------------------
def test_fuse_tool_round_trip_and_metrics(tmp_path, monkeypatch):
    """recon_metrics compares two independent samplings of the surfaces (seeds s and s + 1), so a mesh scored against itself
    gives the samplings' own nearest-neighbour distance, not 0: for N points spread evenly over an area A that is
    0.5 sqrt(A / N) (a planar Poisson process).  With N = 4e6 on the 21.1 m^2 mesh that is 0.115 cm (measured on an MI355X:
    self 0.115 / 0.115 cm, against the float64 model's mesh 0.120 / 0.119 cm), below voxel / 10 = 0.4 cm, the bound for the mesh against the float64 model's; the self-score is held to twice the sampling figure and
    the 2D metric of the mesh with itself is exactly 0."""
    from myslam_amd.src.tools import eval_recon as ev, tsdf_fuse
    from myslam_amd.src.utils import datasets
    from myslam_amd.src.utils.Mesher import read_ply, write_ply
    s = R.shared_input()
    sc = s.sc
    v, f, c = tsdf_fuse.fuse_frames(s.frames, s.K, sc.H, sc.W, sc.bound, R.VOXEL, R.TRUNC)
    gv, gf, gc = _shared_gpu_mesh()
    assert np.array_equal(v, gv.cpu().numpy()) and np.array_equal(f, gf.cpu().numpy()) and np.array_equal(c, gc.cpu().numpy())
    path = tmp_path / "fused.ply"
    write_ply(str(path), v, f, c)
    v1, f1, c1 = read_ply(str(path))
    assert np.array_equal(v1, v) and np.array_equal(f1, f) and np.abs(c1 - np.clip(c, 0, 1)).max() <= 0.5 / 255 + 1e-6
    # the command line, on a reader that yields the shared frames
    cfg = tmp_path / "toy.yaml"
    b = sc.bound.double().tolist()
    cfg.write_text(f"scale: 1\ncam: {{H: {sc.H}, W: {sc.W}, fx: {sc.fx}, fy: {sc.fy}, cx: {sc.cx}, cy: {sc.cy}}}\n"
                   f"mapping: {{bound: {b}, marching_cubes_bound: {b}}}\n")
    monkeypatch.setattr(datasets, "get_dataset", lambda cfg, args, scale, device="cuda:0": s.frames)
    out = tmp_path / "cli.ply"
    tsdf_fuse.main([str(cfg), "--output", str(out), "--voxel", str(R.VOXEL), "--trunc", str(R.TRUNC)])
    v2, f2, c2 = read_ply(str(out))
    assert np.array_equal(v2, v1) and np.array_equal(f2, f1) and np.array_equal(c2, c1)
    every = tmp_path / "every.ply"
    tsdf_fuse.main([str(cfg), "--output", str(every), "--voxel", str(R.VOXEL), "--trunc", str(R.TRUNC), "--every", "2"])
    assert 0 < len(read_ply(str(every))[1]) < len(f1)
    # metrics
    n = 4000000
    tri = v.astype(np.float64)[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1).sum()
    floor_cm = 0.5 * np.sqrt(area / n) * 100
    r_self = ev.recon_metrics(v, f, v, f, align=False, num_points=n)
    r2d = ev.depth_l1_metric(v, f, v, f, align=False, n_imgs=4, seed=1)
    v64, f64 = R.shared_mesh("float64")
    r = ev.recon_metrics(v, f, v64, f64, align=False, num_points=n)
    print(f"\narea {area:.1f} m^2, sampling figure {floor_cm:.3f} cm; self {r_self}; against the float64 model {r}")
    assert r2d["depth_l1"] == 0.0
    assert r_self["accuracy"] <= 2 * floor_cm and r_self["completion"] <= 2 * floor_cm and r_self["completion_ratio"] == 100.0
    assert r["accuracy"] <= R.VOXEL / 10 * 100 and r["completion"] <= R.VOXEL / 10 * 100
