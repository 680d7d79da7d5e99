"""Mesh extraction on the GPU: the SDF on an implicit grid (eslam_sdf_grid), marching cubes (eslam_mc_count / _emit)
against the numpy reference of tests/mesh_ref.py and on analytic SDFs, and Mesher.get_mesh end to end."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import mesh_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def _dev():
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------
# the field
# ----------------------------------------------------------------------------------------------
def _field_setup():
    from myslam_amd import harness
    wl = harness.make_workload("room0", 64, 24, 8, device=_dev(), planes="synth")
    b = wl.scene.bound
    axes = [torch.linspace(float(b[k, 0]) - 0.3, float(b[k, 1]) + 0.3, n) for k, n in enumerate((41, 33, 70))]
    axes[0][5] = b[0, 0]
    axes[1][-4] = b[1, 1]                                  # points exactly on a face are outside (strict test)
    return wl, axes


def _ref_points(axes):
    """The reference's points (Mesher.py:182-184: meshgrid indexing='xy' -> [ny, nx, nz] order) and the same points in
    [nx, ny, nz] order."""
    gx, gy, gz = torch.meshgrid(*axes, indexing="xy")
    pts_ref = torch.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], 1)
    nx, ny, nz = (len(a) for a in axes)
    pts = pts_ref.reshape(ny, nx, nz, 3).permute(1, 0, 2, 3).reshape(-1, 3).contiguous()
    return pts_ref, pts


def test_sdf_grid_equals_decode_on_the_same_points():
    from myslam_amd import _hip, ops
    from myslam_amd.src.utils.Mesher import eval_points
    from oracle import eslam_oracle as orc
    dev = _dev()
    wl, axes = _field_setup()
    nx, ny, nz = (len(a) for a in axes)
    pts_ref, pts = _ref_points(axes)
    vol = ops.sdf_grid(wl.planes, wl.decoders, [a.to(dev) for a in axes], wl.scene.bound)
    assert vol.shape == (nx, ny, nz)
    # eslam_decode_fwd(SDF_ONLY | MASK_OUTSIDE) on the materialised points, bit for bit
    lib = _hip.lib()
    p = pts.to(dev)
    geo = tuple(wl.planes[:3]) + tuple(wl.planes[:3])
    arr, _ = _hip.make_planes(tuple([t.detach() for t in g] for g in geo))
    dec, keep = _hip.make_decoders([t.detach() for t in ops.decoder_params(wl.decoders)], ops.beta_tensor(10, dev))
    raw = torch.empty(p.shape[0], device=dev)
    _hip.check(lib.eslam_decode_fwd(arr, ctypes.byref(dec), _hip.make_bound(ops.bound_to_host(wl.scene.bound)), _hip.ptr(p), p.shape[0], 3,
                                    _hip.ptr(raw), None, _hip.stream_handle(dev)), "eslam_decode_fwd")
    assert torch.equal(vol.reshape(-1), raw)
    # the reference's volume: its z in meshgrid order, reshape(ny, nx, nz).transpose(1, 0, 2)
    mesher = SimpleNamespace(points_batch_size=10000, bound=wl.scene.bound)
    z = eval_points(mesher, pts_ref.to(dev), wl.planes, wl.decoders)[:, -1].cpu()
    zr = z.reshape(ny, nx, nz).permute(1, 0, 2)
    assert float((vol.cpu() - zr).abs().max()) <= 1e-6
    cparams = {k: v.detach().cpu() for k, v in wl.decoders.state_dict().items() if k != "beta"}
    cplanes = tuple([t.detach().cpu().contiguous() for t in grp] for grp in wl.planes)
    ref = orc.decode(pts, cplanes, cparams, wl.scene.bound)[:, -1]
    b = wl.scene.bound
    inside = ((pts < b[:, 1]) & (pts > b[:, 0])).all(dim=1)
    assert 0.2 < float(inside.float().mean()) < 0.9
    ref[~inside] = -1
    assert hp.rel_err(vol.reshape(-1).cpu().numpy(), ref.numpy()) <= RTOL


def test_sdf_grid_halfspace_mask():
    from myslam_amd import ops
    from myslam_amd.src.utils.Mesher import halfspaces_from_points
    dev = _dev()
    wl, axes = _field_setup()
    _, pts = _ref_points(axes)
    b = wl.scene.bound.double()
    g = torch.Generator().manual_seed(3)
    # a rotated, shrunken cloud: a hull with many oblique faces that cuts through the grid
    cloud = (torch.rand(4000, 3, generator=g, dtype=torch.float64) - 0.5) @ torch.tensor(
        [[0.8, 0.5, 0.1], [-0.5, 0.8, 0.2], [0.0, -0.2, 0.9]], dtype=torch.float64)
    cloud = cloud * (b[:, 1] - b[:, 0]) * 0.7 + b.mean(1)
    hs = halfspaces_from_points(cloud, 1.02)
    plain = ops.sdf_grid(wl.planes, wl.decoders, [a.to(dev) for a in axes], wl.scene.bound).reshape(-1).cpu()
    vol = ops.sdf_grid(wl.planes, wl.decoders, [a.to(dev) for a in axes], wl.scene.bound, hs.to(dev)).reshape(-1).cpu()
    val = pts.double() @ hs[:, :3].T + hs[:, 3]                 # float64 test
    outside = (val > 0).any(dim=1)
    clear = (val.abs() > 1e-5).all(dim=1)
    assert 0.1 < float(outside.float().mean()) < 0.9
    assert torch.equal(vol[clear & outside], torch.full((int((clear & outside).sum()),), -1.0))
    assert torch.equal(vol[clear & ~outside], plain[clear & ~outside])


# ----------------------------------------------------------------------------------------------
# marching cubes
# ----------------------------------------------------------------------------------------------
def _mc(vol, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    from myslam_amd import ops
    v, f = ops.marching_cubes(torch.as_tensor(vol).to(_dev()).contiguous(), level, origin, spacing)
    return v.cpu(), f.cpu()


@pytest.mark.parametrize("shape", [(2, 2, 2), (1, 8, 8), (37, 5, 64), (64, 64, 64)])
@pytest.mark.parametrize("level", [0.0, 0.3])
def test_marching_cubes_matches_numpy_reference(shape, level):
    rng = np.random.default_rng(hash((shape, level)) % 2 ** 32)
    vol = rng.normal(0.2, 0.5, size=shape).astype(np.float32)
    vol[rng.random(shape) < 0.1] = np.float32(level)                  # values exactly at the level
    origin, spacing = (-1.25, 0.5, 2.0), (0.01, 0.02, 0.015)
    v, f = _mc(vol, level, origin, spacing)
    rv, rf = mesh_ref.marching_cubes(vol, level, origin, spacing)
    assert torch.equal(f, torch.from_numpy(rf))
    assert v.shape == rv.shape
    assert not torch.isnan(v).any()
    extent = max(s * (n - 1) for s, n in zip(spacing, shape)) or 1.0
    if len(rv):
        assert float((v - torch.from_numpy(rv)).abs().max()) <= 1e-6 * extent
    if shape == (1, 8, 8):
        assert f.shape[0] == 0


def _sphere(n=64, c=(0.47, 0.53, 0.51), r=0.37):
    g = np.stack(np.meshgrid(*[np.linspace(0, 1, n)] * 3, indexing="ij"), -1)
    return (np.linalg.norm(g - np.array(c), axis=-1) - r).astype(np.float32)


def _topology(v, f):
    f = f.numpy().astype(np.int64)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = de[:, 0] * (len(v) + 1) + de[:, 1]
    rkey = de[:, 1] * (len(v) + 1) + de[:, 0]
    und = np.unique(np.minimum(key, rkey))
    # components of the vertex graph
    parent = np.arange(len(v))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in de:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    comps = len({find(a) for a in np.unique(f)})
    return key, rkey, len(und), comps


def _area_volume(v, f):
    v = v.double().numpy()
    f = f.numpy()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cr = np.cross(b - a, c - a)
    return 0.5 * np.linalg.norm(cr, axis=1).sum(), (np.einsum("ij,ij->i", a, cr) / 6.0).sum()


def test_marching_cubes_sphere_is_closed_and_outward():
    n, r = 64, 0.37
    vol = _sphere(n, r=r)
    sp = 1.0 / (n - 1)
    v, f = _mc(vol, 0.0, (0.0, 0.0, 0.0), (sp, sp, sp))
    key, rkey, E, comps = _topology(v, f)
    # closed: every directed edge once, its reverse once
    assert len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rkey))
    assert len(v) - E + len(f) == 2 and comps == 1
    # the vertex set is numpy's crossing-edge set
    assert len(v) == int(mesh_ref.crossings(vol, np.float32(0)).sum())
    area, volume = _area_volume(v, f)
    assert abs(area / (4 * np.pi * r * r) - 1) < 0.01
    assert volume > 0 and abs(volume / (4 / 3 * np.pi * r ** 3) - 1) < 0.01


def test_marching_cubes_torus_and_two_spheres():
    n = 64
    g = np.stack(np.meshgrid(*[np.linspace(0, 1, n)] * 3, indexing="ij"), -1) - 0.5
    q = np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2) - 0.28
    torus = (np.sqrt(q ** 2 + g[..., 2] ** 2) - 0.1).astype(np.float32)
    v, f = _mc(torus, 0.0)
    _, _, E, comps = _topology(v, f)
    assert len(v) - E + len(f) == 0 and comps == 1
    two = np.minimum(np.linalg.norm(g - np.array([-0.2, 0, 0]), axis=-1) - 0.15,
                     np.linalg.norm(g - np.array([0.22, 0.05, 0]), axis=-1) - 0.12).astype(np.float32)
    v, f = _mc(two, 0.0)
    _, _, E, comps = _topology(v, f)
    assert comps == 2 and len(v) - E + len(f) == 4


def test_marching_cubes_plane_boundary_on_grid_faces():
    n = 40
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij"), -1)
    vol = (g @ np.array([0.3, 0.5, 0.81]) - 30.3).astype(np.float32)
    v, f = _mc(vol, 0.0)
    key, rkey, _, _ = _topology(v, f)
    fn = f.numpy().astype(np.int64)
    de = np.concatenate([fn[:, [0, 1]], fn[:, [1, 2]], fn[:, [2, 0]]])
    boundary = de[~np.isin(key, rkey)]
    assert len(boundary) > 0
    pv = v.numpy()
    on_face = lambda p: ((np.abs(p) < 1e-4) | (np.abs(p - (n - 1)) < 1e-4)).any(axis=-1)
    assert on_face(pv[boundary[:, 0]]).all() and on_face(pv[boundary[:, 1]]).all()


def test_marching_cubes_is_deterministic():
    vol = _sphere(64)
    v1, f1 = _mc(vol, 0.0)
    v2, f2 = _mc(vol, 0.0)
    assert torch.equal(v1, v2) and torch.equal(f1, f2)


def test_marching_cubes_past_int32_points():
    from myslam_amd import ops
    shape = (1300, 1300, 1300)                       # 2.197e9 points > 2^31
    need = ops.mc_workspace_bytes(shape) + 4 * shape[0] * shape[1] * shape[2] + (1 << 30)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB free")
    small = torch.from_numpy(_sphere(64))
    vs, fs = _mc(small, 0.0)
    dev = _dev()
    big = torch.ones(shape, device=dev)
    o = shape[0] - 64                                # the far corner: linear indices past 2^31
    big[o:, o:, o:] = small.to(dev)
    v, f = ops.marching_cubes(big, 0.0, (-o, -o, -o), (1.0, 1.0, 1.0))      # the offset taken out in float64
    del big
    assert torch.equal(f.cpu(), fs)
    assert torch.equal(v.cpu(), vs)


# ----------------------------------------------------------------------------------------------
# Mesher end to end
# ----------------------------------------------------------------------------------------------
_run_cache = {}


def _toy_run():
    if "r" not in _run_cache:
        from myslam_amd import scene as scn, slam, synthscene
        sc = scn.make_scene("toy")
        cfg = slam.SlamConfig(tracking_pixels=500, tracking_iters=8, ignore_edge_H=10, ignore_edge_W=10, mapping_pixels=1000,
                              iters_first=100, iters=10, every_frame=4, keyframe_every=4)
        dev = _dev()
        frames = synthscene.make_sequence(sc, 13, device=dev)
        torch.manual_seed(0)
        s = slam.Slam(sc, cfg, device=dev, seed=0)
        s.run(frames)
        _run_cache["r"] = (sc, s)
    return _run_cache["r"]


def _mesher(sc, resolution=0.02, level=0.0):
    return SimpleNamespace(H=sc.H, W=sc.W, fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy, scale=1.0, resolution=resolution,
                           level_set=level, mesh_bound_scale=1.02, bound=sc.bound, points_batch_size=500000,
                           marching_cubes_bound=sc.bound.double())


def test_get_mesh_end_to_end(tmp_path):
    """Thresholds set before measuring.  Observed on the MI355X (toy loop, 13 frames, 0.02 grid, two runs): V = 53.3 k,
    F = 106.6 k; near-surface vertices: median 0.42-0.47 cm, p90 2.33 cm from the analytic room; coverage 99.0 %."""
    from myslam_amd import synthscene
    from myslam_amd.src.utils import Mesher as M
    from tests.test_mesh_host import _read_ply
    sc, s = _toy_run()
    m = _mesher(sc)
    out = tmp_path / "mesh.ply"
    M.get_mesh(m, str(out), s.all_planes, s.decoders, s.keyframe_dict, device="cuda:0")
    head, v, f = _read_ply(out)
    V, F = len(v), len(f)
    assert V > 0 and F > 0
    verts = np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float64)
    assert (f["v"] >= 0).all() and (f["v"] < V).all() and (v["a"] == 255).all()
    # inside the scaled hull, within one voxel
    hull = M.get_bound_from_frames(m, s.keyframe_dict)
    hs = hull.halfspaces.cpu()
    assert float((torch.from_numpy(verts) @ hs[:, :3].T + hs[:, 3]).max()) <= 0.02 * np.sqrt(3)
    # distance to the analytic surface, over vertices near the observed depth
    room = synthscene.AnalyticRoom(sc.bound)
    dev = _dev()
    kp = M.keyframe_points(m, s.keyframe_dict)
    kp = kp[: kp.shape[0] - len(s.keyframe_dict)]
    vg = torch.from_numpy(verts).float().to(dev)
    dmin = torch.full((V,), float("inf"), device=dev)
    for lo in range(0, kp.shape[0], 20000):
        dmin = torch.minimum(dmin, torch.cdist(vg, kp[lo:lo + 20000]).min(dim=1).values)
    near = (dmin < 0.10).cpu()
    vt = torch.from_numpy(verts)
    walls = torch.minimum((vt - room.lo).abs().min(dim=1).values, (room.hi - vt).abs().min(dim=1).values)
    surf = walls
    for c, r in room.spheres:
        surf = torch.minimum(surf, ((vt - c).norm(dim=1) - r).abs())
    e = surf[near]
    med, p90 = float(e.median()), float(e.quantile(0.9))
    g = torch.Generator().manual_seed(0)
    sub = kp[torch.randperm(kp.shape[0], generator=g)[:10000].to(dev)]
    dk = torch.full((sub.shape[0],), float("inf"), device=dev)
    for lo in range(0, V, 20000):
        dk = torch.minimum(dk, torch.cdist(sub, vg[lo:lo + 20000]).min(dim=1).values)
    cover = float((dk < 0.03).double().mean())
    print(f"\nget_mesh toy: V={V} F={F} near={int(near.sum())} median {med*100:.2f} cm p90 {p90*100:.2f} cm "
          f"coverage {cover*100:.1f} %")
    assert med <= 0.02 and p90 <= 0.05
    assert cover >= 0.8


def test_get_mesh_no_surface(tmp_path, capsys):
    from myslam_amd.src.utils import Mesher as M
    sc, s = _toy_run()
    m = _mesher(sc, resolution=0.05, level=1.5)              # tanh keeps the field below 1
    out = tmp_path / "none.ply"
    M.get_mesh(m, str(out), s.all_planes, s.decoders, s.keyframe_dict, device="cuda:0")
    assert not out.exists()
    assert M.NO_SURFACE in capsys.readouterr().out
