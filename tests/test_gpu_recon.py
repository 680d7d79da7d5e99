"""Mesh culling and the 3D reconstruction metrics on the GPU: exact nearest neighbours (eslam_nn_*) against brute
force, the visibility test (eslam_cull_vertices) against a torch implementation of its five steps, ICP (eslam_icp_moments
+ the host solve) against known motions and a numpy loop, the metrics on analytic meshes, and get_mesh -> cull_mesh ->
calc_3d_metric end to end.  Every reference computation here is written from the formulas in include/eslam_hip.h."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------
# nearest neighbours
# ----------------------------------------------------------------------------------------------
def _brute(ref, q):
    """float64 brute force on the device: (nearest distance, index, second-nearest distance)."""
    r, qq = ref.double(), q.double()
    d2 = ((qq[:, None, :] - r[None, :, :]) ** 2).sum(-1)
    k = min(2, r.shape[0])
    v, i = d2.topk(k, dim=1, largest=False)
    second = v[:, 1].sqrt() if k == 2 else torch.full_like(v[:, 0], math.inf)
    return v[:, 0].sqrt(), i[:, 0], second


def _check_exact(ref, q, dist, idx):
    d_ref, i_ref, second = _brute(ref, q)
    assert torch.isfinite(dist).all() and (idx >= 0).all()
    rel = (dist.double() - d_ref).abs() / d_ref.clamp(min=1e-30)
    assert float(rel.max()) <= 1e-6 or float((dist.double() - d_ref).abs().max()) <= 1e-7
    clear = second > d_ref * (1 + 1e-6) + 1e-9
    assert torch.equal(idx.long()[clear], i_ref[clear])
    # the chosen point is at the reported distance
    dd = (ref[idx.long()].double() - q.double()).norm(dim=1)
    assert float(((dd - d_ref).abs() / d_ref.clamp(min=1e-30)).max()) <= 1e-6 or float((dd - d_ref).abs().max()) <= 1e-7


def _clouds():
    g = torch.Generator().manual_seed(0)
    uni = torch.rand(3000, 3, generator=g) * torch.tensor([4.0, 3.0, 2.0]) - 1.0
    dirs = torch.randn(4000, 3, generator=g)
    sph = dirs / dirs.norm(dim=1, keepdim=True) * 0.7 + torch.tensor([0.2, -0.1, 0.3])
    plane = torch.rand(2000, 3, generator=g) * torch.tensor([2.0, 2.0, 0.0])
    surf = torch.cat([sph, plane], 0)
    q_in = torch.rand(2500, 3, generator=g) * torch.tensor([5.0, 4.0, 3.0]) - 1.5
    far = torch.randn(300, 3, generator=g)
    q_far = far / far.norm(dim=1, keepdim=True) * 10.0 + torch.tensor([1.0, 0.5, 0.0])   # 10 m outside the box
    return {"uniform": uni, "surface": surf}, torch.cat([q_in, q_far], 0)


@pytest.mark.parametrize("kind", ["uniform", "surface"])
def test_nn_exact(kind):
    from myslam_amd import ops
    dev = _dev()
    clouds, q = _clouds()
    ref, q = clouds[kind].to(dev), q.to(dev)
    grid = ops.NNGrid(ref)
    d1, i1 = grid.query(q)
    _check_exact(ref, q, d1, i1)
    d2, i2 = grid.query(q)                                  # bit-identical run to run,
    d3, i3 = ops.NNGrid(ref).query(q, sort=False)           # across builds and in input order
    assert torch.equal(d1, d2) and torch.equal(i1, i2) and torch.equal(d1, d3) and torch.equal(i1, i3)


def test_nn_duplicates_single_point_and_far_queries():
    from myslam_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(1)
    base = torch.rand(500, 3, generator=g)
    ref = torch.cat([base, base[:200], base[100:300], base[:50]], 0).to(dev)       # every point of base[:300] repeated
    q = torch.cat([base[:300] + 1e-3 * torch.randn(300, 3, generator=g), base[:300]], 0).to(dev)
    d, i = ops.NNGrid(ref).query(q)
    _check_exact(ref, q, d, i)
    # exact duplicates are at equal distance: the smallest index wins
    d_ref, _, _ = _brute(ref, q)
    d2 = ((q.double()[:, None, :] - ref.double()[None]) ** 2).sum(-1)
    ties = (d2 == d2.min(dim=1, keepdim=True).values)
    first = ties.float().argmax(dim=1)
    assert torch.equal(i.long(), first)
    assert torch.equal(d[300:], torch.zeros(300, device=dev))
    # one reference point, queries everywhere (and far away)
    one = torch.tensor([[0.25, -0.5, 2.0]], device=dev)
    qq = torch.cat([torch.randn(1000, 3, generator=g) * 20.0, torch.zeros(1, 3)], 0).to(dev)
    d1, i1 = ops.NNGrid(one).query(qq)
    assert (i1 == 0).all()
    assert float(((d1.double() - (qq.double() - one.double()).norm(dim=1)).abs() / d1.double()).max()) <= 1e-6
    # a flat cloud (all z equal) with queries above and below
    flat = torch.rand(2000, 3, generator=g)
    flat[:, 2] = 0.3
    grid = ops.NNGrid(flat.to(dev))
    assert grid.dims[2] == 1
    qf = (torch.rand(1500, 3, generator=g) * 3 - 1).to(dev)
    df, jf = grid.query(qf)
    _check_exact(flat.to(dev), qf, df, jf)


def test_nn_max_dist():
    from myslam_amd import ops
    dev = _dev()
    clouds, q = _clouds()
    ref, q = clouds["surface"].to(dev), q.to(dev)
    grid = ops.NNGrid(ref)
    d_all, i_all = grid.query(q)
    for md in (0.01, 0.1, 0.5):
        d, i = grid.query(q, max_dist=md)
        inside = d_all < md                                 # strict: the float32 distance below max_dist
        assert torch.equal(d[inside], d_all[inside]) and torch.equal(i[inside], i_all[inside])
        assert torch.isinf(d[~inside]).all() and (i[~inside] == -1).all()
        assert 0 < int(inside.sum()) < q.shape[0]
    # a query exactly at max_dist from its only neighbour is out
    one = torch.tensor([[0.0, 0.0, 0.0]], device=dev)
    d, i = ops.NNGrid(one).query(torch.tensor([[0.5, 0.0, 0.0]], device=dev), max_dist=0.5)
    assert math.isinf(float(d[0])) and int(i[0]) == -1
    d, i = ops.NNGrid(one).query(torch.tensor([[0.5, 0.0, 0.0]], device=dev), max_dist=0.5000001)
    assert float(d[0]) == 0.5 and int(i[0]) == 0


def test_nn_450k_against_cdist():
    """450 k x 450 k surface-like points; 20 k random queries checked against float64 cdist in chunks of < 1 GB."""
    from myslam_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(2)
    n = 450000
    dirs = torch.randn(n, 3, device=dev, generator=g)
    ref = dirs / dirs.norm(dim=1, keepdim=True) * 1.5
    ref[: n // 3, 2] = -1.2                                          # a third on a floor plane
    ref[: n // 3, :2] = torch.rand(n // 3, 2, device=dev, generator=g) * 4 - 2
    q = ref[torch.randperm(n, device=dev, generator=g)] + 0.01 * torch.randn(n, 3, device=dev, generator=g)
    grid = ops.NNGrid(ref)
    d, i = grid.query(q)
    sub = torch.randperm(n, device=dev, generator=g)[:20000]
    best = torch.empty(sub.shape[0], dtype=torch.float64, device=dev)
    arg = torch.empty(sub.shape[0], dtype=torch.int64, device=dev)
    r64 = ref.double()
    for lo in range(0, sub.shape[0], 250):                          # 250 x 450 k float64 = 0.9 GB
        dd = torch.cdist(q[sub[lo:lo + 250]].double(), r64)
        v, a = dd.min(dim=1)
        best[lo:lo + 250], arg[lo:lo + 250] = v, a
        del dd
    assert float(((d[sub].double() - best).abs() / best).max()) <= 1e-6
    same = i[sub].long() == arg
    dsel = (ref[i[sub].long()].double() - q[sub].double()).norm(dim=1)
    assert bool((same | ((dsel - best).abs() <= 1e-6 * best)).all())


# ----------------------------------------------------------------------------------------------
# culling
# ----------------------------------------------------------------------------------------------
def _torch_cull(verts, frames, fx, fy, cx, cy, H, W, trunc, depth_test):
    """Steps 1-5 of eslam_cull_vertices in torch (float32): (seen [V], borderline [V]) where borderline marks a vertex
    within 1e-3 px of an image edge or 1e-4 m of the depth comparison in some frame."""
    dev = verts.device
    seen = torch.zeros(verts.shape[0], dtype=torch.bool, device=dev)
    border = torch.zeros_like(seen)
    for depth, c2w in frames:
        w2c = torch.linalg.inv(c2w.double().cpu()).float().to(dev)
        c = verts @ w2c[:3, :3].T + w2c[:3, 3]
        a = fx * (-c[:, 0]) + cx * c[:, 2]
        b = fy * c[:, 1] + cy * c[:, 2]
        zz = c[:, 2] + 1e-5
        u, v = a / zz, b / zz
        ok = (-zz >= 0) & (u < W) & (u > 0) & (v < H) & (v > 0)
        edge = torch.stack([u.abs(), (u - W).abs(), v.abs(), (v - H).abs()], 1).min(dim=1).values < 1e-3
        bd = edge & (-zz >= 0)
        if depth_test:
            grid = torch.stack([u / W, v / H], 1) * 2 - 1
            d = F.grid_sample(depth.to(dev)[None, None], grid[None, None], padding_mode="zeros", align_corners=True).reshape(-1)
            bd = bd | (ok & ((d + trunc + zz).abs() < 1e-4))
            ok = ok & (d + trunc >= -zz)
        seen |= ok
        border |= bd
    return seen, border


def _room_frames(n=13):
    from myslam_amd import scene as scn, synthscene
    sc = scn.make_scene("toy")
    return sc, synthscene.make_sequence(sc, n, device=_dev())


@pytest.mark.parametrize("depth_test", [True, False])
def test_cull_against_torch(depth_test):
    from myslam_amd import ops
    dev = _dev()
    sc, frames = _room_frames()
    g = torch.Generator(device=dev).manual_seed(3)
    b = sc.bound.to(dev).float()
    inside = torch.rand(200000, 3, device=dev, generator=g) * (b[:, 1] - b[:, 0]) + b[:, 0]
    # points near the observed surface (back-projected depth, jittered by up to 10 cm)
    near = []
    for _, _, depth, c2w in frames[::3]:
        ro, rd = ops.image_rays(sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy, c2w)
        dd = depth.reshape(-1)
        near.append(ro + rd * dd[:, None] + 0.05 * torch.randn(rd.shape, device=dev, generator=g))
    verts = torch.cat([inside] + near, 0).contiguous()
    trunc = float(sc.truncation)
    fr = [(f[2], f[3]) for f in frames]
    seen = ops.cull_vertices(verts, fr, (sc.fx, sc.fy, sc.cx, sc.cy), sc.H, sc.W, trunc, depth_test, chunk=4)
    ref, border = _torch_cull(verts, fr, sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, trunc, depth_test)
    mism = seen != ref
    print(f"\ncull depth_test={depth_test}: V={verts.shape[0]} seen={int(seen.sum())} mismatches={int(mism.sum())} "
          f"(borderline {int(border.sum())})")
    assert not bool((mism & ~border).any())
    assert 0 < int(seen.sum()) < verts.shape[0]
    # chunking does not change the result
    assert torch.equal(seen, ops.cull_vertices(verts, fr, (sc.fx, sc.fy, sc.cx, sc.cy), sc.H, sc.W, trunc, depth_test))


def test_cull_hand_placed():
    from myslam_amd import ops
    dev = _dev()
    sc, frames = _room_frames(1)
    from myslam_amd import synthscene
    _, _, depth, c2w = frames[0]
    c2w64 = c2w.double().cpu()
    o, R = c2w64[:3, 3], c2w64[:3, :3]
    fwd = -R[:, 2]                                     # the camera looks along its -z
    right = R[:, 0]
    dc = float(synthscene.AnalyticRoom(sc.bound).cast(o, fwd[None])[0][0])     # the surface on the optical axis
    pts = torch.stack([
        o + 0.5 * fwd * dc,                            # in front of the wall: seen
        o - 1.0 * fwd,                                 # behind the camera
        o + 1.0 * fwd + 5.0 * right,                   # outside the frustum (far to the side)
        o + (dc + 0.3) * fwd,                          # behind the wall by 0.3 m > truncation
    ]).float().to(dev)
    assert 0.3 > sc.truncation
    f = [(depth, c2w)]
    k = (sc.fx, sc.fy, sc.cx, sc.cy)
    assert ops.cull_vertices(pts, f, k, sc.H, sc.W, sc.truncation, True).tolist() == [True, False, False, False]
    assert ops.cull_vertices(pts, f, k, sc.H, sc.W, sc.truncation, False).tolist() == [True, False, False, True]


# ----------------------------------------------------------------------------------------------
# ICP
# ----------------------------------------------------------------------------------------------
def _room_sdf_mesh(bound, res, room=None):
    """(verts float32 [V,3], faces int32 [F,3]) on the GPU: marching cubes of the analytic room's SDF (the box walls
    and the spheres: positive in free space) at `res` metres."""
    from myslam_amd import ops, synthscene
    dev = _dev()
    room = room or synthscene.AnalyticRoom(bound)
    b = bound.double()
    axes = [torch.arange(float(b[k, 0]), float(b[k, 1]) + res / 2, res, dtype=torch.float64) for k in range(3)]
    gx = axes[0].to(dev)[:, None, None]
    gy = axes[1].to(dev)[None, :, None]
    gz = axes[2].to(dev)[None, None, :]
    lo, hi = room.lo.to(dev), room.hi.to(dev)
    sdf = torch.minimum(torch.minimum(torch.minimum(gx - lo[0], hi[0] - gx), torch.minimum(gy - lo[1], hi[1] - gy)),
                        torch.minimum(gz - lo[2], hi[2] - gz))
    for c, r in room.spheres:
        c = c.to(dev)
        sdf = torch.minimum(sdf, ((gx - c[0]) ** 2 + (gy - c[1]) ** 2 + (gz - c[2]) ** 2).sqrt() - r)
    vol = sdf.float().contiguous()
    del sdf
    return ops.marching_cubes(vol, 0.0, (float(axes[0][0]), float(axes[1][0]), float(axes[2][0])), (res, res, res))


def _rigid(deg, axis, t):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    th = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = t
    return T


def test_icp_recovers_motion_and_identity():
    from myslam_amd.src.tools.eval_recon import icp
    from myslam_amd import scene as scn
    sc = scn.make_scene("toy")
    v, _ = _room_sdf_mesh(sc.bound, 0.03)
    M = _rigid(2.0, [0.2, 0.3, 1.0], [0.03, 0.0, 0.0])        # 2 degrees, 3 cm
    Minv = np.linalg.inv(M)
    vd = v.double()
    Mi = torch.from_numpy(Minv).to(v.device)
    src = (vd @ Mi[:3, :3].T + Mi[:3, 3]).float()            # the target moved by M^-1: ICP must find M
    T, info = icp(src, v)
    print(f"\nicp: V={v.shape[0]} rounds={info['rounds']} fitness={info['fitness']:.6f} rmse={info['inlier_rmse']:.3e}")
    assert np.abs(T - M).max() < 1e-4, np.abs(T - M).max()
    T0, info0 = icp(v, v)
    assert np.abs(T0 - np.eye(4)).max() < 1e-9 and info0["fitness"] == 1.0 and info0["inlier_rmse"] < 1e-9


def _numpy_icp(src, tgt, thr=0.1, rounds=30):
    """open3d's point-to-point loop in numpy float64 with brute-force correspondences."""
    from myslam_amd.src.tools.eval_recon import umeyama_from_moments
    T = np.eye(4)

    def corr(T):
        s = src @ T[:3, :3].T + T[:3, 3]
        d2 = ((s[:, None, :] - tgt[None]) ** 2).sum(-1)
        j = d2.argmin(1)
        d = np.sqrt(d2[np.arange(len(s)), j])
        ok = d < thr
        ss, tt = s[ok], tgt[j[ok]]
        m = np.concatenate([[ok.sum(), (d[ok] ** 2).sum()], ss.sum(0), tt.sum(0), (ss[:, :, None] * tt[:, None, :]).sum(0).ravel()])
        return m, ok.sum() / len(s), (np.sqrt(m[1] / m[0]) if m[0] > 0 else 0.0)

    m, f, r = corr(T)
    n = 0
    for _ in range(rounds):
        T = umeyama_from_moments(m) @ T
        n += 1
        pf, pr = f, r
        m, f, r = corr(T)
        if abs(pf - f) < 1e-6 and abs(pr - r) < 1e-6:
            break
    return T, n


def test_icp_matches_numpy_loop():
    from myslam_amd.src.tools.eval_recon import icp
    rng = np.random.default_rng(7)
    tgt = rng.uniform(-1, 1, size=(2000, 3))
    tgt[:1000, 2] = -1.0                                      # a floor and a box of points
    M = _rigid(4.0, [1.0, -0.4, 0.7], [0.02, -0.03, 0.015])
    src = (tgt[:1500] + 0.002 * rng.normal(size=(1500, 3))) @ np.linalg.inv(M)[:3, :3].T + np.linalg.inv(M)[:3, 3]
    src, tgt = src.astype(np.float32).astype(np.float64), tgt.astype(np.float32).astype(np.float64)
    T_np, n_np = _numpy_icp(src, tgt)
    T, info = icp(torch.from_numpy(src), torch.from_numpy(tgt))
    print(f"\nicp 2k: rounds {info['rounds']} (numpy {n_np}), max |T - T_numpy| = {np.abs(T - T_np).max():.2e}")
    assert info["rounds"] == n_np
    assert np.abs(T - T_np).max() < 1e-5
    T2, _ = icp(torch.from_numpy(src), torch.from_numpy(tgt))
    assert np.array_equal(T, T2)                              # bit-reproducible


# ----------------------------------------------------------------------------------------------
# metrics
# ----------------------------------------------------------------------------------------------
def _sphere_mesh(r, res=0.01):
    from myslam_amd import ops
    dev = _dev()
    ax = torch.arange(-1.2, 1.2 + res / 2, res, dtype=torch.float64)
    g = ax.to(dev)
    vol = ((g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2).sqrt() - r).float().contiguous()
    return ops.marching_cubes(vol, 0.0, (float(ax[0]),) * 3, (res, res, res))


def test_metrics_concentric_spheres():
    from myslam_amd.src.tools.eval_recon import recon_metrics
    gv, gf = _sphere_mesh(1.0)
    r2 = recon_metrics(*_sphere_mesh(1.02), gv, gf, align=False, num_points=450000)
    print(f"\nspheres 2 cm: {r2}")
    assert abs(r2["accuracy"] - 2.0) < 0.1 and abs(r2["completion"] - 2.0) < 0.1
    assert r2["completion_ratio"] == 100.0
    r7 = recon_metrics(*_sphere_mesh(1.07), gv, gf, align=False, num_points=450000)
    print(f"spheres 7 cm: {r7}")
    assert abs(r7["accuracy"] - 7.0) < 0.2 and r7["completion_ratio"] < 0.01


def test_metrics_equal_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    from myslam_amd import ops
    from myslam_amd.src.tools import eval_recon as ev
    gv, gf = _sphere_mesh(1.0, 0.02)
    rv, rf = _sphere_mesh(1.03, 0.02)
    rv = rv + torch.tensor([0.01, -0.02, 0.0], device=rv.device)
    n = 100000
    r = ev.recon_metrics(rv, rf, gv, gf, align=False, num_points=n, seed=5)
    rec_pc = ops.sample_surface(rv, rf, n, 5)[0].float().double().cpu().numpy()
    gt_pc = ops.sample_surface(gv, gf, n, 6)[0].float().double().cpu().numpy()
    acc = spatial.cKDTree(gt_pc).query(rec_pc)[0]
    comp = spatial.cKDTree(rec_pc).query(gt_pc)[0]
    assert abs(r["accuracy"] - acc.mean() * 100) <= 1e-6 * acc.mean() * 100
    assert abs(r["completion"] - comp.mean() * 100) <= 1e-6 * comp.mean() * 100
    assert abs(r["completion_ratio"] - (comp < 0.05).mean() * 100) <= 1e-3
    # the reference's three functions, numpy in
    assert abs(ev.accuracy(gt_pc, rec_pc) - acc.mean()) <= 1e-6 * acc.mean()
    assert abs(ev.completion(gt_pc, rec_pc) - comp.mean()) <= 1e-6 * comp.mean()
    assert abs(ev.completion_ratio(gt_pc, rec_pc) - (comp < 0.05).mean()) <= 1e-5


# ----------------------------------------------------------------------------------------------
# end to end: get_mesh -> cull_mesh -> calc_3d_metric
# ----------------------------------------------------------------------------------------------
def test_cull_and_metrics_end_to_end(tmp_path, monkeypatch, capsys):
    """Thresholds set before measuring (accuracy and completion <= 5 cm, ratio >= 50 %).  Observed on the MI355X (toy
    loop, 13 frames, 0.02 grid, two runs): culled mesh V = 20.4-20.6 k of 53.3 k; aligned accuracy 0.45-0.46 cm,
    completion 0.59-0.60 cm, ratio 98.1-98.2 %; not aligned 0.50-0.56 cm, 0.63-0.69 cm, 98.2-98.3 %."""
    from myslam_amd import synthscene
    from myslam_amd.src.tools import cull_mesh as cm, eval_recon as ev
    from myslam_amd.src.utils import Mesher as M, datasets
    from myslam_amd.src.utils.Mesher import read_ply, write_ply
    from tests.test_gpu_mesh import _mesher, _toy_run
    sc, s = _toy_run()
    frames = synthscene.make_sequence(sc, 13, device=_dev())
    mesh = tmp_path / "mesh.ply"
    M.get_mesh(_mesher(sc), str(mesh), s.all_planes, s.decoders, s.keyframe_dict, device="cuda:0")
    cfg = {"meshing": {"eval_rec": True}, "model": {"truncation": sc.truncation},
           "cam": {"H": sc.H, "W": sc.W, "fx": sc.fx, "fy": sc.fy, "cx": sc.cx, "cy": sc.cy}}
    monkeypatch.setattr(datasets, "get_dataset", lambda cfg, args, scale, device="cuda:0": frames)
    est = [c.clone() for c in s.estimate_c2w_list]
    cm.cull_mesh(str(mesh), cfg, None, "cuda:0", estimate_c2w_list=est)
    culled = tmp_path / "mesh_culled.ply"
    v0, f0, _ = read_ply(str(mesh))
    v1, f1, c1 = read_ply(str(culled))
    assert 0 < len(f1) <= len(f0) and 0 < len(v1) <= len(v0) and c1 is not None
    # ground truth: the analytic room's SDF at 1 cm, culled with the ground-truth poses
    gv, gf = _room_sdf_mesh(sc.bound, 0.01)
    gt = cm.cull_mesh_arrays(gv.cpu().numpy(), gf.cpu().numpy(), None, frames, sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy,
                             sc.truncation, True)
    gt_path = tmp_path / "gt.ply"
    write_ply(str(gt_path), gt[0], gt[1])
    capsys.readouterr()
    r = ev.calc_3d_metric(str(culled), str(gt_path))
    out = capsys.readouterr().out
    assert "accuracy: " in out and "completion: " in out and "completion ratio: " in out
    r0 = ev.calc_3d_metric(str(culled), str(gt_path), align=False)
    with capsys.disabled():
        print(f"\nend to end: rec V={len(v1)} F={len(f1)} (uncut {len(v0)} / {len(f0)}), GT V={len(gt[0])} F={len(gt[1])}; "
              f"aligned {r}; not aligned {r0}")
    for res in (r, r0):
        assert res["accuracy"] <= 5.0 and res["completion"] <= 5.0 and res["completion_ratio"] >= 50.0
    # the command line of the reference's eval_recon.py, in a fresh process
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "myslam_amd.src.tools.eval_recon", "--rec_mesh", str(culled), "--gt_mesh",
                        str(gt_path), "-3d"], cwd=root, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(("accuracy: ", "completion: ", "completion ratio: "))]
    assert len(lines) == 3 and float(lines[0].split()[-1]) == r["accuracy"]
