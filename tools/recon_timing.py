"""Device time of mesh culling and the 3D reconstruction metrics on room0 (1200x680 frames), with two baselines: chunked
torch.cdist + min on the same GPU, and scipy's cKDTree on the host when scipy is importable.

    python tools/recon_timing.py [--frames 64] [--points 450000] [--out DIR] [--no-baselines]

Meshes: "gt" = marching cubes of the analytic room's SDF (synthscene.AnalyticRoom of room0) at 1 cm; "median" = the
median-level mesh of DESIGN.md section 14 (scene.synth_planes of room0 on the 1 cm grid inside the frame hull, cut at the
field's median).  Frames: the synthetic sequence at room0's camera (synthscene.make_sequence).  Nearest neighbours: the
surfaces sampled at --points each (ops.sample_surface), a grid built on one set and queried with the other, both
directions, in cell order and in input order: "near" = the gt surface against itself moved by 2 degrees / 3 cm (what the
metrics meet), "far" = the gt surface against the median mesh (0.5-2 m apart: long searches).  ICP: the moved gt
vertices aligned back (time per round).  Prints one JSON line (and writes it to DIR/recon_timing.json when --out is given).
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps=1):
    fn()                                                  # warm-up (allocations, first launches)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / reps


def room_sdf_mesh(room, bound, res, dev):
    from myslam_amd import ops
    b = bound.double()
    axes = [torch.arange(float(b[k, 0]), float(b[k, 1]) + res / 2, res, dtype=torch.float64) for k in range(3)]
    gx, gy, gz = (a.to(dev).float() for a in axes)
    lo, hi = room.lo.float().to(dev), room.hi.float().to(dev)
    vol = torch.empty(len(gx), len(gy), len(gz), device=dev)
    for i in range(len(gx)):                             # slab by slab: no float64 volume
        x = gx[i]
        s = torch.minimum(torch.minimum(torch.minimum(x - lo[0], hi[0] - x), torch.minimum(gy[:, None] - lo[1], hi[1] - gy[:, None])),
                          torch.minimum(gz[None, :] - lo[2], hi[2] - gz[None, :]))
        for c, r in room.spheres:
            c = c.float().to(dev)
            s = torch.minimum(s, ((x - c[0]) ** 2 + (gy[:, None] - c[1]) ** 2 + (gz[None, :] - c[2]) ** 2).sqrt() - r)
        vol[i] = s
    v, f = ops.marching_cubes(vol, 0.0, (float(axes[0][0]), float(axes[1][0]), float(axes[2][0])), (res, res, res))
    return v, f


def median_mesh(wl, sc, kfs, dev):
    from myslam_amd import ops, scene as scn
    from myslam_amd.src.utils import Mesher as M
    m = SimpleNamespace(H=sc.H, W=sc.W, fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy, scale=1.0, resolution=0.01, level_set=0.0,
                        mesh_bound_scale=1.02, bound=sc.bound, points_batch_size=500000,
                        marching_cubes_bound=torch.tensor(scn._SCENES["room0"]["bound"], dtype=torch.float64))
    x, y, z = M.grid_axes(m.marching_cubes_bound, m.resolution)
    axes = [torch.from_numpy(a).float().to(dev) for a in (x, y, z)]
    hull = M.get_bound_from_frames(m, kfs)
    vol = ops.sdf_grid(wl.planes, wl.decoders, axes, m.bound, hull.halfspaces)
    inside = vol[vol > -1.0]
    level = float(inside[:: inside.numel() // (1 << 23) + 1].quantile(0.5))
    del inside
    return ops.marching_cubes(vol, level, (x[0], y[0], z[0]), (x[2] - x[1], y[2] - y[1], z[2] - z[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--points", type=int, default=450000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-baselines", action="store_true")
    args = ap.parse_args()
    from myslam_amd import harness, ops, synthscene
    from myslam_amd.src.tools import eval_recon as ev
    dev = torch.device("cuda:0")
    wl = harness.make_workload("room0", 64, 24, 8, device=dev, planes="synth")
    sc = wl.scene
    res = {"scene": "room0", "image": [sc.W, sc.H], "frames": args.frames, "points": args.points}
    frames = synthscene.make_sequence(sc, args.frames, device=dev)
    kfs = [{"est_c2w": c2w, "depth": depth, "color": color, "idx": idx} for idx, color, depth, c2w in frames[:13:4]]
    room = synthscene.AnalyticRoom(sc.bound)
    meshes = {"gt": room_sdf_mesh(room, sc.bound, 0.01, dev), "median": median_mesh(wl, sc, kfs, dev)}
    torch.cuda.synchronize()
    fr = [(f[2], f[3]) for f in frames]
    K = (sc.fx, sc.fy, sc.cx, sc.cy)
    for name, (v, f) in meshes.items():
        res[f"{name}_V"], res[f"{name}_F"] = int(v.shape[0]), int(f.shape[0])
        for dt in (True, False):
            seen, ms = timed(lambda: ops.cull_vertices(v, fr, K, sc.H, sc.W, sc.truncation, dt))
            key = f"cull_{name}_{'depth' if dt else 'nodepth'}"
            res[key + "_ms_per_frame"] = ms / len(fr)
            res[key + "_seen"] = int(seen.sum())
        print(name, res, flush=True)
    n = args.points
    gv, gf = meshes["gt"]
    rv, rf = meshes["median"]
    # the gt vertices moved by 2 degrees about an oblique axis and 3 cm: the ICP source, and a surface near the gt one
    th = np.radians(2.0)
    ax = np.array([0.2, 0.3, 1.0]) / np.linalg.norm([0.2, 0.3, 1.0])
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = torch.from_numpy(np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx).to(dev)
    src = (gv.double() @ R.T + torch.tensor([0.03, 0.0, 0.0], dtype=torch.float64, device=dev)).float()
    gt_pc = ops.sample_surface(gv, gf, n, 1)[0].float()
    rec_pc = ops.sample_surface(rv, rf, n, 0)[0].float()
    moved_pc = ops.sample_surface(src, gf, n, 0)[0].float()
    # near: the moved gt surface (what the metrics meet); far: the median-level mesh, 0.5-2 m from the room's surface
    pairs = {"near_gt_from_moved": (gt_pc, moved_pc), "near_moved_from_gt": (moved_pc, gt_pc),
             "far_gt_from_rec": (gt_pc, rec_pc), "far_rec_from_gt": (rec_pc, gt_pc)}
    for name, (a, b) in pairs.items():
        grid, res[f"nn_build_{name}_ms"] = timed(lambda: ops.NNGrid(a), reps=3)
        res[f"nn_grid_{name}"] = list(grid.dims)
        (d, i), res[f"nn_query_{name}_ms"] = timed(lambda: grid.query(b), reps=3)
        (d2, i2), res[f"nn_query_{name}_unsorted_ms"] = timed(lambda: grid.query(b, sort=False), reps=3)
        assert torch.equal(d, d2) and torch.equal(i, i2)
        res[f"nn_mean_{name}_m"] = float(d.double().mean())
    print("nn", res, flush=True)
    tgrid = ops.NNGrid(gv)
    (T, info), ms = timed(lambda: ev.icp(src, gv, target_grid=tgrid))
    res["icp_V"] = int(src.shape[0])
    res["icp_rounds"] = info["rounds"]
    res["icp_ms_per_round"] = ms / (info["rounds"] + 1)          # rounds + the initial correspondence search
    res["icp_total_ms"] = ms
    for al in (True, False):
        r, ms = timed(lambda: ev.recon_metrics(src, gf, gv, gf, align=al, num_points=n))
        res[f"calc_3d_metric_{'align' if al else 'noalign'}_ms"] = ms
        res[f"calc_3d_metric_{'align' if al else 'noalign'}"] = r
    print("icp/metric", res, flush=True)
    if not args.no_baselines:
        def cdist_min(a, b, chunk=1024):                          # 1024 x 450 k float32 = 1.8 GB
            out = torch.empty(b.shape[0], device=dev)
            for lo in range(0, b.shape[0], chunk):
                out[lo:lo + chunk] = torch.cdist(b[lo:lo + chunk], a).min(dim=1).values
            return out
        for name, (a, b) in (("near_gt_from_moved", (gt_pc, moved_pc)), ("far_gt_from_rec", (gt_pc, rec_pc))):
            dc, res[f"baseline_cdist_{name}_ms"] = timed(lambda: cdist_min(a, b))
            res[f"baseline_cdist_{name}_mean_m"] = float(dc.double().mean())
            try:
                from scipy.spatial import cKDTree
            except ImportError:
                res["baseline_ckdtree"] = "scipy not importable"
                continue
            an, bn = a.double().cpu().numpy(), b.double().cpu().numpy()
            t0 = time.perf_counter()
            tree = cKDTree(an)
            t1 = time.perf_counter()
            dk = tree.query(bn)[0]
            t2 = time.perf_counter()
            res[f"baseline_ckdtree_{name}_build_ms"] = (t1 - t0) * 1e3
            res[f"baseline_ckdtree_{name}_query_ms"] = (t2 - t1) * 1e3
            res[f"baseline_ckdtree_{name}_mean_m"] = float(dk.mean())
    res["device"] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "recon_timing.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
