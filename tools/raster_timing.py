"""Device time of the 2D reconstruction metric's stages on room0: the depth rasteriser (clear + raster + resolve of one
eslam_raster_depth call per chunk of 32 views) on three meshes, the depth-L1 reduction, the view test, and the whole metric.

    python tools/raster_timing.py [--views 64] [--areas 16,64,256,1024] [--metric-views 1000] [--out DIR] [--no-median]

Meshes: "gt" = marching cubes of the analytic room's SDF at 1 cm (tools/recon_timing.py; triangles of about a pixel),
"median" = the median-level mesh of DESIGN.md section 14 (the largest mesh the mesher produces here), "box" = the 12
triangles of the room's bounding box (every triangle covers much of the image).  Views: 500 x 500, focal 300, sampled
inside the gt mesh's camera box as the metric samples them (eval_recon.get_cam_position / sample_views, seed 0).  Each
mesh is timed at every size threshold of --areas (eslam_raster_depth's large_area) and at the library's default.  The
view test runs on --views candidate views against 10^6 points; the metric is depth_l1_metric(gt moved by 2 cm, gt) over
--metric-views views, a host clock around it (it ends in a copy to the host).  Prints one JSON line (and writes it to
DIR/raster_room0_timing.json when --out is given).  For a per-kernel table run it under
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/raster_timing.py --metric-views 0 --no-median`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from recon_timing import median_mesh, room_sdf_mesh, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--areas", default="16,64,256,1024")
    ap.add_argument("--metric-views", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-median", action="store_true")
    args = ap.parse_args()
    from myslam_amd import harness, ops, synthscene
    from myslam_amd.src.tools import eval_recon as ev
    dev = torch.device("cuda:0")
    wl = harness.make_workload("room0", 64, 24, 8, device=dev, planes="synth")
    sc = wl.scene
    room = synthscene.AnalyticRoom(sc.bound)
    meshes = {"gt": room_sdf_mesh(room, sc.bound, 0.01, dev)}
    if not args.no_median:
        frames = synthscene.make_sequence(sc, 16, device=dev)
        kfs = [{"est_c2w": c2w, "depth": depth, "color": color, "idx": idx} for idx, color, depth, c2w in frames[:13:4]]
        meshes["median"] = median_mesh(wl, sc, kfs, dev)
    b = sc.bound.double().cpu().numpy()
    lo, hi = b[:, 0], b[:, 1]
    bv = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    bf = np.array([t for p, q, r, s in quads for t in ((p, q, r), (p, r, s))], dtype=np.int32)
    meshes["box"] = (torch.from_numpy(bv).to(dev), torch.from_numpy(bf).to(dev))
    torch.cuda.synchronize()
    gv, gf = meshes["gt"]
    res = {"scene": "room0", "image": [ev.IMG_W, ev.IMG_H], "views": args.views, "default_large_area": ops._hip.RASTER_LARGE_AREA}
    extents, transform = ev.get_cam_position(gv)
    views, _ = ev.sample_views(extents, transform, args.views, None, 0)
    K = (ev.FOCAL, ev.FOCAL, ev.IMG_CX, ev.IMG_CY)
    areas = [int(a) for a in args.areas.split(",") if a] + [0]
    images = {}
    for name, (v, f) in meshes.items():
        v, f = v.float().contiguous(), f.to(torch.int32).contiguous()
        res[f"{name}_V"], res[f"{name}_F"] = int(v.shape[0]), int(f.shape[0])
        for rep in range(2):                                   # two rounds, alternating the settings: the spread
            for a in areas:
                img, ms = timed(lambda: ops.render_mesh_depth(v, f, views, K, ev.IMG_H, ev.IMG_W, large_area=a), reps=2)
                res.setdefault(f"raster_{name}_area{a or 'default'}_ms_per_view", []).append(ms / len(views))
                if name in images:
                    assert torch.equal(images[name], img), (name, a)
                images[name] = img
        res[f"raster_{name}_hit_share"] = float((images[name] > 0).float().mean())
        print(name, res, flush=True)
    other = images.get("median", images["box"])
    out, ms = timed(lambda: ops.depth_l1(images["gt"], other), reps=10)
    res["depth_l1_ms_per_view"] = ms / len(views)
    res["depth_l1_mean_cm"] = float(out.mean()) / (ev.IMG_H * ev.IMG_W) * 100
    g = torch.Generator(device=dev).manual_seed(0)
    pts = torch.rand(1000000, 3, device=dev, generator=g) * torch.tensor(hi - lo, device=dev).float() + torch.tensor(lo, device=dev).float()
    seen, ms = timed(lambda: ops.views_see_points(pts, views, K, ev.IMG_H, ev.IMG_W), reps=5)
    res["views_see_points_1e6_ms_per_view"] = ms / len(views)
    res["views_see_points_seen"] = int(seen.sum())
    if args.metric_views > 0:
        moved = gv.double() + torch.tensor([0.02, 0.0, 0.0], dtype=torch.float64, device=dev)
        ev.depth_l1_metric(moved, gf, gv, gf, align=False, n_imgs=32)          # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ev.depth_l1_metric(moved, gf, gv, gf, align=False, n_imgs=args.metric_views)
        torch.cuda.synchronize()
        res["metric_views"] = args.metric_views
        res["metric_total_ms"] = (time.perf_counter() - t0) * 1e3
        res["metric_depth_l1_cm"] = r["depth_l1"]
    res["device"] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "raster_room0_timing.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
