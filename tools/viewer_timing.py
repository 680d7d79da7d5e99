"""Device time of the offline viewer's frame on room0 at the reference's window size, next to the depth rasteriser on the
same mesh, pose and size (ops.render_mesh_depth: the yardstick that predates the viewer).

    python tools/viewer_timing.py [--repeats 7] [--out DIR] [--small]

Mesh: the median-level mesh of DESIGN.md section 14 (11.9 M vertices, 23.8 M triangles) with a colour per vertex; two
trajectories of 2000 poses and the two camera actors, as the viewer holds them.  Views: the viewer's pose for the first
frame (4 m behind it) and the top view.  Per view, alternated in every repeat after a warm-up round: the whole frame
(SLAMFrontend.render: begin, mesh, 4 point calls, resolve), the mesh alone in colour, the mesh alone without vertex
colours (no colour loads: the 64-bit keys' share), the points alone, and the depth pass.  Device-event times, medians with
[min, max].  Also the host time of a frame's copy to the host and of writing it as JPEG.  Prints one JSON line (and writes
it to DIR/viewer_room0_timing.json when --out is given).  --small: the 1 cm analytic room instead of the median mesh."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from recon_timing import median_mesh, room_sdf_mesh  # noqa: E402


def _once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _stats(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(min(xs)), "max_ms": float(max(xs)), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    from myslam_amd import harness, ops, synthscene
    from myslam_amd.src.tools import visualizer_util as vu
    from myslam_amd.visualizer import top_view_pose
    dev = torch.device("cuda:0")
    wl = harness.make_workload("room0", 64, 24, 8, device=dev, planes="synth")
    sc = wl.scene
    frames = synthscene.make_sequence(sc, 16, device=dev)
    if args.small:
        v, f = room_sdf_mesh(synthscene.AnalyticRoom(sc.bound), sc.bound, 0.01, dev)
    else:
        kfs = [{"est_c2w": c2w, "depth": depth, "color": color, "idx": idx} for idx, color, depth, c2w in frames[:13:4]]
        v, f = median_mesh(wl, sc, kfs, dev)
    v, f = v.float().contiguous(), f.to(torch.int32).contiguous()
    g = torch.Generator(device=dev).manual_seed(0)
    col = torch.randint(0, 256, (v.shape[0], 4), device=dev, generator=g, dtype=torch.uint8)
    # two trajectories of 2000 poses: the sequence's own, stretched, and a copy 2 cm off
    n = 2000
    traj = synthscene.trajectory(n, sc.bound).double().cpu().numpy()
    gt = traj.copy()
    gt[:, :3, 3] += 0.02
    H, W = vu.WINDOW_H, vu.WINDOW_W
    res = {"scene": "room0", "image": [W, H], "V": int(v.shape[0]), "F": int(f.shape[0]), "trajectory_poses": n,
           "repeats": args.repeats}
    inits = {"first_frame": gt[0].copy(), "top_view": top_view_pose(v)}
    with tempfile.TemporaryDirectory() as tmp:
        for name, init in inits.items():
            fe = vu.SLAMFrontend(tmp, init, cam_scale=0.2, estimate_c2w_list=traj, gt_c2w_list=gt)
            fe.mesh = (v, f, col)
            for is_gt, poses in ((False, traj), (True, gt)):
                fe.update_pose(1, poses[n - 1], gt=is_gt)
                fe.update_cam_trajectory(n, gt=is_gt)
            view, K = fe.view[None], fe.K
            kw = dict(z_near=fe.z_near, z_far=vu.Z_FAR)
            pts = [(p, vu.RED if key < vu.GT_KEY else vu.GREEN) for key, (p, _) in sorted(fe.cameras.items())]
            pts += [(p, vu.GREEN if is_gt else vu.RED) for is_gt, p in sorted(fe.traj.items())]
            pts = [(p, torch.tensor(c, dtype=torch.uint8), vu.POINT_SIZE) for p, c in pts]
            runs = {
                "frame": fe.render,
                "colour_mesh": lambda: ops.render_view([(v, f, col)], [], view, K, H, W, chunk=1, **kw),
                "colour_mesh_no_vertex_colours": lambda: ops.render_view([(v, f, None)], [], view, K, H, W, chunk=1, **kw),
                "points": lambda: ops.render_view([], pts, view, K, H, W, chunk=1, **kw),
                "depth": lambda: ops.render_mesh_depth(v, f, view, K, H, W, chunk=1, **kw),
            }
            for fn in runs.values():                                    # warm-up round (allocations, first launches)
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in runs}
            for _ in range(args.repeats):                                # alternated: drift falls on every variant alike
                for k, fn in runs.items():
                    times[k].append(_once(fn))
            r = {k: _stats(t) for k, t in times.items()}
            r["colour_over_depth"] = r["colour_mesh"]["median_ms"] / r["depth"]["median_ms"]
            r["frame_over_depth"] = r["frame"]["median_ms"] / r["depth"]["median_ms"]
            img, d = ops.render_view([(v, f, col)], pts, view, K, H, W, chunk=1, return_depth=True, **kw)
            r["hit_share"] = float((d > 0).float().mean())
            r["red_or_green_pixels"] = int(((img[0] == torch.tensor(vu.RED, device=dev, dtype=torch.uint8)).all(-1) |
                                            (img[0] == torch.tensor(vu.GREEN, device=dev, dtype=torch.uint8)).all(-1)).sum())
            assert torch.equal(fe.render(), img[0])
            copy_ms, write_ms = [], []
            for k in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = img[0].cpu().numpy()
                t1 = time.perf_counter()
                from PIL import Image
                Image.fromarray(host).save(os.path.join(tmp, f"{k:06d}.jpg"), quality=95)
                t2 = time.perf_counter()
                copy_ms.append((t1 - t0) * 1e3)
                write_ms.append((t2 - t1) * 1e3)
            r["copy_to_host"] = _stats(copy_ms)
            r["jpeg_write"] = _stats(write_ms)
            res[name] = r
            print(name, json.dumps(r), flush=True)
    res["device"] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "viewer_room0_timing.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
