"""Per-stage device time of mesh extraction on room0 at the reference's resolution (configs/ESLAM.yaml:14, 0.01 m):
the frame hull, the field, marching cubes (count + scan, emit), vertex colours and the PLY write.

    python tools/mesh_timing.py [--res 0.01] [--frames 13] [--out DIR] [--level-quantile Q] [--mixed]

--mixed: the field (eslam_sdf_grid) and the vertex colours (eval_points) also on the planes' half copies
(ops.mixed_precision(half, points=True)), against float32 in the same process: the two are timed in alternating windows of
--mixed-reps calls each, --mixed-rounds times; the JSON gets the median window and the spread of both.

Grid: room0's marching_cubes_bound (configs/Replica/room0.yaml:4).  Planes: scene.synth_planes of room0
(harness.make_workload(..., planes="synth")), whose field need not cross 0: --level-quantile picks a level that cuts it,
so that the emit, colour and PLY stages see a surface.  Keyframes: every 4th frame of the
synthetic sequence (synthscene.make_sequence) at room0's camera, with est_c2w = the ground-truth pose.  Prints one JSON
line (and writes it to DIR/mesh_timing.json when --out is given).
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=float, default=0.01)
    ap.add_argument("--frames", type=int, default=13)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-ply", action="store_true")
    ap.add_argument("--level", type=float, default=None, help="marching-cubes level (default: the reference's 0)")
    ap.add_argument("--level-quantile", type=float, default=None, help="level = this quantile of the field inside the hull")
    ap.add_argument("--mixed", action="store_true", help="also time the field and the vertex colours on the half copies")
    ap.add_argument("--mixed-reps", type=int, default=10)
    ap.add_argument("--mixed-rounds", type=int, default=5)
    args = ap.parse_args()
    from myslam_amd import harness, ops, scene as scn, synthscene
    from myslam_amd.src.utils import Mesher as M
    dev = torch.device("cuda:0")
    wl = harness.make_workload("room0", 64, 24, 8, device=dev, planes="synth")
    sc = wl.scene
    frames = synthscene.make_sequence(sc, args.frames, device=dev)
    kfs = [{"est_c2w": c2w, "depth": depth, "color": color, "idx": idx} for idx, color, depth, c2w in frames[::4]]
    m = SimpleNamespace(H=sc.H, W=sc.W, fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy, scale=1.0, resolution=args.res, level_set=0.0,
                        mesh_bound_scale=1.02, bound=sc.bound, points_batch_size=500000,
                        marching_cubes_bound=torch.tensor(scn._SCENES["room0"]["bound"], dtype=torch.float64))

    def stage(fn, reps=1):
        fn()                                                  # warm-up (allocations, first launches)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1) / reps

    res = {"scene": "room0", "resolution": args.res, "keyframes": len(kfs)}
    x, y, z = M.grid_axes(m.marching_cubes_bound, m.resolution)
    axes = [torch.from_numpy(a).float().to(dev) for a in (x, y, z)]
    res["grid"] = [len(x), len(y), len(z)]
    hull, res["hull_ms"] = stage(lambda: M.get_bound_from_frames(m, kfs))
    print("hull", res["hull_ms"], flush=True)
    vol, res["field_ms"] = stage(lambda: ops.sdf_grid(wl.planes, wl.decoders, axes, m.bound, hull.halfspaces), reps=3)
    print("field", res["field_ms"], flush=True)
    vol_nohull, res["field_no_hull_ms"] = stage(lambda: ops.sdf_grid(wl.planes, wl.decoders, axes, m.bound), reps=3)
    del vol_nohull
    if args.level is not None:
        m.level_set = args.level
    elif args.level_quantile is not None:       # a level that cuts the synthetic field (its level 0 may not)
        inside = vol[vol > -1.0]
        m.level_set = float(inside.float().quantile(args.level_quantile)) if inside.numel() < (1 << 24) else \
            float(inside[:: inside.numel() // (1 << 23) + 1].quantile(args.level_quantile))
    res["level"] = m.level_set
    (ws, counts), res["mc_count_scan_ms"] = stage(lambda: ops.mc_count(vol, m.level_set), reps=3)
    V, F = (int(v) for v in counts.tolist())
    res["V"], res["F"] = V, F
    print("count", res["mc_count_scan_ms"], V, F, flush=True)
    origin = (x[0], y[0], z[0])
    spacing = (x[2] - x[1], y[2] - y[1], z[2] - z[1])
    (verts, faces), res["mc_emit_ms"] = stage(lambda: ops.mc_emit(vol, m.level_set, origin, spacing, ws, V, F), reps=3)
    print("emit", res["mc_emit_ms"], flush=True)
    del ws
    _, res["marching_cubes_total_ms"] = stage(lambda: ops.marching_cubes(vol, m.level_set, origin, spacing))
    cols, res["colours_ms"] = stage(lambda: M.eval_points(m, verts, wl.planes, wl.decoders)[:, :3])
    print("colours", res["colours_ms"], flush=True)
    if args.mixed:
        from myslam_amd import lowp
        half = lowp.HalfPlanes(wl.planes)

        def on_copies(fn):
            def g():
                with ops.mixed_precision(half, points=True):
                    return fn()
            return g

        def alternate(f32, mixed):
            """ms per call (median window, min, max) of both, from alternating windows of device-event time."""
            t = {"float32": [], "mixed": []}
            for _ in range(args.mixed_rounds):
                for name, fn in (("float32", f32), ("mixed", mixed)):
                    t[name].append(stage(fn, reps=args.mixed_reps)[1])
            return {k: [sorted(v)[len(v) // 2], min(v), max(v)] for k, v in t.items()}

        field = lambda: ops.sdf_grid(wl.planes, wl.decoders, axes, m.bound, hull.halfspaces)
        colours = lambda: M.eval_points(m, verts, wl.planes, wl.decoders)[:, :3]
        field_no_hull = lambda: ops.sdf_grid(wl.planes, wl.decoders, axes, m.bound)
        res["mixed"] = {"reps": args.mixed_reps, "rounds": args.mixed_rounds, "field_ms": alternate(field, on_copies(field)),
                        "field_no_hull_ms": alternate(field_no_hull, on_copies(field_no_hull)),
                        "colours_ms": alternate(colours, on_copies(colours))}
        d = (on_copies(field)() - field())[vol > -1.0].abs()
        res["mixed"]["field_abs_diff_max"] = float(d.max())
        print("mixed", res["mixed"], flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    if not args.no_ply:
        path = os.path.join(args.out or "/tmp", "mesh_timing.ply")
        v_np, f_np, c_np = verts.cpu().numpy(), faces.cpu().numpy(), cols.cpu().numpy()
        t0 = time.perf_counter()
        M.write_ply(path, v_np, f_np, c_np)
        res["ply_write_ms"] = (time.perf_counter() - t0) * 1e3
        res["ply_bytes"] = os.path.getsize(path)
        os.remove(path)
    res["device"] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(os.path.join(args.out, "mesh_timing.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
