"""Time the exact point-to-mesh distance (ops.MeshDistance) on a room-sized marching-cubes mesh, on one GPU, in one process:

    python tools/meshdist_timing.py [--resolution 0.02] [--samples 450000] [--rounds 7] [--inner 10] [--out FILE]

Mesh: the synthetic room0 field's level set (ops.sdf_grid + ops.marching_cubes on harness's synth planes and seeded
decoders, at the field's median, as tools/bench_sdf_gradient.py obtains one).  Each figure is a device-event time around
`inner` back-to-back calls divided by `inner`, the median (and min, max) over `rounds`, after a warm-up of every call:

    build_ms            eslam_tri_build alone (count, scan, fill) on the planned grid
    construct_ms        ops.MeshDistance(verts, faces): the plan's statistics, the entry count (two host syncs) and the build
    query_samples_ms    .query of `samples` surface samples of the mesh moved by 1 cm (cell order; the sort included)
    query_vertices_ms   .query of all vertices, moved likewise
    nn_build_query_ms   the yardstick: ops.NNGrid(samples of the mesh).query(the same moved samples) - what the sampled
                        metrics do for one direction (one host sync for the bounding box inside)

and the bias the exact distance removes: recon_report's accuracy of the mesh against a copy of itself displaced by 1 cm
(along the diagonal), exact and sampled, at `samples` points.  Prints one JSON line and writes it to --out.  Needs a GPU;
there is no fallback."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def room_mesh(wl, resolution):
    from myslam_amd import ops
    from myslam_amd.src.utils.Mesher import grid_axes
    dev = wl.device
    x, y, z = grid_axes(wl.scene.bound.double(), resolution)
    axes = [torch.from_numpy(a).float().to(dev) for a in (x, y, z)]
    vol = ops.sdf_grid(wl.planes, wl.decoders, axes, wl.scene.bound)
    level = float(vol[vol > -1.0].median())
    verts, faces = ops.marching_cubes(vol, level, (x[0], y[0], z[0]), (x[2] - x[1], y[2] - y[1], z[2] - z[1]))
    if faces.shape[0] == 0:
        raise RuntimeError("the synthetic field has no level set at its median")
    return verts, faces, level


def timed(fn, rounds, inner):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    ms.sort()
    return {"median": round(ms[len(ms) // 2], 3), "min": round(ms[0], 3), "max": round(ms[-1], 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=float, default=0.02)
    ap.add_argument("--samples", type=int, default=450000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--scene", default="room0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshdist_room0_timing.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("meshdist_timing needs a GPU")
    from myslam_amd import _hip, harness, ops
    from myslam_amd.src.tools import eval_recon as er
    dev = torch.device("cuda:0")
    wl = harness.make_workload(args.scene, 64, 24, 8, device=dev, planes="synth")
    with torch.no_grad():
        verts, faces, level = room_mesh(wl, args.resolution)
    shift = torch.full((3,), 0.01 / 3 ** 0.5, device=dev)
    moved = (verts + shift).contiguous()
    samples = ops.sample_surface(verts, faces, args.samples, 0)[0].float().contiguous()
    moved_samples = (samples + shift).contiguous()
    md = ops.MeshDistance(verts, faces)
    lib = _hip.lib()

    def build():
        _hip.check(lib.eslam_tri_build(_hip.ptr(md.verts), md.verts.shape[0], _hip.ptr(md.faces), md.faces.shape[0],
                                       ctypes.byref(md.grid), _hip.ptr(md.ws), _hip.stream_handle(dev)), "eslam_tri_build")

    out = {"scene": args.scene, "resolution": args.resolution, "level": level, "vertices": int(verts.shape[0]),
           "faces": int(faces.shape[0]), "dims": list(md.dims), "cell": float(md.grid.cell), "entries": md.entries,
           "entries_per_face": round(md.entries / faces.shape[0], 3), "workspace_mib": round(md.ws.numel() / 2 ** 20, 1),
           "samples": args.samples, "rounds": args.rounds, "inner": args.inner, "device": torch.cuda.get_device_name(0)}
    out["build_ms"] = timed(build, args.rounds, args.inner)
    out["construct_ms"] = timed(lambda: ops.MeshDistance(verts, faces), args.rounds, args.inner)
    out["query_samples_ms"] = timed(lambda: md.query(moved_samples), args.rounds, args.inner)
    out["query_samples_input_order_ms"] = timed(lambda: md.query(moved_samples, sort=False), args.rounds, args.inner)
    out["query_vertices_ms"] = timed(lambda: md.query(moved), args.rounds, args.inner)
    out["nn_build_query_ms"] = timed(lambda: ops.NNGrid(samples).query(moved_samples), args.rounds, args.inner)
    d_exact = md.query(moved_samples)[0]
    d_nn = ops.NNGrid(samples).query(moved_samples)[0]
    out["moved_samples_mean_dist_cm"] = {"exact": float(d_exact.double().mean()) * 100, "to_samples": float(d_nn.double().mean()) * 100}
    # the bias: the mesh against itself displaced by 1 cm, exact and sampled
    kw = dict(align=False, num_points=args.samples)
    ex = er.recon_report(moved, faces, verts, faces, exact=True, **kw)
    sa = er.recon_report(moved, faces, verts, faces, exact=False, **kw)
    out["displaced_1cm"] = {"exact": {k: ex[k] for k in ("accuracy", "completion", "f_score", "normal_consistency")},
                            "sampled": {k: sa[k] for k in ("accuracy", "completion", "f_score", "normal_consistency")},
                            "accuracy_bias_cm": sa["accuracy"] - ex["accuracy"]}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
