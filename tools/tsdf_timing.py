"""Per-stage device time of TSDF fusion on room0's marching-cubes bound (configs/Replica/room0.yaml:4) with synthetic
keyframes of room0's camera (1200 x 680): integrate per chunk, the masked marching cubes (count + scan, emit), and the
hull of Mesher.get_bound_from_frames_tsdf end to end beside the default get_bound_from_frames.

    python tools/tsdf_timing.py [--voxel 0.02] [--frames 32] [--chunk 32] [--colour] [--out DIR]

Keyframes: `--frames` frames of the synthetic sequence (synthscene.make_sequence, every 4th of 4 x frames), est_c2w = the
ground-truth pose.  For integrate the JSON also gives the share of the volume's runs that the call touched and the time
that reading and writing the whole volume once at `--hbm-gbs` GB/s would take, as a fraction of the measured time
(bytes: 8 per voxel, 20 with colour).  Prints one JSON line (and writes DIR/tsdf_timing_<voxel>.json when --out is given).
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--colour", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM rate for the bytes-once figure (MI355X: 8 TB/s peak)")
    ap.add_argument("--no-hull", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from myslam_amd import ops, scene as scn, synthscene
    from myslam_amd.src.utils import Mesher as M
    dev = torch.device("cuda:0")
    sc = scn.make_scene("room0")
    bound = torch.tensor(scn._SCENES["room0"]["bound"], dtype=torch.float64)
    frames = synthscene.make_sequence(sc, 4 * args.frames, device=dev)[::4]
    K = (sc.fx, sc.fy, sc.cx, sc.cy)
    trunc = 0.04

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

    res = {"scene": "room0", "voxel": args.voxel, "trunc": trunc, "keyframes": len(frames), "chunk": args.chunk,
           "image": [sc.W, sc.H], "colour": bool(args.colour)}
    vol = ops.TSDFVolume(bound, args.voxel, trunc, color=args.colour, device=dev)
    res["dims"] = list(vol.dims)
    n = vol.dims[0] * vol.dims[1] * vol.dims[2]
    res["voxels"] = n
    res["volume_bytes"] = 4 * n * (5 if args.colour else 2)
    # integrate: the kernel alone, one chunk per call, inputs staged beforehand (TSDFVolume.integrate also stacks the frames)
    chunk = frames[:args.chunk]
    d = torch.stack([f[2] for f in chunk]).contiguous()
    col = torch.stack([f[1] for f in chunk]).contiguous() if args.colour else None
    w2c = ops._w2c_rows(torch.stack([f[3] for f in chunk]), dev, flip_yz=True)
    dmax = d.reshape(len(chunk), -1).amax(dim=1).contiguous()
    import ctypes
    from myslam_amd import _hip
    o3 = (ctypes.c_float * 3)(*vol.origin)

    def integrate_chunk():
        with _hip.on_device(dev):
            _hip.check(_hip.lib().eslam_tsdf_integrate(_hip.ptr(vol.tsdf), _hip.ptr(vol.weight), _hip.ptr(vol.color), *vol.dims, o3,
                                                       vol.voxel, vol.trunc, _hip.ptr(d), _hip.ptr(col), _hip.ptr(w2c),
                                                       _hip.ptr(dmax), len(chunk), sc.H, sc.W, *[float(k) for k in K],
                                                       _hip.stream_handle(dev)), "eslam_tsdf_integrate")

    _, res["integrate_chunk_ms"] = stage(integrate_chunk, reps=args.reps)
    once_ms = 2 * res["volume_bytes"] / (args.hbm_gbs * 1e9) * 1e3
    res["volume_bytes_once_ms"] = once_ms
    res["bytes_once_fraction"] = once_ms / res["integrate_chunk_ms"]
    print("integrate", res["integrate_chunk_ms"], flush=True)
    # the public call, from the frame tuples (stacking, pose inversion, depth maxima and the kernel), on a fresh volume
    for t in (vol.tsdf, vol.weight) + ((vol.color,) if args.colour else ()):
        t.zero_()
    _, res["integrate_public_ms"] = stage(lambda: vol.integrate(frames, K, chunk=args.chunk))
    for t in (vol.tsdf, vol.weight) + ((vol.color,) if args.colour else ()):
        t.zero_()
    vol.integrate(frames, K, chunk=args.chunk)
    res["observed_share"] = float((vol.weight > 0).float().mean())
    (ws, counts), res["mc_count_masked_ms"] = stage(lambda: ops.mc_count_masked(vol.tsdf, vol.weight, 0.0), reps=args.reps)
    V, F = (int(v) for v in counts.tolist())
    res["V"], res["F"] = V, F
    print("count", res["mc_count_masked_ms"], V, F, flush=True)
    origin = tuple(o + 0.5 * vol.voxel for o in vol.origin)
    _, res["mc_emit_ms"] = stage(lambda: ops.mc_emit(vol.tsdf, 0.0, origin, (vol.voxel,) * 3, ws, V, F), reps=args.reps)
    _, res["mc_count_unmasked_ms"] = stage(lambda: ops.mc_count(vol.tsdf, 0.0), reps=args.reps)
    del ws
    if args.colour:
        verts = vol.extract_mesh()[0]
        _, res["sample_colour_ms"] = stage(lambda: vol.sample_color(verts), reps=args.reps)
    del vol
    if not args.no_hull:
        kfs = [{"est_c2w": c2w, "depth": depth, "color": color, "idx": idx} for idx, color, depth, c2w in frames]
        m = SimpleNamespace(H=sc.H, W=sc.W, fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy, scale=1.0, mesh_bound_scale=1.02,
                            bound=sc.bound, marching_cubes_bound=bound)
        _, res["hull_tsdf_ms"] = stage(lambda: M.get_bound_from_frames_tsdf(m, kfs, voxel=args.voxel))
        _, res["hull_default_ms"] = stage(lambda: M.get_bound_from_frames(m, kfs))
        print("hull", res["hull_tsdf_ms"], res["hull_default_ms"], flush=True)
    res["device"] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"tsdf_timing_{args.voxel:g}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
