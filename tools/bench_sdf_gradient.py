"""Time the fused SDF gradient against the autograd route and against the SDF alone, on one GPU, in one process:

    python tools/bench_sdf_gradient.py [--n 1000000] [--rounds 20] [--inner 40] [--resolution 0.08] [--warmup 3] [--scene room0]

Points: the vertices of the synthetic scene's level set (ops.sdf_grid + ops.marching_cubes on harness's synth planes and
seeded decoders, at the field's median so that a surface exists: what Mesher.extract_mesh evaluates, without the frame
hull), tiled to N - a mesh-like set, neighbouring points on neighbouring texels.  Three figures, the rounds interleaved
(a, b, c, a, b, c, ...) so that drift hits all alike, each a device-event time around `inner` back-to-back calls divided by `inner` (40 calls: a
window of 10 ms for the fastest of the three), median over the rounds:

    a  ops.sdf_gradient                     one launch of eslam_sdf_grad
    b  Decoders.forward + backward of raw[:, 3].sum() with frozen planes and decoders (p.requires_grad only)
    c  ops.decode_sdf_only                  the floor: one gather of the six geometry planes, no gradient

Prints one JSON line.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def level_set_points(wl, n, resolution):
    from myslam_amd import ops
    from myslam_amd.src.utils.Mesher import grid_axes
    dev = wl.device
    x, y, z = grid_axes(wl.scene.bound.double(), resolution)
    axes = [torch.from_numpy(a).float().to(dev) for a in (x, y, z)]
    vol = ops.sdf_grid(wl.planes, wl.decoders, axes, wl.scene.bound)
    inside = vol[vol > -1.0]
    level = float(inside.median())
    verts, faces = ops.marching_cubes(vol, level, (x[0], y[0], z[0]), (x[2] - x[1], y[2] - y[1], z[2] - z[1]))
    if verts.shape[0] == 0:
        raise RuntimeError("the synthetic field has no level set at its median")
    idx = torch.arange(n, device=dev) % verts.shape[0]
    return verts[idx].contiguous(), int(verts.shape[0]), level


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scene", default="room0")
    ap.add_argument("--resolution", type=float, default=0.08)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_sdf_gradient needs a GPU")
    from myslam_amd import harness, ops
    dev = torch.device("cuda:0")
    wl = harness.make_workload(args.scene, 64, 24, 8, device=dev, planes="synth")
    for grp in wl.planes:
        for p in grp:
            p.requires_grad_(False)
    for t in wl.decoders.parameters():
        t.requires_grad_(False)
    with torch.no_grad():
        pts, n_verts, level = level_set_points(wl, args.n, args.resolution)
    bound6 = ops.bound_to_host(wl.scene.bound)
    dec, planes = wl.decoders, wl.planes

    def fused():
        return ops.sdf_gradient(pts, bound6, planes, dec)

    def autograd():
        p = pts.detach().requires_grad_(True)
        raw = dec(p, all_planes=planes)
        raw[:, 3].sum().backward()
        return raw, p.grad

    def sdf_only():
        return ops.decode_sdf_only(pts, bound6, planes, dec)

    calls = (("sdf_grad_us", fused), ("autograd_us", autograd), ("sdf_only_us", sdf_only))
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    torch.cuda.synchronize()
    # the two routes agree on what they compute, at the size that is timed
    sdf, grad = fused()
    raw, g = autograd()
    err = float((grad - g).abs().max() / g.abs().max())
    times = {k: [] for k, _ in calls}
    for _ in range(args.rounds):
        for k, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / args.inner)
    out = {"n_points": int(pts.shape[0]), "mesh_vertices": n_verts, "level": level, "rounds": args.rounds, "inner": args.inner,
           "max_rel_diff_fused_vs_autograd": err, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        v = sorted(v)
        out[k] = round(v[len(v) // 2], 1)
        out[k + "_min_max"] = [round(v[0], 1), round(v[-1], 1)]
    out["fused_faster_than_autograd"] = out["sdf_grad_us"] < out["autograd_us"]
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
