"""Device time of the mesh clean-up (ops.weld_vertices, ops.mesh_components, ops.component_face_counts and the whole
clean_mesh.clean_mesh_arrays) next to its host baselines: np.unique(axis=0) for the merge, and scipy's
csgraph.connected_components for the components when scipy is importable.

    python tools/meshclean_timing.py [--res 0.01] [--out profiles] [--no-baselines]

Meshes: "room" = marching cubes of the analytic room's SDF of room0 at 1 cm (the "gt" mesh of tools/recon_timing.py:
V = 2.88 M, F = 5.77 M, welded), and "soup" = the same faces with one vertex per corner (V = 3 F), the corners in shuffled
order.  Kernel times are device events around the op (its aminmax check of the faces included), the median of --reps calls
after a warm-up; clean_mesh_arrays is wall time, host copies included.  Prints one JSON line and writes it to
<out>/meshclean_timing.json.
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


def device_ms(fn, reps):
    out = fn()                                            # warm-up (allocations, first launches)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return out, float(np.median(ts))


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-baselines", action="store_true")
    args = ap.parse_args()
    from myslam_amd import ops, scene as scn, synthscene
    from myslam_amd.src.tools import clean_mesh as cm
    from recon_timing import room_sdf_mesh
    dev = torch.device("cuda:0")
    sc = scn.make_scene("room0")
    v, f = room_sdf_mesh(synthscene.AnalyticRoom(sc.bound), sc.bound, args.res, dev)
    f = f.long()
    g = torch.Generator(device="cpu").manual_seed(0)
    order = torch.randperm(3 * f.shape[0], generator=g).to(dev)
    sv = torch.empty(3 * f.shape[0], 3, device=dev)
    sv[order] = v[f.reshape(-1)]
    meshes = {"room": (v, f), "soup": (sv, order.reshape(-1, 3))}
    res = {"scene": "room0", "resolution": args.res, "reps": args.reps}
    for name, (mv, mf) in meshes.items():
        r = {"V": int(mv.shape[0]), "F": int(mf.shape[0])}
        rep, r["weld_ms"] = device_ms(lambda: ops.weld_vertices(mv), args.reps)
        wf = rep.long()[mf]                               # the faces the components step sees in clean_mesh_arrays
        lab, r["components_ms"] = device_ms(lambda: ops.mesh_components(wf, mv.shape[0]), args.reps)
        cnt, r["counts_ms"] = device_ms(lambda: ops.component_face_counts(wf, lab), args.reps)
        r["positions"] = int((rep == torch.arange(mv.shape[0], device=dev)).sum())
        r["components"] = int((cnt > 0).sum())
        r["largest"] = int(cnt.max())
        hv, hf = mv.cpu().numpy(), mf.cpu().numpy()
        cm.clean_mesh_arrays(hv[:1000], np.zeros((0, 3), np.int64), None)
        out, r["clean_mesh_arrays_wall_ms"] = wall_ms(lambda: cm.clean_mesh_arrays(hv, hf, None, min_faces=100))
        r["clean_V"], r["clean_F"] = int(len(out[0])), int(len(out[1]))
        if not args.no_baselines:
            t = time.perf_counter()
            uniq, inv = np.unique(hv + np.float32(0.0), axis=0, return_inverse=True)
            r["host_np_unique_ms"] = (time.perf_counter() - t) * 1e3
            assert len(uniq) == r["positions"], (len(uniq), r["positions"])
            try:
                from scipy.sparse import coo_matrix
                from scipy.sparse.csgraph import connected_components
                wfh = wf.cpu().numpy()
                t = time.perf_counter()
                e = np.concatenate([wfh[:, [0, 1]], wfh[:, [1, 2]]])
                graph = coo_matrix((np.ones(len(e), dtype=np.int8), (e[:, 0], e[:, 1])), shape=(len(hv), len(hv)))
                n_comp, ids = connected_components(graph, directed=False)
                r["host_scipy_components_ms"] = (time.perf_counter() - t) * 1e3
                used = np.zeros(len(hv), dtype=bool)
                used[wfh.reshape(-1)] = True
                assert len(np.unique(ids[used])) == r["components"], (len(np.unique(ids[used])), r["components"])
            except ImportError:
                r["host_scipy_components_ms"] = None
        res[name] = r
        print(name, r, flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "meshclean_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
