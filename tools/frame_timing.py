"""Per-frame delivery time, file to tensors on the device ready for Slam.track, of the three frame paths (DESIGN.md
section 18):
    (a) the host reader:  reader[k], colour cast to float32, both uploaded         (FrameStream(native=False))
    (b) FrameStream(native=True, prefetch=0): decode, pinned staging, upload, ops.prepare_frame, inline
    (c) FrameStream(native=True, prefetch=2) consumed by the real loop: what the loop waits for a frame
on 680 x 1200 Replica-layout frames (nothing to resample) and 480 x 640 TUM-layout frames (undistortion, crop_size
[384, 512], crop_edge 8), 50 frames after 5 warm-up frames, plus the decode time alone (PIL's, on the host in every
path) and the loop's frames/s fed by (a) and by (c) with the Replica iteration counts of tools/slam_run.py.
    python tools/frame_timing.py [out.json] [eager|graph]
Times are host clocks around work that ends in a device synchronise.  The Replica frames are the analytic room's, so
the loop tracks them; the TUM frames are smooth noise (delivery only: (c) there is paced by the measured Replica loop).
"""
import json
import os
import shutil
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myslam_amd import scene as scn, slam, synthscene            # noqa: E402
from myslam_amd.src.utils import datasets as ds                  # noqa: E402

WARM, TIMED = 5, 50
N = WARM + TIMED
DEV = torch.device("cuda:0")


def write_replica(root, sc):
    from PIL import Image
    os.makedirs(os.path.join(root, "results"))
    frames = synthscene.make_sequence(sc, N, device=DEV, variant="rich")
    with open(os.path.join(root, "traj.txt"), "w") as f:
        for k, color, depth, c2w in frames:
            Image.fromarray((color.cpu().numpy() * 255).round().astype(np.uint8)).save(
                os.path.join(root, "results", f"frame{k:06d}.jpg"), quality=95)
            Image.fromarray((depth.cpu().numpy() * 6553.5).round().astype(np.uint16)).save(
                os.path.join(root, "results", f"depth{k:06d}.png"))
            m = c2w.cpu().double().numpy().copy()
            m[:3, 1:3] *= -1
            f.write(" ".join(f"{x:.9e}" for x in m.reshape(-1)) + "\n")
    return dict(dataset="replica", data=dict(input_folder=root),
                cam=dict(H=sc.H, W=sc.W, fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy, png_depth_scale=6553.5, crop_edge=0))


def write_tum(root):
    from PIL import Image
    rng = np.random.default_rng(0)
    H, W = 480, 640
    os.makedirs(os.path.join(root, "rgb"))
    os.makedirs(os.path.join(root, "depth"))
    rows = {"rgb": [], "depth": [], "groundtruth": ["# timestamp tx ty tz qx qy qz qw"]}
    for k in range(N):
        t = 100.0 + 0.1 * k
        small = rng.integers(0, 256, (H // 8, W // 8, 3)).astype(np.uint8)
        Image.fromarray(small).resize((W, H), Image.BICUBIC).save(os.path.join(root, "rgb", f"{t:.6f}.png"))
        d = (5000 + 8 * np.arange(W)[None] + 6 * np.arange(H)[:, None] + rng.integers(0, 40, (H, W))).astype(np.uint16)
        Image.fromarray(d).save(os.path.join(root, "depth", f"{t:.6f}.png"))
        rows["rgb"].append(f"{t:.6f} rgb/{t:.6f}.png")
        rows["depth"].append(f"{t:.6f} depth/{t:.6f}.png")
        rows["groundtruth"].append(f"{t:.6f} {0.01 * k:.6f} 0 0 0 0 0 1")
    for name, r in rows.items():
        with open(os.path.join(root, name + ".txt"), "w") as f:
            f.write("\n".join(r) + "\n")
    return dict(dataset="tumrgbd", data=dict(input_folder=root),
                cam=dict(H=H, W=W, fx=517.3, fy=516.5, cx=318.6, cy=255.3, png_depth_scale=5000.0, crop_edge=8,
                         crop_size=[384, 512], distortion=[0.2624, -0.9531, -0.0054, 0.0026, 1.1633]))


def stats(ms):
    a = np.asarray(ms[WARM:], dtype=np.float64)
    return dict(mean_ms=round(float(a.mean()), 3), median_ms=round(float(np.median(a)), 3),
                p90_ms=round(float(np.percentile(a, 90)), 3), n=int(a.size))


def time_delivery(stream):
    """ms per frame of next(stream) followed by a device synchronise."""
    out = []
    it = iter(stream)
    for _ in range(N):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        item = next(it)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        del item
    list(it)
    return stats(out)


def time_decode(reader):
    out = []
    for k in range(N):
        t0 = time.perf_counter()
        ds._imread_color(reader.color_paths[k])
        ds._imread_depth(reader.depth_paths[k])
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


class Timed:
    """Wraps a frame iterable: the host time each next() takes (what the loop waits for a frame)."""

    def __init__(self, frames, pace_s=0.0):
        self.frames, self.waits, self.pace_s = frames, [], pace_s

    def __iter__(self):
        it = iter(self.frames)
        while True:
            t0 = time.perf_counter()
            try:
                item = next(it)
            except StopIteration:
                return
            self.waits.append((time.perf_counter() - t0) * 1e3)
            yield item
            if self.pace_s:
                time.sleep(self.pace_s)                  # a stand-in loop: the consumer is busy this long per frame


def run_loop(sc, frames, mode):
    """The tracking + mapping loop over `frames` (Replica counts; 100 first-frame iterations): frames/s after frame 0."""
    cfg = slam.SlamConfig(iters_first=100)
    torch.manual_seed(0)
    if mode == "graph":
        from myslam_amd.slam_graph import GraphedSlam
        s = GraphedSlam(sc, cfg, device=DEV, seed=0)
    else:
        s = slam.Slam(sc, cfg, device=DEV, seed=0)
    marks = []

    def on_frame(s_, i):
        torch.cuda.synchronize()
        marks.append(time.perf_counter())

    timed = Timed(frames)
    s.run(timed, on_frame=on_frame)
    # frames WARM .. N-1, graph builds (which fall on early frames) left out by starting after the warm-up frames
    span = marks[-1] - marks[WARM - 1]
    return dict(frames_per_s=round((N - WARM) / span, 2), ms_per_frame=round(span / (N - WARM) * 1e3, 3),
                wait_for_frame=stats(timed.waits), capture_seconds=round(s.stats.get("capture_seconds", 0.0), 2))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    mode = sys.argv[2] if len(sys.argv) > 2 else "eager"
    root = tempfile.mkdtemp(prefix="frame_timing_")
    res = dict(device=torch.cuda.get_device_name(0), warmup_frames=WARM, timed_frames=TIMED, loop_mode=mode)
    try:
        sc = scn.make_scene("room0")
        args = SimpleNamespace(input_folder=None)
        layouts = {"replica_680x1200": write_replica(os.path.join(root, "replica"), sc), "tum_480x640": write_tum(os.path.join(root, "tum"))}
        for name, cfg in layouts.items():
            reader = ds.get_dataset(cfg, args, 1.0, device=DEV)
            r = res[name] = {}
            r["decode_only"] = time_decode(reader)
            # alternate the paths, twice, so that drift of the shared host shows as spread between repeats
            for rep in range(2):
                r[f"a_host_reader_rep{rep}"] = time_delivery(ds.FrameStream(reader, DEV, native=False))
                r[f"b_native_prefetch0_rep{rep}"] = time_delivery(ds.FrameStream(reader, DEV, prefetch=0))
            print(name, json.dumps(r), flush=True)
        reader = ds.get_dataset(layouts["replica_680x1200"], args, 1.0, device=DEV)
        loops = res["loop_replica"] = {}
        for rep in range(2):
            loops[f"a_host_reader_rep{rep}"] = run_loop(sc, ds.FrameStream(reader, DEV, native=False), mode)
            loops[f"c_native_prefetch2_rep{rep}"] = run_loop(sc, ds.FrameStream(reader, DEV, prefetch=2), mode)
            print("loop", rep, json.dumps({k: v for k, v in loops.items() if k.endswith(str(rep))}), flush=True)
        # TUM frames at the pace of that loop: what a consumer busy for one Replica loop frame waits for the next frame
        pace = loops["c_native_prefetch2_rep1"]["ms_per_frame"] / 1e3
        reader = ds.get_dataset(layouts["tum_480x640"], args, 1.0, device=DEV)
        timed = Timed(ds.FrameStream(reader, DEV, prefetch=2), pace_s=pace)
        for item in timed:
            torch.cuda.synchronize()
        res["tum_480x640"]["c_native_prefetch2_paced"] = dict(wait_for_frame=stats(timed.waits), pace_ms=round(pace * 1e3, 3))
        print("tum paced", json.dumps(res["tum_480x640"]["c_native_prefetch2_paced"]), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
