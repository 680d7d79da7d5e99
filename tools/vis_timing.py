"""Times of the render metrics and the visualiser's panel at 680 x 1200 (Replica's frame size) on one GPU, each against the
same quantity formed from torch operations on the same GPU (the only thing there is to compare with):
    frame_stats   vs  masked abs-sum, squared-error sum, count and max in torch (float64 accumulation)
    ssim          vs  two separable F.conv2d passes over the five moment images and the formula in torch
    vis_panel     vs  the panel assembled with torch indexing, clamps and casts
    save_imgs     a whole Frame_Visualizer.save_imgs on the room0 scene (render_img of 816 000 rays, stats, panel, SSIM,
                  download, JPEG encode and write), with its parts
    python tools/vis_timing.py [out.json]
Device times are HIP events around REPS back-to-back calls after WARM warm-up calls, median of 5 such batches; save_imgs is
a host clock around calls that end synchronised.  No time here is a pass criterion."""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myslam_amd import ops, scene as scn, slam            # noqa: E402
from myslam_amd.src.utils.Frame_Visualizer import Frame_Visualizer    # noqa: E402

DEV = torch.device("cuda:0")
H, W = 680, 1200
WARM, REPS, BATCHES = 5, 20, 5


def device_ms(fn):
    for _ in range(WARM):
        fn()
    out = []
    for _ in range(BATCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / REPS)
    return round(float(np.median(out)), 4)


def torch_stats(d, c, gd, gc):
    valid = gd > 0
    return torch.stack([valid.sum().double(), ((d - gd).abs() * valid).double().sum(), ((c - gc).double() ** 2).sum(),
                        gd.max().double()])


def torch_ssim(a, b, win):
    x, y = a.clamp(0, 1).permute(2, 0, 1)[None], b.clamp(0, 1).permute(2, 0, 1)[None]
    C = x.shape[1]
    kh, kv = win.view(1, 1, 1, -1).repeat(C, 1, 1, 1), win.view(1, 1, -1, 1).repeat(C, 1, 1, 1)
    blur = lambda v: F.conv2d(F.conv2d(v, kh, groups=C), kv, groups=C)
    ux, uy = blur(x), blur(y)
    vx, vy, vxy = blur(x * x) - ux * ux, blur(y * y) - uy * uy, blur(x * y) - ux * uy
    s = ((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4)) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))
    return s.double().mean()


def torch_panel(d, c, gd, gc, lut):
    vmax = gd.max()
    vmax = torch.where(vmax == 0, torch.ones_like(vmax), vmax)
    hole = gd == 0
    dres = torch.where(hole, torch.zeros_like(gd), (gd - d).abs())
    cres = torch.where(hole[..., None], torch.zeros_like(gc), (gc - c).abs())

    def plasma(v):
        t = v / vmax
        idx = torch.where(t > 0, (t.clamp(max=1) * 256).long().clamp(max=255), torch.zeros_like(t, dtype=torch.long))
        return lut[idx]
    top = torch.cat([plasma(gd), plasma(d), plasma(dres)], 1)
    bot = torch.cat([(v.clamp(0, 1) * 255 + 0.5).to(torch.uint8) for v in (gc, c, cres)], 1)
    return torch.cat([top, bot], 0)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    g = torch.Generator(device=DEV).manual_seed(0)
    gd = torch.rand(H, W, device=DEV, generator=g) * 4 + 0.5
    gd[torch.rand(H, W, device=DEV, generator=g) < 0.1] = 0
    d = gd + 0.1 * torch.randn(H, W, device=DEV, generator=g)
    gc = torch.rand(H, W, 3, device=DEV, generator=g)
    c = gc + 0.1 * torch.randn(H, W, 3, device=DEV, generator=g)
    lut = ops.plasma_lut(DEV)
    from tests import vis_ref as vr
    win = torch.from_numpy(vr.window()).to(DEV)
    stats = ops.frame_stats(d, c, gd, gc)
    res = dict(device=torch.cuda.get_device_name(0), H=H, W=W, warmup=WARM, reps=REPS, batches=BATCHES, unit="ms per call (median)")
    # the two forms compute the same thing (so the comparison is of like with like)
    assert torch.allclose(torch_stats(d, c, gd, gc), stats, rtol=1e-5)
    assert abs(float(torch_ssim(c, gc, win)) - float(ops.ssim(c, gc))) < 1e-3
    differ = (torch_panel(d, c, gd, gc, lut) != ops.vis_panel(d, c, gd, gc, stats=stats)).float().mean()
    assert float(differ) < 1e-3, float(differ)           # (torch may fuse c * 255 + 0.5; the kernel does not)
    res["frame_stats"] = dict(hip=device_ms(lambda: ops.frame_stats(d, c, gd, gc)), torch=device_ms(lambda: torch_stats(d, c, gd, gc)))
    res["ssim"] = dict(hip=device_ms(lambda: ops.ssim(c, gc)), torch=device_ms(lambda: torch_ssim(c, gc, win)))
    res["vis_panel"] = dict(hip=device_ms(lambda: ops.vis_panel(d, c, gd, gc, stats=stats)),
                            torch=device_ms(lambda: torch_panel(d, c, gd, gc, lut)))
    print(json.dumps(res), flush=True)

    # a whole save_imgs on the room0 scene (untrained planes: the render's cost does not depend on their values)
    sc = scn.make_scene("room0")
    assert (sc.H, sc.W) == (H, W)
    torch.manual_seed(0)
    s = slam.Slam(sc, slam.SlamConfig(), device=DEV, seed=0)
    pose = scn.center_pose(sc).to(DEV)
    root = tempfile.mkdtemp(prefix="vis_timing_")
    try:
        vis = Frame_Visualizer(1, 1, root, s.be.renderer, sc.truncation, False, device=DEV)

        def host_ms(fn, n=5):
            fn()
            out = []
            for _ in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            return round(float(np.median(out)), 3)
        whole = host_ms(lambda: vis.save_imgs(0, 0, gd, gc, pose, s.all_planes, s.decoders))
        render = host_ms(lambda: s.be.renderer.render_img(s.all_planes, s.decoders, pose, sc.truncation, DEV, gt_depth=gd))
        dd, cc = s.be.renderer.render_img(s.all_planes, s.decoders, pose, sc.truncation, DEV, gt_depth=gd)
        device_part = host_ms(lambda: (ops.vis_panel(dd, cc, gd, gc), ops.frame_metrics(dd, cc, gd, gc)))
        panel = ops.vis_panel(dd, cc, gd, gc)
        download = host_ms(lambda: panel.cpu().numpy())
        res["save_imgs"] = dict(whole_ms=whole, render_img_ms=render, stats_panel_metrics_ms=device_part, download_ms=download,
                                titles_encode_write_ms=round(whole - render - device_part - download, 3))
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
