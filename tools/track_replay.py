"""The replayed tracking iteration (2000 rays x 40 samples, decoders frozen, planes detached, pose gradients only) for a
profiler:  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/track_replay.py [f32 | lowp] [replays]
f32: the float32 kernels; lowp: ops.mixed_precision(half, ray_grads=True) - LOWP forward, LOWP decoder backward without weight
gradients, coord_bwd_lowp_kernel."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myslam_amd import harness, losses, lowp, ops
mode = sys.argv[1] if len(sys.argv) > 1 else 'f32'
n = int(sys.argv[2]) if len(sys.argv) > 2 else 200
dev = torch.device('cuda:0')
wl = harness.make_workload('room0', 2000, 32, 8, device=dev, rays_grad=True)
planes = tuple([p.detach() for p in grp] for grp in wl.planes)
for p in wl.decoders.parameters(): p.requires_grad_(False)
half = lowp.HalfPlanes(wl.planes)
def track():
    wl.rays_o.grad = None; wl.rays_d.grad = None
    d, c, s, z = wl.renderer.render_batch_ray(planes, wl.decoders, wl.rays_d, wl.rays_o, dev, wl.truncation, gt_depth=wl.gt_depth)
    losses.tracking_loss(d, c, s, z, wl.gt_depth, wl.gt_color, wl.truncation).backward()
def track_lp():
    with ops.mixed_precision(half, ray_grads=True):
        track()
g = harness.GraphedStep(track_lp if mode == 'lowp' else track, [wl.rays_o, wl.rays_d])
for _ in range(n): g()
torch.cuda.synchronize()
print(f"{mode}: {n} replays of the tracking iteration {wl.R} x {wl.S}")
