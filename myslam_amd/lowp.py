"""Mixed precision (BASELINE.json configs[4]: fp16 planes + bf16 MFMA decoders), forward AND backward.

The planes stay float32 masters (the optimiser's copy, exactly as in the reference); HalfPlanes holds their channels-last
float16 copies and refreshes all 12 in one launch (eslam_planes_to_half) after an optimiser step.  Under
`ops.mixed_precision(half)` the renderer's kernels gather texels from the copies (float32 accumulation), run both decoders on
bf16 MFMA with float32 accumulation - in the backward pass too - and accumulate plane gradients in float32 for the masters.
Sampling (z_vals), the loss, the composite and its backward, the scatter and the optimiser are the float32 path.

Pose gradients: under `ops.mixed_precision(half, ray_grads=True)` rays that require grad get g_rays_o / g_rays_d from the half
copies too (coord_bwd_lowp_kernel: the bilinear derivative acts on the fp16-rounded texels the forward pass interpolated),
with the separate losses and with render_batch_ray_with_loss - so the path can track and run the joint mapping iteration
(slam.SlamConfig.mixed_precision).  Without ray_grads such rays raise, as they always did.

Free points: under `ops.mixed_precision(half, points=True)` ops.DecodeFn (Decoders.forward, get_raw_sdf, get_raw_rgb),
ops.decode_sdf_only, Mesher.eval_points and ops.sdf_grid - hence Mesher.extract_mesh / get_mesh - run on the copies too, with
gradients for points, planes and decoders (eslam_decode_bwd; saved features bf16), so the mesh is that of the field that was
trained and rendered.  Without `points` those calls stay on the float32 masters, bit for bit as outside the context.  The
depth-less rays' importance sampler stays on the masters either way: sampling is the float32 path.

The copies are the IEEE round-to-nearest-even conversion of the masters, half subnormals included; a master beyond the half
range (|x| >= 65520) becomes +-inf in its copy and stays inf - nothing clamps it.  A copy is as old as its last refresh: an
optimiser step changes the masters only.
"""
import ctypes

import torch

from . import _hip, ops


class HalfPlanes:
    def __init__(self, all_planes):
        for grp in all_planes:
            for p in grp:
                if not (p.is_cuda and p.dtype == torch.float32 and p.dim() == 4 and
                        p.is_contiguous(memory_format=torch.channels_last)):
                    raise RuntimeError("mixed precision needs float32 channels_last planes on the GPU")
        self.planes = tuple([torch.empty_like(p.detach(), dtype=torch.float16) for p in grp] for grp in all_planes)
        self.flat = [p for grp in self.planes for p in grp]
        self.refresh(all_planes)

    def refresh(self, all_planes):
        """float32 masters -> float16 copies, all 12 planes in one launch."""
        arr, _ = _hip.make_planes(tuple([p.detach() for p in grp] for grp in all_planes), half=self.flat)
        dev = self.flat[0].device
        with _hip.on_device(dev):
            _hip.check(_hip.lib().eslam_planes_to_half(arr, _hip.stream_handle(dev)), "eslam_planes_to_half")
        return self


def half_planes(all_planes):
    """float16, channels-last copies of the 12 planes (one texel = 64 contiguous bytes), as a HalfPlanes."""
    return HalfPlanes(all_planes)


def render_batch_ray_lowp(renderer, all_planes, planes_f16, decoders, rays_d, rays_o, truncation, gt_depth, _rand=None):
    """Renderer.render_batch_ray (reference src/utils/Renderer.py:63-147) on the mixed-precision kernels, no autograd:
    returns depth [R], rgb [R,3], sdf [R,S], z_vals [R,S]."""
    with torch.no_grad(), ops.mixed_precision(planes_f16):
        return renderer.render_batch_ray(all_planes, decoders, rays_d, rays_o, rays_o.device, truncation, gt_depth=gt_depth,
                                         _rand=_rand)
