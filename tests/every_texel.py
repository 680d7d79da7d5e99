"""Batches without ReLU-ambiguous samples: filter the rays, not the texels.

hp.plane_grads_close sets aside every texel a ReLU-ambiguous sample touches (hp.ambiguous_samples: two correct float32
evaluations may gate such a sample differently).  The set-aside is per texel: on the coarse planes, where a texel collects
hundreds of samples, a few dozen ambiguous samples remove half to nine tenths of the touched texels from the comparison, and on
2 x 2 planes one such sample removes all of them (test section; tests/test_every_texel_ref.py pins the figures).

The samplers are per-ray functions of (ray, its row of the injected uniform numbers) - tests/test_gpu_sampler_packed.py holds
that bit for bit.  So a test samples a POOL of rays, drops the rays that own an ambiguous sample and renders the first R of the
rest with their own rows: the z_vals are the same bits, no sample is ambiguous, plane_grads_close(max_excluded=0.0) compares
every touched texel and the decoder gradients get no slack.  Test-only; CPU code (the GPU tests hand it CPU tensors).

Plane shape sets the C ABI accepts and scene.plane_shapes never produces (`with_shapes`): see SHAPE_SETS.
"""
import dataclasses
from types import SimpleNamespace

import torch

from tests import helpers as hp
from tests import hostile_rays as hr

excluded_share = hp.excluded_share

# (h, w) coarse then fine, for xy / xz / yz, SDF planes then colour planes; PAIRS: planes of both decoders that agree in shape
SHAPE_SETS = {
    "one_cell": [[(2, 2), (2, 2)]] * 6,
    "slivers": [[(2, 37), (3, 3)], [(41, 2), (2, 2)], [(3, 5), (129, 2)],
                [(2, 37), (3, 3)], [(2, 41), (5, 2)], [(7, 3), (2, 129)]],
    "levels_swapped": [[(52, 68), (13, 17)], [(44, 68), (11, 17)], [(44, 52), (11, 13)],
                       [(13, 17), (13, 17)], [(11, 17), (23, 35)], [(11, 13), (44, 52)]],
}
PAIRS = {"one_cell": 6, "slivers": 2, "levels_swapped": 1}


def pair_count(plane_shapes):
    """Entries of the paired scatter's work list that are pairs: (orientation, level) slots whose two decoders' planes agree."""
    flat = [tuple(s) for grp in plane_shapes for s in grp]
    return sum(flat[p] == flat[p + 6] for p in range(6))


def with_shapes(scene, name, c_dim=32):
    """`scene` with the plane shapes of SHAPE_SETS[name] (same bound, camera and sample counts)."""
    shapes = [[(1, c_dim, h, w) for h, w in grp] for grp in SHAPE_SETS[name]]
    assert pair_count(shapes) == PAIRS[name], (name, shapes)
    return dataclasses.replace(scene, plane_shapes=shapes)


def harness_rays(scene, R, zero_frac=0.0, seed=0):
    """The rays of harness.Workload(scene, R, ...) in the oracle's float32 arithmetic on the CPU: R pixels of the synthetic
    image from the centre pose, then the callers' AABB pre-filter (reference src/Mapper.py:322-332).  rays_o, rays_d, gt_depth,
    gt_color of the rays that pass, in order."""
    from myslam_amd import scene as scn, synth
    from oracle import eslam_oracle as orc
    depth = torch.from_numpy(synth.depth_image(scene.H, scene.W, 10 + seed, zero_frac))[None]
    color = torch.from_numpy(synth.color_image(scene.H, scene.W, 12 + seed))[None]
    idx = torch.from_numpy(synth.hash_randint(scene.H * scene.W, (R,), 50_000 + seed))
    ro, rd, gd, gc = orc.rays_from_pixels(idx, 0, scene.H, 0, scene.W, scene.fx, scene.fy, scene.cx, scene.cy,
                                          scn.center_pose(scene)[None], depth, color)
    keep = orc.aabb_exit(ro, rd, scene.bound) >= gd
    return SimpleNamespace(rays_o=ro[keep].contiguous(), rays_d=rd[keep].contiguous(), gt_depth=gd[keep].contiguous(),
                           gt_color=gc[keep].contiguous())


def take(b, idx):
    """The rays `idx` of a batch (any namespace with rays_o, rays_d, gt_depth and, optionally, gt_color)."""
    out = SimpleNamespace(rays_o=b.rays_o[idx], rays_d=b.rays_d[idx], gt_depth=b.gt_depth[idx])
    if getattr(b, "gt_color", None) is not None:
        out.gt_color = b.gt_color[idx]
    return out


def unambiguous_rays(mdl, scene, batch, z, R):
    """int64 [R]: the first R rays of the pool `batch` none of whose samples at z [P,S] is ambiguous (hr.ambiguous, at its
    default eps).  The pool must hold at least R of them."""
    P, S = z.shape
    _, amb = hr.ambiguous(mdl, scene, batch, z)
    good = (~amb.view(P, S).any(1)).nonzero().squeeze(1)
    assert good.numel() >= R, f"{good.numel()} of {P} pool rays are free of ambiguous samples, {R} asked for"
    return good[:R]


def unambiguous_points(mdl, scene, pts, N):
    """int64 [N]: the first N of the free points pts [P,3] (world coordinates, any of them outside the bound) that are not
    ambiguous (hp.ambiguous_samples on orc.normalize_points)."""
    from oracle import eslam_oracle as orc
    planes, params, _ = mdl
    cv = lambda t: t.detach().cpu().double()
    pn = orc.normalize_points(cv(pts), scene.bound.double())
    amb = hp.ambiguous_samples(pn, tuple([cv(p).contiguous() for p in grp] for grp in planes), {k: cv(v) for k, v in params.items()})
    good = (~amb).nonzero().squeeze(1)
    assert good.numel() >= N, f"{good.numel()} of {pts.shape[0]} pool points are unambiguous, {N} asked for"
    return good[:N]


def free_points(scene, n, outside=0.1, stream=300):
    """n float32 points uniform in the bound, except every (1 / outside)-th one: up to a quarter of the box's extent beyond its
    faces along two axes, inside along the third (the border clamp of the lookup)."""
    from myslam_amd import synth
    u = torch.from_numpy(synth.hash_uniform((n, 3), stream)).double()
    lo, hi = scene.bound[:, 0].double(), scene.bound[:, 1].double()
    inside = lo + u * (hi - lo)
    beyond = torch.where(u < 0.5, lo - (0.5 - u) * 0.5 * (hi - lo), hi + (u - 0.5) * 0.5 * (hi - lo))
    i = torch.arange(n)
    every = int(round(1.0 / outside))
    out = (i % every == every - 1)[:, None] & (torch.arange(3)[None] != (i // every % 3)[:, None])
    return torch.where(out, beyond, inside).float()
