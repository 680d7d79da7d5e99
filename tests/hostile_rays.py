"""Rays the callers' AABB pre-filter removes - and the kernels still see: the graph-captured loop and MappingWindow keep the
filter as a ray_mask (static shapes), render_img has none, and the C entries are public.  A plain torch builder (CPU, no
kernel), the float64 statement of the interval eslam_mark_rays documents, and the acceptance criteria shared by
tests/test_hostile_rays_ref.py (float32 oracle against float64 oracle: a correct float32 implementation CAN meet them on
this batch) and tests/test_gpu_hostile_rays.py (the kernels against both).  Test-only.

Classes (`cls` of make()):
  1  origin outside the bound, pointing away, depth-less: AABB exit < -0.01, far < 0, samples in [far, 0]
  2  origin outside, pointing through the box, depth-less
  3  origin outside, gt_depth > 0: even rays end in front of the box (every sample outside), odd rays cross the face
  4  origin inside, gt_depth beyond the AABB exit (what the pre-filter's t >= gt_depth removes)
  5  0 < gt_depth < 1.5 truncation: the surface samples start at negative z
  6  directions with one and with two zero components, +0.0 and -0.0, with and without depth
  7  origin inside within 0.006 of a face, pointing out, depth-less: 0 < far < 0.02, the uniform samples nearly coincide
  8  NON-FINITE: origin exactly on a face, that axis' direction component zero, depth-less: the exit is 0/0
Directions are unnormalised, |d| in [1, 1.5], as get_rays gives them.
"""
from types import SimpleNamespace

import numpy as np
import torch

from tests import helpers as hp

RTOL = 1e-4
AMBIGUOUS_CAP = 5e-3                  # test_gpu_parity.test_random_configurations_against_oracle
FINITE_CLASSES = (1, 2, 3, 4, 5, 6, 7)
ALL_CLASSES = FINITE_CLASSES + (8,)
SIZES = ((24, 8), (72, 24))           # S = 96: the depth-less transmittance scan takes two 64-lane chunks, S % 64 != 0
STATES = ("initial", "trained")


def make(scene, per_class=12, seed=0, classes=ALL_CLASSES):
    """rays_o [R,3], rays_d [R,3], gt_depth [R], gt_color [R,3] (float32, CPU) and cls [R] (int64), per_class rays of each
    class in `classes`, class by class."""
    g = torch.Generator().manual_seed(1234 + seed)
    lo, hi = scene.bound[:, 0].double(), scene.bound[:, 1].double()
    ctr, ext = (lo + hi) / 2, hi - lo
    tau = float(scene.truncation)
    U = lambda a, b, *shape: a + (b - a) * torch.rand(tuple(shape), generator=g, dtype=torch.float64)

    def inside(frac):                 # a point of the central `frac` of the box
        return ctr + U(-0.5, 0.5, 3) * ext * frac

    def direction(d):                 # |d| in [1, 1.5]
        return d / d.norm() * U(1.0, 1.5)

    def exit_of(o, d):
        t = torch.stack([(lo - o) / d, (hi - o) / d], -1)
        return float(t.max(-1).values.min())

    def beyond(k, side, a, b):        # a point of the box's middle moved past face `side` of axis k by U(a, b)
        o = inside(0.6)
        o[k] = (hi[k] + U(a, b)) if side else (lo[k] - U(a, b))
        return o

    O, D, GD, C = [], [], [], []
    for c in classes:
        for i in range(per_class):
            k, side = i % 3, (i // 3) % 2
            sgn = 1.0 if side else -1.0
            gd = 0.0
            if c == 1:
                o = beyond(k, side, 0.3, 1.0)
                d = U(-0.5, 0.5, 3)
                d[k] = sgn * U(0.5, 1.0)
                d = direction(d)
            elif c in (2, 3):
                o = beyond(k, side, 0.5, 1.0)
                d = direction(inside(0.5) - o)
                if c == 3:
                    t_in = float(((hi[k] if side else lo[k]) - o[k]) / d[k])          # where the ray enters through its face
                    assert t_in > 0.2
                    gd = t_in * (0.4 if i % 2 == 0 else float(U(1.1, 1.6)))
            elif c == 4:
                o = inside(0.8)
                d = direction(U(-1.0, 1.0, 3))
                gd = exit_of(o, d) * float(U(1.1, 2.0)) + 0.1
            elif c == 5:
                o = inside(0.8)
                d = direction(U(-1.0, 1.0, 3))
                gd = 1.5 * tau * float(U(0.1, 0.95))
            elif c == 6:
                o = inside(0.8)
                d = U(0.3, 1.0, 3) * torch.where(torch.rand(3, generator=g) < 0.5, -1.0, 1.0).double()
                zeros = [(k,), (k,), (k, (k + 1) % 3), (k, (k + 2) % 3)][i % 4]
                signs = [(0.0,), (-0.0,), (0.0, -0.0), (-0.0, -0.0)][i % 4]
                for ax, z in zip(zeros, signs):
                    d[ax] = z
                d = direction(d)                                  # (scaling keeps a zero and its sign)
                if i % 3:
                    gd = exit_of(o, d) * float(U(0.3, 0.9))
            elif c == 7:
                o = inside(0.6)
                o[k] = (hi[k] - U(0.001, 0.006)) if side else (lo[k] + U(0.001, 0.006))
                d = U(-0.4, 0.4, 3)
                d[k] = sgn * U(0.8, 1.0)
                d = direction(d)                                  # |d[k]| >= 0.8: exit <= 0.0075
            elif c == 8:
                o = inside(0.6)
                d = U(-1.0, 1.0, 3)
                d[k] = 0.0 if i % 2 else -0.0
                d = direction(d)
            else:
                raise ValueError(c)
            O.append(o); D.append(d); GD.append(gd); C.append(c)
    ro, rd = torch.stack(O).float(), torch.stack(D).float()
    for r in [j for j, c in enumerate(C) if c == 8]:              # exactly on the face, in float32
        k, side = (r % per_class) % 3, ((r % per_class) // 3) % 2
        ro[r, k] = scene.bound[k, 1 if side else 0]
    return SimpleNamespace(rays_o=ro, rays_d=rd, gt_depth=torch.tensor(GD, dtype=torch.float32),
                           gt_color=torch.rand(len(C), 3, generator=g), cls=torch.tensor(C, dtype=torch.int64))


def select(b, classes):
    """The rays of `b` whose class is in `classes`, in order."""
    m = torch.isin(b.cls, torch.tensor(list(classes)))
    return SimpleNamespace(rays_o=b.rays_o[m], rays_d=b.rays_d[m], gt_depth=b.gt_depth[m], gt_color=b.gt_color[m], cls=b.cls[m])


def rand_for(R, ns, ni, stream=7):
    """The injected uniform numbers of a render of R rays (t_rand [R,S], t_rand_uni [R,ns], u [R,ni]), float32 CPU."""
    from myslam_amd import synth
    return tuple(torch.from_numpy(synth.hash_uniform(shape, stream + j)) for j, shape in enumerate(((R, ns + ni), (R, ns), (R, ni))))


def cotangent(R, S, stream=10):
    from myslam_amd import synth
    return torch.from_numpy(synth.hash_uniform((R, S), stream)) - 0.5


def interval(b, scene):
    """float64 (lo, hi) [R]: the ordered sample interval of every ray as include/eslam_hip.h states it for eslam_mark_rays."""
    from oracle import eslam_oracle as orc
    gd = b.gt_depth.double()
    c15 = 1.5 * float(scene.truncation)
    far = orc.aabb_exit(b.rays_o.double(), b.rays_d.double(), scene.bound.double()) + 0.01
    zero = torch.zeros_like(gd)
    lo = torch.where(gd > 0, torch.minimum(zero, gd - c15), torch.minimum(zero, far))
    hi = torch.where(gd > 0, torch.maximum(1.2 * gd, gd + c15), torch.maximum(zero, far))
    return lo, hi


def plane_hw(scene):
    """12 (h, w) in all_planes order (group, level)."""
    return [tuple(s[2:]) for grp in scene.plane_shapes for s in grp]


def block_base(scene):
    """(index of each plane's first texel in the 12 planes laid end to end, total texel count)."""
    base, n = [], 0
    for h, w in plane_hw(scene):
        base.append(n)
        n += h * w
    return base, n


def texel_mask(scene, p_nor):
    """bool [n texels of all 12 planes]: the bilinear corners of the normalised points p_nor [N,3] (hp.texels_of)."""
    base, n = block_base(scene)
    out = torch.zeros(n, dtype=torch.bool)
    for b0, t in zip(base, hp.texels_of(p_nor, scene.plane_shapes)):
        out[b0 + t.reshape(-1)] = True
    return out


def reach_mask(scene, b, steps_per_texel=4):
    """bool [n texels]: the texels the documented interval of the rays reaches, by dense stepping in float64 (at most a
    quarter of the finest texel per step along any axis)."""
    from oracle import eslam_oracle as orc
    lo, hi = interval(b, scene)
    o, d = b.rays_o.double(), b.rays_d.double()
    bound = scene.bound.double()
    wmax = max(max(hw) for hw in plane_hw(scene))
    cells = (d.abs() / (bound[:, 1] - bound[:, 0]) * wmax).max(1).values * (hi - lo)
    out = torch.zeros(block_base(scene)[1], dtype=torch.bool)
    for r in range(o.shape[0]):
        n = int(min(float(cells[r]) * steps_per_texel + 2, 200000))
        z = lo[r] + (hi[r] - lo[r]) * torch.linspace(0.0, 1.0, n, dtype=torch.float64)
        out |= texel_mask(scene, orc.normalize_points(o[r] + d[r] * z[:, None], bound))
    return out


def dilate(scene, mask, radius=2):
    """`mask` (bool [n texels]) grown by `radius` texels in both directions of every plane."""
    out = torch.zeros_like(mask)
    for b0, (h, w) in zip(block_base(scene)[0], plane_hw(scene)):
        m = mask[b0:b0 + h * w].view(1, 1, h, w).float()
        out[b0:b0 + h * w] = torch.nn.functional.max_pool2d(m, 2 * radius + 1, 1, radius).view(-1) > 0
    return out


def model(scene, state, dtype=torch.float32):
    """(planes, params, beta) on the CPU as harness.Workload(scene, planes="synth", state=state) holds them on the GPU:
    synth planes, default-initialised decoders of seed 0, "trained" = planes x 60 and the SDF head's bias + 0.55."""
    from myslam_amd import scene as scn
    from myslam_amd.src.networks.decoders import Decoders
    planes = scn.synth_planes(scene, channels_last=False)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        dec = Decoders(learnable_beta=scene.learnable_beta)
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    beta = sd.pop("beta") if "beta" in sd else torch.tensor([10.0])
    if state == "trained":
        planes = tuple([p * 60.0 for p in grp] for grp in planes)
        sd["output_linear.bias"] = sd["output_linear.bias"] + 0.55
    elif state != "initial":
        raise ValueError(state)
    return (tuple([p.to(dtype) for p in grp] for grp in planes), {k: v.to(dtype) for k, v in sd.items()}, beta.to(dtype))


def oracle_z(mdl, scene, b, ns, ni, rand, dtype):
    """orc.sample_z of the batch in `dtype` on the model (planes, params, beta of any dtype)."""
    from oracle import eslam_oracle as orc
    planes, params, beta = mdl
    cv = lambda t: t.detach().cpu().to(dtype)
    with torch.no_grad():
        return orc.sample_z(cv(b.rays_o), cv(b.rays_d), cv(b.gt_depth), tuple([cv(p) for p in grp] for grp in planes),
                            {k: cv(v) for k, v in params.items()}, cv(beta), scene.bound.to(dtype), float(scene.truncation), ns, ni,
                            *(None if t is None else cv(t) for t in rand))


def oracle_step(mdl, scene, b, z, cot, dtype):
    """Forward and backward of the oracle in `dtype` on given z_vals with the linear cotangents of
    test_gpu_parity.test_edge_shapes_against_oracle (0.7 depth + 0.3 colour + cot . sdf).  Returns the dict `accept` takes:
    depth, color, sdf, planes (12 gradients), dec {name: gradient, beta included}, ro, rd (ray gradients) - numpy float64."""
    from oracle import eslam_oracle as orc
    planes, params, beta = mdl
    cv = lambda t: t.detach().cpu().to(dtype)
    planes = tuple([cv(p).contiguous().requires_grad_(True) for p in grp] for grp in planes)
    params = {k: cv(v).requires_grad_(True) for k, v in params.items()}
    beta = cv(beta).requires_grad_(True)
    ro, rd = cv(b.rays_o).requires_grad_(True), cv(b.rays_d).requires_grad_(True)
    S = z.shape[1]
    od, oc, os_, _ = orc.render_batch_ray(planes, params, beta, scene.bound, rd, ro, float(scene.truncation), cv(b.gt_depth),
                                          S, 0, z_vals=cv(z))
    ((od * 0.7).sum() + (oc * 0.3).sum() + (os_ * cv(cot)).sum()).backward()
    n = lambda t: t.detach().double().numpy()
    dec = {k: n(v.grad) for k, v in params.items()}
    dec["beta"] = n(beta.grad)
    return dict(depth=n(od), color=n(oc), sdf=n(os_), planes=[n(p.grad) for p in hp.flat_planes(planes)], dec=dec,
                ro=n(ro.grad), rd=n(rd.grad))


def ambiguous(mdl, scene, b, z):
    """(p_nor [R*S,3] float64, amb bool [R*S]) of the samples at z: hp.ambiguous_samples under the float64 oracle."""
    from oracle import eslam_oracle as orc
    planes, params, _ = mdl
    cv = lambda t: t.detach().cpu().double()
    pts = cv(b.rays_o)[:, None, :] + cv(b.rays_d)[:, None, :] * cv(z)[..., None]
    pn = orc.normalize_points(pts.reshape(-1, 3), scene.bound.double())
    amb = hp.ambiguous_samples(pn, tuple([cv(p).contiguous() for p in grp] for grp in planes), {k: cv(v) for k, v in params.items()})
    return pn, amb


def accept(mine, o32, o64, pn, amb, scene, report=None, label="", max_excluded=None):
    """THE acceptance criteria of a forward + backward on this batch, as test_edge_shapes_against_oracle states them:
    outputs within RTOL of the float64 oracle; plane gradients by hp.plane_grads_close; decoder gradients against the float32
    oracle (comparator) and the float64 one (conditioning bound) with the ambiguous-sample slack; ray gradients: 97 % of the
    rays within RTOL, the rest bounded by 0.05.  report: a dict that receives the worst value / bar per criterion.
    max_excluded: handed to hp.plane_grads_close (the share of a plane's touched texels the comparison may set aside)."""
    rep = {} if report is None else report
    worst = lambda k, v: rep.__setitem__(k, max(rep.get(k, 0.0), float(v)))
    for k in ("depth", "color", "sdf"):
        e = hp.rel_err(mine[k], o64[k])
        worst("out:" + k, e / RTOL)
        assert e <= RTOL, (label, k, e)
    pr = []
    ok, msg = hp.plane_grads_close(mine["planes"], o32["planes"], o64["planes"], pn, amb, scene.plane_shapes, RTOL, report=pr,
                                   max_excluded=max_excluded)
    if pr:
        worst("plane_grad", max(v for _, v in pr))
    assert ok, (label, msg, int(amb.sum()))
    slack = 4.0 * float(amb.sum()) / max(1, amb.numel())
    for k, a in mine["dec"].items():
        e32 = hp.rel_err(a, o32["dec"][k])
        e64 = hp.rel_err(a, o64["dec"][k])
        cond = hp.rel_err(o32["dec"][k], o64["dec"][k])
        worst("dec_grad", max(e32 / (RTOL + slack), e64 / (max(RTOL, 1.5 * cond) + slack)))
        assert e32 <= RTOL + slack, (label, k, e32)
        assert e64 <= max(RTOL, 1.5 * cond) + slack, (label, k, e64, cond)
    for k in ("ro", "rd"):
        per_ray = np.abs(mine[k] - o64[k]).max(1) / (np.abs(o64[k]).max() + 1e-30)
        q = float(np.quantile(per_ray, 0.97))
        worst("ray_grad:q97", q / RTOL)
        worst("ray_grad:max", per_ray.max() / 0.05)
        assert q <= RTOL and per_ray.max() <= 0.05, (label, k, q, float(per_ray.max()))
    return rep


def check_z(z, zo32, zo64, gt_depth, report=None, label=""):
    """Sampler criteria of test_edge_shapes_against_oracle: rows of rays with depth bit-equal to the float32 oracle (or within
    1e-6 of the float64 one), depth-less rows within RTOL of the float64 oracle, every row ascending."""
    rep = {} if report is None else report
    z, zo32, zo64 = z.detach().cpu(), zo32.detach().cpu(), zo64.detach().cpu()
    has = gt_depth.detach().cpu() > 0
    assert bool((z[:, 1:] >= z[:, :-1]).all()), (label, "z_vals must be ascending")
    if has.any():
        e = hp.rel_err(z[has].numpy(), zo64[has].numpy())
        if not torch.equal(z[has], zo32.float()[has]):
            rep["z:depth"] = max(rep.get("z:depth", 0.0), e / 1e-6)
            assert e <= 1e-6, (label, e)
    if (~has).any():
        e = hp.rel_err(z[~has].numpy(), zo64[~has].numpy())
        rep["z:depth-less"] = max(rep.get("z:depth-less", 0.0), e / RTOL)
        assert e <= RTOL, (label, e)
    return rep
