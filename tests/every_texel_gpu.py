"""GPU side of tests/test_gpu_every_texel.py, shared with its child process (python -m tests.every_texel_gpu, the deterministic
mode, which is read once per process).  Test-only.

run(case) is the flow every case follows (tests/every_texel.py has the why):
  a workload whose ray pool is 1.6 - 3 x R  ->  ops.sample_z on the pool with injected rows  ->  every_texel.unambiguous_rays
  ->  render and backward on the picked rays with the picked rows  ->  the z_vals are the pool's bits, no sample is ambiguous,
  the call took the kernel path the case names, all twelve oracle gradients are non-zero, and the criteria of
  hostile_rays.accept hold with max_excluded = 0.0: every touched texel compared, no slack on the decoder gradients.
"""
import json
import sys
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np
import torch

from tests import every_texel as et
from tests import helpers as hp
from tests import hostile_rays as hr

RTOL = hr.RTOL
SMALL = (37, 23, 6, 0.0, 1024)            # R, n_strat, n_imp, zero_frac, bundle: 1015 + 58 samples, two per thread
LARGE = (640, 56, 8, 0.1, 2048)           # bundles of exactly 2048, four per thread, 240 workgroups


class Case(NamedTuple):
    size: tuple = SMALL
    state: str = "trained"
    pairing: int = 0                      # eslam_scatter_pairing mode
    res: str = "default"                  # room0: the colour planes' resolutions (test_gpu_paired_scatter._set_res)
    shapes: Optional[str] = None          # a set of every_texel.SHAPE_SETS, on the toy bound; None: room0 as shipped
    rays_grad: bool = False
    channels_last: bool = True
    loss: str = "linear"                  # "linear": 0.7 depth + 0.3 colour + cot . sdf; "fused": the mapping loss, MODE 2

    @property
    def label(self):
        R, ns, ni = self.size[:3]
        parts = [self.shapes or f"room0/{self.res}", f"{R}x{ns}+{ni}", self.state, f"pairing {self.pairing}"]
        parts += ["ray gradients"] * self.rays_grad + ["NCHW"] * (not self.channels_last) + ["fused loss"] * (self.loss == "fused")
        return " ".join(parts)


def _n(t):
    return t.detach().cpu().double().numpy()


def _lib():
    from myslam_amd import _hip
    return _hip.lib()


def cpu_model(wl):
    cv = lambda t: t.detach().cpu().float()
    return (tuple([cv(p).contiguous() for p in grp] for grp in wl.planes),
            {k: cv(v) for k, v in wl.decoders.state_dict().items() if k != "beta"}, cv(wl.decoders.beta))


def set_shapes(wl, state, name, channels_last=True):
    """Replace the workload's planes by synth planes of the shapes SHAPE_SETS[name] (and its scene by one that states them)."""
    from myslam_amd import scene as scn
    sc = et.with_shapes(wl.scene, name)
    pl = scn.synth_planes(sc, device=wl.device, channels_last=channels_last)
    k = 60.0 if state == "trained" else 1.0
    wl.planes = tuple([torch.nn.Parameter(p * k) for p in grp] for grp in pl)
    wl.scene = sc
    wl._plane_list = wl._params = None
    assert [tuple(p.shape[2:]) for p in wl.plane_list] == [hw for grp in et.SHAPE_SETS[name] for hw in grp]
    return wl


def workload(case, dev):
    """The pool: room0 keeps nearly every ray it asks for, the toy camera loses half to the pre-filter."""
    from myslam_amd import harness
    from tests import test_gpu_paired_scatter as tps
    R, ns, ni, zero_frac, _ = case.size
    toy = case.shapes is not None
    ask = {37: 120 if toy else 64, 640: 2000 if toy else 1100}[R]
    wl = harness.make_workload("toy" if toy else "room0", ask, ns, ni, device=dev, zero_frac=zero_frac, planes="synth",
                               state=case.state, channels_last=case.channels_last)
    if toy:
        return set_shapes(wl, case.state, case.shapes, case.channels_last)
    return tps._set_res(wl, case.state, case.res, case.channels_last)


def pick(wl, case):
    """(keep, z_pool, rand_pool): the first R pool rays without an ambiguous sample, on the kernel's own z_vals of the pool."""
    from myslam_amd import ops
    R, ns, ni = case.size[:3]
    dev = wl.device
    P = wl.R
    rand = tuple(t.to(dev) for t in hr.rand_for(P, ns, ni))
    ro, rd, gd = wl.rays_o.detach(), wl.rays_d.detach(), wl.gt_depth
    with torch.no_grad():
        z = ops.sample_z(ro, rd, gd, ops.planes_for_kernels(wl.planes, P * (ns + ni)), wl.decoders, wl.renderer._bound6, wl.truncation,
                         ns, ni, True, rand)
    torch.cuda.synchronize()
    pool = SimpleNamespace(rays_o=ro.cpu(), rays_d=rd.cpu(), gt_depth=gd.cpu())
    keep = et.unambiguous_rays(cpu_model(wl), wl.scene, pool, z.cpu(), R)
    return keep.to(dev), z, rand


def _oracle_loss_step(mdl, scene, b, z, mask, dtype):
    """The mapping iteration in the oracle on given z_vals, the loss over the rays the mask keeps (src/Mapper.py:329-346; as
    tests/test_gpu_saved_hidden.py::_oracle)."""
    from oracle import eslam_oracle as orc
    planes, params, beta = mdl
    cv = lambda t: t.detach().cpu().to(dtype)
    planes = tuple([cv(p).contiguous().requires_grad_(True) for p in grp] for grp in planes)
    params = {k: cv(v).requires_grad_(True) for k, v in params.items()}
    beta = cv(beta).clone().requires_grad_(True)
    ro, rd, gd, gc, zz = cv(b.rays_o), cv(b.rays_d), cv(b.gt_depth), cv(b.gt_color), cv(z)
    od, oc, os_, _ = orc.render_batch_ray(planes, params, beta, scene.bound, rd, ro, float(scene.truncation), gd, z.shape[1], 0, z_vals=zz)
    loss = orc.mapping_loss(od[mask], oc[mask], os_[mask], zz[mask], gd[mask], gc[mask], float(scene.truncation))
    loss.backward()
    dec = {k: _n(v.grad) for k, v in params.items()}
    dec["beta"] = _n(beta.grad)
    return dict(loss=float(loss), depth=_n(od), color=_n(oc), sdf=_n(os_), planes=[_n(p.grad) for p in hp.flat_planes(planes)], dec=dec)


def run(case, dev=None):
    """One case, every assertion of the flow.  Returns what the tests look at afterwards: the workload, the picked rays (device),
    the float64 oracle's result, the margins (value / bar per criterion) and which kernels the library dispatched."""
    from myslam_amd import losses
    from tests import test_gpu_rank16_scatter as t16
    dev = dev or torch.device("cuda:0")
    lib = _lib()
    det = int(lib.eslam_deterministic())
    R, ns, ni, _, bundle = case.size
    S = ns + ni
    wl = workload(case, dev)
    keep, z_pool, rand_pool = pick(wl, case)
    ro, rd = wl.rays_o.detach()[keep].contiguous(), wl.rays_d.detach()[keep].contiguous()
    gd, gc = wl.gt_depth[keep].contiguous(), wl.gt_color[keep].contiguous()
    rand = tuple(t[keep].contiguous() for t in rand_pool)
    if case.rays_grad:
        ro, rd = ro.requires_grad_(True), rd.requires_grad_(True)
    cot = hr.cotangent(R, S)
    mask = None
    before = lib.eslam_scatter_pairing(-1)
    lib.eslam_scatter_pairing(case.pairing)
    try:
        t16._fresh(wl)
        if case.loss == "fused":
            mask = (torch.arange(R, device=dev) % 3) != 1                  # every third ray masked
            depth, color, sdf, z, pre = wl.renderer.render_batch_ray_with_loss(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gd, gc,
                                                                              losses.MAPPING_W, ray_mask=mask, _rand=rand)
            loss = losses.mapping_loss(depth, color, sdf, z, gd, gc, wl.truncation, precomputed=pre)
            # the loss is an output of the render node itself: its gradient is formed inside the backward kernel (MODE 2)
            assert "RenderFn" in type(loss.grad_fn).__name__ and loss.grad_fn is sdf.grad_fn, type(loss.grad_fn).__name__
        else:
            depth, color, sdf, z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd, _rand=rand)
            loss = (depth * 0.7).sum() + (color * 0.3).sum() + (sdf * cot.to(dev)).sum()
        loss.backward()
        torch.cuda.synchronize()
        rank16, paired = int(lib.eslam_last_backward_rank16()), int(lib.eslam_last_scatter_paired())
    finally:
        lib.eslam_scatter_pairing(before)
    label = case.label + (" deterministic" if det else "")
    # the batch is the pool's: same bits, and nothing ambiguous on the render's own z_vals
    assert z.shape == (R, S) and torch.equal(z, z_pool[keep]), (label, "the render's z_vals are not the pool's rows")
    mdl = cpu_model(wl)
    b = SimpleNamespace(rays_o=ro.detach().cpu(), rays_d=rd.detach().cpu(), gt_depth=gd.cpu(), gt_color=gc.cpu())
    used = b if mask is None else et.take(b, mask.cpu())
    pn, amb = hr.ambiguous(mdl, wl.scene, used, z.detach().cpu() if mask is None else z.detach().cpu()[mask.cpu()])
    assert int(amb.sum()) == 0, (label, int(amb.sum()))
    assert hp.excluded_share(pn, amb, wl.scene.plane_shapes) == [0.0] * 12
    # the kernel path
    pairs = et.pair_count(wl.scene.plane_shapes)
    if case.shapes is not None:
        assert pairs == et.PAIRS[case.shapes]
    full_width = case.rays_grad or det
    assert rank16 == (0 if full_width else 1), (label, rank16)
    if case.rays_grad:
        t16._assert_full_width_path(ro, rd)
    if not full_width:
        t16._assert_rank16_path(wl, ro, rd, R, S, bundle)
        assert paired == int(case.pairing == 2 and pairs > 0), (label, paired, pairs)
    if not det:
        assert lib.eslam_scatter_bundle_samples(R, S, 1) == bundle
    # against the oracle
    mine = dict(depth=_n(depth), color=_n(color), sdf=_n(sdf), planes=[_n(p.grad) for p in wl.plane_list],
                dec={k: _n(t.grad) for k, t in wl.decoders.named_parameters()})
    if case.loss == "fused":
        o64, o32 = (_oracle_loss_step(mdl, wl.scene, b, z, mask.cpu(), dt) for dt in (torch.float64, torch.float32))
        e = abs(float(loss) - o64["loss"]) / abs(o64["loss"])
        print(f"margin {label}: {'loss':<12s} {e / RTOL:.3f}")
        assert e <= RTOL, (label, float(loss), o64["loss"])
    else:
        o64, o32 = (hr.oracle_step(mdl, wl.scene, b, z, cot, dt) for dt in (torch.float64, torch.float32))
    assert all(np.abs(g).max() > 0 for g in o64["planes"]), (label, "an oracle plane gradient is zero")
    if case.rays_grad:
        mine.update(ro=_n(ro.grad), rd=_n(rd.grad))
        assert np.abs(o64["ro"]).max() > 0 and np.abs(o64["rd"]).max() > 0
        rep = hr.accept(mine, o32, o64, pn, amb, wl.scene, label=label, max_excluded=0.0)
        for k, v in rep.items():
            print(f"margin {label}: {k:<12s} {v:.3f}")
    else:
        t16._accept(mine, o32, o64, pn, amb, wl.scene, label, max_excluded=0.0)
    t16._fresh(wl)
    return SimpleNamespace(wl=wl, ro=ro.detach(), rd=rd.detach(), gd=gd, z=z.detach(), o64=o64, rank16=rank16, paired=paired, det=det,
                           pairs=pairs)


# what the deterministic child runs: the shipped shapes through the paired list's mode and with ray gradients, both sizes
DET_CASES = [Case(size=s, pairing=2) for s in (SMALL, LARGE)] + [Case(size=s, rays_grad=True) for s in (SMALL, LARGE)]


def main():
    """Child: ESLAM_DETERMINISTIC=1 (the fixed-point scatter, full-width rows whatever the rays ask for)."""
    res = dict(det=int(_lib().eslam_deterministic()), cases={})
    for case in DET_CASES:
        try:
            r = run(case)
            res["cases"][case.label] = dict(ok=True, rank16=r.rank16, paired=r.paired)
        except AssertionError as e:
            res["cases"][case.label] = dict(ok=False, error=repr(e)[:2000])
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    sys.exit(main())
