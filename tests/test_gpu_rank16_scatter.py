"""The rank-16 render backward: rays whose positions need no gradient (mapping with fixed poses - the benchmarked step) store
the 16-wide gradient at the decoders' first hidden layer, and the scatter sums it per texel cell and expands each cell's sums by
the plane's slice of W1 once (mlp_bwd_kernel<GZ> / scatter_sort_kernel<GZ>; tests/rank16_ref.py restates it in numpy).  Rays that
DO need gradients keep the full-width feature-gradient rows: the same library computes both, which test 2 uses.

  1  against the oracle: the shapes and criteria of test_gpu_parity.test_edge_shapes_against_oracle, minus the ray gradients
  2  against the full-width path on the same inputs and cotangents
  3  the rays the callers' pre-filter removes (tests/hostile_rays.py)

Every test asserts that its call takes the new path the way bwd_common decides it: float32 planes that receive gradients, rays
that do not, not deterministic mode - and which bundle size (1024: two samples per thread, 2048: four) its shape runs.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import hostile_rays as hr

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _n(t):
    return t.detach().cpu().double().numpy()


def _assert_rank16_path(wl, ro, rd, R, S, bundle=None):
    """The dispatch's conditions, seen from the caller: after a backward the planes hold gradients and the rays hold none."""
    from myslam_amd import _hip
    lib = _hip.lib()
    assert lib.eslam_deterministic() == 0
    assert lib.eslam_last_backward_rank16() == 1, "the last backward wrote full-width rows"
    assert not ro.requires_grad and not rd.requires_grad and ro.grad is None and rd.grad is None
    assert all(p.dtype == torch.float32 and p.grad is not None for p in wl.plane_list)
    got = lib.eslam_scatter_bundle_samples(R, S, 1)
    assert got in (1024, 2048) and (bundle is None or got == bundle), (R, S, got, bundle)
    return got


def _last_backward_rank16():
    from myslam_amd import _hip
    return _hip.lib().eslam_last_backward_rank16()


def _assert_full_width_path(ro, rd):
    assert ro.requires_grad and rd.requires_grad and ro.grad is not None and rd.grad is not None


def _accept(mine, o32, o64, pn, amb, scene, label, max_excluded=None):
    """hostile_rays.accept (= the criteria of test_edge_shapes_against_oracle) without the ray gradients this path never has."""
    rep = {}
    for k in ("depth", "color", "sdf"):
        e = hp.rel_err(mine[k], o64[k])
        rep["out:" + k] = e / RTOL
        assert e <= RTOL, (label, k, e)
    pr = []
    ok, msg = hp.plane_grads_close(mine["planes"], o32["planes"], o64["planes"], pn, amb, scene.plane_shapes, RTOL, report=pr,
                                   max_excluded=max_excluded)
    if pr:
        rep["plane_grad"] = max(v for _, v in pr)
    assert ok, (label, msg, int(amb.sum()))
    slack = 4.0 * float(amb.sum()) / max(1, amb.numel())
    for k, a in mine["dec"].items():
        e32, e64 = hp.rel_err(a, o32["dec"][k]), hp.rel_err(a, o64["dec"][k])
        cond = hp.rel_err(o32["dec"][k], o64["dec"][k])
        rep["dec_grad"] = max(rep.get("dec_grad", 0.0), e32 / (RTOL + slack), e64 / (max(RTOL, 1.5 * cond) + slack))
        assert e32 <= RTOL + slack, (label, k, e32)
        assert e64 <= max(RTOL, 1.5 * cond) + slack, (label, k, e64, cond)
    for k, v in rep.items():
        print(f"margin {label}: {k:<12s} {v:.3f}")


def _print_excluded(label, pn, amb, scene):
    """What the criterion leaves out here: per plane the share of the touched texels set aside with the ambiguous samples
    (tests/test_gpu_every_texel.py runs batches where it is zero)."""
    share = hp.excluded_share(pn, amb, scene.plane_shapes)
    print(f"excluded {label}: {int(amb.sum())} ambiguous samples, share of touched texels not compared " + " ".join(f"{v:.2f}" for v in share))


def _cpu_model(wl):
    cv = lambda t: t.detach().cpu().float()
    return (tuple([cv(p).contiguous() for p in grp] for grp in wl.planes),
            {k: cv(v) for k, v in wl.decoders.state_dict().items() if k != "beta"}, cv(wl.decoders.beta))


def _fresh(wl):
    for p in wl.params():
        p.grad = None


def _render_backward(wl, ro, rd, gd, rand, cot):
    _fresh(wl)
    dev = wl.device
    depth, color, sdf, z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd, _rand=rand)
    ((depth * 0.7).sum() + (color * 0.3).sum() + (sdf * cot.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    return dict(depth=_n(depth), color=_n(color), sdf=_n(sdf), planes=[_n(p.grad) for p in wl.plane_list],
                dec={k: _n(t.grad) for k, t in wl.decoders.named_parameters()}), z.detach()


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------
SHAPES = [(1, 24, 8, 0.0, 1024), (3, 5, 3, 0.0, 1024), (33, 16, 0, 0.0, 1024), (65, 200, 56, 0.2, 1024), (200, 24, 8, 0.0, 1024),
          (640, 56, 8, 0.1, 2048)]


@pytest.mark.parametrize("R,ns,ni,zero_frac,bundle", SHAPES)
@pytest.mark.parametrize("state", ["initial", "trained"])
def test_rank16_backward_against_oracle(R, ns, ni, zero_frac, bundle, state):
    """A single ray, S not a multiple of 16, four chunks per ray, 1024-sample bundles (two samples per thread) and 2048-sample
    ones (four; 240 scatter workgroups) - forward outputs, plane, decoder and beta gradients against the float32 / float64 oracle
    on the kernel's own z_vals."""
    from myslam_amd import harness
    dev = _dev()
    wl = harness.make_workload("room0", max(R, 8), ns, ni, device=dev, zero_frac=zero_frac, planes="synth", state=state)
    S = ns + ni
    ro, rd, gd = wl.rays_o[:R].detach(), wl.rays_d[:R].detach(), wl.gt_depth[:R]
    rand = tuple(t.to(dev) for t in hr.rand_for(R, ns, ni))
    cot = hr.cotangent(R, S)
    mine, z = _render_backward(wl, ro, rd, gd, rand, cot)
    _assert_rank16_path(wl, ro, rd, R, S, bundle)
    if bundle == 2048:
        assert -(-R // (2048 // S)) * 12 > 192
    for k in ("depth", "color", "sdf"):
        assert np.isfinite(mine[k]).all(), k
    b = SimpleNamespace(rays_o=ro.cpu(), rays_d=rd.cpu(), gt_depth=gd.cpu())
    mdl = _cpu_model(wl)
    o64, o32 = (hr.oracle_step(mdl, wl.scene, b, z, cot, dt) for dt in (torch.float64, torch.float32))
    pn, amb = hr.ambiguous(mdl, wl.scene, b, z)
    _print_excluded(f"rank16 {R}x{ns}+{ni} {state}", pn, amb, wl.scene)
    _accept(mine, o32, o64, pn, amb, wl.scene, f"rank16 {R}x{ns}+{ni} {state}")


# ---- 2. against the full-width path ----------------------------------------------------------------------------------------
def _max_normalised(a, b):
    return max(hp.rel_err(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("R,ns,ni,bundle,kw", [(200, 24, 8, 1024, {}), (640, 56, 8, 2048, {}), (400, 40, 8, None, dict(cams=4)),
                                               (200, 24, 8, 1024, dict(channels_last=False))])
def test_rank16_path_equals_full_width_path(R, ns, ni, bundle, kw):
    """The same rays, numbers and cotangents with ray gradients requested (full-width rows) and without (rank 16): plane gradients
    within 1e-5 max-normalised (the threshold tools/ab_outputs.py uses between builds) - or four times what two runs of the
    full-width path differ by among themselves (x: unordered float atomics), should that be more; decoder and beta gradients and
    the loss of step() within 1e-6.

    x measured on an MI355X (max-normalised difference of two runs of the full-width path on the same input), and what the rank-16
    path differs from it by:  200 x 32: x = 6.9e-7, planes 6.5e-7;  640 x 64: x = 8.2e-7, planes 8.1e-7;  400 x 48 from four
    cameras: x = 4.8e-7, planes 5.5e-7;  200 x 32 NCHW: x = 4.4e-7, planes 5.6e-7.  4x stays below 1e-5 in every case, so the bar
    that holds is 1e-5.  Decoder and beta gradients came out bit-identical, the step's loss within 1.1e-7 ... 2.3e-7."""
    from myslam_amd import harness
    dev = _dev()
    mk = lambda rg: harness.Workload("room0", R, ns, ni, dev, planes="synth", state="trained", rays_grad=rg, **kw)
    old, new = mk(True), mk(False)
    S = ns + ni
    assert torch.equal(old.rays_o.detach(), new.rays_o) and all(torch.equal(a.detach(), b.detach()) for a, b in zip(old.params(), new.params()))

    def grads(wl):
        g = wl.backward_with(wl.forward(fixed_rand=True))
        torch.cuda.synchronize()
        assert _last_backward_rank16() == (0 if wl is old else 1), "the library dispatched the other pair of kernels"
        return [_n(t) for t in g]

    g_old, g_old2, g_new = grads(old), grads(old), grads(new)
    _assert_full_width_path(old.rays_o, old.rays_d)
    got = _assert_rank16_path(new, new.rays_o, new.rays_d, new.R, S, bundle)
    x = _max_normalised(g_old2[:12], g_old[:12])
    bar = max(1e-5, 4.0 * x)
    e_planes = _max_normalised(g_new[:12], g_old[:12])
    e_rest = _max_normalised(g_new[12:], g_old[12:])
    print(f"margin rank16 vs full width {R}x{S} {kw} (bundle {got}): x = {x:.3e}, planes {e_planes:.3e} (bar {bar:.1e}), "
          f"decoders + beta {e_rest:.3e} (bar 1e-06)")
    assert len(g_new) > 12 and all(np.abs(g).max() > 0 for g in g_old[:12])
    assert e_planes <= bar, (e_planes, bar, x)
    assert e_rest <= 1e-6, e_rest
    # the fused-loss step (loss gradient, composite and decoder backward in one launch)
    old.renderer.perturb = new.renderer.perturb = False
    l_old = float(old.step())
    assert _last_backward_rank16() == 0
    l_new = float(new.step())
    torch.cuda.synchronize()
    _assert_full_width_path(old.rays_o, old.rays_d)
    _assert_rank16_path(new, new.rays_o, new.rays_d, new.R, S, bundle)
    s_old, s_new = [_n(p.grad) for p in old.params()], [_n(p.grad) for p in new.params()]
    e_loss = abs(l_new - l_old) / abs(l_old)
    e_planes, e_rest = _max_normalised(s_new[:12], s_old[:12]), _max_normalised(s_new[12:], s_old[12:])
    print(f"margin rank16 vs full width step {R}x{S} {kw}: loss {e_loss:.3e}, planes {e_planes:.3e} (bar {bar:.1e}), decoders + beta {e_rest:.3e}")
    assert e_loss <= 1e-6 and e_rest <= 1e-6 and e_planes <= bar, (e_loss, e_rest, e_planes, bar)


# ---- 3. the rays the pre-filter removes ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _toy(ns, ni, state):
    from myslam_amd import harness
    return harness.make_workload("toy", 256, ns, ni, device=_dev(), planes="synth", state=state)


@functools.lru_cache(maxsize=None)
def _hostile(finite):
    from myslam_amd import scene as scn
    return hr.make(scn.make_scene("toy"), classes=hr.FINITE_CLASSES if finite else hr.ALL_CLASSES)


@pytest.mark.parametrize("state", hr.STATES)
@pytest.mark.parametrize("ns,ni", hr.SIZES)
def test_rank16_unmasked_hostile_rays_against_oracle(ns, ni, state):
    """Classes 1-7 (origins outside the bound, zero or negative exits, depths beyond the box, axis-parallel directions), rendered
    and back-propagated without ray gradients: the criteria of test 1."""
    wl = _toy(ns, ni, state)
    dev = wl.device
    b = _hostile(True)
    ro, rd, gd = b.rays_o.to(dev), b.rays_d.to(dev), b.gt_depth.to(dev)
    R, S = ro.shape[0], ns + ni
    rand = tuple(t.to(dev) for t in hr.rand_for(R, ns, ni))
    cot = hr.cotangent(R, S)
    mine, z = _render_backward(wl, ro, rd, gd, rand, cot)
    _assert_rank16_path(wl, ro, rd, R, S)
    assert all(np.isfinite(g).all() for g in mine["planes"]) and all(np.isfinite(g).all() for g in mine["dec"].values())
    mdl = _cpu_model(wl)
    o64, o32 = (hr.oracle_step(mdl, wl.scene, b, z, cot, dt) for dt in (torch.float64, torch.float32))
    pn, amb = hr.ambiguous(mdl, wl.scene, b, z)
    _accept(mine, o32, o64, pn, amb, wl.scene, f"rank16 hostile {ns}+{ni} {state}")
    _fresh(wl)


@pytest.mark.parametrize("state", hr.STATES)
@pytest.mark.parametrize("ns,ni", hr.SIZES)
def test_rank16_masked_hostile_rays_contribute_exactly_nothing(ns, ni, state):
    """64 benign rays + all eight hostile classes (class 8 renders NaN) under a ray_mask that keeps the benign ones, fused-loss
    step without ray gradients: every gradient finite and equal to the benign rays' alone (RTOL, as
    test_gpu_hostile_rays.test_masked_hostile_rays_contribute_exactly_nothing), and exact zeros in every 128-byte
    plane-gradient block only masked rays can reach."""
    from myslam_amd import losses, ops, parallel
    wl = _toy(ns, ni, state)
    dev = wl.device
    b = _hostile(False)
    ro = torch.cat([wl.rays_o[:64].detach(), b.rays_o.to(dev)])
    rd = torch.cat([wl.rays_d[:64].detach(), b.rays_d.to(dev)])
    gd, gc = torch.cat([wl.gt_depth[:64], b.gt_depth.to(dev)]), torch.cat([wl.gt_color[:64], b.gt_color.to(dev)])
    mask = torch.zeros(ro.shape[0], dtype=torch.bool, device=dev)
    mask[:64] = True
    rand = tuple(t.to(dev) for t in hr.rand_for(ro.shape[0], ns, ni, stream=40))

    def step(ro, rd, gd, gc, mask, rand):
        _fresh(wl)
        depth, color, sdf, z, pre = wl.renderer.render_batch_ray_with_loss(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gd, gc,
                                                                          losses.MAPPING_W, ray_mask=mask, _rand=rand)
        loss = losses.mapping_loss(depth, color, sdf, z, gd, gc, wl.truncation, precomputed=pre)
        loss.backward()
        torch.cuda.synchronize()
        _assert_rank16_path(wl, ro, rd, ro.shape[0], ns + ni)
        return float(loss), [p.grad.detach().clone() for p in wl.plane_list], {k: t.grad.detach().clone() for k, t in wl.decoders.named_parameters()}

    loss, planes, dec = step(ro, rd, gd, gc, mask, rand)
    loss1, planes1, dec1 = step(ro[:64], rd[:64], gd[:64], gc[:64], None, tuple(t[:64] for t in rand))
    _fresh(wl)
    assert np.isfinite(loss) and all(bool(torch.isfinite(t).all()) for t in planes + list(dec.values()))
    assert abs(loss - loss1) <= RTOL * abs(loss1)
    assert max(hp.rel_err(_n(a), _n(c)) for a, c in zip(planes, planes1)) <= RTOL
    assert max(hp.rel_err(_n(dec[k]), _n(dec1[k])) for k in dec1) <= RTOL
    base, n_blocks = hr.block_base(wl.scene)
    b6 = ops.bound_to_host(wl.scene.bound)
    mark = lambda sl: parallel.mark_rays(None, b6, ro[sl], rd[sl], gd[sl], wl.truncation, base, n_blocks, planes=wl.planes).bool()
    benign, hostile = mark(slice(0, 64)), mark(slice(64, None))
    assert int((hostile & ~benign).sum()) > 100
    rows = torch.cat([g.permute(0, 2, 3, 1).reshape(-1, 32) for g in planes])
    assert rows.shape[0] == n_blocks
    assert int((rows[~benign] != 0).sum()) == 0, "a masked ray left something in a block only masked rays reach"
