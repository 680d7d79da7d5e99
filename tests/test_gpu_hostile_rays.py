"""The kernels on the rays the callers' AABB pre-filter removes (tests/hostile_rays.py): origins outside the bound, a zero or
negative AABB exit, depths shorter than the surface band or beyond the box, axis-parallel directions, a 0/0 exit.  The
graph-captured loop and MappingWindow keep the pre-filter as a ray_mask, render_img has none and the C entries are public, so
the sampler, the render kernels, the losses and the ray-sharded step all see such rays; no other test shows them any.

  sampler      injected and in-kernel numbers against orc.sample_z (classes 1 and 7 alone: the all-pairs rank sort)
  render       forward and backward against the float64 oracle on the kernel's own z_vals, both plane layouts, and the
               mixed-precision forward against tests/lowp_ref.py
  masked rays  contribute exactly nothing, NaN rays included (fused-loss path, separate mapping and tracking losses)
  marking      eslam_mark_rays is a tight superset of what a backward touches, per class; ShardedMapper steps repeat
  companions   ops.prefilter / ops.aabb_exit / ops.loss_set_sizes on the batch

The criteria are those of test_gpu_parity.test_edge_shapes_against_oracle (hostile_rays.accept / check_z), which
tests/test_hostile_rays_ref.py shows the float32 oracle to meet on this batch.  Every test prints `margin ...` lines (value /
bar; pytest -s); profiles/hostile_rays_margins.txt keeps those of one MI355X run.

Run time on an MI355X: see README.md (the float32 / float64 oracle of 84 rays x 96 samples on the host is most of it).
"""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import hostile_rays as hr
from tests import rng_ref

pytestmark = pytest.mark.gpu
RTOL = hr.RTOL


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _wl(ns, ni, state, channels_last=True):
    from myslam_amd import harness
    return harness.make_workload("toy", 256, ns, ni, device=_dev(), planes="synth", state=state, channels_last=channels_last)


def _fresh(wl):
    for p in wl.params():
        p.grad = None
    return wl


def _cpu_model(wl):
    cv = lambda t: t.detach().cpu().float()
    return (tuple([cv(p).contiguous() for p in grp] for grp in wl.planes),
            {k: cv(v) for k, v in wl.decoders.state_dict().items() if k != "beta"}, cv(wl.decoders.beta))


@functools.lru_cache(maxsize=None)
def _batch(finite=True):
    from myslam_amd import scene as scn
    return hr.make(scn.make_scene("toy"), classes=hr.FINITE_CLASSES if finite else hr.ALL_CLASSES)


def _on(dev, b):
    return b.rays_o.to(dev), b.rays_d.to(dev), b.gt_depth.to(dev), b.gt_color.to(dev)


def _margins(label, rep):
    for k, v in rep.items():
        print(f"margin {label}: {k:<16s} {v:.3f}")


def _render_z(wl, ro, rd, gd, rand):
    with torch.no_grad():
        return wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, wl.device, wl.truncation, gt_depth=gd, _rand=rand)[3]


def _check_z_all(z, wl, b, ns, ni, rand, label):
    """hr.check_z for the whole batch and for classes 1 and 7 alone (far <= 0 and near-coincident samples: the only inputs that
    reach the all-pairs rank sort of importance_z_kernel)."""
    mdl = _cpu_model(wl)
    zo32, zo64 = (hr.oracle_z(mdl, wl.scene, b, ns, ni, rand, dt) for dt in (torch.float32, torch.float64))
    assert z.shape == (b.rays_o.shape[0], ns + ni) and bool(torch.isfinite(z).all())
    rep = hr.check_z(z, zo32, zo64, b.gt_depth, label=label)
    for k in (1, 7):
        m = b.cls == k
        r = hr.check_z(z.cpu()[m], zo32[m], zo64[m], b.gt_depth[m], label=f"{label} class {k}")
        rep.update({f"{key} (class {k})": v for key, v in r.items()})
    lo, hi = hr.interval(b, wl.scene)
    zc = z.cpu().double()
    span = (hi - lo)[:, None]
    assert bool((zc >= lo[:, None] - 1e-6 * (1 + span)).all()) and bool((zc <= hi[:, None] + 1e-6 * (1 + span)).all()), label
    _margins(label, rep)


# ---- the workload's model is the one the CPU reference tests ran on ------------------------------------------------------
@pytest.mark.parametrize("state", hr.STATES)
def test_workload_model_equals_the_cpu_reference_model(state):
    wl = _wl(24, 8, state)
    planes, params, beta = _cpu_model(wl)
    rp, rparams, rbeta = hr.model(wl.scene, state)
    assert all(torch.equal(a, b) for ga, gb in zip(planes, rp) for a, b in zip(ga, gb))
    assert set(params) == set(rparams) and all(torch.equal(params[k], rparams[k]) for k in params) and torch.equal(beta, rbeta)


# ---- 2. the sampler ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
@pytest.mark.parametrize("state", hr.STATES)
@pytest.mark.parametrize("ns,ni", hr.SIZES)
def test_sampler_with_injected_numbers_against_the_oracle(ns, ni, state, layout):
    wl = _wl(ns, ni, state, layout == "channels_last")
    b = _batch()
    ro, rd, gd, _ = _on(wl.device, b)
    rand = hr.rand_for(ro.shape[0], ns, ni)
    z = _render_z(wl, ro, rd, gd, tuple(t.to(wl.device) for t in rand))
    _check_z_all(z, wl, b, ns, ni, rand, f"sampler injected {ns}+{ni} {state} {layout}")


@pytest.mark.parametrize("state", hr.STATES)
@pytest.mark.parametrize("ns,ni", hr.SIZES)
def test_sampler_with_in_kernel_numbers_against_the_oracle(ns, ni, state):
    """eslam_sample_z_all_rng (the default entry) at two consecutive steps of the counter, against orc.sample_z fed the host
    replica's numbers of that step (tests/rng_ref.py), at the same bars."""
    from myslam_amd import ops
    wl = _wl(ns, ni, state)
    dev = wl.device
    b = _batch()
    ro, rd, gd, _ = _on(dev, b)
    seed = (0xBAD << 32) | (ns * 131 + ni)
    try:
        ops.seed(seed)
        key = ops._rng_seed(dev)
        assert key == rng_ref.key_for(dev, seed) and int(ops._rng_state(dev)[0]) == 0
        zs = []
        for step in range(2):
            assert int(ops._rng_state(dev)[0]) == step
            zs.append(_render_z(wl, ro, rd, gd, None))
    finally:
        ops.seed(None)
    assert not torch.equal(zs[0], zs[1]), "fresh numbers every step"
    for step, z in enumerate(zs):
        nums = tuple(torch.from_numpy(a) for a in rng_ref.sampler_numbers(key, step, ro.shape[0], ns, ni))
        _check_z_all(z, wl, b, ns, ni, nums, f"sampler in-kernel {ns}+{ni} {state} step {step}")


# ---- 3. forward and backward on the kernel's own z_vals ------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
@pytest.mark.parametrize("state", hr.STATES)
@pytest.mark.parametrize("ns,ni", hr.SIZES)
def test_forward_and_backward_against_the_oracle(ns, ni, state, layout):
    wl = _fresh(_wl(ns, ni, state, layout == "channels_last"))
    dev = wl.device
    b = _batch()
    ro, rd, gd, _ = _on(dev, b)
    ro, rd = ro.requires_grad_(True), rd.requires_grad_(True)
    R, S = ro.shape[0], ns + ni
    rand = tuple(t.to(dev) for t in hr.rand_for(R, ns, ni))
    cot = hr.cotangent(R, S)
    depth, color, sdf, z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd, _rand=rand)
    assert z.shape == (R, S) and sdf.shape == (R, S) and depth.shape == (R,) and color.shape == (R, 3)
    ((depth * 0.7).sum() + (color * 0.3).sum() + (sdf * cot.to(dev)).sum()).backward()
    n = lambda t: t.detach().cpu().double().numpy()
    mine = dict(depth=n(depth), color=n(color), sdf=n(sdf), planes=[n(p.grad) for p in wl.plane_list],
                dec={k: n(t.grad) for k, t in wl.decoders.named_parameters()}, ro=n(ro.grad), rd=n(rd.grad))
    for k in ("depth", "color", "sdf", "ro", "rd"):
        assert np.isfinite(mine[k]).all(), k
    mdl = _cpu_model(wl)
    o64, o32 = (hr.oracle_step(mdl, wl.scene, b, z, cot, dt) for dt in (torch.float64, torch.float32))
    pn, amb = hr.ambiguous(mdl, wl.scene, b, z)
    label = f"render {ns}+{ni} {state} {layout}"
    print(f"{label}: ambiguous samples {int(amb.sum())} of {amb.numel()}")
    _margins(label, hr.accept(mine, o32, o64, pn, amb, wl.scene, label=label))
    _fresh(wl)


@pytest.mark.parametrize("state", hr.STATES)
@pytest.mark.parametrize("ns,ni", hr.SIZES)
def test_mixed_precision_forward_against_the_rounding_model(ns, ni, state):
    """The same batch through the fp16-plane / bf16-decoder forward (ops.mixed_precision), against tests/lowp_ref.py on the
    kernel's own z_vals with the criteria test_gpu_lowp_parity.py uses for the fixture of the same state, unchanged."""
    from myslam_amd import lowp, ops
    from tests import lowp_ref as lr
    wl = _fresh(_wl(ns, ni, state))
    dev = wl.device
    b = _batch()
    ro, rd, gd, _ = _on(dev, b)
    rand = tuple(t.to(dev) for t in hr.rand_for(ro.shape[0], ns, ni))
    f = lambda t: t.detach().float().cpu().numpy()
    with ops.mixed_precision(lowp.HalfPlanes(wl.planes)):
        depth, color, sdf, z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd, _rand=rand)
        raw_rgb, feat = sdf.grad_fn.saved_tensors[4], sdf.grad_fn.saved_tensors[5]
        assert feat.dtype == torch.bfloat16 and tuple(feat.shape) == (sdf.numel(), 128)
        got = dict(depth=f(depth), color=f(color), sdf=f(sdf), raw_rgb=f(raw_rgb), feat=f(feat))
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    planes, params, beta = _cpu_model(wl)
    d = lambda t: t.double()
    args = (tuple([d(p) for p in grp] for grp in planes), {k: d(v) for k, v in params.items()}, d(beta), wl.scene.bound,
            d(b.rays_o), d(b.rays_d), d(z.detach().cpu()))
    with torch.no_grad():
        free = {k: v.numpy() for k, v in lr.Model().render(*args).items()}
        ref = {k: v.numpy() for k, v in lr.Model().render(*args, feat=torch.from_numpy(got["feat"])).items()}
    case = lr.TRACKING_FIXTURE if state == "initial" else lr.MIXED_FIXTURES[1]         # initial / trained-like criteria
    lr.assert_agrees(got, ref, b.gt_depth.numpy() > 0, lr.criteria(case, ref), None, free, label=f"lowp {ns}+{ni} {state}")


# ---- 4. a masked ray contributes exactly nothing ---------------------------------------------------------------------------
def _masked_inputs(wl, ns, ni):
    """64 benign rays of the workload followed by all eight hostile classes; the mask selects the benign ones."""
    dev = wl.device
    assert wl.R >= 64
    b = _batch(finite=False)
    ho, hd, hgd, hgc = _on(dev, b)
    ro = torch.cat([wl.rays_o[:64].detach(), ho]).requires_grad_(True)
    rd = torch.cat([wl.rays_d[:64].detach(), hd]).requires_grad_(True)
    gd, gc = torch.cat([wl.gt_depth[:64], hgd]), torch.cat([wl.gt_color[:64], hgc])
    mask = torch.zeros(ro.shape[0], dtype=torch.bool, device=dev)
    mask[:64] = True
    rand = tuple(t.to(dev) for t in hr.rand_for(ro.shape[0], ns, ni, stream=40))
    return ro, rd, gd, gc, mask, rand


def _loss_step(wl, path, ro, rd, gd, gc, mask, rand):
    from myslam_amd import losses
    _fresh(wl)
    r, dev, tau = wl.renderer, wl.device, wl.truncation
    if path == "fused":
        depth, color, sdf, z, pre = r.render_batch_ray_with_loss(wl.planes, wl.decoders, rd, ro, dev, tau, gd, gc, losses.MAPPING_W,
                                                                 ray_mask=mask, _rand=rand)
        loss = losses.mapping_loss(depth, color, sdf, z, gd, gc, tau, precomputed=pre)
    else:
        depth, color, sdf, z = r.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, tau, gt_depth=gd, _rand=rand)
        fn = losses.mapping_loss if path == "mapping" else losses.tracking_loss
        loss = fn(depth, color, sdf, z, gd, gc, tau, ray_mask=mask)
    loss.backward()
    torch.cuda.synchronize()
    out = dict(loss=loss.detach().clone(), planes=[p.grad.detach().clone() for p in wl.plane_list],
               dec={k: t.grad.detach().clone() for k, t in wl.decoders.named_parameters()}, ro=ro.grad.clone(), rd=rd.grad.clone())
    _fresh(wl)
    return out


@pytest.mark.parametrize("path", ["fused", "mapping", "tracking"])
@pytest.mark.parametrize("state", hr.STATES)
@pytest.mark.parametrize("ns,ni", hr.SIZES)
def test_masked_hostile_rays_contribute_exactly_nothing(ns, ni, state, path):
    """64 benign rays + 96 hostile ones (class 8 renders NaN) under a ray_mask that selects the benign rays: loss and every
    gradient finite and equal to rendering the benign rays alone (RTOL, the bar of test_full_size_properties' shard
    equivalence); every 128-byte plane-gradient block only masked rays can reach and the masked rays' own gradients are 0.0."""
    from myslam_amd import ops, parallel
    wl = _wl(ns, ni, state)
    ro, rd, gd, gc, mask, rand = _masked_inputs(wl, ns, ni)
    got = _loss_step(wl, path, ro, rd, gd, gc, mask, rand)
    ro1, rd1 = ro.detach()[:64].clone().requires_grad_(True), rd.detach()[:64].clone().requires_grad_(True)
    ref = _loss_step(wl, path, ro1, rd1, gd[:64], gc[:64], None, tuple(t[:64] for t in rand))
    label = f"masked {path} {ns}+{ni} {state}"
    bad = [k for k, t in [("loss", got["loss"]), ("ro", got["ro"]), ("rd", got["rd"])] + list(got["dec"].items()) +
           [(f"plane {i}", g) for i, g in enumerate(got["planes"])] if not bool(torch.isfinite(t).all())]
    assert not bad, (label, "not finite", bad)
    n = lambda t: t.cpu().double().numpy()
    rep = {"loss": abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"])) / RTOL}
    rep["planes"] = max(hp.rel_err(n(a), n(b)) for a, b in zip(got["planes"], ref["planes"])) / RTOL
    rep["decoders"] = max(hp.rel_err(n(got["dec"][k]), n(ref["dec"][k])) for k in ref["dec"]) / RTOL
    rep["rays_o"] = hp.rel_err(n(got["ro"][:64]), n(ref["ro"])) / RTOL
    rep["rays_d"] = hp.rel_err(n(got["rd"][:64]), n(ref["rd"])) / RTOL
    _margins(label, rep)
    assert max(rep.values()) <= 1.0, (label, rep)
    assert float(got["ro"][64:].abs().max()) == 0.0 and float(got["rd"][64:].abs().max()) == 0.0, (label, "masked rays' gradients")
    # the blocks the benign rays can reach (eslam_mark_rays: a superset) against those the hostile rays can reach as well
    base, n_blocks = hr.block_base(wl.scene)
    b6 = ops.bound_to_host(wl.scene.bound)
    mark = lambda sl: parallel.mark_rays(None, b6, ro.detach()[sl], rd.detach()[sl], gd[sl], wl.truncation, base, n_blocks,
                                         planes=wl.planes).bool()
    benign, hostile = mark(slice(0, 64)), mark(slice(64, None))
    only_masked = hostile & ~benign
    assert int(only_masked.sum()) > 100, int(only_masked.sum())
    rows = torch.cat([g.permute(0, 2, 3, 1).reshape(-1, 32) for g in got["planes"]])
    assert rows.shape[0] == n_blocks
    assert int((rows[~benign] != 0).sum()) == 0, (label, "a masked ray left something in a block only masked rays reach")


# ---- 5. ray marking and the ray-sharded step -------------------------------------------------------------------------------
def test_marking_is_a_tight_superset_of_what_a_backward_touches_per_class():
    """eslam_mark_rays over each of classes 1-7 alone: a superset of the non-zero 128-byte blocks of a real backward (three
    draws of the in-kernel numbers, rays unmasked), equal to the tensor-op mirror up to the MARK_EPS rounding (the bound of
    test_rays_marking_contains_every_block_the_backward_touches), and within 2 texels of the texels the documented interval
    reaches (float64 dense stepping): no whole-plane boxes."""
    from myslam_amd import ops, parallel
    wl = _fresh(_wl(24, 8, "trained"))
    dev, sc = wl.device, wl.scene
    params = wl.plane_list + ops.decoder_params(wl.decoders) + [wl.decoders.beta]
    fg = parallel.FlatGrads(params)
    base, n_blocks = hr.block_base(sc)
    assert base == [fg.offsets[i] // 32 for i in range(12)]
    b6 = ops.bound_to_host(sc.bound)
    g = torch.Generator().manual_seed(3)
    for k in hr.FINITE_CLASSES:
        bk = hr.select(_batch(), (k,))
        ro, rd, gd, _ = _on(dev, bk)
        marked = parallel.mark_rays(None, b6, ro, rd, gd, wl.truncation, base, n_blocks, planes=wl.planes).bool()
        seen = torch.zeros_like(marked)
        for it in range(3):
            fg.flat.zero_()
            cot = [torch.randn(s, generator=g).to(dev) for s in ((12,), (12, 3), (12, 32))]
            with ops.grad_sink(fg):
                depth, color, sdf, z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd)
                ((depth * cot[0]).sum() + (color * cot[1]).sum() + (sdf * cot[2]).sum()).backward()
            nz = (fg.flat[:n_blocks * 32].view(-1, 32) != 0).any(1)
            seen |= nz
            assert int(nz.sum()) > 0
            assert int((nz & ~marked).sum()) == 0, (k, it, int((nz & ~marked).sum()), "texels received gradient without being marked")
        cpu = parallel.mark_rays(hr.plane_hw(sc), b6, bk.rays_o, bk.rays_d, bk.gt_depth, wl.truncation, base, n_blocks).bool()
        diff = int((cpu != marked.cpu()).sum())
        assert diff <= 0.002 * int(marked.sum()) + 4, (k, diff, int(marked.sum()))
        near = hr.dilate(sc, hr.reach_mask(sc, bk), 2)
        assert int((marked.cpu() & ~near).sum()) == 0, (k, int((marked.cpu() & ~near).sum()), int(marked.sum()))
        print(f"margin marking class {k}: marked {int(marked.sum())}, touched in 3 draws {int(seen.sum())}, reached by the interval "
              f"{int(hr.reach_mask(sc, bk).sum())}, device != mirror {diff} (bar {0.002 * int(marked.sum()) + 4:.1f})")
    _fresh(wl)


def test_marking_of_non_finite_rays_stays_in_bounds():
    """Class 8 (exit 0/0): marked in one step by the clamped box - something is marked, and a backward of those rays (NaN
    samples clamp to texel 0 in the kernels) touches nothing outside it."""
    from myslam_amd import ops, parallel
    wl = _fresh(_wl(24, 8, "trained"))
    dev, sc = wl.device, wl.scene
    fg = parallel.FlatGrads(wl.plane_list + ops.decoder_params(wl.decoders) + [wl.decoders.beta])
    base, n_blocks = hr.block_base(sc)
    bk = hr.select(_batch(finite=False), (8,))
    ro, rd, gd, _ = _on(dev, bk)
    marked = parallel.mark_rays(None, ops.bound_to_host(sc.bound), ro, rd, gd, wl.truncation, base, n_blocks, planes=wl.planes).bool()
    assert 0 < int(marked.sum()) <= n_blocks
    with ops.grad_sink(fg):
        depth, color, sdf, z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd)
        (depth.sum() + color.sum() + sdf.sum()).backward()
    touched = (fg.flat[:n_blocks * 32].view(-1, 32) != 0).any(1)               # (NaN != 0 too)
    assert int((touched & ~marked).sum()) == 0, int((touched & ~marked).sum())
    _fresh(wl)


def _hostile_workload(ns, ni):
    """A toy workload whose ray tensors - the whole batch and the (single) rank's slice - are classes 1-7."""
    from myslam_amd import harness
    wl = harness.make_workload("toy", 64, ns, ni, device=_dev(), planes="synth", state="trained")
    ro, rd, gd, gc = _on(wl.device, _batch())
    wl.all_rays_o, wl.all_rays_d, wl.all_gt_depth = ro.clone(), rd.clone(), gd.clone()
    wl.rays_o, wl.rays_d, wl.gt_depth, wl.gt_color = ro, rd, gd, gc
    wl.R = wl.R_total = int(ro.shape[0])
    wl.ray_lo = 0
    wl.renderer.perturb = False
    return wl


def test_sharded_mapper_steps_repeat_on_hostile_rays():
    """ShardedMapper in one process, no optimiser, perturb off, the step counter of the in-kernel numbers held at 0: three
    consecutive steps leave the same plane gradients (2e-5, the bar of test_sharded_mapper_one_rank_rccl), with the block-sparse
    exchange (compact=True: the list-driven clear) and the dense one, and the two agree.  A texel that is scattered to but not
    marked is never cleared in compact mode and doubles on the second step."""
    from myslam_amd import ops
    from myslam_amd.parallel import ShardedMapper
    grads = {}
    try:
        ops.seed(77)
        for compact in (True, False):
            wl = _hostile_workload(24, 8)
            mapper = ShardedMapper(wl, compact=compact)
            assert mapper.compact == compact
            for it in range(3):
                mapper._step.zero_()
                mapper.step()
                torch.cuda.synchronize()
                g = [p.grad.detach().clone() for p in mapper.plane_list]
                assert all(bool(torch.isfinite(t).all()) for t in g) and float(mapper.loss) == float(mapper.loss)
                if it == 0:
                    grads[compact] = g
                    assert sum(int((t != 0).sum()) for t in g) > 1000
                else:
                    worst = max(hp.rel_err(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(g, grads[compact]))
                    print(f"margin sharded step compact={compact}: step {it + 1} vs step 1 {worst / 2e-5:.3f}")
                    assert worst <= 2e-5, (compact, it, worst)
            del mapper
    finally:
        ops.seed(None)
    worst = max(hp.rel_err(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(grads[True], grads[False]))
    print(f"margin sharded step: compact vs dense {worst / 2e-5:.3f}")
    assert worst <= 2e-5, worst


# ---- 6. companions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("need_depth", [False, True])
def test_prefilter_and_aabb_exit_on_the_hostile_batch(need_depth):
    from myslam_amd import ops
    dev = _dev()
    b = _batch(finite=False)
    sc = _wl(24, 8, "initial").scene
    ro, rd, gd, _ = _on(dev, b)
    b6 = ops.bound_to_host(sc.bound)
    t = (sc.bound.unsqueeze(0).to(dev) - ro.unsqueeze(-1)) / rd.unsqueeze(-1)          # Mapper.py:325-327
    t, _ = torch.min(torch.max(t, dim=2)[0], dim=1)
    ref = t >= gd
    if need_depth:
        ref = ref & (gd > 0)
    keep = ops.prefilter(ro, rd, gd, b6, need_depth)
    assert keep.dtype == torch.bool and torch.equal(keep, ref), (keep != ref).nonzero().squeeze(1).tolist()
    assert bool(torch.isnan(t[b.cls.to(dev) == 8]).all()) and 0 < int(ref.sum()) < ref.numel()
    ext = ops.aabb_exit(ro, rd, b6)
    same = (ext == t) | (torch.isnan(ext) & torch.isnan(t))
    assert bool(same.all()), (ext[~same], t[~same])


@pytest.mark.parametrize("ns,ni", hr.SIZES)
def test_loss_set_sizes_on_the_hostile_batch(ns, ni):
    from myslam_amd import ops, parallel
    wl = _wl(ns, ni, "trained")
    dev = wl.device
    b = _batch(finite=False)
    ro, rd, gd, _ = _on(dev, b)
    rand = tuple(t.to(dev) for t in hr.rand_for(ro.shape[0], ns, ni))
    z = _render_z(wl, ro, rd, gd, rand)
    keep = ops.prefilter(ro, rd, gd, ops.bound_to_host(wl.scene.bound), False)
    cs = list(parallel._ACC_COUNT_SLOTS)
    for mask in (None, keep, ~keep):
        acc = ops.loss_set_sizes(gd, mask, ns, ni, wl.truncation, True, t_rand=rand[0])
        want = parallel.set_sizes_from_z(z, gd, wl.truncation, mask)
        assert torch.equal(acc[cs], want[cs]), (acc[cs], want[cs])
        assert float(acc[list(parallel._ACC_SUM_SLOTS)].abs().sum()) == 0.0
