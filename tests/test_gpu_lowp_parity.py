"""The mixed-precision kernels (fp16 plane copies, bf16-MFMA decoders, forward and backward: the LOWP instantiations of
render_fwd_kernel / mlp_bwd_kernel and planes_to_half_kernel) against a reference of THE SAME OPERATION: tests/lowp_ref.py,
the float64 oracle with the kernels' rounding points.  tests/test_lowp_ref.py pins that model on the CPU and shows that the
acceptance criteria used here (lowp_ref.assert_agrees / lowp_ref.criteria) reject one wrong rounding point.

  (a) half copies: bit-exact conversion, stale until refresh, layout check
  (b) saved bf16 features against the model's
  (c) sdf, raw rgb, rgb, depth: the bulk of the samples at float32 level, no sample beyond the tolerance study's bounds
  (d) exact-arithmetic inputs: no rounding has anything to round -> the plain float64 oracle at the float32 parity tolerance
  (e) one training step (separate and fused loss): loss and every gradient against autograd through the model

Every test prints the figures it measured before it asserts (pytest -s); lowp_ref.KERNEL_MEASURED is their place next to the
CPU figures the criteria are built from.
"""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import lowp_ref as lr

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().float().cpu().numpy()


def _kernel_step(fx, label):
    """One mixed-precision call on a fixture's inputs.  label: "separate" / "fused" = a training step with the loss formed
    outside / inside the kernels, "forward" = no loss, no backward (the tracking fixture).  Returns the dict lowp_ref.measure
    takes as `got`, plus z_vals."""
    from myslam_amd import lowp, losses, ops
    from tests.test_gpu_parity import _dev, build
    dev = _dev()
    sc, planes, dec, renderer = build(fx, dec_grad=label != "forward")
    t_rand, t_uni, u = hp.rand_inputs(fx)
    rand = tuple(None if t is None else t.to(dev) for t in (t_rand, t_uni, u))
    ro, rd, gd, gc = (torch.from_numpy(fx[k]).to(dev) for k in ("rays_o", "rays_d", "gt_depth", "gt_color"))
    tr = float(fx["truncation"])
    half = lowp.HalfPlanes(planes)
    with ops.mixed_precision(half):
        if label == "fused":
            depth, color, sdf, z, pre = renderer.render_batch_ray_with_loss(planes, dec, rd, ro, dev, tr, gd, gc, losses.MAPPING_W,
                                                                            _rand=rand)
            loss = pre.loss
        else:
            depth, color, sdf, z = renderer.render_batch_ray(planes, dec, rd, ro, dev, tr, gt_depth=gd, _rand=rand)
            loss = losses.mapping_loss(depth, color, sdf, z, gd, gc, tr) if label == "separate" else None
        saved = sdf.grad_fn.saved_tensors                 # ops.RenderFn.forward: ..., sdf, raw_rgb [R,S,3], feat [R*S,128] bf16, ...
        raw_rgb, feat = saved[4], saved[5]
        assert feat.dtype == torch.bfloat16 and tuple(feat.shape) == (sdf.numel(), 128)
        got = dict(depth=_np(depth), color=_np(color), sdf=_np(sdf), raw_rgb=_np(raw_rgb), feat=_np(feat), z=_np(z))
        if loss is not None:
            loss.backward()
    torch.cuda.synchronize()
    if loss is not None:
        got["loss"] = float(loss)
        got["planes"] = [_np(p.grad) for p in hp.flat_planes(planes)]
        got["dec"] = {k: _np(p.grad) for k, p in dec.named_parameters() if k != "beta"}
        got["beta"] = _np(dec.beta.grad) if bool(fx["beta_is_param"]) else None
    return got


@functools.lru_cache(maxsize=None)
def _case(case):
    """Per fixture, once per module: the kernels' step(s) and the float64 models on the kernels' z_vals."""
    fx = hp.load(case)
    train = str(fx["loss_kind"]) == "mapping"
    runs = {label: _kernel_step(fx, label) for label in (("separate", "fused") if train else ("forward",))}
    first = next(iter(runs.values()))
    for r in runs.values():                               # one forward kernel, whatever forms the loss
        assert np.array_equal(r["z"], first["z"]) and np.array_equal(r["feat"], first["feat"]) and np.array_equal(r["sdf"], first["sdf"])
    z = first["z"]
    free = lr.run_model(lr.Model(), fx, z, backward=False)
    ref = lr.run_model(lr.Model(), fx, z, backward=train, feat=first["feat"])       # teacher-forced with the saved features
    plain = lr.run_model(lr.Model.identity(), fx, z) if train else None
    return fx, runs, free, ref, plain


# ---- (a) half copies ----------------------------------------------------------------------------------------------------
def _assert_half_equals(half, planes):
    for h, p in zip(half.flat, hp.flat_planes(planes)):
        want = p.detach().cpu().half()                    # the conversion on the CPU
        assert h.dtype == torch.float16 and h.stride() == p.stride()
        assert torch.equal(h.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("case", lr.MIXED_FIXTURES)
def test_half_copies_are_the_cpu_conversion_bit_for_bit(case):
    from myslam_amd import lowp
    from tests.test_gpu_parity import _dev
    sc, planes = hp.scene_and_planes(hp.load(case), device=_dev())
    _assert_half_equals(lowp.HalfPlanes(planes), planes)


def test_half_copies_of_edge_values():
    """Half subnormals (plane initial values ~ N(0, 0.01) produce them), ties, +-0, the largest half, values beyond it
    (which become inf, see lowp.py) - in every plane, at its ends and in a partial last vector of the conversion's grid."""
    from myslam_amd import lowp
    from tests.test_gpu_parity import _dev
    dev = _dev()
    edge = torch.tensor([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.5, 2.0 ** -26, 3e-6, -4.1e-6, 6.0e-5,
                         2.0 ** -14, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 65504.0, 65519.0,
                         65520.0, -65520.0, 7e4, -1e30, 1e-30, 0.1])
    g = torch.Generator().manual_seed(3)
    planes = []
    for k in range(6):
        grp = []
        for shape in ((1, 32, 5 + k, 9), (1, 32, 7, 3 + 2 * k)):
            p = torch.randn(shape, generator=g) * 1e-5                    # mostly half subnormals
            flat = p.permute(0, 2, 3, 1).reshape(-1)                      # channels-last order
            p = flat.clone()
            p[:edge.numel()] = edge
            p[-edge.numel():] = edge.flip(0)
            p = p.reshape(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2)
            grp.append(p.to(dev).contiguous(memory_format=torch.channels_last))
        planes.append(grp)
    half = lowp.HalfPlanes(tuple(planes))
    _assert_half_equals(half, planes)
    h0 = half.flat[0].permute(0, 2, 3, 1).reshape(-1)[:edge.numel()].cpu()
    assert torch.isinf(h0[16:20]).all() and torch.isfinite(h0[:16]).all()
    assert (h0.float()[[2, 3, 7, 8]] != 0).all() and (h0.float()[[2, 3, 7, 8]].abs() < 2.0 ** -14).all()      # subnormals kept
    assert torch.equal(h0[:2].view(torch.int16), torch.tensor([0, -32768], dtype=torch.int16))              # +0, -0


def test_half_copies_are_stale_until_refresh():
    from myslam_amd import lowp, optim
    from tests.test_gpu_parity import _dev
    sc, planes = hp.scene_and_planes(hp.load(lr.MIXED_FIXTURES[0]), device=_dev())
    planes = tuple([torch.nn.Parameter(p) for p in grp] for grp in planes)
    half = lowp.HalfPlanes(planes)
    before = [h.clone() for h in half.flat]
    masters = [p.detach().clone() for p in hp.flat_planes(planes)]
    g = torch.Generator(device=_dev()).manual_seed(5)
    for p in hp.flat_planes(planes):
        p.grad = torch.randn(p.shape, device=p.device, generator=g).contiguous(memory_format=torch.channels_last)
    optim.Adam([{"params": hp.flat_planes(planes), "lr": 5e-3}]).step()
    torch.cuda.synchronize()
    changed = [int((h.float() != p.detach().half().float()).sum()) for h, p in zip(half.flat, hp.flat_planes(planes))]
    assert all(not torch.equal(p.detach(), m) for p, m in zip(hp.flat_planes(planes), masters))
    assert all(torch.equal(h, b) for h, b in zip(half.flat, before)), "the step must not touch the copies"
    assert min(changed) > 0, "every copy is stale after the step"
    assert half.refresh(planes) is half
    _assert_half_equals(half, planes)


def test_planes_that_are_not_channels_last_raise():
    from myslam_amd import lowp
    from tests.test_gpu_parity import _dev
    sc, planes = hp.scene_and_planes(hp.load(lr.TRACKING_FIXTURE), device=_dev(), channels_last=False)
    with pytest.raises(RuntimeError, match="channels_last"):
        lowp.HalfPlanes(planes)


def test_ray_gradients_are_refused():
    """Ray / pose gradients are not built on the mixed-precision path: the forward raises rather than return none."""
    from myslam_amd import lowp, ops
    from tests.test_gpu_parity import _dev, build
    fx = hp.load(lr.TRACKING_FIXTURE)
    dev = _dev()
    sc, planes, dec, renderer = build(fx, planes_grad=False, dec_grad=False)
    ro = torch.from_numpy(fx["rays_o"]).to(dev).requires_grad_(True)
    rd = torch.from_numpy(fx["rays_d"]).to(dev)
    gd = torch.from_numpy(fx["gt_depth"]).to(dev)
    t_rand, t_uni, u = hp.rand_inputs(fx)
    rand = tuple(None if t is None else t.to(dev) for t in (t_rand, t_uni, u))
    with ops.mixed_precision(lowp.HalfPlanes(planes)), pytest.raises(RuntimeError, match="rays"):
        renderer.render_batch_ray(planes, dec, rd, ro, dev, float(fx["truncation"]), gt_depth=gd, _rand=rand)


# ---- (b) (c) (e) the fixtures against the model -----------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["separate", "fused"])
@pytest.mark.parametrize("case", lr.MIXED_FIXTURES)
def test_training_step_against_the_model(case, label):
    """Saved features, every sample's sdf and raw rgb, every ray's rgb and depth, the loss and all gradients of one
    mixed-precision mapping step against the float64 model on the same z_vals (criteria: lowp_ref.criteria)."""
    fx, runs, free, ref, plain = _case(case)
    lr.assert_agrees(runs[label], ref, fx["gt_depth"] > 0, lr.criteria(case, ref), plain, free, label=f"{case} {label}")


def test_tracking_forward_against_the_model():
    """Forward only, S = 40 (two and a half 16-point blocks), frozen decoders."""
    case = lr.TRACKING_FIXTURE
    fx, runs, free, ref, plain = _case(case)
    assert "planes" not in runs["forward"]
    lr.assert_agrees(runs["forward"], ref, fx["gt_depth"] > 0, lr.criteria(case, ref), None, free, label=f"{case} forward")


# ---- (d) exact arithmetic ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", lr.EXACT_SHAPES)
def test_exact_arithmetic_inputs_match_the_plain_oracle(R, S):
    """lowp_ref.exact_case: every rounded quantity is representable, so the mixed-precision kernels must give what the float32
    kernels give - the plain float64 oracle at the float32 parity tolerance (OUT_RTOL of the output tensor's largest magnitude,
    and 1e-4 element by element), on EVERY sample; the saved features bit for bit."""
    from myslam_amd import lowp, ops
    from tests.test_gpu_parity import _dev
    from tests.test_oracle_golden import OUT_RTOL
    dev = _dev()
    c = lr.exact_case(R, S)
    planes = tuple([p.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for p in grp] for grp in c["planes"])
    from oracle.eslam_oracle import DECODER_KEYS
    params = [c["params"][k].to(dev) for k in DECODER_KEYS]                 # the C-ABI order of ops.decoder_params
    beta = torch.full((1,), float(c["beta"]), device=dev)
    half = lowp.HalfPlanes(planes)
    with ops.mixed_precision(half):
        depth, rgb, sdf = ops.RenderFn.apply(c["rays_o"].to(dev), c["rays_d"].to(dev), c["z_vals"].to(dev),
                                             ops.bound_to_host(c["bound"]), beta, None, None, *hp.flat_planes(planes), *params)
    torch.cuda.synchronize()
    raw_rgb, feat = sdf.grad_fn.saved_tensors[4], sdf.grad_fn.saved_tensors[5]
    o = {k: v.numpy() for k, v in c["oracle"].items()}
    assert np.array_equal(_np(feat), o["feat"].astype(np.float32)), \
        f"{int((_np(feat) != o['feat']).sum())} of {feat.numel()} saved features differ"
    for name, a in (("sdf", sdf), ("raw_rgb", raw_rgb), ("color", rgb), ("depth", depth)):
        err = hp.rel_err(_np(a), o[name])
        ok, info = hp.elementwise_close(_np(a), o[name], rtol=1e-4, floor=1e-6)
        print(f"exact {R}x{S} {name}: max-normalised error {err:.2e}, element-wise worst / bar {info[1]:.2e}")
        assert err <= OUT_RTOL, (name, err)
        assert ok, (name, info)


# ---- the round-1 wrapper ----------------------------------------------------------------------------------------------------
def test_round1_wrapper_has_the_bits_of_the_general_entry():
    """eslam_render_fwd_lowp (descriptors whose `data` is the half copy) against eslam_render_fwd given the same half copies through
    data_f16, on 64 rays: the three outputs bit for bit - and not the float32 kernel's."""
    import ctypes
    from myslam_amd import _hip, harness, lowp, ops
    from tests.test_gpu_parity import _dev
    dev = _dev()
    wl = harness.Workload("room0", 256, 24, 8, dev, planes="synth", state="trained")
    R, S = 64, 32
    assert wl.R >= R
    with torch.no_grad():
        z = wl.forward()[3][:R].contiguous()
    ro, rd = wl.rays_o.detach()[:R].contiguous(), wl.rays_d.detach()[:R].contiguous()
    half = lowp.HalfPlanes(wl.planes)
    masters = [p.detach() for p in wl.plane_list]
    arr16, _k16 = _hip.make_planes(half.flat, dtype=torch.float16)
    arr_mixed, _km = _hip.make_planes(masters, half=half.flat)
    arr_f32, _kf = _hip.make_planes(masters)
    dec, _kd = _hip.make_decoders(ops.decoder_params(wl.decoders), ops.beta_tensor(wl.decoders.beta, dev))
    bound, st, p, lib = _hip.make_bound(wl.renderer._bound6), _hip.stream_handle(dev), _hip.ptr, _hip.lib()
    new = lambda: (torch.full((R,), -7.25, device=dev), torch.full((R, 3), -7.25, device=dev), torch.full((R, S), -7.25, device=dev))
    a, b, c = new(), new(), new()
    _hip.check(lib.eslam_render_fwd_lowp(arr16, ctypes.byref(dec), bound, p(ro), p(rd), p(z), R, S, p(a[0]), p(a[1]), p(a[2]), st),
               "eslam_render_fwd_lowp")
    for arr, o in ((arr_mixed, b), (arr_f32, c)):
        _hip.check(lib.eslam_render_fwd(arr, ctypes.byref(dec), bound, p(ro), p(rd), p(z), R, S, p(o[0]), p(o[1]), p(o[2]), None, None, None,
                                        None, st), "eslam_render_fwd")
    torch.cuda.synchronize()
    for name, x, y, w in zip(("depth", "rgb", "sdf"), a, b, c):
        assert bool(torch.isfinite(x).all()) and not bool((x == -7.25).any()), name
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (name, int((x != y).sum()))
        assert 0 < hp.rel_err(_np(x), _np(w)) < 1e-2, (name, "the wrapper ran the float32 kernel, or something else")
