"""GPU parity tests proper: the HIP path (through the C-ABI, via the reference-shaped Python API) against
  (1) the committed golden fixtures = outputs of the reference itself, and
  (2) the CPU oracle on the same inputs,
plus size-independent properties at BASELINE.json's full sizes.

Tolerance (north_star): 1e-4 relative, float32 - relative to the largest magnitude of the compared tensor.
z_vals of rays with depth are required to be BIT-EXACT (the sampler reproduces the reference's rounding).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import helpers as hp

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def build(fx, channels_last=True, planes_grad=True, dec_grad=True):
    """Renderer + Decoders + planes on the GPU for a fixture."""
    from myslam_amd.src.networks.decoders import Decoders
    from myslam_amd.src.utils.Renderer import Renderer
    dev = _dev()
    sc, planes = hp.scene_and_planes(fx, device=dev, channels_last=channels_last)
    if planes_grad:
        planes = tuple([torch.nn.Parameter(p) for p in grp] for grp in planes)   # as Mapper.py:254-266
    dec = Decoders(learnable_beta=bool(fx["beta_is_param"]))
    sd = {k[6:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("param:")}
    dec.load_state_dict(sd)
    dec = dec.to(dev)
    dec.bound = sc.bound                                   # CPU tensor, as reference ESLAM.py:173
    for p in dec.parameters():
        p.requires_grad_(dec_grad)
    cfg = sc.cfg(perturb=bool(fx["perturb"]))
    cfg["rendering"]["n_stratified"] = int(fx["n_stratified"])
    cfg["rendering"]["n_importance"] = int(fx["n_importance"])
    eslam = SimpleNamespace(bound=sc.bound, device=dev, H=sc.H, W=sc.W, fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy)
    return sc, planes, dec, Renderer(cfg, eslam)


def run_hip(fx, channels_last=True, rays_grad=True, fused_loss=False):
    from oracle import eslam_oracle as orc
    dev = _dev()
    sc, planes, dec, renderer = build(fx, channels_last)
    t_rand, t_uni, u = hp.rand_inputs(fx)
    rand = tuple(None if t is None else t.to(dev) for t in (t_rand, t_uni, u))
    ro = torch.from_numpy(fx["rays_o"]).to(dev).requires_grad_(rays_grad)
    rd = torch.from_numpy(fx["rays_d"]).to(dev).requires_grad_(rays_grad)
    gd = torch.from_numpy(fx["gt_depth"]).to(dev)
    gc = torch.from_numpy(fx["gt_color"]).to(dev)
    tr = float(fx["truncation"])
    kind = str(fx["loss_kind"])
    if fused_loss == "forward":     # loss sums formed in the forward kernel's epilogue (mapping loss only)
        from myslam_amd import losses
        assert kind == "mapping"
        depth, color, sdf, z, pre = renderer.render_batch_ray_with_loss(planes, dec, rd, ro, dev, tr, gd, gc,
                                                                        losses.MAPPING_W, _rand=rand)
        loss = losses.mapping_loss(depth, color, sdf, z, gd, gc, tr, precomputed=pre)
        loss.backward()
        torch.cuda.synchronize()
        return dict(depth=depth, color=color, sdf=sdf, z=z, loss=loss, ro=ro, rd=rd, dec=dec, planes=planes, pre=pre)
    depth, color, sdf, z = renderer.render_batch_ray(planes, dec, rd, ro, dev, tr, gt_depth=gd, _rand=rand)
    if fused_loss:
        from myslam_amd import losses
        loss = (losses.mapping_loss if kind == "mapping" else losses.tracking_loss)(depth, color, sdf, z, gd, gc, tr)
    else:   # the oracle's torch-op loss runs fine on GPU tensors: it is only the caller-side loss here
        loss = (orc.mapping_loss if kind == "mapping" else orc.tracking_loss)(depth, color, sdf, z, gd, gc, tr)
    loss.backward()
    torch.cuda.synchronize()
    return dict(depth=depth, color=color, sdf=sdf, z=z, loss=loss, ro=ro, rd=rd, dec=dec, planes=planes)


def check_against_fixture(fx, r, rtol=RTOL):
    pr = fx["probe"]
    has = fx["gt_depth"][pr] > 0
    z = r["z"].detach().cpu().numpy()[pr]
    assert np.array_equal(z[has], fx["z_vals"][has]), "z_vals of rays with depth must be bit-exact"
    if (~has).any():
        assert hp.rel_err(z[~has], fx["z_vals"][~has]) <= rtol
    assert hp.rel_err(r["sdf"].detach().cpu().numpy()[pr], fx["sdf"]) <= rtol
    assert hp.rel_err(r["depth"].detach().cpu().numpy()[pr], fx["depth"]) <= rtol
    assert hp.rel_err(r["color"].detach().cpu().numpy()[pr], fx["color"]) <= rtol
    # and element by element: |a - b| <= 1e-4 |b| + 1e-6 max|b| (the max-normalised check above lets small elements off)
    for name, a, b in (("sdf", r["sdf"], fx["sdf"]), ("depth", r["depth"], fx["depth"]), ("color", r["color"], fx["color"])):
        a = a.detach().cpu().numpy()[pr]
        if (~has).any():
            # depth-less rays sit at importance samples that agree to 1e-4, not bit for bit, and what is rendered along them
            # moves with the samples: the element-wise bar is for rays with depth (bit-equal z_vals)
            a, b = a[has], b[has]
        ok, info = hp.elementwise_close(a, b, rtol=rtol, floor=1e-6)
        assert ok, (name, info)
    assert abs(float(r["sdf"].double().sum()) - float(fx["sdf_sum"])) <= rtol * float(r["sdf"].abs().double().sum())
    assert abs(float(r["loss"]) - float(fx["loss"])) <= rtol * abs(float(fx["loss"]))
    for k, p in r["dec"].named_parameters():
        assert p.grad is not None, k
        assert hp.rel_err(p.grad.cpu().numpy(), fx["grad:" + k]) <= rtol, k
        # ... and element by element, with a floor 5x below the max-normalised bar (sums of ~1e5 contributions in float32; a floor
        # of 1e-5 is missed by 2 of 1024 elements of c_linears.0.weight at 4096 x 64 in the trained-like state, at 1.34x the bar)
        ok, info = hp.elementwise_close(p.grad.cpu().numpy(), fx["grad:" + k], rtol=rtol, floor=2e-5)
        assert ok, (k, info)
    assert hp.rel_err(r["ro"].grad.cpu().numpy()[pr], fx["g_rays_o"]) <= rtol
    assert hp.rel_err(r["rd"].grad.cpu().numpy()[pr], fx["g_rays_d"]) <= rtol
    for name, g, ref in (("g_rays_o", r["ro"].grad, fx["g_rays_o"]), ("g_rays_d", r["rd"].grad, fx["g_rays_d"])):
        ok, info = hp.elementwise_close(g.cpu().numpy()[pr][has], ref[has], rtol=rtol, floor=1e-5)
        assert ok, (name, info)
    assert hp.rel_err(r["ro"].grad.double().sum(0).cpu().numpy(), fx["g_rays_o_sum"]) <= rtol
    hp.check_plane_probes(fx, [p.grad for p in hp.flat_planes(r["planes"])], rtol=rtol)


@pytest.mark.parametrize("case", hp.RENDER_CASES)
def test_render_fwd_bwd_matches_reference_fixture(case):
    fx = hp.load(case)
    check_against_fixture(fx, run_hip(fx))


@pytest.mark.parametrize("relayout", [True, False])
@pytest.mark.parametrize("case", ["room0_200x32", "room0_200x40_zero15", "room0_200x40_trained_zero15"])
def test_render_nchw_planes(case, relayout, monkeypatch):
    """Planes exactly as the reference allocates them (NCHW-contiguous, ESLAM.py:199-210).  relayout: per-call channels-last
    scratch copies in front of the kernels and the gradients brought back to the planes' own strides behind them
    (eslam_planes_relayout; the default from 4096 points up); otherwise the strided kernels read / scatter NCHW directly."""
    from myslam_amd import ops
    monkeypatch.setattr(ops, "_RELAYOUT_MIN_POINTS", 0 if relayout else -1)
    fx = hp.load(case)
    r = run_hip(fx, channels_last=False)
    check_against_fixture(fx, r)
    for p in hp.flat_planes(r["planes"]):
        assert p.grad.stride() == p.stride() and p.is_contiguous()


def test_render_nchw_planes_bench_size_equals_channels_last():
    """4096 x 64, trained-like state: NCHW planes through the layout change give the fixture's results, and plane gradients
    equal to the channels-last run's up to the order of the float atomics."""
    fx = hp.load("room0_4096x64_trained_zero10")
    a = run_hip(fx, channels_last=False)
    check_against_fixture(fx, a)
    b = run_hip(fx, channels_last=True)
    for pa, pb in zip(hp.flat_planes(a["planes"]), hp.flat_planes(b["planes"])):
        assert pa.grad.stride() == pa.stride() and pa.is_contiguous()
        assert hp.rel_err(pa.grad.cpu().numpy(), pb.grad.cpu().numpy()) <= 1e-5


def test_planes_relayout_round_trip_and_errors():
    """eslam_planes_relayout: NCHW -> channels-last -> NCHW is the identity bit for bit on odd shapes (tiles of 64 texels with
    ragged ends), both fields; mixed directions and non-dense planes are refused."""
    from myslam_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(3)
    shapes = [(2, 2), (3, 67), (21, 27), (64, 1 + 64), (111, 164), (5, 13), (2, 64), (7, 9), (33, 31), (128, 2), (9, 7), (84, 111)]
    src = [torch.randn(1, 32, h, w, device=dev, generator=g) for h, w in shapes]
    _, cl = ops._flat_views(src, torch.channels_last)
    ops._relayout(src, cl, 0)
    for a, b in zip(src, cl):
        assert b.is_contiguous(memory_format=torch.channels_last) and torch.equal(a, b)
    _, back = ops._flat_views(src, torch.contiguous_format)
    ops._relayout(cl, back, 1)
    for a, b in zip(src, back):
        assert b.is_contiguous() and torch.equal(a, b)
    with pytest.raises(RuntimeError, match="same way"):
        ops._relayout([src[0]] + cl[1:], [cl[0]] + back[1:], 0)
    with pytest.raises(RuntimeError, match="dense"):
        ops._relayout(src, back, 0)


@pytest.mark.parametrize("case", ["room0_200x32", "room0_200x40_zero15", "room0_200x40_tracking", "room0_200x40_trained_zero15"])
def test_fused_loss_matches(case):
    fx = hp.load(case)
    check_against_fixture(fx, run_hip(fx, fused_loss=True))


@pytest.mark.parametrize("case", ["room0_200x32", "room0_200x40_zero15", "room0_200x40_trained_zero15"])
def test_full_gradients_vs_oracle(case):
    """Every element of every gradient (not only fixture probes) against autograd over the float64 oracle.  In the
    trained-like state float32 round-off is amplified by the loss's 200x-weighted terms (the float32 ORACLE is 5e-4 from the
    float64 one on a plane gradient there), so the comparator is the float32 oracle - the reference's arithmetic - and the
    float64 one bounds it, as in test_random_configurations_against_oracle."""
    from tests.test_oracle_golden import run_oracle
    fx = hp.load(case)
    r = run_hip(fx)
    o = run_oracle(fx, torch.float64)
    o32 = run_oracle(fx, torch.float32) if "trained" in case else None
    assert hp.rel_err(r["sdf"].detach().cpu().numpy(), o["sdf"].detach().numpy()) <= RTOL
    assert hp.rel_err(r["depth"].detach().cpu().numpy(), o["depth"].detach().numpy()) <= RTOL
    assert hp.rel_err(r["color"].detach().cpu().numpy(), o["color"].detach().numpy()) <= RTOL

    def close(a, b64, b32):
        if b32 is None:
            return hp.rel_err(a, b64.numpy()) <= RTOL
        return (hp.rel_err(a, b32.double().numpy()) <= RTOL and
                hp.rel_err(a, b64.numpy()) <= max(RTOL, 1.5 * hp.rel_err(b32.double().numpy(), b64.numpy())))

    if o32 is None:
        for k, (a, b) in enumerate(zip(hp.flat_planes(r["planes"]), hp.flat_planes(o["planes"]))):
            assert close(a.grad.cpu().numpy(), b.grad, None), k
    else:
        from oracle import eslam_oracle as orc
        from myslam_amd import scene as scn
        sc = scn.make_scene(str(fx["scene"]))
        pts = (o["ro"].detach()[:, None, :] + o["rd"].detach()[:, None, :] * o["z"].detach()[..., None]).reshape(-1, 3)
        pn = orc.normalize_points(pts, sc.bound.double())
        amb = hp.ambiguous_samples(pn, tuple([p.detach() for p in grp] for grp in o["planes"]),
                                   {k: v.detach() for k, v in o["params"].items()})
        ok, msg = hp.plane_grads_close([p.grad.cpu().numpy() for p in hp.flat_planes(r["planes"])],
                                       [p.grad.numpy() for p in hp.flat_planes(o32["planes"])],
                                       [p.grad.numpy() for p in hp.flat_planes(o["planes"])], pn, amb, sc.plane_shapes, RTOL)
        assert ok, (msg, int(amb.sum()))
    assert close(r["ro"].grad.cpu().numpy(), o["ro"].grad, o32["ro"].grad if o32 else None)
    assert close(r["rd"].grad.cpu().numpy(), o["rd"].grad, o32["rd"].grad if o32 else None)
    if bool(fx["beta_is_param"]):
        assert close(r["dec"].beta.grad.cpu().numpy(), o["beta"].grad, o32["beta"].grad if o32 else None)


@pytest.mark.parametrize("case", ["room0_4096x64_trained_zero10", "scene0000_8192x96_zero10"])
def test_whole_gradient_tensors_at_full_size(case):
    """EVERY element of all 12 plane gradients at the BASELINE sizes (4096 x 64 in the trained-like state with 10 % depth-less
    rays; 8192 x 96 on scene0000) against autograd over the float32 oracle run on this box's host cores, the float64 oracle as
    the conditioning bound (helpers.plane_grads_close) - the scatter's full-size paths (1536 workgroups in two rounds, the
    XCD map, counting sort and bitonic fallback) seen through whole tensors, not norms and probes.  Decoder, beta and ray
    gradients element by element (|a - b| <= 1e-4 |b| + floor * max|b|) beside the max-normalised bar."""
    from oracle import eslam_oracle as orc
    from myslam_amd import scene as scn
    from tests.test_oracle_golden import run_oracle
    fx = hp.load(case)
    r = run_hip(fx)
    o32 = run_oracle(fx, torch.float32)
    o64 = run_oracle(fx, torch.float64)
    sc = scn.make_scene(str(fx["scene"]))
    pts = (o64["ro"].detach()[:, None, :] + o64["rd"].detach()[:, None, :] * o64["z"].detach()[..., None]).reshape(-1, 3)
    pn = orc.normalize_points(pts, sc.bound.double())
    amb = hp.ambiguous_samples(pn, tuple([p.detach() for p in grp] for grp in o64["planes"]),
                               {k: v.detach() for k, v in o64["params"].items()})
    ok, msg = hp.plane_grads_close([p.grad.cpu().numpy() for p in hp.flat_planes(r["planes"])],
                                   [p.grad.numpy() for p in hp.flat_planes(o32["planes"])],
                                   [p.grad.numpy() for p in hp.flat_planes(o64["planes"])], pn, amb, sc.plane_shapes, RTOL)
    assert ok, (msg, int(amb.sum()))
    assert int(amb.sum()) <= 2e-3 * amb.numel()               # the exclusion stays an exception

    elementwise = lambda name, a, b32, b64, floor: hp.elementwise_vs_oracles(name, a, b32, b64, floor, RTOL)
    # floor: 3e-5 of the tensor's largest element - these are float32 sums of 2.6e5 - 7.9e5 float-atomic / MFMA-ordered
    # contributions; at 1e-5, 2 of the 1024 elements of c_linears.0.weight miss by 1.34x (4096 x 64, trained-like state)
    for k, p in r["dec"].named_parameters():
        if k == "beta":
            continue
        elementwise(k, p.grad.cpu().numpy(), o32["params"][k].grad.numpy(), o64["params"][k].grad.numpy(), 3e-5)
    if bool(fx["beta_is_param"]):
        elementwise("beta", r["dec"].beta.grad.cpu().numpy(), o32["beta"].grad.numpy(), o64["beta"].grad.numpy(), 3e-5)
    # rays: those with depth (depth-less rays sit at importance samples that agree to 1e-4 only) and without a ReLU-ambiguous
    # sample (such a sample's whole contribution legitimately differs between two float32 evaluations: helpers.ambiguous_samples)
    has = (fx["gt_depth"] > 0) & ~amb.view(o64["z"].shape).any(1).numpy()
    elementwise("rays_o", r["ro"].grad.cpu().numpy()[has], o32["ro"].grad.numpy()[has], o64["ro"].grad.numpy()[has], 3e-5)
    elementwise("rays_d", r["rd"].grad.cpu().numpy()[has], o32["rd"].grad.numpy()[has], o64["rd"].grad.numpy()[has], 3e-5)


@pytest.mark.parametrize("case", ["room0_200x32", "room0_200x40_zero15", "room0_4096x64", "scene0000_8192x96_zero10",
                                  "room0_200x40_trained_zero15", "room0_4096x64_trained_zero10"])
def test_loss_sums_in_the_forward_epilogue(case):
    """eslam_render_fwd_loss: the forward kernel forms the loss sums itself; value, accumulators and every gradient must
    match the reference fixture and the separate eslam_loss_value launch."""
    from myslam_amd import ops
    fx = hp.load(case)
    r = run_hip(fx, fused_loss="forward")
    check_against_fixture(fx, r)
    acc_sep = ops.loss_reduce(r["depth"], r["color"], r["sdf"], r["z"], torch.from_numpy(fx["gt_depth"]).to(_dev()),
                              torch.from_numpy(fx["gt_color"]).to(_dev()), float(fx["truncation"]))
    a, b = r["pre"].acc.cpu().numpy()[:10], acc_sep.cpu().numpy()[:10]
    assert np.array_equal(a[[0, 1, 2, 6, 9]], b[[0, 1, 2, 6, 9]])                  # set sizes: exact
    assert hp.rel_err(a, b) <= 1e-5                                               # error sums: summation order only


def test_tracking_mode_pose_gradients_only():
    """Tracker.py:111-112,222-232: decoders frozen, planes detached - only rays carry gradient."""
    fx = hp.load("room0_200x40_tracking")
    dev = _dev()
    sc, planes, dec, renderer = build(fx, planes_grad=False, dec_grad=False)
    t_rand, _, _ = hp.rand_inputs(fx)
    ro = torch.from_numpy(fx["rays_o"]).to(dev).requires_grad_(True)
    rd = torch.from_numpy(fx["rays_d"]).to(dev).requires_grad_(True)
    gd = torch.from_numpy(fx["gt_depth"]).to(dev)
    gc = torch.from_numpy(fx["gt_color"]).to(dev)
    from myslam_amd import losses
    depth, color, sdf, z = renderer.render_batch_ray(planes, dec, rd, ro, dev, float(fx["truncation"]), gt_depth=gd,
                                                     _rand=(t_rand.to(dev), None, None))
    losses.tracking_loss(depth, color, sdf, z, gd, gc, float(fx["truncation"])).backward()
    pr = fx["probe"]
    assert hp.rel_err(ro.grad.cpu().numpy()[pr], fx["g_rays_o"]) <= RTOL
    assert hp.rel_err(rd.grad.cpu().numpy()[pr], fx["g_rays_d"]) <= RTOL
    assert all(p.grad is None for p in dec.parameters())


def test_get_samples_and_get_rays():
    from myslam_amd import scene as scn, synth
    from myslam_amd.src import common
    dev = _dev()
    fx = hp.load("get_samples_room0_b3")
    sc = scn.make_scene("room0")
    b, n = int(fx["b"]), int(fx["n"])
    H0, H1, W0, W1 = (int(v) for v in fx["window"])
    call = fx["rand_calls"].tolist()[0].split(";")
    idx = torch.from_numpy(synth.hash_randint(int(call[2]), (b * n,), int(call[1]))).to(dev)
    depth_img = torch.from_numpy(np.stack([synth.depth_image(sc.H, sc.W, 20 + i) for i in range(b)])).to(dev)
    color_img = torch.from_numpy(np.stack([synth.color_image(sc.H, sc.W, 30 + i) for i in range(b)])).to(dev)
    c2ws = torch.from_numpy(fx["c2ws"]).to(dev).requires_grad_(True)
    ro, rd, d, c = common.get_samples_at(idx, H0, H1, W0, W1, n, sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy, c2ws,
                                         depth_img, color_img)
    assert np.array_equal(d.cpu().numpy(), fx["depth"]) and np.array_equal(c.cpu().numpy(), fx["color"])
    assert np.array_equal(ro.detach().cpu().numpy(), fx["rays_o"])
    assert hp.rel_err(rd.detach().cpu().numpy(), fx["rays_d"]) <= 1e-6
    wo = torch.from_numpy(synth.hash_uniform(tuple(ro.shape), 61_000)).to(dev) - 0.5
    wd = torch.from_numpy(synth.hash_uniform(tuple(rd.shape), 61_001)).to(dev) - 0.5
    ((ro * wo).sum() + (rd * wd).sum()).backward()
    assert hp.rel_err(c2ws.grad.cpu().numpy(), fx["g_c2ws"]) <= 1e-5
    # the public entry draws its own indices: shapes, ranges, determinism under manual_seed
    torch.manual_seed(1)
    a = common.get_samples(H0, H1, W0, W1, n, sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy, c2ws.detach(), depth_img,
                           color_img, dev)
    torch.manual_seed(1)
    b2 = common.get_samples(H0, H1, W0, W1, n, sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy, c2ws.detach(), depth_img,
                            color_img, dev)
    assert a[0].shape == (b * n, 3) and a[2].shape == (b * n,) and all(torch.equal(x, y) for x, y in zip(a, b2))
    # whole-image rays
    fr = hp.load("get_rays_room0")
    ro_i, rd_i = common.get_rays(sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy, torch.from_numpy(fr["c2w"]), dev)
    assert ro_i.shape == (sc.H, sc.W, 3)
    sel = fr["sel"]
    assert hp.rel_err(ro_i.reshape(-1, 3).cpu().numpy()[sel], fr["rays_o"]) <= 1e-7
    assert hp.rel_err(rd_i.reshape(-1, 3).cpu().numpy()[sel], fr["rays_d"]) <= 1e-6


def test_decoders_forward_and_backward():
    """Decoders.forward on free points incl. points outside the AABB (border clamp): fixture + oracle autograd."""
    from myslam_amd import scene as scn
    from myslam_amd.src.networks.decoders import Decoders
    from oracle import eslam_oracle as orc
    dev = _dev()
    fx = hp.load("decoders_room0_points")
    sc = scn.make_scene("room0")
    planes = scn.synth_planes(sc, device=dev)
    planes = tuple([p.requires_grad_(True) for p in grp] for grp in planes)
    dec = Decoders()
    dec.load_state_dict({k[6:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("param:")})
    dec = dec.to(dev)
    dec.bound = sc.bound
    p = torch.from_numpy(fx["points"]).to(dev).requires_grad_(True)
    raw = dec(p.reshape(40, 50, 3), all_planes=planes)        # keyword form used by Mesher.py:151
    assert raw.shape == (40, 50, 4)
    assert hp.rel_err(raw.detach().reshape(-1, 4).cpu().numpy(), fx["raw"]) <= RTOL
    wts = torch.linspace(0.5, 1.5, raw.numel(), device=dev).reshape(raw.shape)
    (raw * wts).sum().backward()
    # oracle, float64
    cp = scn.synth_planes(sc, dtype=torch.float64, channels_last=False)
    cp = tuple([q.requires_grad_(True) for q in grp] for grp in cp)
    params = hp.params_from(fx, dtype=torch.float64, requires_grad=True)
    p64 = torch.from_numpy(fx["points"]).double().requires_grad_(True)
    raw64 = orc.decode(p64, cp, params, sc.bound.double())
    (raw64 * wts.cpu().double().reshape(-1, 4)).sum().backward()
    assert hp.rel_err(p.grad.cpu().numpy(), p64.grad.numpy()) <= RTOL
    for a, b in zip(hp.flat_planes(planes), hp.flat_planes(cp)):
        assert hp.rel_err(a.grad.cpu().numpy(), b.grad.numpy()) <= RTOL
    for k, t in dec.named_parameters():
        if k != "beta":
            assert hp.rel_err(t.grad.cpu().numpy(), params[k].grad.numpy()) <= RTOL, k
    # get_raw_sdf on normalised coordinates, no-grad path (Renderer.py:124-125 style)
    with torch.no_grad():
        pn = torch.from_numpy(fx["p_nor"]).to(dev)
        sdf = dec.get_raw_sdf(pn, planes)
    assert hp.rel_err(sdf.cpu().numpy(), fx["raw"][:, 3]) <= RTOL


def test_decoders_backward_with_frozen_decoders():
    """The free-point backward without weight gradients (mlp_bwd_kernel<0, false, ...>, g_dec NULL) on 70 points - two tiles, the
    second with 6 points: point and plane gradients against oracle autograd, as in test_decoders_forward_and_backward."""
    from myslam_amd import scene as scn
    from myslam_amd.src.networks.decoders import Decoders
    from oracle import eslam_oracle as orc
    dev = _dev()
    fx = hp.load("decoders_room0_points")
    n = 70
    sc = scn.make_scene("room0")
    planes = scn.synth_planes(sc, device=dev)
    planes = tuple([p.requires_grad_(True) for p in grp] for grp in planes)
    dec = Decoders()
    dec.load_state_dict({k[6:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("param:")})
    dec = dec.to(dev)
    dec.bound = sc.bound
    for t in dec.parameters():
        t.requires_grad_(False)
    p = torch.from_numpy(fx["points"][:n]).to(dev).requires_grad_(True)
    raw = dec(p, all_planes=planes)
    assert raw.shape == (n, 4)
    assert hp.rel_err(raw.detach().cpu().numpy(), fx["raw"][:n]) <= RTOL
    wts = torch.linspace(0.5, 1.5, raw.numel(), device=dev).reshape(raw.shape)
    (raw * wts).sum().backward()
    assert all(t.grad is None for t in dec.parameters())
    cp = scn.synth_planes(sc, dtype=torch.float64, channels_last=False)
    cp = tuple([q.requires_grad_(True) for q in grp] for grp in cp)
    params = hp.params_from(fx, dtype=torch.float64, requires_grad=False)
    p64 = torch.from_numpy(fx["points"][:n]).double().requires_grad_(True)
    raw64 = orc.decode(p64, cp, params, sc.bound.double())
    (raw64 * wts.cpu().double()).sum().backward()
    assert np.abs(p64.grad.numpy()).max() > 0
    assert hp.rel_err(p.grad.cpu().numpy(), p64.grad.numpy()) <= RTOL
    for a, b in zip(hp.flat_planes(planes), hp.flat_planes(cp)):
        assert np.abs(b.grad.numpy()).max() > 0
        assert hp.rel_err(a.grad.cpu().numpy(), b.grad.numpy()) <= RTOL


def _bench_like(R, n_strat, n_imp, scene="room0", zero_frac=0.0, seed=0):
    from myslam_amd import harness
    return harness.make_workload(scene, R, n_strat, n_imp, device=_dev(), zero_frac=zero_frac, seed=seed)


@pytest.mark.parametrize("cfg", [("room0", 4096, 56, 8, 0.0), ("scene0000", 8192, 88, 8, 0.1)])
def test_full_size_properties(cfg):
    """Size-independent properties at BASELINE.json sizes: sorted z, weights in [0,1] => depth inside the sampled
    range and colour inside [0,1]; linearity of the backward pass in the upstream gradient; ray-shard equivalence
    (1 shard == sum of 4 shards), which is exactly what the multi-GPU path relies on."""
    scene, R, ns, ni, zf = cfg
    wl = _bench_like(R, ns, ni, scene, zf)
    dev = _dev()
    out = wl.forward()
    depth, color, sdf, z = out
    assert torch.all(z[:, 1:] >= z[:, :-1]), "z_vals must be ascending"
    assert torch.all(color >= 0) and torch.all(color <= 1 + 1e-6)
    assert torch.all(depth >= torch.clamp(z[:, 0], max=0) - 1e-5) and torch.all(depth <= z[:, -1] + 1e-5)
    assert torch.all(sdf.abs() <= 1)
    # linearity: bwd(2 g) == 2 bwd(g)
    g1 = wl.backward_with(out, scale=1.0)
    g2 = wl.backward_with(wl.forward(), scale=2.0)
    for a, b in zip(g1, g2):
        assert hp.rel_err((2 * a).cpu().numpy(), b.cpu().numpy()) <= 5e-5   # float atomics: order-dependent rounding
    # shard equivalence
    acc = None
    for k in range(4):
        gs = wl.backward_with(wl.forward(shard=(k, 4)), scale=1.0, shard=(k, 4))
        acc = gs if acc is None else [x + y for x, y in zip(acc, gs)]
    for a, b in zip(g1, acc):
        assert hp.rel_err(a.cpu().numpy(), b.cpu().numpy()) <= RTOL


def test_render_img_shapes_and_dtype():
    from myslam_amd import harness
    wl = _bench_like(64, 32, 8)
    r = wl.renderer
    r.H, r.W = 48, 64                      # small image, same intrinsics
    gt = torch.full((48, 64), 1.5, device=_dev())
    depth, color = r.render_img(wl.planes, wl.decoders, wl.c2w.to(_dev()), wl.truncation, _dev(), gt_depth=gt)
    assert depth.dtype == torch.float64 and depth.shape == (48, 64) and color.shape == (48, 64, 3)
    assert torch.isfinite(depth).all() and torch.isfinite(color).all()


@pytest.mark.parametrize("channels_last", [True, False])
def test_render_img_matches_reference_fixture(channels_last):
    """Renderer.render_img (src/utils/Renderer.py:155-204) against outputs of the reference itself: three chunks of its
    ray batching with a ragged last one, 58 depth-less pixels (importance branch), perturbation on, rotated camera."""
    from types import SimpleNamespace
    from myslam_amd import scene as scn, synth
    from myslam_amd.src.networks.decoders import Decoders
    from myslam_amd.src.utils.Renderer import Renderer
    fx = hp.load("render_img_room0_30x44")
    dev = _dev()
    sc = scn.make_scene("room0")
    planes = scn.synth_planes(sc, device=dev, channels_last=channels_last)
    dec = Decoders(learnable_beta=True).to(dev)
    dec.load_state_dict({k: v.to(dev) for k, v in hp.params_from(fx).items()} | {"beta": torch.tensor([10.0], device=dev)})
    dec.bound = sc.bound
    H, W = int(fx["H"]), int(fx["W"])
    cfg = sc.cfg(perturb=True)
    cfg["rendering"]["n_stratified"], cfg["rendering"]["n_importance"] = int(fx["n_stratified"]), int(fx["n_importance"])
    eslam = SimpleNamespace(bound=sc.bound, device=dev, H=H, W=W, fx=float(fx["fx"]), fy=float(fx["fy"]),
                            cx=float(fx["cx"]), cy=float(fx["cy"]))
    r = Renderer(cfg, eslam, ray_batch_size=int(fx["ray_batch_size"]))
    gd = torch.from_numpy(synth.depth_image(H, W, int(fx["depth_stream"]), float(fx["zero_frac"])))
    rands = [tuple(None if t is None else t.to(dev) for t in ch) for ch in hp.render_img_chunk_rands(fx, gd.reshape(-1).numpy())]
    depth, color = r.render_img(planes, dec, torch.from_numpy(fx["c2w"]).to(dev), float(fx["truncation"]), dev,
                                gt_depth=gd.to(dev), _rand_chunks=rands)
    assert depth.dtype == torch.float64 and tuple(depth.shape) == (H, W) and tuple(color.shape) == (H, W, 3)
    assert hp.rel_err(depth.cpu().numpy(), fx["depth"]) <= RTOL
    assert hp.rel_err(color.cpu().numpy(), fx["color"]) <= RTOL
    has = (gd > 0).numpy()
    ok, info = hp.elementwise_close(depth.cpu().numpy()[has], fx["depth"][has], rtol=RTOL)
    assert ok, info
    ok, info = hp.elementwise_close(color.cpu().numpy()[has], fx["color"][has], rtol=RTOL, floor=1e-5)
    assert ok, info


def test_plane_gradient_buffers_are_reused_only_when_nobody_holds_them():
    """ops._alloc_plane_grads hands the previous iteration's flat gradient buffer + its 12 views out again when the caller
    has dropped them (13 tensor constructions less per eager iteration); gradients somebody still holds, and a forward pass
    whose backward has not run yet, get buffers of their own."""
    from myslam_amd import harness
    dev = _dev()
    wl = harness.make_workload("room0", 300, 24, 8, device=dev, planes="synth", state="trained")
    wl.renderer.perturb = False
    wl.step()
    g1 = [p.grad for p in wl.plane_list]
    ptr1 = g1[0].data_ptr()
    ref = [g.clone() for g in g1]
    wl.step()                                     # g1 still referenced here: a fresh buffer, the old values untouched
    assert wl.plane_list[0].grad.data_ptr() != ptr1
    for a, b in zip(g1, ref):
        assert torch.equal(a, b)
    del g1
    for p in wl.params():
        p.grad = None
    held = wl.plane_list[0].grad
    wl.step()
    ptr2 = wl.plane_list[0].grad.data_ptr()
    for p in wl.params():
        p.grad = None
    wl.step()                                     # nothing held: the same memory again, same gradients
    assert wl.plane_list[0].grad.data_ptr() == ptr2
    for a, b in zip([p.grad for p in wl.plane_list], ref):
        assert hp.rel_err(a.cpu().numpy(), b.cpu().numpy()) <= 1e-5
    # two forward passes, then their two backward passes: each needs a buffer of its own
    for p in wl.params():
        p.grad = None
    outs = [wl.forward(fixed_rand=False) for _ in range(2)]
    for o in outs:
        (o[0].sum() + o[1].sum()).backward()
    twice = [p.grad.clone() for p in wl.plane_list]
    for p in wl.params():
        p.grad = None
    o = wl.forward(fixed_rand=False)
    (o[0].sum() + o[1].sum()).backward()
    for a, b in zip(twice, [p.grad for p in wl.plane_list]):
        assert hp.rel_err(a.cpu().numpy(), 2 * b.cpu().numpy()) <= 1e-5


@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
def test_compiled_host_glue_equals_python_path(layout, monkeypatch):
    """eslam_torch_ext (one compiled call for ray order + clear + sampler + forward, one for the backward) against the Python /
    ctypes glue it shortcuts: same kernels, same random numbers (seed, step, ray index), so the outputs are bit-identical and
    the gradients equal up to the order of the float atomics - fused loss, separate loss with a ray mask, pose-only gradients
    (tracking), and a no_grad call."""
    from myslam_amd import harness, losses, ops
    if ops.torch_ext() is None:
        pytest.skip("eslam_torch_ext is not built (make -C myslam_amd/csrc torch_ext)")
    dev = _dev()
    ext = ops.torch_ext()

    def run(use_ext, mode):
        monkeypatch.setattr(ops, "_ext_mod", ext if use_ext else None)
        wl = harness.make_workload("room0", 1500, 32, 8, device=dev, zero_frac=0.1, state="trained", channels_last=(layout == "channels_last"),
                                   rays_grad=(mode == "tracking"))
        ops.seed(77)
        if mode == "tracking":
            for p in wl.decoders.parameters():
                p.requires_grad_(False)
            planes = tuple([p.detach() for p in grp] for grp in wl.planes)
        else:
            planes = wl.planes
        g = torch.Generator().manual_seed(1)
        mask = (torch.rand(wl.R, generator=g) > 0.2).to(dev)
        if mode == "no_grad":
            with torch.no_grad():
                d, c, s, z = wl.renderer.render_batch_ray(planes, wl.decoders, wl.rays_d, wl.rays_o, dev, wl.truncation, gt_depth=wl.gt_depth)
            return [d, c, s, z], []
        if mode == "fused":
            d, c, s, z, pre = wl.renderer.render_batch_ray_with_loss(planes, wl.decoders, wl.rays_d, wl.rays_o, dev, wl.truncation, wl.gt_depth,
                                                                     wl.gt_color, losses.MAPPING_W, ray_mask=mask)
            loss = losses.mapping_loss(d, c, s, z, wl.gt_depth, wl.gt_color, wl.truncation, precomputed=pre)
        else:
            d, c, s, z = wl.renderer.render_batch_ray(planes, wl.decoders, wl.rays_d, wl.rays_o, dev, wl.truncation, gt_depth=wl.gt_depth)
            loss = (losses.tracking_loss if mode == "tracking" else losses.mapping_loss)(d, c, s, z, wl.gt_depth, wl.gt_color, wl.truncation,
                                                                                      ray_mask=mask)
        loss.backward()
        leaves = [wl.rays_o, wl.rays_d] if mode == "tracking" else wl.params()
        assert all(p.grad is not None for p in leaves)
        if mode != "tracking":
            assert all(p.grad.stride() == p.stride() for p in wl.plane_list)
        return [d, c, s, z, loss], [p.grad.clone() for p in leaves]
    try:
        for mode in ("fused", "separate", "tracking", "no_grad"):
            oa, ga = run(True, mode)
            ob, gb = run(False, mode)
            for a, b in zip(oa[:4], ob[:4]):
                assert torch.equal(a.detach(), b.detach()), mode
            if len(oa) > 4:                               # (the loss's sums are float atomics over the workgroups: last bits)
                assert abs(float(oa[4]) - float(ob[4])) <= 1e-6 * abs(float(ob[4])), mode
            for a, b in zip(ga, gb):
                assert hp.rel_err(a.cpu().numpy(), b.cpu().numpy()) <= 1e-5, mode
    finally:
        ops.seed(None)


def test_cpu_tensors_fail_loudly():
    fx = hp.load("room0_200x32")
    sc, planes, dec, renderer = build(fx)
    ro = torch.from_numpy(fx["rays_o"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        renderer.render_batch_ray(planes, dec, ro, ro, "cpu", 0.06, gt_depth=torch.from_numpy(fx["gt_depth"]))


def test_sharded_mapper_one_rank_rccl():
    """parallel.ShardedMapper over a 1-rank RCCL group: the flat-buffer gradient path (loss phases + all-reduce + grad
    sink) must give the same gradients as the plain autograd path.  (N > 1 is covered by the 2-rank gloo test on the CPU
    and by test_full_size_properties' shard equivalence; one GPU cannot host two RCCL ranks.)"""
    import os
    import socket
    import torch.distributed as dist
    from myslam_amd import harness, losses
    from myslam_amd.parallel import ShardedMapper
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = _dev()
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        wl = harness.make_workload("room0", 512, 32, 8, device=dev, planes="synth")
        wl.renderer.perturb = False                     # same z_vals in both runs
        mapper = ShardedMapper(wl)
        mapper.step()
        loss_dp = mapper.loss
        g_dp = [p.grad.detach().clone() for p in mapper.params]
        loss = wl.step()
        g_ref = [p.grad.detach().clone() for p in mapper.params]
        assert abs(float(loss_dp) - float(loss)) <= 1e-6 * abs(float(loss))
        for a, b in zip(g_dp, g_ref):
            assert a.stride() == b.stride()
            assert hp.rel_err(a.cpu().numpy(), b.cpu().numpy()) <= 2e-5
        # the same step as two captured hipGraphs with the all-reduces between the replays
        mapper.capture()
        for _ in range(2):
            mapper.step()
        loss_g = mapper.loss
        torch.cuda.synchronize()
        assert abs(float(loss_g) - float(loss)) <= 1e-6 * abs(float(loss))
        for p, b in zip(mapper.params, g_ref):
            assert hp.rel_err(p.grad.cpu().numpy(), b.cpu().numpy()) <= 2e-5
        # with the optimiser in the loop (third graph; the step clears the flat gradient buffer it consumed):
        # 3 eager + 3 replayed iterations == 6 iterations of the plain single-GPU loop with the same Adam
        from myslam_amd import optim
        wa = harness.make_workload("room0", 512, 32, 8, device=dev, planes="synth")
        wb = harness.make_workload("room0", 512, 32, 8, device=dev, planes="synth")
        wa.renderer.perturb = wb.renderer.perturb = False
        ma = ShardedMapper(wa)
        ma.make_optimizer(fused_zero_grad=True, capturable=True)
        for _ in range(3):
            ma.step()
        ma.capture(warmup=0)
        for _ in range(3):
            ma.step()
        la = ma.loss
        torch.cuda.synchronize()
        assert float(ma.grads.flat[:ma.grads.offsets[-1]].abs().max()) == 0.0      # consumed gradients were cleared in the Adam pass
        dec_b = list(wb.decoders.parameters())
        ob = optim.Adam([{"params": dec_b, "lr": 0.001}, {"params": wb.plane_list[:6], "lr": 0.005},
                         {"params": wb.plane_list[6:], "lr": 0.005}])
        for _ in range(6):
            lb = wb.step()
            ob.step()
        # 1e-4 / 3e-4 (commit a6bd2ae widened them from 1e-5): the run-to-run noise of the float atomics' last bits, amplified by
        # Adam for near-zero gradients (lr * dg / eps per step), is heavy-tailed - 1.6e-6 in one run of these 6 steps, 1.0e-5
        # in the next.  tests/test_gpu_determinism.py shows that it IS noise: with ESLAM_DETERMINISTIC=1 the two loops agree
        # bit for bit (0.0 <= 1e-5).
        assert abs(float(la) - float(lb)) <= 1e-4 * abs(float(lb))
        for a, b in zip(wa.params(), wb.params()):
            assert hp.rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy()) <= 3e-4
    finally:
        dist.destroy_process_group()


def test_mesher_eval_points_against_oracle():
    """Mesher.eval_points (src/utils/Mesher.py:130-157): batches of the marching-cubes grid through the decoders, sdf
    = -1 for points not strictly inside the bound.  Grid straddles the bound, ragged last batch."""
    from oracle import eslam_oracle as orc
    from myslam_amd import harness
    from myslam_amd.src.utils.Mesher import eval_points
    dev = _dev()
    wl = harness.make_workload("room0", 64, 24, 8, device=dev, planes="synth")
    b = wl.scene.bound
    axes = [torch.linspace(float(b[k, 0]) - 0.3, float(b[k, 1]) + 0.3, n) for k, n in enumerate((41, 33, 29))]
    axes[0][5] = b[0, 0]
    axes[1][-4] = b[1, 1]                                  # points exactly on a face are outside (strict test)
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    mesher = SimpleNamespace(points_batch_size=10000, bound=b)
    got = eval_points(mesher, pts.to(dev), wl.planes, wl.decoders).cpu()
    cparams = {k: v.detach().cpu() for k, v in wl.decoders.state_dict().items() if k != "beta"}
    cplanes = tuple([p.detach().cpu().contiguous() for p in grp] for grp in wl.planes)
    ref = orc.decode(pts, cplanes, cparams, b)
    inside = ((pts < b[:, 1]) & (pts > b[:, 0])).all(dim=1)
    assert 0.2 < float(inside.float().mean()) < 0.9
    ref[~inside, -1] = -1
    assert got.shape == (pts.shape[0], 4)
    assert torch.equal(got[~inside, 3], torch.full((int((~inside).sum()),), -1.0))
    assert hp.rel_err(got.numpy(), ref.numpy()) <= RTOL
    # a mesher bound different from the decoders' falls back to masking with the mesher's own bound
    mesher2 = SimpleNamespace(points_batch_size=7777, bound=b * 0.5)
    got2 = eval_points(mesher2, pts.to(dev), wl.planes, wl.decoders).cpu()
    inside2 = ((pts < b[:, 1] * 0.5) & (pts > b[:, 0] * 0.5)).all(dim=1)
    assert torch.equal(got2[~inside2, 3], torch.full((int((~inside2).sum()),), -1.0))
    assert hp.rel_err(got2[inside2].numpy(), ref[inside2].numpy()) <= RTOL


def _two_rank_worker(rank, world, port, ret):
    """One of two processes sharing the single GPU of the box, talking over gloo (RCCL refuses two ranks on one device):
    the complete ShardedMapper path - whole batch on every rank, set sizes and texel marking without a collective, the
    slice's forward / backward, device-side texel list, pack / ONE all-reduce / unpack, graphs."""
    import os
    import torch.distributed as dist
    from myslam_amd import harness
    from myslam_amd.parallel import ShardedMapper
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda:0")
        torch.manual_seed(11)
        wl = harness.make_workload("room0", 1200, 32, 8, device=dev, planes="synth", seed=0, zero_frac=0.1, shard=(rank, world))
        out = {}
        for label, compact in (("dense", False), ("sparse", True)):
            torch.manual_seed(11)                        # same jitter numbers in every run (the step counter restarts)
            from myslam_amd import ops
            ops._rng_key.clear()
            m = ShardedMapper(wl, compact=compact)
            assert m.compact == compact and (m.lo, m.hi) == (wl.ray_lo, wl.ray_lo + wl.R)
            m.step()
            torch.cuda.synchronize()
            ng = m.grads.offsets[-1]                 # the 16 loss sums ride behind the gradients in the flat buffer
            out[label] = (float(m.loss), m.grads.flat[:ng].cpu().numpy().copy())
            if compact:
                out["exchange"] = m.last_exchange
                m.capture(warmup=1)
                for _ in range(2):
                    m.step()
                torch.cuda.synchronize()
                out["graph_runs"] = (float(m.loss), bool(torch.isfinite(m.grads.flat).all()))
                # one graph per step: [back of the previous iteration, front of this one], then the all-reduce; flush() completes
                # the last one.  perturb off: every iteration sees the same samples, so every step reproduces the eager result
                wl.renderer.perturb = False
                mp_ = ShardedMapper(wl, compact=True)
                mp_.step()
                torch.cuda.synchronize()
                ref_flat = mp_.grads.flat[:ng].clone()
                mp_.capture(warmup=1, pipeline=True)
                for _ in range(3):
                    mp_.step()
                mp_.flush()
                torch.cuda.synchronize()
                out["pipeline"] = float((mp_.grads.flat[:ng] - ref_flat).abs().max() / ref_flat.abs().max())
                wl.renderer.perturb = True
        if rank == 0:
            ret.update(out)
    finally:
        dist.destroy_process_group()


def test_sharded_mapper_two_ranks_on_one_gpu():
    import socket
    import torch.multiprocessing as mp
    from myslam_amd import harness, ops
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_two_rank_worker, args=(2, port, ret), nprocs=2, join=True)
    # the unsharded reference: the whole batch through the plain autograd path, same seed -> same in-kernel jitter numbers
    # (keyed on the global ray index) and same importance samples
    dev = _dev()
    w0 = harness.make_workload("room0", 1200, 32, 8, device=dev, planes="synth", seed=0, zero_frac=0.1)
    torch.manual_seed(11)                                # (after the workload: building it seeds torch for the decoders)
    ops._rng_key.clear()
    loss = w0.step()
    params = w0.plane_list + ops.decoder_params(w0.decoders) + [w0.decoders.beta]      # order of the flat buffer
    flat_ref = torch.cat([p.grad.detach().permute(0, 2, 3, 1).reshape(-1) if p.dim() == 4 else p.grad.detach().reshape(-1)
                          for p in params]).cpu().numpy()
    for label in ("dense", "sparse"):
        lv, flat = ret[label]
        assert abs(lv - float(loss)) <= 1e-5 * abs(float(loss)), label
        assert hp.rel_err(flat, flat_ref) <= 2e-5, label
    lv, finite = ret["graph_runs"]                       # replays draw fresh jitter: the loss moves a little, nothing breaks
    assert finite and abs(lv - float(loss)) <= 0.05 * abs(float(loss))
    sent, dense = ret["exchange"]
    assert sent < 0.3 * dense, (sent, dense)
    assert ret["pipeline"] <= 2e-5, ret["pipeline"]       # (float atomics' order)


def _window_inputs(dev, sc, b):
    from myslam_amd import scene as scn, synth
    from myslam_amd.src import common
    c0 = scn.center_pose(sc).to(dev)
    c2ws = c0[None].repeat(b, 1, 1)
    for k in range(1, b):
        q = torch.tensor([1.0, 0.03 * k, -0.02 * k, 0.04 * k])
        c2ws[k, :3, :3] = common.quaternion_to_matrix(q / q.norm()).to(dev) @ c0[:3, :3]
        c2ws[k, :3, 3] += torch.tensor([0.25 * k, -0.15 * k, 0.05 * k], device=dev)
    gds = torch.stack([torch.from_numpy(synth.depth_image(sc.H, sc.W, 40 + k, 0.1)) for k in range(b)]).to(dev)
    gds[1] *= 2.5                                   # depths beyond the bound: the pre-filter mask drops those rays
    gcs = torch.stack([torch.from_numpy(synth.color_image(sc.H, sc.W, 60 + k)) for k in range(b)]).to(dev)
    return c2ws, gds, gcs


def _window_worker(rank, world, port, ret, backend):
    import os
    import torch.distributed as dist
    from myslam_amd import harness, ops, parallel
    from myslam_amd.src import common
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda:0")
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        wl = harness.make_workload("room0", 64, 32, 8, device=dev, planes="synth", state="trained")
        b = 5
        c2ws, gds, gcs = _window_inputs(dev, wl.scene, b)
        poses = torch.nn.Parameter(common.matrix_to_cam_pose(c2ws[1:]).detach().clone())
        win = parallel.MappingWindow(wl.renderer, gds, gcs, c2ws, 3000, cam_poses=poses)
        torch.manual_seed(21)
        ops._rng_key.clear()
        m = parallel.ShardedMapper(win, planes=wl.planes, decoders=wl.decoders, truncation=wl.truncation)
        assert m.pose_param is poses and m.R_total == 3000
        m.step()
        torch.cuda.synchronize()
        ng = m.grads.offsets[-1]
        out = dict(first=(float(m.loss), m.grads.flat[:ng].cpu().numpy().copy(), poses.grad.detach().cpu().numpy().copy()))
        # 6 iterations with the fused Adam (decoders, planes, colour planes AND the window's poses), the last 3 as graph replays
        m.make_optimizer(fused_zero_grad=True, capturable=True)
        for _ in range(3):
            m.step()
        m.capture(warmup=0)
        for _ in range(3):
            m.step()
        torch.cuda.synchronize()
        out["after"] = (float(m.loss), poses.detach().cpu().numpy().copy(),
                        [p.detach().cpu().numpy().copy() for p in m.params[12:24]], float(m.params[1].detach().abs().sum()))
        if rank == 0:
            ret.update(out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,backend", [(1, "nccl"), (2, "gloo")])
def test_sharded_mapping_window_with_pose_gradients(world, backend):
    """The reference's mapping iteration ray-sharded (src/Mapper.py:308-350 with joint_opt): every iteration draws fresh pixels
    from a 5-frame window (one torch.randint, same seed on every rank), the AABB pre-filter is a mask, each rank renders its
    slice, and plane / decoder / beta / POSE gradients come back from the one all-reduce.  Against the plain single-GPU loop:
    first-iteration gradients, then parameters and poses after 7 Adam iterations (3 of them replayed graphs)."""
    import socket
    import torch.multiprocessing as mp
    from myslam_amd import harness, losses, ops, optim, parallel
    from myslam_amd.src import common
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_window_worker, args=(world, port, ret, backend), nprocs=world, join=True)
    # the plain loop, one process: get_samples -> pre-filter mask -> render with the fused loss -> backward -> Adam
    dev = _dev()
    wl = harness.make_workload("room0", 64, 32, 8, device=dev, planes="synth", state="trained")
    b = 5
    c2ws, gds, gcs = _window_inputs(dev, wl.scene, b)
    poses = torch.nn.Parameter(common.matrix_to_cam_pose(c2ws[1:]).detach().clone())
    win = parallel.MappingWindow(wl.renderer, gds, gcs, c2ws, 3000, cam_poses=poses)
    params = wl.plane_list + ops.decoder_params(wl.decoders) + [wl.decoders.beta, poses]
    torch.manual_seed(21)
    ops._rng_key.clear()

    def iteration():
        for p in params:
            p.grad = None
        ro, rd, gd, gc, keep = win.batch()
        depth, color, sdf, z, pre = wl.renderer.render_batch_ray_with_loss(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gd, gc,
                                                                          losses.MAPPING_W, ray_mask=keep)
        loss = losses.mapping_loss(depth, color, sdf, z, gd, gc, wl.truncation, precomputed=pre)
        loss.backward()
        return loss, keep
    loss, keep = iteration()
    assert 0.5 < float(keep.float().mean()) < 0.98
    lv, flat, pg = ret["first"]
    flat_ref = torch.cat([p.grad.detach().permute(0, 2, 3, 1).reshape(-1) if p.dim() == 4 else p.grad.detach().reshape(-1)
                          for p in params]).cpu().numpy()
    assert abs(lv - float(loss)) <= 1e-5 * abs(float(loss))
    assert hp.rel_err(flat, flat_ref) <= 3e-5
    g_ref = poses.grad.detach().cpu().numpy()
    assert np.abs(g_ref).max() > 0 and hp.rel_err(pg, g_ref) <= 1e-4
    opt = optim.Adam([{"params": params[12:25], "lr": 0.001}, {"params": params[0:6], "lr": 0.005}, {"params": params[6:12], "lr": 0.005},
                      {"params": [poses], "lr": 0.001}])
    for _ in range(6):
        loss, _ = iteration()                            # (the sharded mapper's `loss` is its last iteration's, before that step)
        opt.step()
    la, pa, dec_a, plane_l1 = ret["after"]
    assert abs(la - float(loss)) <= 1e-3 * abs(float(loss))
    # (float atomics' arrival order, amplified by Adam for near-zero gradients: test_gpu_determinism.py)
    assert hp.rel_err(pa, poses.detach().cpu().numpy()) <= 3e-4
    for a, p in zip(dec_a, params[12:24]):
        assert hp.rel_err(a, p.detach().cpu().numpy()) <= 3e-4
    assert abs(plane_l1 - float(params[1].detach().abs().sum())) <= 1e-4 * plane_l1


def test_graft_smoke_entry():
    import __graft_entry__ as g
    g.smoke()


def test_matched_loss_over_adam_iterations():
    """"At matched loss": 25 mapping iterations with Adam on the planes and decoders (the learning rates of
    configs/ESLAM.yaml:58-61), HIP path on the GPU vs the oracle on the CPU, same rays and the same jitter numbers each
    iteration.  The two loss curves must stay together - a check with the optimiser in the loop that no gradient is
    subtly wrong (a wrong sign or scale would separate the curves within a few steps)."""
    from oracle import eslam_oracle as orc
    from myslam_amd import losses, synth
    fx = hp.load("room0_200x32")
    dev = _dev()
    sc, planes, dec, renderer = build(fx)
    ro = torch.from_numpy(fx["rays_o"]).to(dev)
    rd = torch.from_numpy(fx["rays_d"]).to(dev)
    gd = torch.from_numpy(fx["gt_depth"]).to(dev)
    gc = torch.from_numpy(fx["gt_color"]).to(dev)
    tr = float(fx["truncation"])
    R, S = gd.shape[0], int(fx["n_stratified"]) + int(fx["n_importance"])
    plist = hp.flat_planes(planes)
    opt = torch.optim.Adam([{"params": list(dec.parameters()), "lr": 0.001}, {"params": plist[:6], "lr": 0.005},
                            {"params": plist[6:], "lr": 0.005}])
    # oracle twin on the CPU (NCHW planes, same values)
    cplanes = tuple([torch.nn.Parameter(p.detach().cpu().contiguous()) for p in grp] for grp in planes)
    cparams = {k: torch.nn.Parameter(v.detach().cpu().clone()) for k, v in dec.state_dict().items() if k != "beta"}
    cbeta = torch.nn.Parameter(dec.beta.detach().cpu().clone())
    cplist = hp.flat_planes(cplanes)
    copt = torch.optim.Adam([{"params": list(cparams.values()) + [cbeta], "lr": 0.001},
                             {"params": cplist[:6], "lr": 0.005}, {"params": cplist[6:], "lr": 0.005}])
    hip_losses, ref_losses = [], []
    for it in range(25):
        t_rand = torch.from_numpy(synth.hash_uniform((R, S), 200_000 + it))
        opt.zero_grad(set_to_none=True)
        depth, color, sdf, z = renderer.render_batch_ray(planes, dec, rd, ro, dev, tr, gt_depth=gd,
                                                         _rand=(t_rand.to(dev), None, None))
        loss = losses.mapping_loss(depth, color, sdf, z, gd, gc, tr)
        loss.backward()
        opt.step()
        hip_losses.append(float(loss))
        copt.zero_grad(set_to_none=True)
        cd, cc, cs, cz = orc.render_batch_ray(cplanes, cparams, cbeta, sc.bound, rd.cpu(), ro.cpu(), tr, gd.cpu(),
                                              int(fx["n_stratified"]), int(fx["n_importance"]), t_rand, None, None)
        closs = orc.mapping_loss(cd, cc, cs, cz, gd.cpu(), gc.cpu(), tr)
        closs.backward()
        copt.step()
        ref_losses.append(float(closs))
    hip_losses, ref_losses = np.array(hip_losses), np.array(ref_losses)
    assert ref_losses[-1] < 0.8 * ref_losses[0], "the optimisation should make progress"
    assert np.abs(hip_losses - ref_losses).max() <= 2e-3 * ref_losses[0], (hip_losses, ref_losses)


@pytest.mark.parametrize("R,ns,ni,zero_frac", [(1, 24, 8, 0.0), (3, 5, 3, 0.0), (7, 32, 8, 1.0), (130, 100, 28, 0.3),
                                               (33, 16, 0, 0.0), (65, 200, 56, 0.2)])
@pytest.mark.parametrize("state", ["initial", "trained"])
def test_edge_shapes_against_oracle(R, ns, ni, zero_frac, state):
    """Ragged sizes: a single ray, R not a multiple of the 4 rays per workgroup, S not a multiple of 16, S > 64 (two and
    four 64-sample chunks per ray, up to the 256 maximum), every ray without depth, no surface samples at all."""
    from oracle import eslam_oracle as orc
    from myslam_amd import harness, synth
    dev = _dev()
    wl = harness.make_workload("room0", max(R, 8) * 4, ns, ni, device=dev, zero_frac=zero_frac, planes="synth",
                               rays_grad=True, state=state)
    sl = slice(0, R)
    ro, rd = wl.rays_o[sl].detach().requires_grad_(True), wl.rays_d[sl].detach().requires_grad_(True)
    gd, gc = wl.gt_depth[sl], wl.gt_color[sl]
    S = ns + ni
    rand = (torch.from_numpy(synth.hash_uniform((R, S), 7)).to(dev), torch.from_numpy(synth.hash_uniform((R, ns), 8)).to(dev),
            torch.from_numpy(synth.hash_uniform((R, ni), 9)).to(dev))
    depth, color, sdf, z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd,
                                                        _rand=rand)
    assert z.shape == (R, S) and sdf.shape == (R, S) and depth.shape == (R,) and color.shape == (R, 3)
    cot = torch.from_numpy(synth.hash_uniform((R, S), 10)).to(dev) - 0.5
    ((depth * 0.7).sum() + (color * 0.3).sum() + (sdf * cot).sum()).backward()
    # float64 oracle on the CPU with the kernel's own z_vals (the samplers are checked against the fixtures)
    def oracle_run(dtype, check_z=False):
        cv = lambda t: t.detach().cpu().to(dtype)
        cplanes = tuple([cv(p).contiguous().requires_grad_(True) for p in grp] for grp in wl.planes)
        cparams = {k: cv(v).requires_grad_(True) for k, v in wl.decoders.state_dict().items() if k != "beta"}
        cbeta = cv(wl.decoders.beta).requires_grad_(True)
        cro, crd = cv(ro).requires_grad_(True), cv(rd).requires_grad_(True)
        if check_z:
            has = (gd > 0).cpu()
            zo = orc.sample_z(cro.detach(), crd.detach(), cv(gd), cplanes, cparams, cbeta.detach(), wl.scene.bound.to(dtype),
                              wl.truncation, ns, ni, *(cv(t) for t in rand))
            assert torch.equal(z.cpu()[has], zo.float()[has]) or hp.rel_err(z.cpu()[has].numpy(), zo[has].numpy()) <= 1e-6
            if (~has).any():
                assert hp.rel_err(z.cpu()[~has].numpy(), zo[~has].numpy()) <= RTOL
        od, oc, os_, _ = orc.render_batch_ray(cplanes, cparams, cbeta, wl.scene.bound, crd, cro, wl.truncation, cv(gd),
                                              ns, ni, z_vals=cv(z))
        ((od * 0.7).sum() + (oc * 0.3).sum() + (os_ * cv(cot)).sum()).backward()
        return dict(out=(od, oc, os_), planes=cplanes, params=cparams, beta=cbeta, ro=cro, rd=crd)

    o = oracle_run(torch.float64, check_z=True)
    od, oc, os_ = o["out"]
    assert hp.rel_err(depth.detach().cpu().numpy(), od.detach().numpy()) <= RTOL
    assert hp.rel_err(color.detach().cpu().numpy(), oc.detach().numpy()) <= RTOL
    assert hp.rel_err(sdf.detach().cpu().numpy(), os_.detach().numpy()) <= RTOL
    # The position gradient of a bilinear lookup jumps at texel boundaries, and float32 vs float64 sample positions put
    # a few of the ~10^5 coordinates on different sides of one (|ix - round(ix)| < float32 eps happens ~6e-5 of the
    # time).  Those rays differ by a finite amount that is not an error of either side: require 97 % of the rays inside
    # the tolerance and the rest bounded.  (Against the float32 fixtures of the reference the full 1e-4 holds.)
    for a, b in ((ro.grad.cpu().numpy(), o["ro"].grad.numpy()), (rd.grad.cpu().numpy(), o["rd"].grad.numpy())):
        per_ray = np.abs(a - b).max(1) / (np.abs(b).max() + 1e-30)
        assert np.quantile(per_ray, 0.97) <= RTOL and per_ray.max() <= 0.05, (np.quantile(per_ray, 0.97), per_ray.max())
    # plane gradients: float32 oracle as comparator, float64 as the conditioning bound, texels of ReLU-ambiguous samples
    # set aside (helpers.ambiguous_samples; they only occur in the trained-like state)
    o32 = oracle_run(torch.float32)
    pts = (o["ro"].detach()[:, None, :] + o["rd"].detach()[:, None, :] * z.detach().cpu().double()[..., None]).reshape(-1, 3)
    pn = orc.normalize_points(pts, wl.scene.bound.double())
    amb = hp.ambiguous_samples(pn, tuple([p.detach() for p in grp] for grp in o["planes"]), {k: v.detach() for k, v in o["params"].items()})
    ok, msg = hp.plane_grads_close([p.grad.cpu().numpy() for p in wl.plane_list], [p.grad.numpy() for p in hp.flat_planes(o32["planes"])],
                                   [p.grad.numpy() for p in hp.flat_planes(o["planes"])], pn, amb, wl.scene.plane_shapes, RTOL)
    assert ok, (msg, int(amb.sum()))
    slack = 4.0 * float(amb.sum()) / max(1, amb.numel())
    for k, t in wl.decoders.named_parameters():
        ref = o["beta"].grad if k == "beta" else o["params"][k].grad
        ref32 = o32["beta"].grad if k == "beta" else o32["params"][k].grad
        assert hp.rel_err(t.grad.cpu().numpy(), ref32.double().numpy()) <= RTOL + slack, k
        assert hp.rel_err(t.grad.cpu().numpy(), ref.numpy()) <= max(RTOL, 1.5 * hp.rel_err(ref32.double().numpy(), ref.numpy())) + slack, k


@pytest.mark.parametrize("seed", range(8))
def test_random_configurations_against_oracle(seed):
    """Randomised shapes and geometry: scene (room0 / toy), plane layout (channels_last / NCHW), 1-5 cameras with random
    rotations and positions (rays that leave the bound, bundles whose cell boxes overflow the counting sort), ray count,
    sample counts and the share of depth-less rays.  Forward outputs and every gradient against the oracle on the same
    z_vals, linear cotangents; float32 oracle as comparator for gradients, the float64 one as the conditioning bound."""
    from oracle import eslam_oracle as orc
    from myslam_amd import harness, synth
    from myslam_amd.src.common import get_samples_at
    rng = np.random.default_rng(1000 + seed)
    dev = _dev()
    scene_name = ["room0", "toy"][int(rng.integers(2))]
    ns, ni = int(rng.integers(3, 90)), int(rng.integers(0, 24))
    b = int(rng.integers(1, 6))
    n = int(rng.integers(1, 160))
    zero_frac = float(rng.choice([0.0, 0.1, 0.5]))
    cl = bool(rng.integers(2))
    # odd seeds: the trained-like state (harness.Workload), where every sample of a ray carries compositing weight
    wl = harness.make_workload(scene_name, 16, ns, ni, device=dev, planes="synth", channels_last=cl,
                               state="trained" if seed % 2 else "initial")
    sc = wl.scene
    c2ws = torch.eye(4).repeat(b, 1, 1)
    for i in range(b):
        qm, rm = np.linalg.qr(rng.normal(size=(3, 3)))
        qm = qm * np.sign(np.diag(rm))
        if np.linalg.det(qm) < 0:
            qm[:, 0] = -qm[:, 0]
        c2ws[i, :3, :3] = torch.from_numpy(qm).float()
        c2ws[i, :3, 3] = sc.bound.mean(1) + torch.from_numpy(rng.uniform(-0.4, 0.4, 3)).float() * (sc.bound[:, 1] - sc.bound[:, 0])
    c2ws = c2ws.to(dev)
    depth_img = torch.from_numpy(np.stack([synth.depth_image(sc.H, sc.W, 400 + 10 * seed + i, zero_frac) for i in range(b)])).to(dev)
    color_img = torch.from_numpy(np.stack([synth.color_image(sc.H, sc.W, 500 + 10 * seed + i) for i in range(b)])).to(dev)
    idx = torch.from_numpy(rng.integers(0, sc.H * sc.W, size=(b * n,))).to(dev)
    with torch.no_grad():
        ro, rd, gd, gc = get_samples_at(idx, 0, sc.H, 0, sc.W, n, sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy, c2ws, depth_img, color_img)
    ro, rd = ro.requires_grad_(True), rd.requires_grad_(True)
    R, S = ro.shape[0], ns + ni
    rand = tuple(torch.from_numpy(rng.random(shape, dtype=np.float32)).to(dev) for shape in ((R, S), (R, ns), (R, ni)))
    depth, color, sdf, z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd, _rand=rand)
    cot = [torch.from_numpy(rng.normal(size=shape).astype(np.float32)).to(dev) for shape in ((R,), (R, 3), (R, S))]
    ((depth * cot[0]).sum() + (color * cot[1]).sum() + (sdf * cot[2]).sum()).backward()

    def oracle_run(dtype):
        cv = lambda t: t.detach().cpu().to(dtype)
        planes = tuple([cv(p).contiguous().requires_grad_(True) for p in grp] for grp in wl.planes)
        params = {k: cv(v).requires_grad_(True) for k, v in wl.decoders.state_dict().items() if k != "beta"}
        beta = cv(wl.decoders.beta).requires_grad_(True)
        cro, crd = cv(ro).requires_grad_(True), cv(rd).requires_grad_(True)
        od, oc, os_, _ = orc.render_batch_ray(planes, params, beta, sc.bound, crd, cro, wl.truncation, cv(gd), ns, ni, z_vals=cv(z))
        ((od * cv(cot[0])).sum() + (oc * cv(cot[1])).sum() + (os_ * cv(cot[2])).sum()).backward()
        grads = [p.grad.double().numpy() for p in hp.flat_planes(planes)]
        grads += [(beta.grad if k == "beta" else params[k].grad).double().numpy() for k, _ in wl.decoders.named_parameters()]
        return [t.detach().double().numpy() for t in (od, oc, os_)], grads, [cro.grad.double().numpy(), crd.grad.double().numpy()]

    o64, g64, r64 = oracle_run(torch.float64)
    _, g32, _ = oracle_run(torch.float32)
    desc = f"{scene_name} cl={cl} b={b} n={n} S={ns}+{ni} zero={zero_frac}"
    assert np.all(np.diff(z.cpu().numpy(), axis=1) >= 0), desc
    for a, r in zip((depth, color, sdf), o64):
        assert hp.rel_err(a.detach().cpu().numpy(), r) <= RTOL, desc
    mine = [p.grad.cpu().double().numpy() for p in wl.plane_list] + [t.grad.cpu().double().numpy() for _, t in wl.decoders.named_parameters()]
    pts = (ro.detach().cpu().double()[:, None, :] + rd.detach().cpu().double()[:, None, :] * z.cpu().double()[..., None])
    pn = orc.normalize_points(pts.reshape(-1, 3), sc.bound.double())
    cv64 = lambda t: t.detach().cpu().double()
    amb = hp.ambiguous_samples(pn, tuple([cv64(p).contiguous() for p in grp] for grp in wl.planes),
                               {k: cv64(v) for k, v in wl.decoders.state_dict().items() if k != "beta"})
    assert amb.float().mean() <= 5e-3, (desc, int(amb.sum()))
    ok, msg = hp.plane_grads_close(mine[:12], g32[:12], g64[:12], pn, amb, sc.plane_shapes, RTOL)
    assert ok, (desc, msg, int(amb.sum()))
    for k, (a, r32, r64_) in enumerate(zip(mine[12:], g32[12:], g64[12:])):
        # a decoder gradient sums over all samples: an ambiguous sample moves it by its own share
        slack = 4.0 * float(amb.sum()) / max(1, amb.numel())
        assert hp.rel_err(a, r32) <= RTOL + slack, (desc, k)
        assert hp.rel_err(a, r64_) <= max(RTOL, 1.5 * hp.rel_err(r32, r64_)) + slack, (desc, k)
    # Ray gradients: the position gradient of a bilinear lookup jumps at texel boundaries, so a ray may differ by a finite
    # amount when float32 and float64 put one of its samples on different sides of one.  Every ray outside the tolerance
    # must be explained that way: one of its samples lies within 2e-4 texels of a boundary of one of the 12 planes.
    pn = pn.reshape(R, S, 3)
    amb_ray = amb.reshape(R, S).any(1).numpy()
    near = torch.full((R,), 1e9, dtype=torch.float64)
    for g, (ax, ay) in enumerate([(0, 1), (0, 2), (1, 2)] * 2):
        for lvl in range(2):
            h, w = sc.plane_shapes[g][lvl][2:]
            for coord, size in ((pn[..., ax], w), (pn[..., ay], h)):
                ix = (coord + 1) / 2 * (size - 1)
                inside = (ix > 0) & (ix < size - 1)
                dist = torch.where(inside, (ix - ix.round()).abs(), torch.full_like(ix, 1e9))
                near = torch.minimum(near, dist.min(dim=1).values)
    for a, r in ((ro.grad.cpu().numpy(), r64[0]), (rd.grad.cpu().numpy(), r64[1])):
        per_ray = np.abs(a - r).max(1) / (np.abs(r).max() + 1e-30)
        bad = per_ray > RTOL
        assert bad.mean() <= 0.03, (desc, bad.mean())
        assert np.all((near.numpy()[bad] < 2e-4) | amb_ray[bad]), (desc, per_ray[bad], near.numpy()[bad])


MIXED_CASES = {
    # case: (forward bounds: sdf, rgb, relative depth), (training bounds: loss, plane gradients, 1 - cosine, decoder gradients)
    "freiburg1_desk_5000x56_zero10": ((5e-3, 5e-3, 2e-2), (2e-4, 1e-2, 1e-4, 1.2e-2)),
    # the trained-like state: O(1) features, compositing weights spread over ~20 samples of a ray
    # measured: sdf 8.7e-4 / 1.4e-3 (vs reference float32 / float64 oracle), rgb 4e-5 / 7e-5, depth 1.4e-3 / 1.9e-3; training
    # step: loss 8.7e-6, plane gradients 6.8e-3 (cosine 0.999963), decoder gradients 4.9e-3
    "room0_4096x64_trained_zero10": ((3e-3, 5e-4, 5e-3), (2e-4, 1.5e-2, 1e-4, 1.2e-2)),
}


@pytest.mark.parametrize("case", list(MIXED_CASES))
def test_mixed_precision_tolerance_study(case):
    """BASELINE.json configs[4]: freiburg1_desk, 5000 rays x 56 samples, fp16 planes + bf16 MFMA decoders.  A tolerance
    STUDY against (a) the outputs of the REFERENCE itself (the float32 fixture) and (b) the float64 oracle on the same
    rays and z_vals: the bounds are what the formats allow (half has 11 significant bits, bf16 8), recorded in DESIGN.md -
    not the 1e-4 parity bar, which only the float32 path is held to."""
    from myslam_amd import lowp
    from tests.test_oracle_golden import run_oracle
    fx = hp.load(case)
    b_sdf, b_rgb, b_dep = MIXED_CASES[case][0]
    dev = _dev()
    sc, planes, dec, renderer = build(fx, planes_grad=False, dec_grad=False)
    t_rand, t_uni, u = hp.rand_inputs(fx)
    rand = tuple(None if t is None else t.to(dev) for t in (t_rand, t_uni, u))
    ro = torch.from_numpy(fx["rays_o"]).to(dev)
    rd = torch.from_numpy(fx["rays_d"]).to(dev)
    gd = torch.from_numpy(fx["gt_depth"]).to(dev)
    tr = float(fx["truncation"])
    ph = lowp.half_planes(planes)
    d16, c16, s16, z16 = lowp.render_batch_ray_lowp(renderer, planes, ph, dec, rd, ro, tr, gd, _rand=rand)
    pr = fx["probe"]
    has = fx["gt_depth"][pr] > 0
    # (a) the reference's own float32 outputs
    assert np.array_equal(z16.cpu().numpy()[pr][has], fx["z_vals"][has])
    e_sdf = float(np.abs(s16.cpu().numpy()[pr][has] - fx["sdf"][has]).max())
    e_rgb = float(np.abs(c16.cpu().numpy()[pr] - fx["color"]).max())
    e_dep = float((np.abs(d16.cpu().numpy()[pr] - fx["depth"]) / np.maximum(np.abs(fx["depth"]), 1e-3)).max())
    print(f"{case}: mixed precision vs the reference's float32 outputs: max|sdf| {e_sdf:.2e}  max|rgb| {e_rgb:.2e}  max rel depth {e_dep:.2e}")
    assert e_sdf < b_sdf and e_rgb < b_rgb and e_dep < b_dep
    # (b) the float64 oracle, every ray (z_vals of depth-less rays differ at 1e-4 between the paths: compare rays with depth)
    o = run_oracle(fx, torch.float64)
    hd = fx["gt_depth"] > 0
    e_sdf = float(np.abs(s16.cpu().numpy()[hd] - o["sdf"].detach().numpy()[hd]).max())
    e_rgb = float(np.abs(c16.cpu().numpy()[hd] - o["color"].detach().numpy()[hd]).max())
    e_dep = float((np.abs(d16.cpu().numpy()[hd] - o["depth"].detach().numpy()[hd]) /
                   np.maximum(np.abs(o["depth"].detach().numpy()[hd]), 1e-3)).max())
    print(f"{case}: mixed precision vs the float64 oracle ({int(hd.sum())} rays): max|sdf| {e_sdf:.2e}  max|rgb| {e_rgb:.2e}  max rel depth {e_dep:.2e}")
    assert e_sdf < b_sdf and e_rgb < b_rgb and e_dep < b_dep


@pytest.mark.parametrize("case", list(MIXED_CASES))
def test_mixed_precision_training_step_gradient_study(case):
    """BASELINE.json configs[4] as a TRAINING configuration: forward and backward of a mapping iteration on the mixed-precision
    kernels (fp16 plane copies, bf16-MFMA decoders both ways, float32 accumulation and float32 plane gradients) against
    autograd over the float64 oracle on the freiburg1_desk fixture (5000 rays x 56 samples, 10 % depth-less).  A tolerance
    STUDY: the gradients of a bf16 network are not the float32 network's to 1e-4; the bounds are what was measured, with
    margin, and are recorded in DESIGN.md."""
    from myslam_amd import lowp, losses, ops
    from tests.test_oracle_golden import run_oracle
    fx = hp.load(case)
    b_loss, b_planes, b_cos, b_dec = MIXED_CASES[case][1]
    dev = _dev()
    sc, planes, dec, renderer = build(fx)
    t_rand, t_uni, u = hp.rand_inputs(fx)
    rand = tuple(None if t is None else t.to(dev) for t in (t_rand, t_uni, u))
    ro = torch.from_numpy(fx["rays_o"]).to(dev)
    rd = torch.from_numpy(fx["rays_d"]).to(dev)
    gd = torch.from_numpy(fx["gt_depth"]).to(dev)
    gc = torch.from_numpy(fx["gt_color"]).to(dev)
    tr = float(fx["truncation"])
    half = lowp.HalfPlanes(planes)
    res = {}
    for label in ("separate", "fused"):
        for p in hp.flat_planes(planes) + list(dec.parameters()):
            p.grad = None
        with ops.mixed_precision(half):
            if label == "fused":      # loss sums in the forward's epilogue, loss gradients inside the backward kernel
                depth, color, sdf, z, pre = renderer.render_batch_ray_with_loss(planes, dec, rd, ro, dev, tr, gd, gc,
                                                                                losses.MAPPING_W, _rand=rand)
                loss = pre.loss
            else:
                depth, color, sdf, z = renderer.render_batch_ray(planes, dec, rd, ro, dev, tr, gt_depth=gd, _rand=rand)
                loss = losses.mapping_loss(depth, color, sdf, z, gd, gc, tr)
            loss.backward()
        torch.cuda.synchronize()
        res[label] = (float(loss), [p.grad.detach().clone() for p in hp.flat_planes(planes)],
                      {k: p.grad.detach().clone() for k, p in dec.named_parameters()})
    # the two formulations of the same mixed-precision step agree like the float32 ones do
    assert abs(res["fused"][0] - res["separate"][0]) <= 1e-5 * abs(res["separate"][0])
    for a, b in zip(res["fused"][1], res["separate"][1]):
        assert hp.rel_err(a.cpu().numpy(), b.cpu().numpy()) <= 1e-4
    o = run_oracle(fx, torch.float64)
    lv, pg, dg = res["fused"]
    e_loss = abs(lv - float(o["loss"])) / abs(float(o["loss"]))
    e_planes = [hp.rel_err(a.cpu().numpy(), b.grad.numpy()) for a, b in zip(pg, hp.flat_planes(o["planes"]))]
    e_dec = {k: hp.rel_err(g.cpu().numpy(), (o["params"][k].grad if k != "beta" else o["beta"].grad).numpy()) for k, g in dg.items()
             if k != "beta" or bool(fx["beta_is_param"])}
    cos = [float((a.cpu().double().flatten() @ b.grad.flatten()) / (a.cpu().double().norm() * b.grad.norm() + 1e-300))
           for a, b in zip(pg, hp.flat_planes(o["planes"]))]
    print(f"{case}: mixed-precision training step vs float64 oracle: loss rel {e_loss:.2e}; plane gradients max-normalised error "
          f"{max(e_planes):.2e} (geometry {max(e_planes[:6]):.2e}, colour {max(e_planes[6:]):.2e}), cosine >= {min(cos):.6f}; "
          f"decoder gradients {max(e_dec.values()):.2e} ({max(e_dec, key=e_dec.get)})")
    # measured on MI355X: loss 2.5e-5, plane gradients 3.2e-3 (cosine 0.999997), decoder gradients 4.0e-3
    assert e_loss < b_loss
    assert max(e_planes) < b_planes and 1.0 - min(cos) < b_cos
    assert max(e_dec.values()) < b_dec


def test_multi_camera_batch_against_oracle():
    """A mapping batch as the reference forms it (src/Mapper.py:318-319): rays of several keyframes with different poses
    in one call.  Exercises the ray ordering / bundling with several origins and directions; compared in full with
    autograd over the float64 oracle."""
    from oracle import eslam_oracle as orc
    from myslam_amd import harness, scene as scn, synth, losses
    from myslam_amd.src.common import get_samples_at
    dev = _dev()
    wl = harness.make_workload("room0", 64, 32, 8, device=dev, planes="synth")
    sc = wl.scene
    b, n = 6, 150
    c2ws = torch.eye(4).repeat(b, 1, 1)
    for i in range(b):
        m = synth.hash_uniform((3, 3), 300 + i).astype(np.float64) - 0.5
        qm, rm = np.linalg.qr(m)
        qm = qm * np.sign(np.diag(rm))
        if np.linalg.det(qm) < 0:
            qm[:, 0] = -qm[:, 0]
        c2ws[i, :3, :3] = torch.from_numpy(qm).float()
        c2ws[i, :3, 3] = sc.bound.mean(1) + (torch.from_numpy(synth.hash_uniform((3,), 320 + i)) - 0.5) * 2.0
    c2ws = c2ws.to(dev)
    depth_img = torch.from_numpy(np.stack([synth.depth_image(sc.H, sc.W, 330 + i, 0.1) for i in range(b)])).to(dev)
    color_img = torch.from_numpy(np.stack([synth.color_image(sc.H, sc.W, 340 + i) for i in range(b)])).to(dev)
    idx = torch.from_numpy(synth.hash_randint(sc.H * sc.W, (b * n,), 350)).to(dev)
    with torch.no_grad():
        ro, rd, gd, gc = get_samples_at(idx, 0, sc.H, 0, sc.W, n, sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy, c2ws,
                                        depth_img, color_img)
    R, S = ro.shape[0], wl.S
    rand = (torch.from_numpy(synth.hash_uniform((R, S), 360)).to(dev), torch.from_numpy(synth.hash_uniform((R, 32), 361)).to(dev),
            torch.from_numpy(synth.hash_uniform((R, 8), 362)).to(dev))
    depth, color, sdf, z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd,
                                                        _rand=rand)
    losses.mapping_loss(depth, color, sdf, z, gd, gc, wl.truncation).backward()
    def oracle_run(dtype):
        cv = lambda t: t.detach().cpu().to(dtype)
        planes = tuple([cv(p).contiguous().requires_grad_(True) for p in grp] for grp in wl.planes)
        params = {k: cv(v).requires_grad_(True) for k, v in wl.decoders.state_dict().items() if k != "beta"}
        beta = cv(wl.decoders.beta).requires_grad_(True)
        od, oc, os_, _ = orc.render_batch_ray(planes, params, beta, sc.bound, cv(rd), cv(ro), wl.truncation, cv(gd), 32, 8,
                                              z_vals=cv(z))
        orc.mapping_loss(od, oc, os_, cv(z), cv(gd), cv(gc), wl.truncation).backward()
        grads = [p.grad.double().numpy() for p in hp.flat_planes(planes)]
        grads += [(beta.grad if k == "beta" else params[k].grad).double().numpy() for k, _ in wl.decoders.named_parameters()]
        return od.detach().double().numpy(), oc.detach().double().numpy(), grads

    od, oc, g64 = oracle_run(torch.float64)
    _, _, g32 = oracle_run(torch.float32)
    assert hp.rel_err(depth.detach().cpu().numpy(), od) <= RTOL
    assert hp.rel_err(color.detach().cpu().numpy(), oc) <= RTOL
    mine = [p.grad.cpu().double().numpy() for p in wl.plane_list] + [t.grad.cpu().double().numpy() for _, t in wl.decoders.named_parameters()]
    # With 200x-weighted sdf terms on a handful of samples, one hidden unit whose pre-activation sits within float32
    # rounding of zero moves the first-layer / sdf-plane gradients by ~1e-3 of their maximum between float32 and
    # float64 arithmetic (measured: the float32 oracle is 7e-4..1.8e-3 away from the float64 one on exactly those
    # tensors, and the kernels are 6e-7 away from the float32 oracle).  The reference computes in float32, so the
    # float32 oracle is the comparator; the float64 one bounds how far both may be from exact.
    for k, (a, r32, r64) in enumerate(zip(mine, g32, g64)):
        assert hp.rel_err(a, r32) <= RTOL, k
        assert hp.rel_err(a, r64) <= max(RTOL, 1.5 * hp.rel_err(r32, r64)), k


@pytest.mark.parametrize("scene,R,ns,ni", [("toy", 64, 32, 8), ("room0", 37, 120, 8), ("room0", 5, 9, 2), ("room0", 130, 56, 8)])
@pytest.mark.parametrize("channels_last", [True, False])
def test_saved_features_and_raw_colour_of_every_sample(scene, R, ns, ni, channels_last):
    """What the forward pass SAVES for the backward pass, element by element against the float64 oracle: the 128 features
    and the raw colour of EVERY sample, in the trained-like state (O(1) features).  The composited outputs cannot see
    them in the reference's initial state - there the first sample of a ray takes 99.9 % of the weight - which is how a
    forward kernel that gathered the colour features of samples 16.. at the wrong positions (an inline-asm statement
    without its SCC clobber next to a select) once passed every other test of this file."""
    import ctypes
    from oracle import eslam_oracle as orc
    from myslam_amd import _hip, harness, ops
    dev = _dev()
    wl = harness.make_workload(scene, max(R, 8) * 2, ns, ni, device=dev, planes="synth", channels_last=channels_last,
                               state="trained")
    R = min(R, wl.R)                      # (rays that leave the bound before their depth are dropped by the workload)
    ro, rd, gd = wl.rays_o[:R].detach().contiguous(), wl.rays_d[:R].detach().contiguous(), wl.gt_depth[:R].contiguous()
    with torch.no_grad():
        z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd)[3].contiguous()
    S = ns + ni
    feat, raw = torch.full((R * S, 128), -7.0, device=dev), torch.full((R * S, 3), -7.0, device=dev)
    depth, rgb, sdf = torch.empty(R, device=dev), torch.empty(R, 3, device=dev), torch.empty(R, S, device=dev)
    arr, _keep = _hip.make_planes(tuple([p.detach() for p in grp] for grp in wl.planes))
    dec, _keep2 = _hip.make_decoders([p.detach() for p in ops.decoder_params(wl.decoders)],
                                     ops.beta_tensor(wl.decoders.beta, dev).detach())
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_render_fwd(arr, ctypes.byref(dec), _hip.make_bound(ops.bound_to_host(wl.scene.bound)),
                                               _hip.ptr(ro), _hip.ptr(rd), _hip.ptr(z), R, S, _hip.ptr(depth), _hip.ptr(rgb),
                                               _hip.ptr(sdf), _hip.ptr(raw), _hip.ptr(feat), None, None,
                                               _hip.stream_handle(dev)), "eslam_render_fwd")
    torch.cuda.synchronize()
    cv = lambda t: t.detach().cpu().double()
    planes = tuple([cv(p).contiguous() for p in grp] for grp in wl.planes)
    params = {k: cv(v) for k, v in wl.decoders.state_dict().items() if k != "beta"}
    pts = (cv(ro)[:, None, :] + cv(rd)[:, None, :] * cv(z)[..., None]).reshape(-1, 3)
    pn = orc.normalize_points(pts, wl.scene.bound.double())
    ref_feat = torch.cat([orc.plane_features(pn, *planes[:3]), orc.plane_features(pn, *planes[3:])], -1)
    ref_raw = orc.raw_rgb(pn, planes, params)
    ref_sdf = orc.raw_sdf(pn, planes, params).reshape(R, S)
    assert float(ref_feat.abs().mean()) > 0.05                          # O(1) features, not the 1e-2 of the initial state
    # per 16-sample block of the rays (the unit the kernel decodes), so that a failure names the block
    f, r = feat.cpu().double().reshape(R, S, 128), ref_feat.reshape(R, S, 128)
    for b in range((S + 15) // 16):
        sl = slice(16 * b, min(S, 16 * b + 16))
        for d in range(2):
            err = float((f[:, sl, 64 * d:64 * d + 64] - r[:, sl, 64 * d:64 * d + 64]).abs().max())
            assert err <= RTOL * float(r.abs().max()), f"features of decoder {d}, samples {sl}: {err}"
    for name, a, b in (("raw colour", raw, ref_raw), ("sdf", sdf, ref_sdf)):
        ok, info = hp.elementwise_close(a.cpu().double().numpy(), b.numpy(), rtol=RTOL, floor=1e-5)
        assert ok, (name, info)
