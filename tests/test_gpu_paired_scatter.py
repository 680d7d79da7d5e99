"""The rank-16 scatter's paired grid (scatter_sort_kernel<PAIR>): where the SDF decoder's plane and the colour decoder's of one
(orientation, level) agree in resolution and strides, ONE workgroup per bundle computes the cells, sorts them once and walks the
sorted records twice - per walk with the decoder's half of gz, its slice of W1 (restaged between the walks) and its gradient
plane.  The planes that do not agree keep a workgroup each.  The scenes' default shapes (the reference's planes_res /
c_planes_res) agree at the coarse level only: three pairs and six single planes per bundle; with c_planes_res = planes_res all
six pairs agree.  Both are run here, forced with eslam_scatter_pairing(2) - the auto rule pairs only batches that still fill
the chip, far larger than a test's.

The criteria are those of tests/test_gpu_rank16_scatter.py and tests/test_gpu_quad_walk.py (_accept, hp.plane_grads_close at
RTOL = 1e-4; max(1e-5, 4 x the difference of two runs of the comparator) between two paths):

  1  against the float32 / float64 oracle: one ray (nearly all padding: all-padding waves in both walks), S = 29 (1015 and 58
     samples, two samples per thread), bundles of exactly 2048 (four per thread); initial and trained state; channels-last and
     NCHW; a wide and a narrow fan, so that both grid orders run (asserted from the fan's extents)
  2  paired against unpaired (mode 0) on the same inputs and cotangents; decoder and beta gradients bit-equal
  3  cotangents on depth and sdf only: the six colour-plane gradients are exactly zero - a walk that read the other decoder's
     rows or slice, or wrote the other plane, would leave something there
  4  the hostile rays (tests/hostile_rays.py) on planes fine enough that paired workgroups take the bitonic fallback
  5  colour planes that agree with the SDF planes at NO level: mode 2 reports unpaired, and the result passes the oracle
  6  the auto rule: a small batch in mode 1 reports unpaired; its arithmetic on 4096 x 64, 8192 x 96, 2048 x 64, 200 x 32 (host
     only, no GPU)

Margins measured on an MI355X (`pytest -s`, the lines starting with "margin"): profiles/r10/paired_margins.txt.
"""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import hostile_rays as hr
from tests import test_gpu_rank16_scatter as t16

gpu = pytest.mark.gpu

# colour-plane resolutions: as shipped (coarse pairs agree), as the SDF planes (all six agree), agreeing at no level
C_SAME = dict(coarse=0.24, fine=0.06)
C_OTHER = dict(coarse=0.3, fine=0.03)
PAIRS = {"default": 3, "same": 6, "other": 0, "fine": 6}


@pytest.fixture
def pairing():
    """Sets the pairing mode for a test and restores what was set before."""
    from myslam_amd import _hip
    lib = _hip.lib()
    before = lib.eslam_scatter_pairing(-1)          # (an invalid mode changes nothing and returns the current one)
    yield lambda mode: lib.eslam_scatter_pairing(mode)
    lib.eslam_scatter_pairing(before)


def _paired():
    from myslam_amd import _hip
    return _hip.lib().eslam_last_scatter_paired()


def _set_res(wl, state, res, channels_last=True):
    """Replace the workload's planes by synth planes of other resolutions (and its scene by one that states their shapes).
    res: "default" leaves everything; "same" / "other": the colour planes' resolutions above; "fine": SDF and colour planes
    both at (0.24, 0.03) - all six pairs agree and a bundle's box in a fine plane can exceed the counting sort."""
    from myslam_amd import scene as scn
    if res != "default":
        kw = dict(c_planes_res=C_SAME if res == "same" else C_OTHER) if res != "fine" else \
            dict(planes_res=dict(coarse=0.24, fine=0.03, bound_dividable=0.24), c_planes_res=dict(coarse=0.24, fine=0.03))
        sc = dataclasses.replace(wl.scene, plane_shapes=scn.plane_shapes(wl.scene.bound, **kw))
        pl = scn.synth_planes(sc, device=wl.device, channels_last=channels_last)
        k = 60.0 if state == "trained" else 1.0
        wl.planes = tuple([torch.nn.Parameter(p * k) for p in grp] for grp in pl)
        wl.scene = sc
        wl._plane_list = wl._params = None
    shapes = [tuple(p.shape) for p in wl.plane_list]
    agree = sum(shapes[p] == shapes[p + 6] for p in range(6))
    assert agree == PAIRS[res], (res, shapes)
    return wl


def _workload(R, ns, ni, zero_frac, state, res, scene="room0", **kw):
    from myslam_amd import harness
    wl = harness.make_workload(scene, max(R, 8), ns, ni, device=t16._dev(), zero_frac=zero_frac, planes="synth", state=state, **kw)
    return _set_res(wl, state, res, kw.get("channels_last", True))


def _plane_major(ro, rd):
    """The grid order the kernel chooses for these rays: plane-major when the second largest of the fan's three extents (from
    the ray ordering kernel, behind the three orders) reaches 1.4 rad."""
    from myslam_amd import ops
    R = ro.shape[0]
    perm, side = ops.ray_order_async(ro, rd)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    fan = perm[3 * R:3 * R + 3].view(torch.float32).cpu().numpy()
    return bool(np.sort(fan)[1] >= 1.4), fan


def _oracle_check(wl, R, ns, ni, bundle, label, want_paired=1):
    dev, S = wl.device, ns + ni
    ro, rd, gd = wl.rays_o[:R].detach(), wl.rays_d[:R].detach(), wl.gt_depth[:R]
    assert ro.shape[0] == R
    rand = tuple(t.to(dev) for t in hr.rand_for(R, ns, ni))
    cot = hr.cotangent(R, S)
    mine, z = t16._render_backward(wl, ro, rd, gd, rand, cot)
    assert _paired() == want_paired
    t16._assert_rank16_path(wl, ro, rd, R, S, bundle)
    b = SimpleNamespace(rays_o=ro.cpu(), rays_d=rd.cpu(), gt_depth=gd.cpu())
    mdl = t16._cpu_model(wl)
    o64, o32 = (hr.oracle_step(mdl, wl.scene, b, z, cot, dt) for dt in (torch.float64, torch.float32))
    pn, amb = hr.ambiguous(mdl, wl.scene, b, z)
    t16._print_excluded(label, pn, amb, wl.scene)
    t16._accept(mine, o32, o64, pn, amb, wl.scene, label)
    return ro, rd, z


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------
# (R, n_strat, n_imp, zero_frac, bundle the shape must run with)
SHAPES = [(1, 5, 3, 0.0, 1024), (37, 23, 6, 0.0, 1024), (640, 56, 8, 0.1, 2048)]


@gpu
@pytest.mark.parametrize("R,ns,ni,zero_frac,bundle", SHAPES)
@pytest.mark.parametrize("state", ["initial", "trained"])
def test_paired_scatter_against_oracle(R, ns, ni, zero_frac, bundle, state, pairing):
    """All six pairs agree: six workgroups per bundle, each walking twice."""
    pairing(2)
    wl = _workload(R, ns, ni, zero_frac, state, "same")
    _oracle_check(wl, R, ns, ni, bundle, f"paired {R}x{ns}+{ni} {state}")
    if (R, ns + ni) == (640, 64):
        assert 2048 // 64 * 64 == 2048 and R % (2048 // 64) == 0             # every bundle holds exactly 2048 samples
    if (R, ns + ni) == (37, 29):
        assert (1024 // 29 * 29, (R % (1024 // 29)) * 29) == (1015, 58)


@gpu
@pytest.mark.parametrize("R,ns,ni,zero_frac,bundle", SHAPES[1:])
@pytest.mark.parametrize("kw", [dict(res="default"), dict(res="default", channels_last=False), dict(res="same", channels_last=False)])
def test_paired_scatter_partial_list_and_nchw_against_oracle(R, ns, ni, zero_frac, bundle, kw, pairing):
    """The shapes as shipped - six single planes (both decoders' fine ones) in front of three pairs - and NCHW strides."""
    pairing(2)
    kw = dict(kw)
    wl = _workload(R, ns, ni, zero_frac, "trained", kw.pop("res"), **kw)
    _oracle_check(wl, R, ns, ni, bundle, f"paired {R}x{ns}+{ni} {kw}")


@gpu
@pytest.mark.parametrize("focal_scale,want_plane_major", [(1.0, True), (3.0, False)])
@pytest.mark.parametrize("res", ["same", "default"])
def test_paired_scatter_both_grid_orders_against_oracle(focal_scale, want_plane_major, res, pairing):
    """A wide fan runs the grid plane-major (every bundle of the first list entry, then of the second, ...), a narrow one
    bundle-major; which one ran follows from the fan's extents, which the kernel reads too."""
    pairing(2)
    R, ns, ni, zero_frac, bundle = SHAPES[2]
    wl = _workload(R, ns, ni, zero_frac, "trained", res, focal_scale=focal_scale)
    ro, rd, _ = _oracle_check(wl, R, ns, ni, bundle, f"paired {R}x{ns}+{ni} focal x{focal_scale} {res}")
    got, fan = _plane_major(ro, rd)
    print(f"margin paired grid order focal x{focal_scale}: fan extents {fan}, plane-major {got}")
    assert got == want_plane_major, fan


# ---- 2. paired against unpaired --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("R,ns,ni,bundle,res,kw", [(200, 24, 8, 1024, "same", {}), (640, 56, 8, 2048, "same", {}),
                                                  (37, 23, 6, 1024, "same", {}), (640, 56, 8, 2048, "default", {}),
                                                  (200, 24, 8, 1024, "default", dict(channels_last=False)),
                                                  (640, 56, 8, 2048, "same", dict(channels_last=False))])
def test_paired_equals_unpaired(R, ns, ni, bundle, res, kw, pairing):
    """The same rays, numbers and cotangents through the 12-plane grid (mode 0) and the paired one (mode 2).  The records of a
    pair are the same entry for entry, so a cell's sum is formed from the same contributions; only the order inside a cell (the
    counting sort's tickets) and of the atomics differs, as between two unpaired runs - whose difference sets the bar.  Decoder
    and beta gradients do not pass through the scatter and must not change by a bit."""
    from myslam_amd import harness
    wl = _set_res(harness.Workload("room0", R, ns, ni, t16._dev(), planes="synth", state="trained", **kw), "trained", res,
                  kw.get("channels_last", True))
    S = ns + ni

    def grads(mode, want):
        pairing(mode)
        g = wl.backward_with(wl.forward(fixed_rand=True))
        torch.cuda.synchronize()
        assert t16._last_backward_rank16() == 1 and _paired() == want
        return [t.detach().clone() for t in g]

    g_old, g_old2, g_new = grads(0, 0), grads(0, 0), grads(2, 1)
    got = t16._assert_rank16_path(wl, wl.rays_o, wl.rays_d, wl.R, S, bundle)
    n = lambda ts: [t16._n(t) for t in ts]
    x = t16._max_normalised(n(g_old2[:12]), n(g_old[:12]))
    bar = max(1e-5, 4.0 * x)
    e_planes = t16._max_normalised(n(g_new[:12]), n(g_old[:12]))
    same = [bool(torch.equal(a, b)) for a, b in zip(g_new[12:], g_old[12:])]
    print(f"margin paired vs unpaired {wl.R}x{S} {res} {kw} (bundle {got}): x = {x:.3e}, planes {e_planes:.3e} (bar {bar:.1e}), "
          f"decoder + beta gradients equal: {sum(same)} of {len(same)}")
    assert len(g_new) > 12 and all(float(g.abs().max()) > 0 for g in g_old[:12])
    assert e_planes <= bar, (e_planes, bar, x)
    assert all(same), same


# ---- 3. nothing crosses between the decoders -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("R,ns,ni,res", [(37, 23, 6, "same"), (640, 56, 8, "same"), (640, 56, 8, "default")])
def test_paired_walks_keep_the_decoders_apart(R, ns, ni, res, pairing):
    """Cotangents on depth and sdf, none on rgb: the colour decoder's half of gz is exactly zero, so every colour-plane gradient
    is exactly zero - unless a walk reads the SDF decoder's rows, expands by its slice or adds to its partner's plane.  The SDF
    planes' gradients are those of the unpaired grid (the bar of test 2)."""
    wl = _workload(R, ns, ni, 0.0, "trained", res)
    dev = wl.device
    ro, rd, gd = wl.rays_o[:R].detach(), wl.rays_d[:R].detach(), wl.gt_depth[:R]
    rand = tuple(t.to(dev) for t in hr.rand_for(R, ns, ni))
    cot = hr.cotangent(R, ns + ni).to(dev)

    def grads(mode, want):
        pairing(mode)
        t16._fresh(wl)
        depth, color, sdf, _ = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd, _rand=rand)
        ((depth * 0.7).sum() + (sdf * cot).sum()).backward()
        torch.cuda.synchronize()
        assert t16._last_backward_rank16() == 1 and _paired() == want
        return [p.grad.detach().clone() for p in wl.plane_list]

    g0, g0b, g2 = grads(0, 0), grads(0, 0), grads(2, 1)
    for name, g in (("unpaired", g0), ("paired", g2)):
        nz = [int((t != 0).sum()) for t in g[6:]]
        assert nz == [0] * 6, (name, nz)
        assert all(float(t.abs().max()) > 0 for t in g[:6]), name
    n = lambda ts: [t16._n(t) for t in ts]
    x = t16._max_normalised(n(g0b[:6]), n(g0[:6]))
    e = t16._max_normalised(n(g2[:6]), n(g0[:6]))
    print(f"margin paired decoders apart {R}x{ns + ni} {res}: colour planes exactly zero, SDF planes {e:.3e} (x = {x:.3e})")
    assert e <= max(1e-5, 4.0 * x), (e, x)


# ---- 4. the rays the pre-filter removes ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("state", hr.STATES)
@pytest.mark.parametrize("ns,ni", hr.SIZES)
def test_paired_unmasked_hostile_rays_against_oracle(ns, ni, state, pairing):
    """Origins outside the bound, zero or negative exits, depths beyond the box, axis-parallel directions, on fine planes of
    0.03 for both decoders: boxes the counting sort cannot hold, in workgroups that walk twice behind the bitonic fallback."""
    from tests import test_gpu_quad_walk as tqw
    pairing(2)
    wl = _workload(256, ns, ni, 0.0, state, "fine", scene="toy")
    dev = wl.device
    b = t16._hostile(True)
    ro, rd, gd = b.rays_o.to(dev), b.rays_d.to(dev), b.gt_depth.to(dev)
    R, S = ro.shape[0], ns + ni
    rand = tuple(t.to(dev) for t in hr.rand_for(R, ns, ni))
    cot = hr.cotangent(R, S)
    mine, z = t16._render_backward(wl, ro, rd, gd, rand, cot)
    assert _paired() == 1
    t16._assert_rank16_path(wl, ro, rd, R, S)
    assert all(np.isfinite(g).all() for g in mine["planes"]) and all(np.isfinite(g).all() for g in mine["dec"].values())
    # the 12 planes' lists come plane by plane, bundle by bundle: a fine plane of the first six is walked by a paired workgroup
    nb = -(-R // (t16._assert_rank16_path(wl, ro, rd, R, S) // S))
    fits = [counting for _, _, _, _, counting in tqw._lists(wl, ro, rd, z)]
    assert len(fits) == 12 * nb
    fallback = sum(not fits[pi * nb + k] for pi in (1, 3, 5) for k in range(nb))
    print(f"margin paired hostile {ns}+{ni} {state}: {fallback} of {3 * nb} paired fine-plane workgroups take the bitonic fallback")
    assert fallback > 0
    mdl = t16._cpu_model(wl)
    o64, o32 = (hr.oracle_step(mdl, wl.scene, b, z, cot, dt) for dt in (torch.float64, torch.float32))
    pn, amb = hr.ambiguous(mdl, wl.scene, b, z)
    t16._accept(mine, o32, o64, pn, amb, wl.scene, f"paired hostile {ns}+{ni} {state}")


# ---- 5. planes that do not agree -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("R,ns,ni,zero_frac,bundle", SHAPES[1:])
def test_planes_of_other_resolutions_stay_unpaired(R, ns, ni, zero_frac, bundle, pairing):
    pairing(2)
    wl = _workload(R, ns, ni, zero_frac, "trained", "other")
    _oracle_check(wl, R, ns, ni, bundle, f"unpaired (other resolutions) {R}x{ns}+{ni}", want_paired=0)


# ---- 6. the auto rule ------------------------------------------------------------------------------------------------------
@gpu
def test_auto_mode_leaves_a_small_batch_unpaired(pairing):
    pairing(1)
    R, ns, ni, zero_frac, bundle = SHAPES[1]
    wl = _workload(R, ns, ni, zero_frac, "trained", "same")
    _oracle_check(wl, R, ns, ni, bundle, f"auto {R}x{ns}+{ni}", want_paired=0)


def test_auto_rule_arithmetic():
    """Pair when the shorter grid still gives every compute unit three workgroups: bundles x (12 - pairs) >= 3 x CUs (256 on an
    MI355X).  Host arithmetic only."""
    from myslam_amd import _hip
    _hip.load_library()
    lib = _hip.lib()
    auto = lambda R, S, pairs, cus=256: lib.eslam_scatter_pairs_auto(R, S, cus, pairs)
    nb = lambda R, S: -(-R // (lib.eslam_scatter_bundle_samples(R, S, 1) // S))
    assert nb(4096, 64) == 128 and nb(8192, 96) == 391 and nb(2048, 64) == 64
    assert auto(4096, 64, 6) == 1          # 768 = 768: exactly one round at three per CU
    assert auto(4096, 64, 3) == 1          # the shipped shapes: 128 x 9
    assert auto(8192, 96, 6) == 1 and auto(8192, 96, 3) == 1
    assert auto(2048, 64, 6) == 0 and auto(2048, 64, 3) == 0
    assert auto(200, 32, 6) == 0 and auto(200, 32, 3) == 0
    assert auto(4096, 64, 6, cus=257) == 0 and auto(4096, 64, 0) == 0 and auto(4096, 64, 7) == 0
    assert auto(0, 64, 6) == 0 and auto(4096, 0, 6) == 0 and auto(4096, 64, 6, cus=0) == 0
