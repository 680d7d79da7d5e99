"""The rank-16 scatter's walk takes four sorted entries per step (scatter_sort_kernel<GZ>; tests/quad_walk_ref.py restates its
bookkeeping in numpy).  The criteria are those of tests/test_gpu_rank16_scatter.py, on shapes chosen for the new bookkeeping:

  1  against the oracle (float32 / float64, hp.plane_grads_close at RTOL = 1e-4): a single ray, bundles whose sample count is no
     multiple of four (S = 29: 1015 and 58 samples) and exactly 2048, both bundle sizes, initial and trained state
  2  against the full-width path on the same inputs and cotangents: planes within max(1e-5, 4 x the difference of two full-width
     runs), decoder and beta gradients EQUAL; channels-last and NCHW planes
  3  the rays the callers' pre-filter removes (tests/hostile_rays.py): boxes too large for the counting sort, all-padding waves
  4  the inputs of 1-3 reach every case of the bookkeeping: with the kernel's own ray orders and z_vals, the numpy model of the
     sorted lists (quad_walk_ref.kernel_cells / cases) shows a fresh entry at each of the four positions of a step, adjacent and
     not, a cell that spans a 64-entry block and one that spans a wave boundary

Margins measured on an MI355X (`pytest -s`, the lines starting with "margin"): profiles/r08/quad_walk_margins.txt.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import hostile_rays as hr
from tests import quad_walk_ref as qw
from tests import test_gpu_rank16_scatter as t16

pytestmark = pytest.mark.gpu

# (R, n_strat, n_imp, zero_frac, bundle the shape must run with)
SHAPES = [(1, 5, 3, 0.0, 1024), (3, 24, 8, 0.0, 1024), (33, 16, 0, 0.0, 1024), (37, 23, 6, 0.0, 1024), (65, 200, 56, 0.2, 1024),
          (200, 24, 8, 0.0, 1024), (640, 56, 8, 0.1, 2048)]


def _workload(R, ns, ni, zero_frac, state, **kw):
    from myslam_amd import harness
    return harness.make_workload("room0", max(R, 8), ns, ni, device=t16._dev(), zero_frac=zero_frac, planes="synth", state=state, **kw)


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,ns,ni,zero_frac,bundle", SHAPES)
@pytest.mark.parametrize("state", ["initial", "trained"])
def test_quad_walk_against_oracle(R, ns, ni, zero_frac, bundle, state):
    wl = _workload(R, ns, ni, zero_frac, state)
    dev, S = wl.device, ns + ni
    ro, rd, gd = wl.rays_o[:R].detach(), wl.rays_d[:R].detach(), wl.gt_depth[:R]
    assert ro.shape[0] == R
    rand = tuple(t.to(dev) for t in hr.rand_for(R, ns, ni))
    cot = hr.cotangent(R, S)
    mine, z = t16._render_backward(wl, ro, rd, gd, rand, cot)
    t16._assert_rank16_path(wl, ro, rd, R, S, bundle)
    if (R, S) == (640, 64):
        assert 2048 // S * S == 2048 and R % (2048 // S) == 0          # every bundle holds exactly 2048 samples
    if (R, S) == (37, 29):
        assert (1024 // S * S) % 4 and ((R % (1024 // S)) * S) % 4     # 1015 and 58 samples: no multiple of four
    b = SimpleNamespace(rays_o=ro.cpu(), rays_d=rd.cpu(), gt_depth=gd.cpu())
    mdl = t16._cpu_model(wl)
    o64, o32 = (hr.oracle_step(mdl, wl.scene, b, z, cot, dt) for dt in (torch.float64, torch.float32))
    pn, amb = hr.ambiguous(mdl, wl.scene, b, z)
    t16._accept(mine, o32, o64, pn, amb, wl.scene, f"quad walk {R}x{ns}+{ni} {state}")


# ---- 2. against the full-width path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,ns,ni,bundle,kw", [(200, 24, 8, 1024, {}), (640, 56, 8, 2048, {}), (37, 23, 6, 1024, {}),
                                               (200, 24, 8, 1024, dict(channels_last=False)),
                                               (640, 56, 8, 2048, dict(channels_last=False))])
def test_quad_walk_equals_full_width_path(R, ns, ni, bundle, kw):
    """The same rays, numbers and cotangents with ray gradients requested (full-width rows, one entry per step) and without (rank
    16, four per step).  A cell's sum is four partial sums added once - the same contributions in another float order, which the
    unordered atomics already allow between two runs: the bar is the one between two full-width runs.  Decoder and beta gradients
    do not pass through the scatter and must not change by a bit."""
    from myslam_amd import harness
    dev = t16._dev()
    mk = lambda rg: harness.Workload("room0", R, ns, ni, dev, planes="synth", state="trained", rays_grad=rg, **kw)
    old, new = mk(True), mk(False)
    S = ns + ni

    def grads(wl):
        g = wl.backward_with(wl.forward(fixed_rand=True))
        torch.cuda.synchronize()
        assert t16._last_backward_rank16() == (0 if wl is old else 1), "the library dispatched the other pair of kernels"
        return [t.detach().clone() for t in g]

    g_old, g_old2, g_new = grads(old), grads(old), grads(new)
    t16._assert_full_width_path(old.rays_o, old.rays_d)
    got = t16._assert_rank16_path(new, new.rays_o, new.rays_d, new.R, S, bundle)
    n = lambda ts: [t16._n(t) for t in ts]
    x = t16._max_normalised(n(g_old2[:12]), n(g_old[:12]))
    bar = max(1e-5, 4.0 * x)
    e_planes = t16._max_normalised(n(g_new[:12]), n(g_old[:12]))
    same = [bool(torch.equal(a, b)) for a, b in zip(g_new[12:], g_old[12:])]
    print(f"margin quad walk vs full width {new.R}x{S} {kw} (bundle {got}): x = {x:.3e}, planes {e_planes:.3e} (bar {bar:.1e}), "
          f"decoder + beta gradients equal: {sum(same)} of {len(same)}")
    assert len(g_new) > 12 and all(float(g.abs().max()) > 0 for g in g_old[:12])
    assert e_planes <= bar, (e_planes, bar, x)
    assert all(same), same


# ---- 3. the rays the pre-filter removes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", hr.STATES)
@pytest.mark.parametrize("ns,ni", hr.SIZES)
def test_quad_walk_unmasked_hostile_rays_against_oracle(ns, ni, state):
    """Origins outside the bound, zero or negative exits, depths beyond the box, axis-parallel directions: cells spread over boxes
    the counting sort cannot hold (the bitonic fallback) - the criteria of test 1."""
    t16.test_rank16_unmasked_hostile_rays_against_oracle(ns, ni, state)


# ---- 4. what the inputs reach ----------------------------------------------------------------------------------------------
def _lists(wl, ro, rd, z):
    """The sorted cell lists of every (bundle, plane) workgroup of a render backward, from the kernel's own ray orders and z_vals:
    yields (minor, major, step_m, entries a wave walks, whether the cells' box fits the counting sort)."""
    from myslam_amd import _hip, ops
    R, S = z.shape
    bm = _hip.lib().eslam_scatter_bundle_samples(R, S, 1)
    perm, side = ops.ray_order_async(ro, rd)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    perm = perm.cpu().numpy()[:3 * R].reshape(3, R)
    pts = (ro[:, None, :] + rd[:, None, :] * z[:, :, None]).float().cpu().numpy()
    bound = wl.scene.bound.detach().cpu().numpy().astype(np.float32)
    per = bm // S
    for pi, p in enumerate(wl.plane_list):
        o = (pi % 6) >> 1
        ph, pw = int(p.shape[2]), int(p.shape[3])
        for r0 in range(0, R, per):
            rays = perm[o, r0:r0 + per]
            minor, major, step_m = qw.kernel_cells(pts[rays].reshape(-1, 3), bound[:, 0], bound[:, 1], o, pw, ph)
            box = (int(minor.max() - minor.min()) + 2) * (int(major.max() - major.min()) + 1)
            yield minor, major, step_m, bm // 8, box <= 4 * bm


def test_inputs_reach_every_case_of_the_bookkeeping():
    seen, block_span, wave_span, fallback, padding_wave, sizes = set(), False, False, False, False, set()
    with torch.no_grad():
        for R, ns, ni, zero_frac, bundle in SHAPES:
            wl = _workload(R, ns, ni, zero_frac, "trained")
            dev = wl.device
            ro, rd, gd = wl.rays_o[:R].detach(), wl.rays_d[:R].detach(), wl.gt_depth[:R]
            rand = tuple(t.to(dev) for t in hr.rand_for(R, ns, ni))
            z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd, _rand=rand)[3]
            for minor, major, step_m, chunk, counting in _lists(wl, ro, rd, z):
                s, b, w = qw.cases(minor, major, step_m, chunk)
                seen |= s
                block_span |= b
                wave_span |= w
                padding_wave |= len(minor) <= 7 * chunk
                sizes.add(8 * chunk)
        # the hostile rays: boxes the counting sort cannot hold
        wl = t16._toy(*hr.SIZES[0], hr.STATES[0])
        hb = t16._hostile(True)
        ro, rd, gd = hb.rays_o.to(wl.device), hb.rays_d.to(wl.device), hb.gt_depth.to(wl.device)
        ns, ni = hr.SIZES[0]
        rand = tuple(t.to(wl.device) for t in hr.rand_for(ro.shape[0], ns, ni))
        z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, wl.device, wl.truncation, gt_depth=gd, _rand=rand)[3]
        for minor, major, step_m, chunk, counting in _lists(wl, ro, rd, z):
            s, b, w = qw.cases(minor, major, step_m, chunk)
            seen |= s
            fallback |= not counting
    print(f"margin quad walk coverage: cases {sorted(seen)}, block span {block_span}, wave span {wave_span}, bitonic fallback "
          f"{fallback}, all-padding wave {padding_wave}, bundle sizes {sorted(sizes)}")
    assert seen == qw.ALL_CASES, sorted(qw.ALL_CASES - seen)
    assert block_span and wave_span and fallback and padding_wave and sizes == {1024, 2048}
