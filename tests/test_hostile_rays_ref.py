"""What tests/test_gpu_hostile_rays.py rests on, without a GPU: the hostile batch (tests/hostile_rays.py) is what its
docstring says, the float64 oracle handles classes 1-7, the float32 oracle MEETS the acceptance criteria the kernels are held
to on this batch (so a correct float32 implementation can), the share of ReLU-ambiguous samples stays under the suite's cap,
and the tensor-op mirror of eslam_mark_rays marks every texel the oracle's samples touch.

Run time: ~6 s (the toy scene; eight float32 / float64 oracle steps of 84 rays x 32 / 96 samples).
"""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import hostile_rays as hr


@functools.lru_cache(maxsize=None)
def _scene():
    from myslam_amd import scene as scn
    return scn.make_scene("toy")


@functools.lru_cache(maxsize=None)
def _batch(finite=True):
    return hr.make(_scene(), classes=hr.FINITE_CLASSES if finite else hr.ALL_CLASSES)


@functools.lru_cache(maxsize=None)
def _sampled(ns, ni, state, stream=7):
    """The batch's z_vals under the float32 and the float64 oracle, once per configuration."""
    sc, b = _scene(), _batch()
    mdl = hr.model(sc, state)
    rand = hr.rand_for(b.rays_o.shape[0], ns, ni, stream)
    return mdl, hr.oracle_z(mdl, sc, b, ns, ni, rand, torch.float32), hr.oracle_z(mdl, sc, b, ns, ni, rand, torch.float64)


def test_the_batch_is_what_its_classes_say():
    from oracle import eslam_oracle as orc
    sc = _scene()
    b = _batch(finite=False)
    assert b.rays_o.shape == (96, 3) and b.rays_o.dtype == torch.float32 and torch.equal(b.cls, torch.arange(1, 9).repeat_interleave(12))
    lo, hi = sc.bound[:, 0], sc.bound[:, 1]
    inside = ((b.rays_o >= lo) & (b.rays_o <= hi)).all(1)
    ext = orc.aabb_exit(b.rays_o, b.rays_d, sc.bound)
    tau = sc.truncation
    c = lambda k: b.cls == k
    norm = b.rays_d.norm(dim=1)
    assert bool(((norm > 0.99) & (norm < 1.51)).all()), "unnormalised directions, as get_rays gives them"
    assert not inside[c(1) | c(2) | c(3)].any() and inside[c(4) | c(5) | c(6) | c(7) | c(8)].all()
    assert bool((ext[c(1)] < -0.05).all()) and bool((b.gt_depth[c(1) | c(2) | c(7) | c(8)] == 0).all())
    assert bool((ext[c(2)] > 0.5).all())
    # class 3: the sample interval of the even rays ends in front of the box, that of the odd rays crosses the face
    m3 = c(3).nonzero().squeeze(1)
    ilo, ihi = hr.interval(b, sc)
    end_inside = lambda r, t: bool(((b.rays_o[r].double() + b.rays_d[r].double() * t >= lo.double()) &
                                    (b.rays_o[r].double() + b.rays_d[r].double() * t <= hi.double())).all())
    assert bool((b.gt_depth[m3] > 0).all())
    assert not any(end_inside(int(r), ihi[r]) for r in m3[0::2]) and all(end_inside(int(r), ihi[r]) for r in m3[1::2])
    assert bool((b.gt_depth[c(4)] > ext[c(4)]).all()) and bool((ext[c(4)] > 0).all())
    assert bool(((b.gt_depth[c(5)] > 0) & (b.gt_depth[c(5)] < 1.5 * tau)).all())
    nz = (b.rays_d[c(6)] == 0).sum(1)
    assert set(nz.tolist()) == {1, 2} and bool(torch.signbit(b.rays_d[c(6)][b.rays_d[c(6)] == 0]).any()) \
        and not bool(torch.signbit(b.rays_d[c(6)][b.rays_d[c(6)] == 0]).all())
    assert 0 < int((b.gt_depth[c(6)] == 0).sum()) < 12 and bool(torch.isfinite(ext[c(6)]).all())
    assert bool(((ext[c(7)] > 0) & (ext[c(7)] + 0.01 < 0.02)).all())
    assert bool(torch.isnan(ext[c(8)]).all()) and bool(torch.isfinite(ext[~c(8)]).all())
    # the pre-filter (Mapper.py:325-327) removes classes 1, 4 and 8 outright and keeps class 5
    keep = ext >= b.gt_depth
    assert not keep[c(1) | c(4) | c(8)].any() and keep[c(5)].all()


@pytest.mark.parametrize("state", hr.STATES)
@pytest.mark.parametrize("ns,ni", hr.SIZES)
def test_oracle_samples_are_finite_sorted_and_inside_the_documented_interval(ns, ni, state):
    sc, b = _scene(), _batch()
    mdl, z32, z64 = _sampled(ns, ni, state)
    lo, hi = hr.interval(b, sc)
    assert bool((lo <= hi).all()) and bool((lo <= 0).all()) and bool((hi >= 0).all())
    for z, tol in ((z64, 1e-12), (z32.double(), 1e-6)):
        assert z.shape == (84, ns + ni) and bool(torch.isfinite(z).all())
        assert bool((z[:, 1:] >= z[:, :-1]).all())
        span = (hi - lo)[:, None]
        assert bool((z >= lo[:, None] - tol * (1 + span)).all()) and bool((z <= hi[:, None] + tol * (1 + span)).all())
    far_neg = b.cls == 1
    assert bool((z64[far_neg] <= 0).all()) and bool((z64[far_neg][:, 0] < -0.05).all()), "far < 0: z in [far, 0]"
    # the float32 oracle's own rows pass the sampler criteria of the GPU tests - for the whole batch and for the two classes
    # that reach the all-pairs rank sort of the importance sampler (far <= 0, ties)
    hr.check_z(z32, z32, z64, b.gt_depth, label="all")
    for k in (1, 7):
        m = b.cls == k
        hr.check_z(z32[m], z32[m], z64[m], b.gt_depth[m], label=f"class {k}")


@pytest.mark.parametrize("state", hr.STATES)
@pytest.mark.parametrize("ns,ni", hr.SIZES)
def test_float32_oracle_meets_the_acceptance_criteria_of_the_gpu_tests(ns, ni, state):
    """render_batch_ray of the oracle is finite in float32 and float64 on classes 1-7, the float32 one passes hr.accept
    against the float64 one on the float32 sampler's z_vals, and the ambiguous-sample share is under the suite's cap."""
    sc, b = _scene(), _batch()
    mdl, z32, _ = _sampled(ns, ni, state)
    cot = hr.cotangent(84, ns + ni)
    o32, o64 = (hr.oracle_step(mdl, sc, b, z32, cot, dt) for dt in (torch.float32, torch.float64))
    for o in (o32, o64):
        for k in ("depth", "color", "sdf", "ro", "rd"):
            assert np.isfinite(o[k]).all(), k
        assert all(np.isfinite(g).all() for g in o["planes"]) and all(np.isfinite(g).all() for g in o["dec"].values())
    pn, amb = hr.ambiguous(mdl, sc, b, z32)
    share = float(amb.float().mean())
    print(f"ambiguous samples: {int(amb.sum())} of {amb.numel()} = {share:.2e} (cap {hr.AMBIGUOUS_CAP:.0e})")
    assert share <= hr.AMBIGUOUS_CAP
    rep = hr.accept(o32, o32, o64, pn, amb, sc, label=f"{ns}+{ni} {state}")
    print("float32 oracle / bar:", {k: round(v, 3) for k, v in rep.items()})


def test_cpu_marking_contains_every_texel_the_oracle_samples_touch():
    """parallel.mark_rays (the tensor-op mirror of eslam_mark_rays) over classes 1-7 is a superset of the bilinear corners of
    the oracle's samples over several jitter draws, per class - and tight: every marked texel lies within 2 texels of one
    the documented interval reaches (float64 dense stepping)."""
    from oracle import eslam_oracle as orc
    from myslam_amd import parallel
    sc, b = _scene(), _batch()
    base, n = hr.block_base(sc)
    b6 = [float(v) for v in sc.bound.reshape(-1)]
    ns, ni = 24, 8
    for k in hr.FINITE_CLASSES:
        bk = hr.select(b, (k,))
        marked = parallel.mark_rays(hr.plane_hw(sc), b6, bk.rays_o, bk.rays_d, bk.gt_depth, sc.truncation, base, n).bool()
        for state, stream in (("initial", 7), ("trained", 20), ("trained", 33)):
            _, z32, z64 = _sampled(ns, ni, state, stream)
            for z in (z32.double(), z64):
                pts = bk.rays_o.double()[:, None, :] + bk.rays_d.double()[:, None, :] * z[b.cls == k][..., None]
                touched = hr.texel_mask(sc, orc.normalize_points(pts.reshape(-1, 3), sc.bound.double()))
                assert int((touched & ~marked).sum()) == 0, (k, state, int((touched & ~marked).sum()), int(touched.sum()))
        near = hr.dilate(sc, hr.reach_mask(sc, bk), 2)
        assert int((marked & ~near).sum()) == 0, (k, int((marked & ~near).sum()), int(marked.sum()))
        assert int(marked.sum()) > 0
