"""Pins tests/lowp_points_ref.py on the CPU: the free-point model with identity rounders is the plain oracle, the float32
model meets the criteria the GPU test applies to the kernels (tests/test_gpu_lowp_points.py), and those criteria reject the
two things that a free-point path short of the issue would compute:

  mutant 1  the float32 field on the masters - what the free-point entries computed inside ops.mixed_precision before there
            was `points=True` - against the forward criteria;
  mutant 2  the position derivative taken on the float32 masters behind a forward on the copies (an unchanged float32
            coord_bwd_kernel; lowp_pose_ref.ShortcutModel for points) against the point-wise g_pts criterion - and NOT against
            the tensor-wide one, which a single ReLU flip of the float32 model widens past it: nobody may rely on that bar.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import eslam_oracle as orc
from tests import helpers as hp
from tests import lowp_points_ref as P
from tests import lowp_ref as lr

STATES = tuple(P.STATES)


@pytest.mark.parametrize("name", STATES)
def test_identity_model_is_the_plain_oracle(name):
    st = P.state(name)
    n = 2000
    got = P.gradients(lr.Model.identity(), st, n)
    planes = tuple([p.double().requires_grad_(True) for p in grp] for grp in st["planes"])
    params = {k: v.double().requires_grad_(True) for k, v in st["params"].items()}
    pts = st["pts"][:n].double().requires_grad_(True)
    raw = orc.decode(pts, planes, params, st["bound"])
    (raw * st["G"][:n].double()).sum().backward()
    assert hp.rel_err(got["raw"], raw.detach().numpy()) <= 1e-13
    assert hp.rel_err(got["g_pts"], pts.grad.numpy()) <= 1e-12
    for a, p in zip(got["planes"], hp.flat_planes(planes)):
        assert hp.rel_err(a, p.grad.numpy()) <= 1e-12
    for k, p in params.items():
        assert hp.rel_err(got["dec"][k], p.grad.numpy()) <= 1e-12
    b = st["bound"]
    outside = ~((st["pts"] > b[:, 0]) & (st["pts"] < b[:, 1])).all(1)
    assert 0.03 < float(outside.float().mean()) < 0.09                    # the padding puts about 5.5 % of the points outside
    assert (got["g_pts"][outside[:n].numpy()] == 0).any(axis=1).all()     # the border clamp: no gradient for that coordinate


@functools.lru_cache(maxsize=None)
def _float32_run(name):
    """The float32 model free-running on the full set, and the pair forced with its features."""
    st = P.state(name)
    got = P.gradients(lr.Model(torch.float32), st)
    return got, P.model_pair(name, st["pts"].shape[0], got["feat"])


@pytest.mark.parametrize("name", STATES)
def test_float32_model_meets_the_criteria(name):
    """The reference itself stays far inside the caps: 0 % of the points beyond T (T about 3e-7)."""
    got, (ref, f32) = _float32_run(name)
    fig = P.full_set_figures(name)
    rep = []
    bad = P.forward_failures(got, ref, f32, fig["cap"], rep) + P.feature_failures(got, name, rep) + P.gradient_failures(got, ref, f32, rep)
    print(f"{name}: " + "; ".join(rep))
    assert not bad, bad
    assert 2e-3 < fig["feat_rate"] < 1e-2
    m = P._measure(got, ref)
    for k in P.QUANTITIES:
        scale = float(np.abs(P._as_measure(ref)[k]).max())
        T = P.MARGIN * max(float(np.quantile(P._measure(f32, ref)[k], 0.97)), lr.EPS32 * scale)
        assert T < 1e-6 and float((m[k] > T).mean()) == 0.0


@pytest.mark.parametrize("name", STATES)
def test_forward_criteria_reject_the_float32_field(name):
    """Mutant 1.  Its saved features are the bf16 roundings of what it gathered from the masters, and the models are forced
    with them like with any run's: what is left to tell is the decoders' own arithmetic."""
    st = P.state(name)
    mut = P.gradients(lr.Model.identity(torch.float32), st, backward=False)
    mut["feat"] = lr.bf16_rne(torch.from_numpy(mut["feat"])).numpy()
    ref, f32 = P.model_pair(name, st["pts"].shape[0], mut["feat"], backward=False)
    rep = []
    bad = P.forward_failures(mut, ref, f32, P.full_set_figures(name)["cap"], rep)
    print(f"{name}: " + "; ".join(rep))
    assert any(b.startswith("color") for b in bad) and any(b.startswith("sdf") for b in bad), bad
    mg, mf = P._measure(mut, ref), P._measure(f32, ref)
    for k in P.QUANTITIES:
        T = P.MARGIN * max(float(np.quantile(mf[k], 0.97)), lr.EPS32 * float(np.abs(P._as_measure(ref)[k]).max()))
        assert float((mg[k] > T).mean()) >= 0.999, (k, T)
    # and the feature criteria reject it on their own: the masters' features are not the copies'
    assert P.feature_failures(mut, name)


@pytest.mark.parametrize("name", STATES)
def test_pointwise_criterion_rejects_the_derivative_on_the_masters(name):
    """Mutant 2, on the states' unpadded points."""
    from tests.test_oracle_golden import OUT_RTOL
    st = P.state(name)
    n = st["pts_plain"].shape[0]
    model = P.gradients(lr.Model(), st, pts="pts_plain")
    mut = P.gradients(lr.Model(), st, feat=model["feat"], pts="pts_plain", fn=P.shortcut_decode)
    assert np.array_equal(mut["raw"], model["raw"]) and np.array_equal(mut["feat"], model["feat"])      # the forward is the model's
    ref, f32 = P.model_pair(name, n, model["feat"], pts="pts_plain")
    x = P.point_excess(mut, ref, f32)
    e, fig = hp.rel_err(mut["g_pts"], ref["g_pts"]), hp.rel_err(f32["g_pts"], ref["g_pts"])
    print(f"{name}: mutant's worst point at {x:.2f} of its own bar; tensor-wide {e:.2e} against a bar of "
          f"{P.MARGIN * max(fig, OUT_RTOL):.2e} (float32 model {fig:.2e})")
    assert x > 1.5
    assert any(b.startswith("g_pts: a point") for b in P.gradient_failures(mut, ref, f32))
    # the tensor-wide bar alone lets it through: one point of the float32 model with a hidden pre-activation within float32
    # summation error of zero sets that bar
    assert e > OUT_RTOL and e <= P.MARGIN * max(fig, OUT_RTOL)
    # everything but the position derivative is the model's
    assert not P.gradient_failures(mut, ref, f32, which=("planes", "dec"))


def test_sizes_cover_blocks_tiles_and_workgroups():
    assert P.sizes("trained") == P.SIZES
    assert P.sizes("initial") == P.SIZES[:-1] + (6400,)
