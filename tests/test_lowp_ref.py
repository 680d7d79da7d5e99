"""Pins tests/lowp_ref.py, the float64 model of the mixed-precision kernels, on the CPU: its rounders bit for bit against
torch's bfloat16 / half types, the model with identity rounders against the plain oracle, the model in float32 against the
model in float64 under the acceptance criteria the GPU test applies to the kernels (tests/test_gpu_lowp_parity.py) - and those
criteria against six one-rounding-point mutations of the model, each of which they must reject."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import lowp_ref as lr


def _f32(bits):
    return torch.tensor(np.asarray(bits, dtype=np.uint32).view(np.float32))


def _bits(t):
    return t.to(torch.float32).contiguous().view(torch.int32)


def test_bf16_rounder_bits():
    """bf16_rne = f2bf of the kernels = torch's float32 -> bfloat16 conversion, bit for bit."""
    base = np.array([0x3F800000, 0x3F810000, 0x40490000, 0x00800000, 0x7F7E0000, 0x3DCC0000, 0x00010000, 0x33000000], dtype=np.uint32)
    low = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)   # below, at and above the tie
    sweep = (base[:, None] + low[None, :]).reshape(-1)            # even (ties to even) and odd (ties up) kept mantissas
    extra = np.array([0x00000000, 0x80000000,                     # +-0
                      0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x007FFFFF, 0x807FFFFF,     # float32 subnormals
                      0x7F7F0000, 0xFF7F0000,                     # the largest finite bf16
                      0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0xFF7FFFFF,                 # round up to +-inf
                      0x7F800000, 0xFF800000], dtype=np.uint32)
    rng = np.random.default_rng(0)
    rnd = rng.integers(0, 2 ** 32, 200_000, dtype=np.uint64).astype(np.uint32)
    rnd = rnd[(rnd & 0x7F800000) != 0x7F800000]                   # finite (NaN payloads are out of scope)
    for bits in (sweep, sweep | np.uint32(0x80000000), extra, rnd):
        x = _f32(bits)
        assert torch.equal(_bits(lr.bf16_rne(x)), _bits(x.bfloat16().float()))
        assert torch.equal(_bits(lr.bf16_rne(x.double())), _bits(x.bfloat16().float()))      # float64 carrier, same value
    x = _f32(sweep)
    assert not torch.equal(lr.bf16_trunc(x), lr.bf16_rne(x))
    assert (lr.bf16_trunc(x).abs() <= x.abs()).all()


def test_fp16_rounder_bits():
    """fp16_rne = the (_Float16) conversion of planes_to_half_kernel = torch's float32 -> half, bit for bit."""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)         # every finite non-negative half
    mid = (h[:-1] + h[1:]) / 2                                                            # every tie (exact in float32)
    vals = np.concatenate([h, mid, np.nextafter(mid.astype(np.float32), np.float32(0)).astype(np.float64),
                           np.nextafter(mid.astype(np.float32), np.float32(np.inf)).astype(np.float64),
                           [65504.0, 65519.996, 65520.0, 65536.0, 1e5, 3e38, np.inf,      # the last finite half, then inf
                            2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 2.0 ** -26, 1e-10, 0.0]])
    rng = np.random.default_rng(1)
    vals = np.concatenate([vals, rng.normal(0.0, 0.01, 200_000), rng.normal(0.0, 1e-5, 50_000)])   # plane values ~ N(0, 0.01): subnormals occur
    x = torch.tensor(np.concatenate([vals, -vals]).astype(np.float32))
    assert (x.half().float().abs() < 2.0 ** -14).sum() > 1000 and torch.isinf(x.half()).sum() > 4
    got, want = lr.fp16_rne(x), x.half().float()
    assert torch.equal(_bits(got), _bits(want))                   # signed zeros included
    assert torch.equal(_bits(lr.fp16_rne(x.double())), _bits(want))


def _plain_with_z(fx, z):
    """oracle/eslam_oracle.py itself (float64) on given z_vals, with the fixture's loss and autograd."""
    from oracle import eslam_oracle as orc
    dt = torch.float64
    sc, planes = hp.scene_and_planes(fx, channels_last=False)                 # the float32 masters, converted exactly
    planes = tuple([p.to(dt).requires_grad_(True) for p in grp] for grp in planes)
    params = hp.params_from(fx, dtype=dt, requires_grad=True)
    beta = torch.tensor([float(fx["beta"])], dtype=dt, requires_grad=True) if bool(fx["beta_is_param"]) else float(fx["beta"])
    cv = lambda k: torch.from_numpy(fx[k]).to(dt)
    depth, color, sdf, zz = orc.render_batch_ray(planes, params, beta, sc.bound, cv("rays_d"), cv("rays_o"), float(fx["truncation"]),
                                                 cv("gt_depth"), int(fx["n_stratified"]), int(fx["n_importance"]),
                                                 z_vals=torch.from_numpy(z).to(dt))
    loss = (orc.mapping_loss if str(fx["loss_kind"]) == "mapping" else orc.tracking_loss)(
        depth, color, sdf, zz, cv("gt_depth"), cv("gt_color"), float(fx["truncation"]))
    loss.backward()
    return dict(depth=depth, color=color, sdf=sdf, loss=loss, planes=planes, params=params, beta=beta)


def test_identity_rounders_give_the_plain_oracle():
    """With every rounder replaced by the identity the model IS oracle/eslam_oracle.py: outputs and every gradient to 1e-12."""
    fx = hp.load("room0_200x40_trained_zero15")
    z = lr.float32_z(fx)
    o = _plain_with_z(fx, z)
    m = lr.run_model(lr.Model.identity(), fx, z)
    for k in ("depth", "color", "sdf"):
        assert hp.rel_err(m[k], o[k].detach().numpy()) <= 1e-12, k
    assert abs(m["loss"] - float(o["loss"])) <= 1e-12 * abs(float(o["loss"]))
    for a, b in zip(m["planes"], hp.flat_planes(o["planes"])):
        assert hp.rel_err(a, b.grad.numpy()) <= 1e-12
    for k, p in o["params"].items():
        assert hp.rel_err(m["dec"][k], p.grad.numpy()) <= 1e-12, k
    assert hp.rel_err(m["beta"], o["beta"].grad.numpy()) <= 1e-12
    # and the rounded model is a different function, by about the quantisation
    q = lr.run_model(lr.Model(), fx, z, backward=False)
    assert 1e-5 < np.abs(q["sdf"] - m["sdf"]).max() < 5e-3


class _SomeRays:
    """A fixture restricted to every `step`-th ray (the per-ray arrays; everything else is the fixture's)."""
    PER_RAY = ("rays_o", "rays_d", "gt_depth", "gt_color")

    def __init__(self, fx, step):
        self.fx, self.step, self.files = fx, step, fx.files

    def __getitem__(self, k):
        return np.ascontiguousarray(self.fx[k][::self.step]) if k in self.PER_RAY else self.fx[k]


FORWARD_RAY_STEP = 8        # forward-only comparisons are per sample / per ray: every 8th ray (>= 512 rays, >= 28 000 samples,
                            # 3.6 million features) shows the same shares as all of them at an eighth of the float64 model's cost


@functools.lru_cache(maxsize=None)
def _z(case):
    return lr.float32_z(hp.load(case))           # sampled on the whole fixture (the recorded random numbers are per batch)


@functools.lru_cache(maxsize=None)
def _reference(case, step=1):
    """Per fixture (step > 1: forward only, on every step-th ray), once per module: float32 z_vals, the free-running float64
    model, the plain oracle."""
    fx = hp.load(case)
    z = _z(case)
    bw = str(fx["loss_kind"]) == "mapping" and step == 1
    if step > 1:
        fx, z = _SomeRays(fx, step), np.ascontiguousarray(z[::step])
    free = lr.run_model(lr.Model(), fx, z, backward=False)
    plain = lr.run_model(lr.Model.identity(), fx, z) if bw else None
    return fx, z, fx["gt_depth"] > 0, bw, free, plain


def _against_the_model(case, model, backward, label):
    """`model`'s evaluation of a fixture under THE assertion, exactly as the GPU test holds the kernels' to it: features
    against the free-running float64 model, everything else against the float64 model teacher-forced with `model`'s features.
    backward=False: forward quantities only, on every FORWARD_RAY_STEP-th ray."""
    fx, z, hd, bw, free, plain = _reference(case, 1 if backward else FORWARD_RAY_STEP)
    backward = backward and bw
    got = lr.run_model(model, fx, z, backward=backward)
    ref = lr.run_model(lr.Model(), fx, z, backward=backward, feat=got["feat"])
    return lr.assert_agrees(got, ref, hd, lr.criteria(case, ref), plain if backward else None, free, label=f"{case} {label}")


@pytest.mark.parametrize("case", lr.MIXED_FIXTURES + (lr.TRACKING_FIXTURE,))
def test_float32_model_agrees_with_float64_model(case):
    """The reference alone stays inside the criteria: the model accumulated in float32 against the model accumulated in
    float64, on the same float32 z_vals.  The printed line re-measures the figures recorded in lowp_ref.CPU_SELF_AGREEMENT
    (torch's float32 sums depend on its thread count: the gradient figures move by up to 1.5x between runs)."""
    m = _against_the_model(case, lr.Model(torch.float32), True, "float32 model vs float64 model")
    for k, v in lr.CPU_SELF_AGREEMENT[case]["q97"].items():
        assert (m[k] > lr.MARGIN * v).mean() <= 0.03, k                # "the reference alone sits at <= 3 %"


_SHARE = r": \d\.\d+ of the samples beyond"
MUTATIONS = {
    # name: (the mutated model, whether the mutation only shows in the backward pass, the criterion that must be the one to fire
    # - a pattern in lowp_ref.failures' wording)
    "f2bf truncates instead of rounding to nearest even": (dict(bf=lr.bf16_trunc), False, "features: share unequal"),
    "h2 is not rounded to bf16": (dict(round_h2=False), False, "sdf" + _SHARE),
    "biases are rounded to bf16": (dict(bias=lr.bf16_rne), False, "sdf" + _SHARE),
    "planes are rounded to bf16 instead of fp16": (dict(plane=lr.bf16_rne), False, "features: share unequal"),
    "backward operands are not rounded": (dict(round_bwd=False), True, "plane gradients"),
    "two W1 columns are swapped": (dict(swap_w1=(21, 29)), False, "sdf" + _SHARE),
}


@pytest.mark.parametrize("case", lr.MIXED_FIXTURES)
@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_criteria_reject_one_wrong_rounding_point(case, mutation):
    """The acceptance criteria discriminate at the level of ONE wrong rounding point: each mutation of the model, held
    against the true model by the assertion the GPU test uses, on an initial-state and a trained-state fixture, fails - on
    the criterion that is about the mutated quantity, not on any assertion.  (A forward-only mutation is held against the
    model on every FORWARD_RAY_STEP-th ray of the fixture.)"""
    kw, needs_backward, fires = MUTATIONS[mutation]
    with pytest.raises(AssertionError, match=fires) as e:
        _against_the_model(case, lr.Model(**kw), needs_backward, mutation)
    print(e.value)


@pytest.mark.parametrize("R,S", lr.EXACT_SHAPES)
def test_exact_arithmetic_inputs_verify_themselves(R, S):
    """lowp_ref.exact_case asserts that nothing it feeds a rounder has anything to round; the rounded model and the plain
    oracle are then the same numbers (asserted inside).  A wrong rounding point is still visible on these inputs where it
    rounds what should NOT be rounded: biases."""
    c = lr.exact_case(R, S)
    args = (tuple([p.double() for p in grp] for grp in c["planes"]), {k: v.double() for k, v in c["params"].items()}, c["beta"],
            c["bound"], c["rays_o"].double(), c["rays_d"].double(), c["z_vals"].double())
    with torch.no_grad():
        mut = lr.Model(bias=lr.bf16_rne).render(*args)
    assert hp.rel_err(mut["sdf"].numpy(), c["oracle"]["sdf"].numpy()) > 1e-4
