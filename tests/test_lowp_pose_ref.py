"""Pins tests/lowp_pose_ref.py - the host model of the mixed-precision path's ray (pose) gradients - on the CPU, and shows
that the acceptance bar the GPU test applies to the kernel (tests/test_gpu_lowp_pose.py) tells the model apart from three
plausible wrong gradients.  Also the loop's switch, as far as it can be checked without a GPU.

Every test prints the figures it measured before it asserts (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import lowp_pose_ref as pr
from tests import lowp_ref as lr


@pytest.mark.parametrize("case", pr.PINNED_TO_REFERENCE)
def test_unrounded_model_reproduces_the_reference_ray_gradients(case):
    """With every rounder off the helper is the plain oracle: g_rays_o / g_rays_d of the reference itself (the fixture), on
    the reference's own z_vals."""
    from tests.test_oracle_golden import OUT_RTOL
    fx = hp.load(case)
    g_o, g_d, _ = pr.ray_grads(lr.Model.identity(), fx, fx["z_vals"])
    e = pr.errors((g_o, g_d), (fx["g_rays_o"], fx["g_rays_d"]))
    print(f"{case}: identity model against the reference's ray gradients {e[0]:.2e} / {e[1]:.2e}")
    assert e[0] <= OUT_RTOL and e[1] <= OUT_RTOL, e


@functools.lru_cache(maxsize=None)
def _case(case):
    """Once per fixture: the float32 model (free-running; its bf16 features are the forced ones), the float64 model forced
    with them and the bars."""
    fx = hp.load(case)
    z = lr.float32_z(fx)
    g_o, g_d, feat = pr.ray_grads(lr.Model(torch.float32), fx, z)
    ref = pr.ray_grads(lr.Model(), fx, z, feat)[:2]
    figure = pr.errors((g_o, g_d), ref)
    return fx, z, feat, ref, (g_o, g_d), figure, pr.bars(figure)


@pytest.mark.parametrize("case", pr.POSE_FIXTURES)
def test_bar_rejects_wrong_gradients(case):
    fx, z, feat, ref, f32, figure, bar = _case(case)
    print(f"{case}: figure (float32 model vs float64 model) {figure[0]:.2e} / {figure[1]:.2e}  ->  bars {bar[0]:.2e} / {bar[1]:.2e}")
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and np.abs(ref[0]).max() > 0 and np.abs(ref[1]).max() > 0
    mutants = {
        "shortcut (derivative on the float32 masters)": lambda: pr.ray_grads(pr.ShortcutModel(), fx, z, feat),
        "backward operands unrounded": lambda: pr.ray_grads(lr.Model(round_bwd=False), fx, z, feat),
        "plain float32-path gradient": lambda: pr.ray_grads(lr.Model.identity(), fx, z),
    }
    for name, run in mutants.items():
        got = run()[:2]
        e = pr.errors(got, ref)
        x = pr.per_ray_excess(got, ref, f32)
        print(f"{case}: {name}: {e[0]:.2e} / {e[1]:.2e}  ({max(e[0] / bar[0], e[1] / bar[1]):.1f} x the bar; worst ray at "
              f"{max(x):.1f} x its own bar)")
        assert pr.rejected(e, bar), (name, e, bar)
        assert max(x) > 1.0, (name, "the per-ray bars accept it", x)


def test_per_ray_bars_hold_where_one_ray_widens_the_tensor_wide_bar():
    """lowp_pose_ref.per_ray_excess: one ray of the float32 model moved as far as a ReLU flip moves it (1e-3 of the tensor's max)
    quadruples-and-more the tensor-wide bar, under which the shortcut mutant then passes; the per-ray bars still reject it,
    and still accept the float32 model itself."""
    case = pr.POSE_FIXTURES[0]
    fx, z, feat, ref, f32, figure, bar = _case(case)
    worst = int(np.abs(ref[0]).max(-1).argmin())                 # any ray will do; the one with the smallest gradient
    moved = tuple(g.copy() for g in f32)
    for g, r in zip(moved, ref):
        g[worst] += 1e-3 * np.abs(r).max()
    wide = pr.bars(pr.errors(moved, ref))
    mutant = pr.ray_grads(pr.ShortcutModel(), fx, z, feat)[:2]
    e = pr.errors(mutant, ref)
    x = pr.per_ray_excess(mutant, ref, moved)
    print(f"{case}: widened bars {wide[0]:.2e} / {wide[1]:.2e}, shortcut mutant {e[0]:.2e} / {e[1]:.2e}, its worst ray at "
          f"{max(x):.1f} x its own bar")
    assert not pr.rejected(e, wide), "the case this test is about: the widened tensor-wide bar lets the mutant through"
    assert max(x) > 1.0
    assert max(pr.per_ray_excess(moved, ref, moved)) <= 1.0 and max(pr.per_ray_excess(f32, ref, f32)) <= 1.0


def test_slam_config_default_is_float32():
    from myslam_amd import slam
    assert slam.SlamConfig().mixed_precision is False


def test_backend_without_mixed_precision_is_refused():
    from myslam_amd import scene as scn, slam
    from tests.oracle_backend import OracleBackend
    sc = scn.make_scene("toy")
    with pytest.raises(ValueError, match="mixed precision"):
        slam.Slam(sc, slam.SlamConfig(mixed_precision=True), device="cpu", backend=OracleBackend(sc))
    s = slam.Slam(sc, slam.SlamConfig(), device="cpu", backend=OracleBackend(sc))      # the default still constructs
    assert s.half is None
