"""Ray (pose) gradients of the mixed-precision path - coord_bwd_lowp_kernel behind the LOWP decoder backward, through
ops.mixed_precision(half, ray_grads=True) - against tests/lowp_pose_ref.py, the float64 model whose bilinear derivative acts on
the fp16-rounded texels; and the tracking + mapping loop that uses them (slam.SlamConfig.mixed_precision).

Bar of a ray-gradient tensor (lowp_pose_ref): max-normalised error against the float64 model on the kernel's z_vals, forced
with the kernel's saved bf16 features, <= 4 x max(float32 model vs float64 model on the same inputs, OUT_RTOL).  The float32
model's figure is computed here on the host; tests/test_lowp_pose_ref.py shows that the bar rejects the float32 kernel's
derivative on the masters, unrounded backward operands and the float32 path's gradient.

Where one ray's ReLU flip in the float32 model widens a tensor's bar, every ray is also held to its own bar of the same
construction (lowp_pose_ref.per_ray_excess), so the other rays stay at the OUT_RTOL floor.

Shapes: S = 40 (two and a half 16-sample blocks) and 32; R = 200, 197 (the last workgroup has one live wave of four), 1.
Every test prints its figures before it asserts (pytest -s).
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import lowp_pose_gpu as pg
from tests import lowp_pose_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRACKING_CASES = ("room0_200x40_tracking", "room0_200x32")
MAPPING_CASES = ("room0_200x40_zero15", "room0_200x40_trained_zero15")      # 27 depth-less rays: samples up to the bound


def _hold(label, got, model):
    ref, f32, figure, bar = model
    e = pr.errors(got, ref)
    x = pr.per_ray_excess(got, ref, f32)
    print(f"{label}: kernel vs model g_o {e[0]:.2e} g_d {e[1]:.2e}; float32 model vs model {figure[0]:.2e} / {figure[1]:.2e}; "
          f"bars {bar[0]:.2e} / {bar[1]:.2e}; worst ray at {x[0]:.2f} / {x[1]:.2f} of its own bar")
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), label
    assert e[0] <= bar[0] and e[1] <= bar[1], (label, e, bar)
    assert x[0] <= 1.0 and x[1] <= 1.0, (label, "a ray beyond its own bar (lowp_pose_ref.per_ray_excess)", x)


# ---- 1. tracking ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tracking_run(case):
    fx = hp.load(case)
    return fx, pg.step(fx, "tracking")


@pytest.mark.parametrize("case", TRACKING_CASES)
def test_tracking_ray_gradients_against_the_model(case):
    """Planes and decoders frozen, both rays require grad, losses.tracking_loss: the only kernels behind the loss are the LOWP
    decoder backward without weight gradients and the coordinate kernel."""
    fx, r = _tracking_run(case)
    _hold(f"{case} tracking R=200", (r["g_o"], r["g_d"]), pr.model_pair(fx, r["z"], r["feat"], loss_kind="tracking"))
    plain = pg.step(fx, "tracking", False, False, ray_grads=False)
    for k in ("depth", "color", "sdf", "z"):
        assert np.array_equal(r[k], plain[k]), f"{k}: asking for ray gradients changed the forward pass"


@pytest.mark.parametrize("n", [197, 1])
@pytest.mark.parametrize("case", TRACKING_CASES)
def test_tracking_ray_gradients_of_partial_workgroups(case, n):
    fx, r = _tracking_run(case)
    g_o, g_d, feat = pg.sliced(fx, r["z"], n)
    assert g_o.shape == (n, 3) and g_d.shape == (n, 3)
    _hold(f"{case} tracking R={n}", (g_o, g_d), pr.model_pair(fx, r["z"][:n], feat, rows=slice(0, n), loss_kind="tracking"))


# ---- 2. mapping with pose gradients ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mapping_model(case):
    fx = hp.load(case)
    r = pg.step(fx, "separate")
    return fx, r, pr.model_pair(fx, r["z"], r["feat"])


@pytest.mark.parametrize("form", ["separate", "fused"])
@pytest.mark.parametrize("case", MAPPING_CASES)
def test_mapping_ray_gradients_against_the_model(case, form):
    """A mapping step that trains planes and decoders AND takes ray gradients (joint_opt), loss outside / inside the kernels."""
    fx, first, model = _mapping_model(case)
    r = first if form == "separate" else pg.step(fx, form)
    assert np.array_equal(r["z"], first["z"]) and np.array_equal(r["feat"], first["feat"])      # one forward, whatever forms the loss
    _hold(f"{case} {form}", (r["g_o"], r["g_d"]), model)
    for p in r["planes"] + list(r["dec"].values()):
        assert np.isfinite(p).all()
    # only one of the two rays requiring grad: the same values as both together (everything in front of the coordinate kernel -
    # decoder backward, g_feat - has no atomics, and the kernel's own sums have a fixed order)
    only_o, only_d = pg.step(fx, form, True, False), pg.step(fx, form, False, True)
    assert only_o["g_d"] is None and only_d["g_o"] is None
    assert np.array_equal(only_o["g_o"], r["g_o"]) and np.array_equal(only_d["g_d"], r["g_d"])


def test_fused_mapping_step_with_frozen_decoders():
    """mlp_bwd_kernel<2, false, LOWP>, which no other test reaches: the loss formed inside the kernels, planes trained, decoders
    frozen (g_dec NULL: no weight-gradient contractions), rays taking gradients.  The ray gradients are held to the model like
    those of the trained step, and are its bits: everything in front of the coordinate kernel is the same arithmetic with or
    without the contractions and has no atomics."""
    case = MAPPING_CASES[0]
    fx, first, model = _mapping_model(case)
    full = pg.step(fx, "fused")
    r = pg.step(fx, "fused", dec_grad=False)
    assert all(g is None for g in r["dec"].values())
    for k in ("depth", "color", "sdf", "z", "feat"):
        assert np.array_equal(r[k], first[k]), k
    _hold(f"{case} fused, frozen decoders", (r["g_o"], r["g_d"]), model)
    assert np.array_equal(r["g_o"], full["g_o"]) and np.array_equal(r["g_d"], full["g_d"])
    assert all(np.isfinite(p).all() and np.abs(p).max() > 0 for p in r["planes"])
    for a, b in zip(r["planes"], full["planes"]):      # float atomics: order-dependent rounding (tests/test_gpu_determinism.py)
        assert hp.rel_err(a, b) <= 1e-5


def test_ray_gradients_leave_plane_and_decoder_gradients_bit_equal():
    """Plane and decoder gradients of a mapping step with ray gradients are the BITS of the same step without: the coordinate
    kernel runs behind the scatter and writes nothing but g_rays_o / g_rays_d.  Compared in a child process under
    ESLAM_DETERMINISTIC=1: in the default mode the scatter's float atomics leave the plane gradients' last bits different
    from run to run (tests/test_gpu_determinism.py), so two calls cannot be compared bit for bit there."""
    env = dict(os.environ, ESLAM_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, "-m", "tests.lowp_pose_gpu", *MAPPING_CASES], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert d.pop("det") == 1
    assert len(d) == len(MAPPING_CASES) * 2 * 3
    for key, v in d.items():
        print(f"{key}: forward equal {v['forward']}, planes equal {sum(v['planes'])}/12, decoder tensors equal "
              f"{sum(v['dec'].values())}/{len(v['dec'])}")
        assert v["forward"] and all(v["planes"]) and all(v["dec"].values()), (key, v)


# ---- 3. the default is unchanged ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rays_o", "rays_d"])
def test_without_ray_grads_the_refusal_stands(which):
    fx = hp.load(TRACKING_CASES[0])
    with pytest.raises(RuntimeError, match="rays"):
        pg.step(fx, "tracking", which == "rays_o", which == "rays_d", ray_grads=False)
    from myslam_amd import ops
    assert ops._half_planes is None and ops._half_ray_grads is False      # the contexts were left


# ---- 4. the loop ---------------------------------------------------------------------------------------------------------
def test_mixed_precision_loop_tracks_and_maps_like_the_float32_loop():
    """slam.Slam on the toy scene with the configuration of test_graph_captured_loop_matches_eager_loop (25 frames: joint_opt
    engages, so tracking AND joint mapping take pose gradients), float32 against mixed_precision=True from the same seed, held
    to that file's bands."""
    import dataclasses
    from myslam_amd import slam
    from tests.test_gpu_slam_quality import _run
    cfg = slam.SlamConfig(tracking_pixels=500, tracking_iters=8, ignore_edge_H=10, ignore_edge_W=10, mapping_pixels=1000,
                          iters_first=100, iters=10, every_frame=4, keyframe_every=4)
    n_frames = 25
    ate_f, q_f, st_f = _run("hip", n_frames, cfg)
    ate_m, q_m, st_m = _run("hip", n_frames, dataclasses.replace(cfg, mixed_precision=True))
    print(f"\nfloat32 loop:         ATE rmse {ate_f['rmse']*100:.2f} cm, PSNR {q_f['psnr']:.2f} dB, depth L1 {q_f['depth_l1']*100:.2f} cm, {st_f}")
    print(f"mixed-precision loop: ATE rmse {ate_m['rmse']*100:.2f} cm, PSNR {q_m['psnr']:.2f} dB, depth L1 {q_m['depth_l1']*100:.2f} cm, {st_m}")
    assert st_m["tracking_iters"] == st_f["tracking_iters"] == 8 * (n_frames - 1)
    assert st_m["mapping_iters"] == st_f["mapping_iters"] == 100 + 10 * 6
    for ate, q in ((ate_f, q_f), (ate_m, q_m)):
        assert ate["rmse"] < 0.02 and q["psnr"] > 18.0 and q["depth_l1"] < 0.05
    assert abs(q_m["psnr"] - q_f["psnr"]) < 1.5
    assert abs(q_m["depth_l1"] - q_f["depth_l1"]) < 0.3 * max(q_m["depth_l1"], q_f["depth_l1"]) + 0.002
    assert abs(ate_m["rmse"] - ate_f["rmse"]) < 0.5 * max(ate_m["rmse"], ate_f["rmse"]) + 0.002


def test_graph_captured_loop_refuses_mixed_precision():
    from myslam_amd import scene as scn, slam
    from myslam_amd.slam_graph import GraphedSlam
    with pytest.raises(NotImplementedError, match="mixed_precision"):
        GraphedSlam(scn.make_scene("toy"), slam.SlamConfig(mixed_precision=True))
