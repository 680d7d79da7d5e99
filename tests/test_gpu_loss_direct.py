"""The fused loss held directly: the six places that restate reference src/Mapper.py:110-144,337-346 on the GPU - loss_reduce_kernel
<false> (eslam_loss_reduce) and <true> (eslam_loss_value), loss_grad_kernel, the epilogue of render_fwd_kernel<LOSS>, the MODE == 2
branch of mlp_bwd_kernel, and the deterministic finaliser loss_finalize_det - against tests/loss_ref.py, the same operation in
numpy (pinned on the CPU by tests/test_loss_ref.py), on inputs made for it (loss_ref.border_batch): every row holds the float32
neighbours of all four thresholds of the region rule, and the variants empty one of the sets the loss takes a mean over.

All launches are made by tests/loss_direct_gpu.run(), once in this process (default mode: float atomics, the ticket scheme) and
once in a child process under ESLAM_DETERMINISTIC=1 (per-workgroup slots summed in a fixed order); every test below checks one
case of one mode on the host.

Bars.  Counts, NaN-ness and the zeros of rays outside a term are exact.  A sum (and the value, a weighted sum of five means)
may differ from the float64 reference by 4 x gap32 + (W + 16) x 2^-24 relative: gap32 = what the float32 evaluation of the
reference differs from the float64 one by on the same inputs, W = the partial sums that are added one after the other (the
workgroups: <= 256), 16 for the tree inside a workgroup - the worst case of a sum of non-negative terms.  Gradients:
helpers.rel_err <= 4 x gap32 + 8 x 2^-24.  Never more than RTOL = 1e-4.  Every bar prints a `margin` line (pytest -s);
profiles/r09/loss_direct_margins.txt keeps those of one MI355X run.

In deterministic mode two things differ by design and are asserted as such: the scratch keeps the workgroups' slots (only its
ticket line reads back zero), and no backward takes the rank-16 pair.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as hp
from tests import loss_direct_gpu as ldg
from tests import loss_ref as lf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("default", "det")
CASES = list(ldg.cases())
EPS = lf.EPS32


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    default = ldg.run()
    assert int(default["det"]) == 0, "the suite runs in the default mode; the deterministic leg is the child process"
    out = str(tmp_path_factory.mktemp("loss_direct") / "det.npz")
    env = dict(os.environ, ESLAM_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, "-m", "tests.loss_direct_gpu", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    with np.load(out, allow_pickle=False) as f:
        det = {k: f[k] for k in f.files}
    assert int(det["det"]) == 1
    assert sorted(det) == sorted(default)
    return {"default": default, "det": det}


@functools.lru_cache(maxsize=None)
def _refs(name, upstream):
    """float64 and float32 reference of a direct case, computed once for both modes and all three entries."""
    spec = ldg.cases()[name]
    b = ldg.batch_of(spec)
    return b, lf.loss_ref_of(b, spec[2], ldg.W5, upstream), lf.loss_ref_of(b, spec[2], ldg.W5, upstream, dtype=np.float32)


def _check_acc(label, acc, r64, r32, W):
    """Counts exact, unused slots zero, sums within the bar.  -> (worst measured / bar, its name, measured, bar)."""
    a64, a32 = r64[0], r32[0]
    for k in lf.COUNTS:
        assert float(acc[k]) == float(a64[k]), (label, lf.SLOT_NAMES[k], float(acc[k]), float(a64[k]))
    assert not acc[lf.A_COUNT:].any(), (label, "slots behind the ten accumulators", acc[lf.A_COUNT:])
    worst = (0.0, "-", 0.0, 0.0)
    for k in lf.SUMS:
        if a64[k] == 0:
            assert acc[k] == 0, (label, lf.SLOT_NAMES[k], acc[k])
            continue
        bar = lf.sum_bar(lf.rel(a32[k], a64[k]), W)
        e = lf.rel(acc[k], a64[k])
        worst = max(worst, (e / bar, lf.SLOT_NAMES[k], e, bar))
        assert e <= bar, (label, lf.SLOT_NAMES[k], e, bar)
    return worst


def _check_value(label, loss, r64, r32, W):
    l64, l32 = float(r64[1]), float(r32[1])
    assert bool(np.isnan(loss)) == bool(np.isnan(l64)), (label, "NaN-ness of the value", float(loss), l64)
    if np.isnan(l64):
        return (0.0, float("nan"), 0.0)
    bar = lf.sum_bar(lf.rel(l32, l64), W)
    e = lf.rel(loss, l64)
    assert e <= bar, (label, "value", float(loss), l64, e, bar)
    return (e / bar, e, bar)


def _check_grads(label, b, g, r64, r32):
    """Exact zeros for rays outside a term, finite everywhere, max-normalised difference within the bar."""
    mc, m = lf.members(b["gt_depth"], b["ray_mask"])
    g_depth, g_rgb, g_sdf = g
    assert not g_depth[~m].any() and not g_sdf[~m].any() and not g_rgb[~mc].any(), (label, "a ray outside a term has a gradient")
    worst = (0.0, "-", 0.0, 0.0)
    for name, a, w64, w32 in zip(("g_depth", "g_rgb", "g_sdf"), g, r64[2:5], r32[2:5]):
        assert a.shape == w64.shape and np.isfinite(a).all(), (label, name)
        if not w64.any():
            assert not a.any(), (label, name, "the reference's gradient is zero everywhere")
            continue
        bar = lf.grad_bar(lf.max_rel(w32, w64))
        e = hp.rel_err(a, w64)
        worst = max(worst, (e / bar, name, e, bar))
        assert e <= bar, (label, name, e, bar)
    return worst


def _margin(label, acc=None, value=None, grads=None):
    parts = []
    if acc is not None:
        parts.append(f"sums {acc[0]:.3f} ({acc[1]} {acc[2]:.2e} / {acc[3]:.2e})")
    if value is not None:
        parts.append("value NaN as the reference" if np.isnan(value[1]) else f"value {value[0]:.3f} ({value[1]:.2e} / {value[2]:.2e})")
    if grads is not None:
        parts.append(f"gradients {grads[0]:.3f} ({grads[1]} {grads[2]:.2e} / {grads[3]:.2e})")
    print(f"margin loss direct {label}: " + ", ".join(parts))


def _scratch_left_clean(res, key, mode):
    whole, ticket_line = (int(v) for v in res[key])
    if mode == "default":
        assert whole == 0, (key, "the scratch must read back all zero", whole)
    else:       # the deterministic finaliser keeps each workgroup's slot and overwrites it on the next call; the ticket resets
        assert ticket_line == 0, (key, "ticket line", ticket_line)


# ---- the direct entries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("mode", MODES)
def test_direct_entries(results, mode, name):
    """eslam_loss_reduce + eslam_loss_grad (a), eslam_loss_value + eslam_loss_grad with upstream = 0.37 and loss = NULL, then
    with loss alone (b), eslam_mapping_loss on 64 bytes of garbage (c)."""
    res = results[mode]
    R = ldg.cases()[name][0]
    W = ldg.workgroups(R)
    b, r64, r32 = _refs(name, 1.0)
    _, u64, u32 = _refs(name, ldg.UPSTREAM)
    get = lambda form, k: res[f"{name}/{form}/{k}"]
    for form, g64, g32 in (("a", r64, r32), ("b", u64, u32), ("c", r64, r32)):
        label = f"{mode} {name} {form}"
        wa = _check_acc(label, get(form, "acc"), r64, r32, W)
        wv = _check_value(label, get(form, "loss")[0], r64, r32, W)                   # (upstream scales no value)
        wg = _check_grads(label, b, [get(form, k) for k in ("g_depth", "g_rgb", "g_sdf")], g64, g32)
        _margin(label, wa, wv, wg)
    # gradients NULL with loss: the value eslam_loss_grad forms from acc is the one eslam_loss_value wrote, give or take the
    # rounding of five quotients, products and sums of positive terms
    lo, lv = float(get("b", "loss_only")[0]), float(get("b", "loss")[0])
    assert np.isnan(lo) == np.isnan(lv) and (np.isnan(lv) or lf.rel(lo, lv) <= 8 * EPS), (mode, name, lo, lv)
    # upstream scales the gradients: (b) is 0.37 x (a) up to the roundings of the scaled weights
    if r64[4].any():
        assert hp.rel_err(get("b", "g_sdf"), ldg.UPSTREAM * get("a", "g_sdf").astype(np.float64)) <= lf.grad_bar(0.0)
    _scratch_left_clean(res, f"{name}/b/scratch_nonzero", mode)


@pytest.mark.parametrize("name", ldg.HALVES)
@pytest.mark.parametrize("mode", MODES)
def test_reduce_accumulates_two_halves_into_one_acc(results, mode, name):
    R = ldg.cases()[name][0]
    b, r64, r32 = _refs(name, 1.0)
    W = ldg.workgroups(R // 2) + ldg.workgroups(R - R // 2)
    label = f"{mode} {name} two halves"
    _margin(label, _check_acc(label, results[mode][f"halves/{name}/acc"], r64, r32, W))


@pytest.mark.parametrize("mode", MODES)
def test_one_scratch_serves_batches_of_any_size(results, mode):
    """eslam_loss_value three times on one scratch, R = 5, 4099, 1: each result right, the scratch left ready for the next."""
    res = results[mode]
    assert [ldg.cases()[n][0] for n in ldg.REUSE] == [5, 4099, 1]
    for k, name in enumerate(ldg.REUSE):
        b, r64, r32 = _refs(name, 1.0)
        W = ldg.workgroups(ldg.cases()[name][0])
        label = f"{mode} {name} shared scratch, call {k + 1}"
        wa = _check_acc(label, res[f"reuse/{k}/acc"], r64, r32, W)
        wv = _check_value(label, res[f"reuse/{k}/loss"][0], r64, r32, W)
        _margin(label, wa, wv)
        _scratch_left_clean(res, f"reuse/{k}/scratch_nonzero", mode)


ERRORS = {"reduce_no_rays": "eslam_loss_reduce", "value_no_rays": "eslam_loss_value", "grad_no_rays": "eslam_loss_grad",
          "mapping_no_rays": "eslam_loss_reduce", "reduce_null_acc": "eslam_loss_reduce", "value_null_acc": "eslam_loss_value",
          "grad_null_acc": "eslam_loss_grad", "value_null_scratch": "eslam_loss_value", "mapping_null_scratch": "eslam_mapping_loss",
          "grad_depth_without_sdf": "eslam_loss_grad", "grad_depth_alone": "eslam_loss_grad", "grad_nothing_asked": "eslam_loss_grad"}


@pytest.mark.parametrize("mode", MODES)
def test_argument_errors_return_a_code_and_a_message_and_launch_nothing(results, mode):
    res = results[mode]
    for name, who in ERRORS.items():
        rc, msg = int(res[f"err/{name}/rc"]), str(res[f"err/{name}/message"])
        assert rc != 0, name
        assert msg.startswith(who + ":"), (name, msg)
        assert bool(res[f"err/{name}/untouched"]), (name, "an output buffer changed")


# ---- the forms inside the render kernels -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ik_counts(S, variant):
    b = ldg.ik_batch(S, variant)
    return b, lf.loss_ref_of(b, 0.06, ldg.W5)[0]


@pytest.mark.parametrize("S,variant", ldg.IN_KERNEL)
@pytest.mark.parametrize("mode", MODES)
def test_forward_epilogue(results, mode, S, variant):
    """eslam_render_fwd_loss with the border rows as z_vals: the counts of loss_ref on (z, gt_depth, mask); sums and value of
    loss_ref on the kernel's own depth / rgb / sdf; and eslam_loss_value on those outputs."""
    res, tag = results[mode], "ik/" + ldg.ik_tag(S, variant)
    b, acc_in = _ik_counts(S, variant)
    acc, acc_v = res[f"{tag}/acc"], res[f"{tag}/acc_value"]
    for k in lf.COUNTS:
        assert float(acc[k]) == float(acc_in[k]) == float(acc_v[k]), (lf.SLOT_NAMES[k], acc[k], acc_in[k], acc_v[k])
    outs = {k: res[f"{tag}/{k}"] for k in ("depth", "rgb", "sdf")}
    assert all(np.isfinite(v).all() for v in outs.values())
    r64 = lf.loss_ref_of(b, 0.06, ldg.W5, **outs)
    r32 = lf.loss_ref_of(b, 0.06, ldg.W5, dtype=np.float32, **outs)
    W_fwd, W_val = ldg.forward_workgroups(ldg.IK_R), ldg.workgroups(ldg.IK_R)
    label = f"{mode} forward epilogue {ldg.ik_tag(S, variant)}"
    _margin(label, _check_acc(label, acc, r64, r32, W_fwd), _check_value(label, res[f"{tag}/loss"][0], r64, r32, W_fwd))
    label = f"{mode} eslam_loss_value on the forward's outputs {ldg.ik_tag(S, variant)}"
    _margin(label, _check_acc(label, acc_v, r64, r32, W_val), _check_value(label, res[f"{tag}/loss_value"][0], r64, r32, W_val))
    worst = 0.0
    for k in lf.SUMS:                                # the two kernels against each other: both chains of partial sums
        bar = lf.sum_bar(lf.rel(r32[0][k], r64[0][k]), W_fwd + W_val)
        e = lf.rel(acc[k], acc_v[k])
        worst = max(worst, e / bar)
        assert e <= bar, (lf.SLOT_NAMES[k], e, bar)
    print(f"margin loss direct {mode} forward epilogue against eslam_loss_value {ldg.ik_tag(S, variant)}: sums {worst:.3f}")
    _scratch_left_clean(res, f"{tag}/scratch_nonzero", mode)


@pytest.mark.parametrize("cfg", ldg.IK_CONFIGS, ids=ldg.ik_config_tag)
@pytest.mark.parametrize("S,variant", ldg.IN_KERNEL)
@pytest.mark.parametrize("mode", MODES)
def test_backward_forms_the_gradients_eslam_loss_grad_writes(results, mode, S, variant, cfg):
    """eslam_render_bwd_loss(acc) against eslam_render_bwd fed what eslam_loss_grad(acc) wrote (plus the further upstream gradients,
    where given), on the same saved forward: decoder, beta and ray gradients within 1e-6 (the bar of
    test_rank16_path_equals_full_width_path), planes within max(1e-5, 4 x what two runs of the eslam_render_bwd side differ by)."""
    res = results[mode]
    rays, upstream, further = cfg
    key = f"ik/{ldg.ik_tag(S, variant)}/{ldg.ik_config_tag(cfg)}"
    m = {k: float(res[f"{key}/{k}"]) for k in ("x", "planes", "dec", "beta", "rays", "rank16_separate", "rank16_fused", "loss_out", "nonzero",
                                              "rays_nonzero", "finite")}
    bar = max(1e-5, 4.0 * m["x"])
    print(f"margin loss direct {mode} backward {ldg.ik_tag(S, variant)} {ldg.ik_config_tag(cfg)}: x = {m['x']:.3e}, planes {m['planes']:.3e} "
          f"(bar {bar:.1e}), decoders {m['dec']:.3e}, beta {m['beta']:.3e}, rays {m['rays']:.3e} (bar 1e-06)")
    want_rank16 = 0 if (rays or mode == "det") else 1
    assert m["rank16_separate"] == want_rank16 and m["rank16_fused"] == want_rank16, "the library dispatched the other pair of kernels"
    assert m["finite"] == 1.0 and m["nonzero"] > 0 and m["rays_nonzero"] > 0
    assert m["dec"] <= 1e-6 and m["beta"] <= 1e-6 and m["rays"] <= 1e-6, m
    assert m["planes"] <= bar, m
    # loss_out: the value formed from acc - what eslam_loss_grad forms from the same acc, and the float64 value of those sums
    tag = "ik/" + ldg.ik_tag(S, variant)
    assert np.float32(m["loss_out"]) == res[f"{tag}/loss_from_acc"][0]
    assert lf.rel(m["loss_out"], lf.value_from_acc(res[f"{tag}/acc"], ldg.W5)) <= 8 * EPS
