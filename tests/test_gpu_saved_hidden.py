"""The decoder backward on the forward pass's saved first hidden layer (mlp_bwd_kernel<..., SAVEDH>, render_fwd_kernel's
store_hidden_buffer) against the recompute path, in ONE process, through the keyword that selects it.

Layer 1 of the backward was the same instructions on the same values as in the forward pass, so reading its result back changes
no bit: depth / rgb / sdf, every decoder gradient, the beta gradient and - where the rays take gradients - g_rays_o and g_rays_d
must be torch.equal between the two paths.  Plane gradients go through unordered float atomics: they are held to the rule of
tests/test_gpu_rank16_scatter.py, max(1e-5, 4 x) max-normalised, x = what two runs of the recompute path differ by among
themselves, measured here; in deterministic mode (a child process, every case) they must agree bit for bit too.

The loss VALUE is the one quantity neither path reproduces to the bit outside deterministic mode: the forward pass (and
eslam_loss_value) adds its workgroups' partial sums with unordered float atomics (loss_finalize), whichever way the backward
gets h1.  It is held bit for bit where its sums have a fixed order - the deterministic child, every case - and here to the
recompute path's OWN spread, counted in float32 steps: the value of the saved path may be no further from a recompute run than
two recompute runs are from each other, and one step (the format's resolution) where those two happen to agree.  DESIGN.md
section 5 has the figures of a run.

Cases: the smallest shapes at which the block indexing or the one-block-ahead request can go wrong; each varies one property
of the first.
   1  base_37x64            R = 37, S = 64, fused loss (MODE 2), channels-last: R % 4 != 0, the last workgroup is partial
   2  s56_half_block        S = 48 + 8: a ray's last block is half valid
   3  s96_two_chunks        S = 88 + 8: a second chunk of two blocks - the block index continues across chunks
   4  s40                   the last block half valid and R * S no multiple of 64
   5  r1100x32_second_ray   some waves of the persistent backward (256 workgroups x 4 waves) take a second ray: the request
                            across tiles
   6  separate_loss         eslam_render_bwd, MODE 1
   7  frozen_decoders       WGRAD = false: the kernel reads no features at all
   8  ray_gradients         full-width rows and coord_bwd_kernel
   9  nchw                  the strided forward kernel stores the layer
  10  masked_and_depthless  a third of the rays masked out, 10 % without depth
  11  frozen_separate_5x72  MODE 1 with WGRAD = false, which no other case reaches (here on the rank-16 pair, in the deterministic
                            child on full-width rows); R = 5, S = 64 + 8: two chunks, the second of one half-valid block
Cases 1, 6 and 8 run through both host glues.  Every case is also held to the oracle, with the criteria of
tests/test_gpu_parity.py (tests/helpers.py: outputs and loss within 1e-4 of the float64 oracle, plane gradients by
plane_grads_close, decoder gradients against the float32 and float64 oracles with the ambiguous-sample slack, ray gradients as
hostile_rays.accept).
"""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import hostile_rays as hr
from tests import saved_hidden_gpu as sh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4
BOTH_GLUES = ("base_37x64", "separate_loss", "ray_gradients")
PARAMS = [(c, g) for c in sh.CASES for g in (("python", "compiled") if c in BOTH_GLUES else ("python",))]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _n(t):
    return t.detach().cpu().double().numpy()


def _oracle(wl, z, dtype):
    """The iteration in the oracle on the kernel's z_vals: render, mapping loss over the kept rays (src/Mapper.py:329-346)."""
    from oracle import eslam_oracle as orc
    sp = wl.case
    sl = slice(0, sp["R"])
    cv = lambda t: t.detach().cpu().to(dtype)
    planes = tuple([cv(p).contiguous().requires_grad_(True) for p in grp] for grp in wl.planes)
    params = {k: cv(v).requires_grad_(True) for k, v in wl.decoders.state_dict().items() if k != "beta"}
    beta = cv(wl.decoders.beta).clone().requires_grad_(True)
    ro, rd = cv(wl.rays_o[sl]).requires_grad_(True), cv(wl.rays_d[sl]).requires_grad_(True)
    gd, gc, zz = cv(wl.gt_depth[sl]), cv(wl.gt_color[sl]), cv(z)
    od, oc, os_, _ = orc.render_batch_ray(planes, params, beta, wl.scene.bound, rd, ro, float(wl.truncation), gd, z.shape[1], 0, z_vals=zz)
    keep = torch.ones(sp["R"], dtype=torch.bool) if wl.mask is None else wl.mask.cpu()
    loss = orc.mapping_loss(od[keep], oc[keep], os_[keep], zz[keep], gd[keep], gc[keep], float(wl.truncation))
    loss.backward()
    dec = {k: _n(v.grad) for k, v in params.items()}
    dec["beta"] = _n(beta.grad)
    return dict(loss=float(loss), depth=_n(od), color=_n(oc), sdf=_n(os_), planes=[_n(p.grad) for p in hp.flat_planes(planes)], dec=dec,
                ro=_n(ro.grad), rd=_n(rd.grad), keep=keep)


def _against_oracle(wl, mine, label):
    o64, o32 = _oracle(wl, mine["z"], torch.float64), _oracle(wl, mine["z"], torch.float32)
    keep = o64["keep"]
    kn = keep.numpy()
    assert abs(float(mine["loss"]) - o64["loss"]) <= RTOL * abs(o64["loss"]), (label, float(mine["loss"]), o64["loss"])
    for k in ("depth", "color", "sdf"):        # (a masked ray still renders)
        e = hp.rel_err(_n(mine[k]), o64[k])
        assert e <= RTOL, (label, k, e)
    # the samples that reach the gradients: those of the kept rays
    mdl = (tuple([p.detach().cpu().float().contiguous() for p in grp] for grp in wl.planes),
           {k: v.detach().cpu().float() for k, v in wl.decoders.state_dict().items() if k != "beta"}, None)
    sl = slice(0, wl.case["R"])
    b = SimpleNamespace(rays_o=wl.rays_o[sl].detach().cpu()[keep], rays_d=wl.rays_d[sl].detach().cpu()[keep])
    pn, amb = hr.ambiguous(mdl, wl.scene, b, mine["z"][keep])
    ok, msg = hp.plane_grads_close([_n(g) for g in mine["planes"]], o32["planes"], o64["planes"], pn, amb, wl.scene.plane_shapes, RTOL)
    assert ok, (label, msg, int(amb.sum()))
    slack = 4.0 * float(amb.sum()) / max(1, amb.numel())
    for k, g in mine["dec"].items():
        if g is None:
            continue
        a = _n(g).reshape(o64["dec"][k].shape)
        e32, e64, cond = hp.rel_err(a, o32["dec"][k]), hp.rel_err(a, o64["dec"][k]), hp.rel_err(o32["dec"][k], o64["dec"][k])
        assert e32 <= RTOL + slack, (label, k, e32)
        assert e64 <= max(RTOL, 1.5 * cond) + slack, (label, k, e64, cond)
    for k in ("ro", "rd"):
        if mine[k] is None:
            continue
        per_ray = np.abs(_n(mine[k]) - o64[k]).max(1) / (np.abs(o64[k]).max() + 1e-30)
        q = float(np.quantile(per_ray, 0.97))
        assert q <= RTOL and per_ray.max() <= 0.05, (label, k, q, float(per_ray.max()))
        assert not kn.all() or np.abs(o64[k]).max() > 0


def _steps(a, b):
    """How many float32 values lie between two positive float32 scalars (0 = the same bits)."""
    ia, ib = (int(t.detach().cpu().reshape(1).view(torch.int32)) for t in (a, b))
    assert ia > 0 and ib > 0
    return abs(ia - ib)


def _max_normalised(a, b):
    return max(hp.rel_err(_n(x), _n(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("case,glue", PARAMS)
def test_saved_hidden_equals_recompute(case, glue):
    """Measured on an MI355X: see the margins the test prints (x, the plane gradients' difference and their bar)."""
    wl = sh.workload(case, _dev())
    sp = wl.case
    off, off2, on = sh.run(wl, False, glue), sh.run(wl, False, glue), sh.run(wl, True, glue)
    # the case runs the kernels it names
    assert on["rank16"] == off["rank16"] == (0 if sp["rays_grad"] else 1)
    assert (on["ro"] is not None) == sp["rays_grad"] and (on["dec"]["linears.0.weight"] is None) == sp["frozen"]
    assert all(np.abs(_n(g)).max() > 0 for g in on["planes"]) and float(on["loss"]) > 0
    assert torch.equal(off["z"], on["z"]) and on["z"].shape == (sp["R"], sp["ns"] + sp["ni"])
    bad = sh.unequal(off, on, loss=False)
    assert not bad, (case, glue, "differ bit for bit", bad)
    assert not sh.unequal(off, off2, loss=False), "two runs of the recompute path differ outside the loss value and the plane gradients"
    d_ref, d_new = _steps(off2["loss"], off["loss"]), _steps(on["loss"], off["loss"])
    print(f"loss {case} ({glue}): float32 steps between two recompute runs {d_ref}, between saved and recompute {d_new}")
    assert on["loss"].dtype == torch.float32 and d_new <= max(1, d_ref), (case, glue, d_new, d_ref)
    x = _max_normalised(off2["planes"], off["planes"])
    bar = max(1e-5, 4.0 * x)
    e = _max_normalised(on["planes"], off["planes"])
    print(f"margin saved hidden vs recompute {case} ({glue}): x = {x:.3e}, planes {e:.3e} (bar {bar:.1e}); everything else bit-equal")
    assert e <= bar, (case, glue, e, bar, x)
    _against_oracle(wl, on, f"{case} {glue}")


def test_saved_hidden_is_bit_equal_in_deterministic_mode():
    """Every case in ONE child process under ESLAM_DETERMINISTIC=1 (read once per process), where the loss's sums have a fixed
    order and the scatter is reproducible: the loss value and the plane gradients of the two paths are the same bits as well."""
    env = dict(os.environ, ESLAM_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, "-m", "tests.saved_hidden_gpu"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert d["det"] == 1 and list(d["cases"]) == list(sh.CASES)
    for case, v in d["cases"].items():
        assert v["rank16"] == [0, 0], case            # (deterministic mode keeps the full-width rows)
        assert v["unequal"] == [], (case, v["unequal"])
        assert len(v["planes"]) == 12 and all(v["planes"]) and all(v["nonzero"]), (case, v)


def test_only_calls_that_are_back_propagated_save_the_layer():
    """A call that will not be back-propagated allocates no buffer, and the default stays what ops.SAVED_HIDDEN_DEFAULT says."""
    from myslam_amd import ops
    wl = sh.workload("base_37x64", _dev())
    sl = slice(0, 37)
    rand = tuple(t[sl] for t in wl._rand)
    args = (wl.planes, wl.decoders, wl.rays_d[sl], wl.rays_o[sl], wl.device, wl.truncation)
    with torch.no_grad():
        ref = wl.renderer.render_batch_ray(*args, gt_depth=wl.gt_depth[sl], _rand=rand)
    assert ref[2].grad_fn is None
    out = wl.renderer.render_batch_ray(*args, gt_depth=wl.gt_depth[sl], _rand=rand)
    saved = out[2].grad_fn.saved_tensors
    assert len(saved) == (35 if ops.SAVED_HIDDEN_DEFAULT else 34)
    out_off = wl.renderer.render_batch_ray(*args, gt_depth=wl.gt_depth[sl], _rand=rand, saved_hidden=False)
    assert len(out_off[2].grad_fn.saved_tensors) == 34
    out_on = wl.renderer.render_batch_ray(*args, gt_depth=wl.gt_depth[sl], _rand=rand, saved_hidden=True)
    h = out_on[2].grad_fn.saved_tensors[34]
    assert h.numel() == ops.saved_hidden_floats(37, 64) and h.dtype == torch.float32
    for a, b in zip(out_on[:3], out_off[:3]):
        assert torch.equal(a, b)
    # the layer is a ReLU's output: no negative value, and not all zero
    assert float(h.min()) == 0.0 and float(h.max()) > 0.0 and bool(torch.isfinite(h).all())
