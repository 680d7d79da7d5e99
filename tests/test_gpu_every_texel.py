"""Plane gradients on EVERY touched texel, and on planes of shapes scene.plane_shapes never makes.

The oracle comparisons of the render backward end in hp.plane_grads_close, which sets aside every texel a ReLU-ambiguous
sample touches: on the usual batches half to nine tenths of the coarse planes' touched texels, on 2 x 2 planes all of them
(tests/test_every_texel_ref.py pins the figures).  Here the batch is made free of ambiguous samples instead
(tests/every_texel.py: sample a pool, drop the rays that own one, render the rest with their own rows), so the criteria of
hostile_rays.accept run with max_excluded = 0.0: every touched texel is compared and the decoder gradients get no slack.  The
bars are the project's own, RTOL = 1e-4 with the float32 oracle as comparator under the float64 conditioning bound.
tests/every_texel_gpu.py holds the flow and its assertions (same z_vals as the pool's, no ambiguous sample, the kernel path).

Two sizes, the smallest at which each bundle width can go wrong: 37 x (23+6) - 1024-sample bundles, 1015 + 58 samples - and
640 x (56+8) with a tenth of the rays depth-less - bundles of exactly 2048, 240 workgroups.

On the shipped room0 shapes:
  a  initial / trained, unpaired                                       rank-16
  b  paired (mode 2): the shipped list of 3 pairs, and 6 pairs         rank-16, paired
  c  rays that take gradients                                          full-width rows, plus the ray-gradient criteria
  d  NCHW planes at 640 x 64                                           relayout scratch, rank-16
  e  the fused mapping loss at 640 x 64, every third ray masked        MODE 2
  f  b's shipped list and c in ONE child under ESLAM_DETERMINISTIC=1   fixed-point scatter, full-width rows
On plane shapes the C ABI accepts and no scene produces (every_texel.SHAPE_SETS, toy bound): a, b and c at both sizes;
`one_cell` (all twelve planes 2 x 2: every bundle is one cell in every plane - the longest run the walk can meet - and the
all-pairs list has 6 entries) also initial and NCHW; `slivers` (2-texel axes beside 129-texel ones, 2 pairs); `levels_swapped`
(fine levels coarser than coarse ones, colour planes coarser than SDF planes, 1 pair).  Per set: eslam_mark_rays marks every texel
with a non-zero oracle gradient, and a free-point case (2000 + 37 unambiguous points, a tenth outside the bound) through
Decoders.forward / backward and decode_sdf_only against orc.decode in float64.

Margins of one MI355X run (`pytest -s`, the lines starting with "margin"): profiles/r13/every_texel_margins.txt.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import every_texel as et
from tests import every_texel_gpu as eg
from tests import helpers as hp
from tests import hostile_rays as hr
from tests.every_texel_gpu import LARGE, SMALL, Case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = hr.RTOL
SIZES = [SMALL, LARGE]
SETS = list(et.SHAPE_SETS)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _run(case):
    """A case's result, shared by the tests that look at it (the oracle is the long part)."""
    return eg.run(case, _dev())


def _id(v):
    return f"{v[0]}x{v[1]}+{v[2]}" if isinstance(v, tuple) else None


# ---- the shipped room0 shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", hr.STATES)
@pytest.mark.parametrize("size", SIZES, ids=_id)
def test_unpaired_rank16_on_every_texel(size, state):
    r = _run(Case(size=size, state=state))
    assert (r.rank16, r.paired, r.pairs) == (1, 0, 3)


@pytest.mark.parametrize("res,pairs", [("default", 3), ("same", 6)])
@pytest.mark.parametrize("size", SIZES, ids=_id)
def test_paired_rank16_on_every_texel(size, res, pairs):
    r = _run(Case(size=size, pairing=2, res=res))
    assert (r.rank16, r.paired, r.pairs) == (1, 1, pairs)


@pytest.mark.parametrize("size", SIZES, ids=_id)
def test_full_width_rows_and_ray_gradients_on_every_texel(size):
    r = _run(Case(size=size, rays_grad=True))
    assert r.rank16 == 0


def test_nchw_planes_on_every_texel():
    """640 x 64 = 40960 points: the call runs on channels-last scratch copies and carries the gradient back."""
    from myslam_amd import ops
    r = _run(Case(size=LARGE, channels_last=False))
    assert r.rank16 == 1 and ops.wants_relayout(r.wl.planes, 640 * 64)
    assert all(p.is_contiguous() for p in r.wl.plane_list)


def test_fused_loss_with_masked_rays_on_every_texel():
    r = _run(Case(size=LARGE, loss="fused"))
    assert r.rank16 == 1


def test_deterministic_mode_on_every_texel():
    """Every case of every_texel_gpu.DET_CASES in ONE child under ESLAM_DETERMINISTIC=1 (read once per process)."""
    env = dict(os.environ, ESLAM_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, "-m", "tests.every_texel_gpu"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print("\n".join(l for l in p.stdout.splitlines() if l.startswith("margin ")))
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert d["det"] == 1 and list(d["cases"]) == [c.label for c in eg.DET_CASES]
    for label, v in d["cases"].items():
        assert v["ok"], (label, v.get("error"))
        assert v["rank16"] == 0, label               # (deterministic mode keeps the full-width rows)


# ---- plane shapes no scene produces ----------------------------------------------------------------------------------------
def test_shape_sets_are_what_the_docstring_says():
    one, sl, sw = (et.SHAPE_SETS[k] for k in SETS)
    flat = lambda s: [hw for grp in s for hw in grp]
    assert flat(one) == [(2, 2)] * 12 and sum(h * w for h, w in flat(one)) == 48
    assert sum(2 in hw for hw in flat(sl)) == 8 and max(max(hw) for hw in flat(sl)) == 129
    assert all(grp[0][0] * grp[0][1] > grp[1][0] * grp[1][1] for grp in sw[:3]), "SDF fine levels coarser than the coarse ones"
    assert sw[3][0][0] * sw[3][0][1] < sw[0][0][0] * sw[0][0][1], "a colour plane coarser than the SDF plane of its slot"
    assert [et.pair_count([[(1, 32) + hw for hw in grp] for grp in et.SHAPE_SETS[k]]) for k in SETS] == [6, 2, 1]


@pytest.mark.parametrize("mode", ["unpaired", "paired", "ray gradients"])
@pytest.mark.parametrize("size", SIZES, ids=_id)
@pytest.mark.parametrize("name", SETS)
def test_odd_plane_shapes_on_every_texel(name, size, mode):
    r = _run(Case(size=size, shapes=name, pairing=2 if mode == "paired" else 0, rays_grad=mode == "ray gradients"))
    assert r.pairs == et.PAIRS[name]
    assert (r.rank16, r.paired) == {"unpaired": (1, 0), "paired": (1, 1), "ray gradients": (0, r.paired)}[mode]


@pytest.mark.parametrize("kw", [dict(state="initial"), dict(channels_last=False, pairing=2)], ids=["initial", "NCHW paired"])
@pytest.mark.parametrize("size", SIZES, ids=_id)
def test_one_cell_planes_initial_state_and_nchw(size, kw):
    r = _run(Case(size=size, shapes="one_cell", **kw))
    assert (r.rank16, r.paired, r.pairs) == (1, int(kw.get("pairing", 0) == 2), 6)


@pytest.mark.parametrize("name", SETS)
def test_marking_covers_every_texel_with_an_oracle_gradient(name):
    """eslam_mark_rays (the call of test_gpu_rank16_scatter.py) on the rays of the set's unpaired 640 x 64 case: every texel the
    float64 oracle sends gradient to is marked; on 2 x 2 planes that is all 48."""
    from myslam_amd import ops, parallel
    r = _run(Case(size=LARGE, shapes=name))
    wl = r.wl
    base, n_blocks = hr.block_base(wl.scene)
    marked = parallel.mark_rays(None, ops.bound_to_host(wl.scene.bound), r.ro, r.rd, r.gd, wl.truncation, base, n_blocks,
                                planes=wl.planes).bool().cpu()
    nz = torch.cat([torch.from_numpy((g[0] != 0).any(0).reshape(-1)) for g in r.o64["planes"]])
    assert nz.shape == marked.shape == (n_blocks,)
    print(f"margin marking {name}: {int(nz.sum())} texels with an oracle gradient, {int(marked.sum())} of {n_blocks} marked")
    assert int(nz.sum()) > 0 and int((nz & ~marked).sum()) == 0, int((nz & ~marked).sum())
    if name == "one_cell":
        assert n_blocks == 48 and int(marked.sum()) == 48 and int(nz.sum()) == 48


@pytest.mark.parametrize("name", SETS)
def test_free_points_on_odd_plane_shapes(name):
    """2000 + 37 unambiguous points (31 full units of 64 and one of 53), a tenth outside the bound, through Decoders.forward and
    its backward - with point gradients and without (free points keep the full-width rows either way) - and decode_sdf_only,
    against orc.decode in float64 at the bars of test_gpu_parity.test_decoders_forward_and_backward: RTOL, max-normalised, on
    everything."""
    from myslam_amd import harness, ops
    from oracle import eslam_oracle as orc
    from tests import test_gpu_rank16_scatter as t16
    dev = _dev()
    N = 2037
    wl = eg.set_shapes(harness.make_workload("toy", 8, 8, 4, device=dev, planes="synth", state="trained"), "trained", name)
    mdl = eg.cpu_model(wl)
    pool = et.free_points(wl.scene, 2600)
    idx = et.unambiguous_points(mdl, wl.scene, pool, N)
    pts = pool[idx]
    lo, hi = wl.scene.bound[:, 0], wl.scene.bound[:, 1]
    n_out = int(((pts < lo) | (pts > hi)).any(1).sum())
    assert 0.05 * N < n_out < 0.15 * N, n_out
    wts = torch.linspace(0.5, 1.5, N * 4).reshape(N, 4)
    # oracle, float64
    planes, params, _ = mdl
    cp = tuple([p.double().requires_grad_(True) for p in grp] for grp in planes)
    cq = {k: v.double().requires_grad_(True) for k, v in params.items()}
    p64 = pts.double().requires_grad_(True)
    raw64 = orc.decode(p64, cp, cq, wl.scene.bound.double())
    (raw64 * wts.double()).sum().backward()
    assert all(np.abs(g.grad.numpy()).max() > 0 for g in hp.flat_planes(cp)) and np.abs(p64.grad.numpy()).max() > 0
    rep = {}
    for points_grad in (True, False):
        t16._fresh(wl)
        p = pts.to(dev).requires_grad_(points_grad)
        raw = wl.decoders(p, all_planes=wl.planes)
        assert raw.shape == (N, 4)
        (raw * wts.to(dev)).sum().backward()
        torch.cuda.synchronize()
        assert t16._last_backward_rank16() == 0 and (p.grad is not None) == points_grad
        tag = "points" if points_grad else "planes only"
        rep[f"{tag} raw"] = hp.rel_err(raw.detach().cpu().numpy(), raw64.detach().numpy())
        if points_grad:
            rep["points g_p"] = hp.rel_err(p.grad.cpu().numpy(), p64.grad.numpy())
        rep[f"{tag} planes"] = max(hp.rel_err(a.grad.cpu().numpy(), b.grad.numpy()) for a, b in zip(wl.plane_list, hp.flat_planes(cp)))
        rep[f"{tag} decoders"] = max(hp.rel_err(t.grad.cpu().numpy(), cq[k].grad.numpy()) for k, t in wl.decoders.named_parameters()
                                     if k != "beta")
    with torch.no_grad():
        sdf = ops.decode_sdf_only(pts.to(dev), ops.bound_to_host(wl.scene.bound), wl.planes, wl.decoders)
    rep["sdf only"] = hp.rel_err(sdf.cpu().numpy(), raw64.detach().numpy()[:, 3])
    t16._fresh(wl)
    for k, v in rep.items():
        print(f"margin free points {name}: {k:<16s} {v / RTOL:.3f}")
    bad = {k: v for k, v in rep.items() if not v <= RTOL}
    assert not bad, (name, bad)
