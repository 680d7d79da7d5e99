"""What tests/test_gpu_every_texel.py rests on, without a GPU: how much of the plane gradients hp.plane_grads_close never looks
at on the suite's usual batches, that a batch filtered by every_texel.unambiguous_rays loses nothing, that the float32 oracle
meets the criteria of the GPU tests on such a batch with nothing set aside (so a correct float32 implementation can), and that
an error the old criterion lets through is refused on the filtered batch.

Rays: the harness's own (every_texel.harness_rays: synthetic image, centre pose, pre-filter), synth planes, float32 oracle
z_vals.  Run time: ~15 s, most of it the float32 / float64 oracle steps of 640 rays x 64 samples.
"""
import functools

import numpy as np
import pytest
import torch

from tests import every_texel as et
from tests import helpers as hp
from tests import hostile_rays as hr

COARSE = (0, 2, 4, 6, 8, 10)          # all_planes order: (group, level)
# (scene, plane shapes, R, n_strat, n_imp, zero_frac, rays asked for in the pool)
CASES = {
    "room0_640x64": ("room0", None, 640, 56, 8, 0.1, 1100),
    "room0_37x29": ("room0", None, 37, 23, 6, 0.0, 64),
    "one_cell_640x64": ("toy", "one_cell", 640, 56, 8, 0.1, 2000),
}


@functools.lru_cache(maxsize=None)
def _case(name, state="trained"):
    """Pool, its float32-oracle z_vals, the unfiltered batch (the pool's first R rays) and the filtered one (the first R rays
    without an ambiguous sample), each with p_nor and amb of its samples."""
    from myslam_amd import scene as scn
    scene_name, shapes, R, ns, ni, zero_frac, ask = CASES[name]
    sc = scn.make_scene(scene_name)
    if shapes is not None:
        sc = et.with_shapes(sc, shapes)
    mdl = hr.model(sc, state)
    pool = et.harness_rays(sc, ask, zero_frac)
    P = pool.rays_o.shape[0]
    rand = hr.rand_for(P, ns, ni)
    z = hr.oracle_z(mdl, sc, pool, ns, ni, rand, torch.float32)
    keep = et.unambiguous_rays(mdl, sc, pool, z, R)
    out = dict(scene=sc, mdl=mdl, R=R, S=ns + ni, P=P, keep=keep, cot=hr.cotangent(R, ns + ni))
    for key, idx in (("raw", torch.arange(R)), ("flt", keep)):
        b = et.take(pool, idx)
        pn, amb = hr.ambiguous(mdl, sc, b, z[idx])
        out[key] = dict(b=b, z=z[idx], pn=pn, amb=amb, share=hp.excluded_share(pn, amb, sc.plane_shapes))
    return out


@functools.lru_cache(maxsize=None)
def _oracles(name, which):
    c = _case(name)
    d = c[which]
    return tuple(hr.oracle_step(c["mdl"], c["scene"], d["b"], d["z"], c["cot"], dt) for dt in (torch.float32, torch.float64))


def _fmt(share):
    return " ".join(f"{v:.2f}" for v in share)


def test_excluded_share_counts_touched_texels_that_are_set_aside():
    """Two samples on a 3 x 3 / 2 x 2 scene by hand: the ambiguous one sits inside the plane's first cell, the other in its last."""
    shapes = [[(1, 32, 3, 3), (1, 32, 2, 2)]] * 6
    pn = torch.tensor([[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]], dtype=torch.float64)
    amb = torch.tensor([True, False])
    share = hp.excluded_share(pn, amb, shapes)
    # 3 x 3: cells (0,0) and (1,1): 4 + 4 corners, texel (1,1) shared -> 7 touched, 4 set aside; 2 x 2: all four, all set aside
    assert share == [4 / 7, 1.0] * 6
    assert hp.excluded_share(pn, torch.zeros(2, dtype=torch.bool), shapes) == [0.0] * 12
    assert hp.excluded_share(pn[:0], amb[:0], shapes) == [0.0] * 12


def test_the_usual_batch_loses_most_of_its_coarse_texels():
    """room0 640 x (56+8) trained, as tests/test_gpu_rank16_scatter.py and tests/test_gpu_paired_scatter.py run it: more than half
    of the touched texels of at least one coarse plane are never compared - and none after the filter."""
    c = _case("room0_640x64")
    raw, flt = c["raw"], c["flt"]
    print(f"room0 640x64 trained: pool {c['P']}, unfiltered {int(raw['amb'].sum())} ambiguous samples, share {_fmt(raw['share'])}")
    assert int(raw["amb"].sum()) > 0
    assert max(raw["share"][k] for k in COARSE) > 0.5, raw["share"]
    assert int(flt["amb"].sum()) == 0 and flt["share"] == [0.0] * 12
    assert c["keep"].numel() == 640 and bool((c["keep"][1:] > c["keep"][:-1]).all())
    n0 = int((flt["b"].gt_depth == 0).sum())
    print(f"filtered: last pool ray used {int(c['keep'][-1])}, {n0} depth-less rays")
    assert 0 < n0 < 640, "the filtered batch keeps rays of both samplers"


def test_the_smallest_batch_is_filtered_too():
    """37 x (23+6): 1015 + 58 samples.  Whatever the unfiltered batch sets aside (every ambiguous sample costs each plane at least
    one texel), the filtered one sets aside nothing."""
    c = _case("room0_37x29")
    raw, flt = c["raw"], c["flt"]
    print(f"room0 37x29 trained: pool {c['P']}, unfiltered {int(raw['amb'].sum())} ambiguous samples, share {_fmt(raw['share'])}")
    assert all((v > 0) == bool(raw["amb"].any()) for v in raw["share"])
    assert int(flt["amb"].sum()) == 0 and flt["share"] == [0.0] * 12 and c["keep"].numel() == 37


def test_on_2x2_planes_one_ambiguous_sample_empties_the_comparison():
    """All twelve planes 2 x 2: a sample inside the bound touches all four texels of every plane, so one ambiguous sample sets the
    whole gradient aside (plane_grads_close then compares nothing and its margin is 0.0); the filtered batch loses nothing."""
    c = _case("one_cell_640x64")
    raw, flt = c["raw"], c["flt"]
    inside = (raw["pn"].abs() < 1).all(1)
    print(f"2x2 planes 640x64 trained: unfiltered {int(raw['amb'].sum())} ambiguous samples ({int((raw['amb'] & inside).sum())} inside), "
          f"share {_fmt(raw['share'])}")
    assert bool((raw["amb"] & inside).any())
    assert raw["share"] == [1.0] * 12
    o32, o64 = _oracles("one_cell_640x64", "raw")
    pr = []
    ok, _ = hp.plane_grads_close([g + 1.0 for g in o32["planes"]], o32["planes"], o64["planes"], raw["pn"], raw["amb"],
                                 c["scene"].plane_shapes, report=pr)
    assert ok and max(v for _, v in pr) == 0.0, "every gradient off by 1.0 passes: nothing is compared"
    assert int(flt["amb"].sum()) == 0 and flt["share"] == [0.0] * 12


@pytest.mark.parametrize("name", list(CASES))
def test_float32_oracle_meets_the_criteria_with_nothing_set_aside(name):
    """The filtered batch through the float32 and the float64 oracle: hr.accept with max_excluded = 0.0 and no ambiguous sample
    (no texel set aside, no slack on the decoder gradients), all twelve plane gradients non-zero."""
    c = _case(name)
    flt = c["flt"]
    o32, o64 = _oracles(name, "flt")
    assert int(flt["amb"].sum()) == 0
    assert all(np.abs(g).max() > 0 for g in o64["planes"])
    rep = hr.accept(o32, o32, o64, flt["pn"], flt["amb"], c["scene"], label=name, max_excluded=0.0)
    worst32 = max(hp.rel_err(a, b) for a, b in zip(o32["planes"], o64["planes"]))
    print(f"{name}: float32 oracle / bar {({k: round(v, 3) for k, v in rep.items()})}, planes float32 vs float64 {worst32:.2e}")


def test_max_excluded_refuses_the_unfiltered_batch():
    c = _case("room0_640x64")
    raw = c["raw"]
    o32, o64 = _oracles("room0_640x64", "raw")
    args = (o32["planes"], o32["planes"], o64["planes"], raw["pn"], raw["amb"], c["scene"].plane_shapes)
    assert hp.plane_grads_close(*args)[0] and hp.plane_grads_close(*args, max_excluded=None)[0]
    ok, msg = hp.plane_grads_close(*args, max_excluded=0.0)
    assert not ok and "set aside" in msg
    ok, msg = hp.plane_grads_close(*args, max_excluded=0.5)
    assert not ok and "set aside" in msg, "a coarse plane loses more than half"
    assert hp.plane_grads_close(*args, max_excluded=1.0)[0]


def test_a_planted_error_passes_the_old_criterion_and_fails_on_the_filtered_batch():
    """1e-3 of the plane's largest gradient - ten times the bar - added to ONE channel of one coarse-plane texel.  On the
    unfiltered batch, in a texel an ambiguous sample touches: plane_grads_close returns ok.  On the filtered batch every touched
    texel is compared: the same error in any of them is refused."""
    c = _case("room0_640x64")
    shapes = c["scene"].plane_shapes

    def plant(grads, k, texel):
        out = [g.copy() for g in grads]
        flat = out[k].reshape(out[k].shape[1], -1)             # (a view: [C, h*w])
        flat[5, texel] += 1e-3 * np.abs(grads[k]).max()
        return out

    raw = c["raw"]
    o32, o64 = _oracles("room0_640x64", "raw")
    tex = hp.texels_of(raw["pn"], shapes)
    for k in COARSE:
        aside = tex[k][raw["amb"]].reshape(-1)
        texel = int(aside[np.abs(o64["planes"][k].reshape(32, -1)[:, aside.numpy()]).sum(0).argmax()])     # the heaviest of them
        ok, msg = hp.plane_grads_close(plant(o32["planes"], k, texel), o32["planes"], o64["planes"], raw["pn"], raw["amb"], shapes)
        assert ok, (k, texel, msg)
    flt = c["flt"]
    f32, f64 = _oracles("room0_640x64", "flt")
    tex = hp.texels_of(flt["pn"], shapes)
    for k in COARSE:
        touched = torch.unique(tex[k].reshape(-1))
        for texel in (int(touched[0]), int(touched[len(touched) // 2]), int(touched[-1])):
            ok, msg = hp.plane_grads_close(plant(f32["planes"], k, texel), f32["planes"], f64["planes"], flt["pn"], flt["amb"], shapes,
                                           max_excluded=0.0)
            assert not ok and f"plane {k}" in msg, (k, texel, msg)
    assert hp.plane_grads_close(f32["planes"], f32["planes"], f64["planes"], flt["pn"], flt["amb"], shapes, max_excluded=0.0)[0]
