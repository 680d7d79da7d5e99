"""Pins tests/loss_ref.py - the numpy statement of the fused loss the GPU tests of tests/test_gpu_loss_direct.py compare the
kernels with - on the CPU:

  1  against oracle.eslam_oracle.mapping_loss / tracking_loss under float64 autograd, on a batch with no sample near a border of
     the region rule (there float64 and float32 thresholds classify alike): value and the three gradients to 1e-12
  2  its float32 regions against the masks of sdf_losses evaluated in float32 torch on the border batch, where every row holds the
     float32 neighbours of all four thresholds - and against the pattern the strict comparisons imply
  3  the empty-set cases against torch: NaN value, finite or exactly zero gradients (float32 torch on the rays the mask keeps:
     on the border batch only float32 thresholds classify as the reference does)
"""
import numpy as np
import pytest
import torch

from myslam_amd import synth
from oracle import eslam_oracle as orc
from tests import loss_ref as lf


def _wdict(w5):
    return dict(w_fs=w5[0], w_center=w5[1], w_tail=w5[2], w_depth=w5[3], w_color=w5[4])


def _torch_loss(b, truncation, w5, dtype=torch.float64, upstream=1.0):
    """oracle.mapping_loss on the rays the mask keeps (the reference compacts them), autograd gradients scattered back to [R]
    rows (rows of masked rays: zero).  -> value, g_depth, g_rgb, g_sdf as numpy."""
    R = b["gt_depth"].shape[0]
    keep = np.ones(R, bool) if b["ray_mask"] is None else b["ray_mask"] != 0
    idx = torch.from_numpy(np.nonzero(keep)[0])
    leaf = {k: torch.from_numpy(b[k]).to(dtype).requires_grad_(True) for k in ("depth", "rgb", "sdf")}
    cst = {k: torch.from_numpy(b[k]).to(dtype) for k in ("z", "gt_depth", "gt_color")}
    loss = orc.mapping_loss(leaf["depth"][idx], leaf["rgb"][idx], leaf["sdf"][idx], cst["z"][idx], cst["gt_depth"][idx],
                            cst["gt_color"][idx], truncation, _wdict(w5))
    (loss * upstream).backward()
    return (loss.detach().numpy(),) + tuple(leaf[k].grad.numpy() for k in ("depth", "rgb", "sdf"))


def _random_batch(R, S, truncation, stream, zero_every=0):
    """Sorted positive rows round the depth with no sample within 1e-3 of a threshold (samples that fall there are moved)."""
    u = lambda shape, k: synth.hash_uniform(shape, 810_000 + 100 * stream + k)
    gd = (0.5 + 3.5 * u((R,), 0)).astype(np.float32)
    z = (gd[:, None] + (u((R, S), 1) - 0.5) * np.float32(6.0 * truncation)).astype(np.float32)
    for _ in range(8):
        th = np.stack(lf.thresholds(gd, truncation), -1).astype(np.float64)                     # [R,4]
        near = (np.abs(z[:, :, None].astype(np.float64) - th[:, None, :]) < 1e-3).any(-1)
        if not near.any():
            break
        z = np.where(near, z + np.float32(2.5e-3), z).astype(np.float32)
    assert not near.any()
    z = np.sort(z, 1)
    assert (z > 0).all()
    if zero_every:
        gd[::zero_every] = 0.0
    return dict(depth=(gd + (u((R,), 2) - 0.5) * np.float32(0.2)).astype(np.float32), rgb=u((R, 3), 3),
                sdf=((u((R, S), 4) - 0.5) * np.float32(1.9)).astype(np.float32), z=z, gt_depth=gd, gt_color=u((R, 3), 5), ray_mask=None)


# ---- 1. the oracle, away from borders ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("truncation", lf.TRUNCATIONS)
def test_mapping_loss_equals_the_oracle_under_float64_autograd(truncation):
    b = _random_batch(53, 40, truncation, stream=1, zero_every=7)
    acc, loss, g_depth, g_rgb, g_sdf, reg = lf.loss_ref_of(b, truncation, lf.MAPPING_W5, upstream=0.37)
    want = _torch_loss(b, truncation, lf.MAPPING_W5, upstream=0.37)
    assert all(int((reg == c).sum()) > 20 for c in (lf.FRONT, lf.CENTER, lf.TAIL, lf.BACK))
    assert int(acc[lf.A_N_DEPTH]) == 53 - 8 and int(acc[lf.A_N_COLOR]) == 3 * 53
    assert lf.rel(loss, want[0]) <= 1e-12, (loss, want[0])
    for name, a, w in zip(("g_depth", "g_rgb", "g_sdf"), (g_depth, g_rgb, g_sdf), want[1:]):
        assert np.abs(w).max() > 0 and lf.max_rel(a, w) <= 1e-12, (name, lf.max_rel(a, w))
    assert lf.rel(lf.value_from_acc(acc, lf.MAPPING_W5), loss) == 0.0


def test_tracking_loss_equals_the_oracle_under_float64_autograd():
    """The tracker's loss is the same sums over the rays its 10 x median outlier mask keeps (all with depth): the mask goes in
    as ray_mask."""
    truncation = 0.06
    b = _random_batch(61, 24, truncation, stream=2)
    b["depth"][::9] += np.float32(3.0)                                     # outliers
    err = np.abs(b["gt_depth"].astype(np.float64) - b["depth"].astype(np.float64))
    mask = err < 10 * np.sort(err)[(err.size - 1) // 2]                    # torch.median: the lower one
    assert 0 < int((~mask).sum()) < 10
    b["ray_mask"] = mask.astype(np.uint8)
    acc, loss, g_depth, g_rgb, g_sdf, _ = lf.loss_ref_of(b, truncation, lf.TRACKING_W5)
    leaf = {k: torch.from_numpy(b[k]).double().requires_grad_(True) for k in ("depth", "rgb", "sdf")}
    cst = {k: torch.from_numpy(b[k]).double() for k in ("z", "gt_depth", "gt_color")}
    want = orc.tracking_loss(leaf["depth"], leaf["rgb"], leaf["sdf"], cst["z"], cst["gt_depth"], cst["gt_color"], truncation,
                             _wdict(lf.TRACKING_W5))
    want.backward()
    assert int(acc[lf.A_N_COLOR]) == 3 * int(mask.sum()) and int(acc[lf.A_N_DEPTH]) == int(mask.sum())
    assert lf.rel(loss, want.item()) <= 1e-12
    for name, a in (("depth", g_depth), ("rgb", g_rgb), ("sdf", g_sdf)):
        assert lf.max_rel(a, leaf[name].grad.numpy()) <= 1e-12, name
        assert not a[~mask].any(), name


def test_float32_evaluation_stays_close_and_pairwise_sums_are_pairwise():
    b = _random_batch(53, 40, 0.06, stream=3)
    a64, l64 = lf.loss_ref_of(b, 0.06, lf.MAPPING_W5)[:2]
    a32, l32 = lf.loss_ref_of(b, 0.06, lf.MAPPING_W5, dtype=np.float32)[:2]
    assert a32.dtype == np.float32 and a64.dtype == np.float64
    assert all(a32[k] == a64[k] for k in lf.COUNTS)
    assert 0 < max(lf.rel(a32[k], a64[k]) for k in lf.SUMS) < 1e-5 and lf.rel(l32, l64) < 1e-5
    # 2^24 + 1 + 1 + 1 + 1: a running float32 sum stays at 2^24, the pairwise one reaches 2^24 + 4
    x = np.asarray([2.0 ** 24, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0], np.float32)
    assert float(lf.pairwise_sum(x[[1, 2, 3, 4, 0, 5, 6, 7]], np.float32)) == 2.0 ** 24 + 4
    assert float(lf.pairwise_sum(np.zeros(0), np.float32)) == 0.0 and float(lf.pairwise_sum(np.arange(7.0), np.float64)) == 21.0


# ---- 2. regions on the border batch -------------------------------------------------------------------------------------------
def _torch_masks_f32(z, gt_depth, truncation):
    """The four masks as sdf_losses forms them (oracle/eslam_oracle.py, reference src/Mapper.py:124-134), float32 tensors and a
    Python-float truncation."""
    z_vals, d = torch.from_numpy(z), torch.from_numpy(gt_depth)[:, None]
    front = z_vals < (d - truncation)
    back = z_vals > (d + truncation)
    center = (z_vals > (d - 0.4 * truncation)) & (z_vals < (d + 0.4 * truncation))
    tail = (~front) & (~back) & (~center)
    return front.numpy(), center.numpy(), tail.numpy(), back.numpy()


@pytest.mark.parametrize("truncation", lf.TRUNCATIONS)
@pytest.mark.parametrize("S", [29, 77])
def test_regions_equal_float32_torch_on_the_border_batch(S, truncation):
    b = lf.border_batch(12, S, truncation, "plain")
    reg = lf.regions(b["z"], b["gt_depth"], truncation)
    front, center, tail, back = _torch_masks_f32(b["z"], b["gt_depth"], truncation)
    assert not (front & center).any() and not (back & center).any() and not (front & back).any()
    for code, mask in ((lf.FRONT, front), (lf.CENTER, center), (lf.TAIL, tail), (lf.BACK, back)):
        assert np.array_equal(reg == code, mask), code
        assert mask.any(1).all(), "every row holds every region"
    # the float32 value of the float32 oracle: one sample in the wrong region moves a 200x-weighted mean by far more than this
    t = {k: torch.from_numpy(b[k]) for k in ("depth", "rgb", "sdf", "z", "gt_depth", "gt_color")}
    want = float(orc.mapping_loss(t["depth"], t["rgb"], t["sdf"], t["z"], t["gt_depth"], t["gt_color"], truncation, _wdict(lf.MAPPING_W5)))
    got = float(lf.loss_ref_of(b, truncation, lf.MAPPING_W5, dtype=np.float32)[1])
    assert lf.rel(got, want) <= 2e-5, (got, want)
    # every row holds all twelve border values of its depth
    for i in range(12):
        assert np.isin(lf.border_values(b["gt_depth"][i], truncation), b["z"][i]).all(), i


@pytest.mark.parametrize("truncation", lf.TRUNCATIONS)
@pytest.mark.parametrize("d", lf.DEPTHS)
def test_border_values_are_distinct_and_fall_where_strict_comparisons_put_them(d, truncation):
    """Below / on / above d - t: front, tail, tail.  d - 0.4 t: tail, tail, centre.  d + 0.4 t: centre, tail, tail.  d + t: tail,
    tail, back.  A `<=` in place of one `<` moves the middle value of one triple."""
    v = lf.border_values(d, truncation)
    assert v.dtype == np.float32 and np.unique(v).size == 12 and (np.diff(v) > 0).all() and v[0] > 0
    F, C, T, B = lf.FRONT, lf.CENTER, lf.TAIL, lf.BACK
    assert lf.regions(v[None], np.asarray([d], np.float32), truncation)[0].tolist() == [F, T, T, T, T, C, C, T, T, T, T, B]
    # the thresholds are float32 sums of float32 terms: 0.4 * t is multiplied in double and cast once
    t04 = np.float32(0.4 * truncation)
    assert v[4] == np.float32(d) - t04 and v[7] == np.float32(d) + t04


def test_where_a_float32_product_would_move_a_border():
    """What `0.4f * t` would give.  t = 0.06: the same float32, nothing to see.  t = 0.1: one ulp of 0.04 away, which survives the
    addition to the depth only at d = 0.15 - there both centre thresholds move by one float32 step, so the middle value of each
    triple changes region."""
    assert np.float32(0.4) * np.float32(0.06) == np.float32(0.4 * 0.06)
    wrong, right = np.float32(0.4) * np.float32(0.1), np.float32(0.4 * 0.1)
    assert wrong != right
    moved = [d for d in lf.DEPTHS if np.float32(d) - wrong != np.float32(d) - right and np.float32(d) + wrong != np.float32(d) + right]
    assert moved == [0.15]
    d = np.float32(0.15)
    v = lf.border_values(d, 0.1)
    reg = lf.regions(v[None], d[None], 0.1)[0]
    z = v[None]
    center_wrong = (z > d - wrong) & (z < d + wrong)
    assert (center_wrong[0, 3:9] != (reg[3:9] == lf.CENTER)).any()


# ---- 3. empty sets -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("truncation", lf.TRUNCATIONS)
@pytest.mark.parametrize("variant", lf.VARIANTS)
def test_variants_against_torch(variant, truncation):
    b = lf.border_batch(9, 29, truncation, variant)
    acc, loss, g_depth, g_rgb, g_sdf, reg = lf.loss_ref_of(b, truncation, lf.MAPPING_W5)
    # float32 torch: on this batch only float32 thresholds classify as the reference does, so the figures agree to float32
    # rounding (2e-5; a sample in another region moves them by 1e-3 and more) - NaN-ness, finiteness and zeros are exact
    want = _torch_loss(b, truncation, lf.MAPPING_W5, dtype=torch.float32)
    nan = variant in ("no_depth", "all_masked", "no_tail")
    assert bool(np.isnan(loss)) == nan == bool(np.isnan(want[0])), (variant, loss, want[0])
    if not nan:
        assert lf.rel(loss, want[0]) <= 2e-5
    for name, a, w in zip(("g_depth", "g_rgb", "g_sdf"), (g_depth, g_rgb, g_sdf), want[1:]):
        assert np.isfinite(a).all() and np.isfinite(w).all(), name
        assert lf.max_rel(a, w) <= 2e-5, (variant, name, lf.max_rel(a, w))
        assert np.array_equal(a == 0, w == 0), (variant, name)
    mc, m = lf.members(b["gt_depth"], b["ray_mask"])
    assert not g_rgb[~mc].any() and not g_depth[~m].any() and not g_sdf[~m].any() and (reg[~m] == -1).all()
    counts = {lf.SLOT_NAMES[k]: int(acc[k]) for k in lf.COUNTS}
    if variant == "no_depth":
        assert counts == dict(n_front=0, n_center=0, n_tail=0, n_depth=0, n_color=27) and g_rgb.any()
    elif variant == "all_masked":
        assert not any(counts.values()) and not acc.any() and not g_rgb.any()
    elif variant == "no_tail":
        assert counts["n_tail"] == 0 and counts["n_center"] > 0 and counts["n_front"] > 0 and g_sdf.any() and g_depth.any()
    elif variant == "depthless_masked":
        assert counts["n_depth"] == 9 - 4 - 1 and counts["n_color"] == 3 * (9 - 2)
        assert np.isnan(b["gt_depth"]).sum() == 1 and np.signbit(b["gt_depth"][b["gt_depth"] == 0]).tolist() == [False, True]
    else:
        assert counts["n_depth"] == 9 and min(counts.values()) > 0


def test_border_batch_shapes_and_streams():
    for R, S in ((1, 1), (3, 5), (5, 65), (7, 256)):
        b = lf.border_batch(R, S, 0.06, "depthless_masked", stream=R)
        assert b["z"].shape == (R, S) and b["sdf"].shape == (R, S) and b["ray_mask"].shape == (R,)
        assert all(v.dtype == np.float32 for k, v in b.items() if k != "ray_mask")
    a, c = lf.border_batch(9, 29, 0.06, "plain", stream=1), lf.border_batch(9, 29, 0.06, "plain", stream=2)
    assert not np.array_equal(a["sdf"], c["sdf"]) and not np.array_equal(a["z"], c["z"])
    # error terms stay away from zero, so that relative bars on the sums mean something
    for t in lf.TRUNCATIONS:
        b = lf.border_batch(12, 77, t, "plain")
        d = b["gt_depth"][:, None].astype(np.float64)
        assert np.abs(b["z"] + b["sdf"].astype(np.float64) * t - d).min() >= 1e-2 and np.abs(b["sdf"] - 1.0).min() >= 1e-2
        assert np.abs(b["gt_depth"] - b["depth"]).min() >= 1e-2
