"""The render metrics and the visualiser's panel on the GPU (ops.frame_stats, ops.ssim, ops.vis_panel, ops.frame_metrics;
csrc/eslam_vis.hip) against the numpy models of tests/vis_ref.py, Frame_Visualizer's files, and the system run from a
config with the visualisers and the render evaluation on.

Criteria.  SSIM: map and mean within vis_ref.ssim_tolerance of the float64 model - 4 x the float32 model's own worst
deviation from it on exactly these cases (1.8e-4 with the 16 x 32 tile; the mutations of the definition deviate by 2.2e-3
and more: profiles/vis_margins.txt, tests/test_vis_ref.py); the mean of two runs bit-equal.  Stats: n_valid and the maximum
exact, the sums within 1e-12 relative of math.fsum (a float64 tree over <= 2.4e6 terms errs below 22 x 2^-53), bit-equal
run to run.  Panel: bit for bit."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import vis_ref as vr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _tiles():
    from myslam_amd import _hip
    return _hip.SSIM_TILE_H, _hip.SSIM_TILE_W


def _gpu(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _lut():
    from myslam_amd import ops
    return ops.load_plasma_lut()


# ---- SSIM --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ssim_tol():
    return vr.ssim_tolerance(*_tiles())


def _ssim_params():
    from myslam_amd import _hip
    return [(H, W, C) for H, W in vr.ssim_shapes(_hip.SSIM_TILE_H, _hip.SSIM_TILE_W) for C in vr.CHANNELS]


@pytest.mark.parametrize("H,W,C", _ssim_params())
def test_ssim_against_the_float64_model(ssim_tol, H, W, C):
    from myslam_amd import ops
    th, tw = _tiles()
    for kind, a, b in vr.ssim_inputs(H, W, C):
        want_map, want_mean = vr.ssim64(a, b)
        ta, tb = _gpu(a, b)
        mean, smap = ops.ssim(ta, tb, return_map=True)
        assert mean.device == DEV and mean.dtype == torch.float64 and mean.dim() == 0
        assert smap.dtype == torch.float32 and tuple(smap.shape) == (H - 10, W - 10, C)
        dev_map = float(np.abs(smap.cpu().numpy().astype(np.float64) - want_map).max())
        dev_mean = abs(float(mean) - want_mean)
        model_map, model_mean = vr.ssim32(a, b, th, tw)
        print(f"{H}x{W}x{C} {kind}: map {dev_map:.3e} mean {dev_mean:.3e} (tolerance {ssim_tol:.3e}); vs float32 model "
              f"{float(np.abs(smap.cpu().numpy() - model_map).max()):.3e}")
        assert dev_map <= ssim_tol and dev_mean <= ssim_tol, kind
        # the mean is the float64 sum of the float32 map's values; run to run the same bits, with or without the map
        assert abs(float(mean) - float(smap.cpu().numpy().astype(np.float64).mean())) <= 1e-13
        again = ops.ssim(ta, tb)
        assert torch.equal(again, mean)
        if kind == "itself":
            assert float(mean) == 1.0 and bool((smap == 1.0).all())
        if C == 1:                                                       # a [H,W] image is the one-channel case
            m2, s2 = ops.ssim(ta[:, :, 0], tb[:, :, 0], return_map=True)
            assert torch.equal(m2, mean) and tuple(s2.shape) == (H - 10, W - 10) and torch.equal(s2, smap[:, :, 0])


def test_ssim_refuses_bad_arguments():
    from myslam_amd import ops
    a = torch.rand(16, 16, 3, device=DEV)
    with pytest.raises(RuntimeError, match="11"):
        ops.ssim(a[:10], a[:10])
    with pytest.raises(RuntimeError, match="11"):
        ops.ssim(a[:, :10], a[:, :10])
    with pytest.raises(RuntimeError, match="channels"):
        ops.ssim(a[:, :, :2], a[:, :, :2])
    with pytest.raises(RuntimeError, match="one shape"):
        ops.ssim(a, a[:15])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ssim(a.cpu(), a.cpu())
    with pytest.raises(RuntimeError, match="float32"):
        ops.ssim(a.double(), a.double())
    # a non-contiguous view is taken as it reads
    t = torch.rand(3, 20, 24, device=DEV).permute(1, 2, 0)
    assert torch.equal(ops.ssim(t, t.flip(2)), ops.ssim(t.contiguous(), t.flip(2).contiguous()))


# ---- stats -------------------------------------------------------------------------------------------------------------
def _stats_case(H, W, depth_kind, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    gd = rng.uniform(0.3, 5.0, (H, W)).astype(f)
    if depth_kind == "zeros":
        gd[rng.uniform(size=(H, W)) < 0.3] = 0
    elif depth_kind == "invalid":
        gd[:] = 0
    d = (gd + rng.normal(0, 0.2, (H, W))).astype(f)
    gc = rng.uniform(0, 1, (H, W, 3)).astype(f)
    c = (gc + rng.normal(0, 0.2, (H, W, 3))).astype(f)                   # unclipped: values outside [0, 1] stay
    return d, c, gd, gc


def _stats_params():
    from myslam_amd import _hip
    n = _hip.STATS_BLOCK_PIXELS
    assert n == 64 * 64 and n + 1 == 17 * 241
    return [(1, 1, "full"), (64, n // 64, "full"), (17, 241, "zeros"), (240, 320, "zeros"), (240, 320, "full"),
            (37, 45, "invalid"), (1, 1, "invalid")]


@pytest.mark.parametrize("H,W,kind", _stats_params())
def test_frame_stats_against_the_model(H, W, kind):
    from myslam_amd import ops
    d, c, gd, gc = _stats_case(H, W, kind, seed=H * W)
    want = vr.stats64(d, c, gd, gc)
    td, tc, tgd, tgc = _gpu(d, c, gd, gc)
    out = ops.frame_stats(td, tc, tgd, tgc)
    assert out.device == DEV and out.dtype == torch.float64 and tuple(out.shape) == (4,)
    got = out.cpu().tolist()
    print(f"{H}x{W} {kind}: got {got} want {want}")
    assert got[0] == want[0] and got[3] == want[3]
    for k in (1, 2):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k
    if kind == "invalid":
        assert got[0] == 0.0 and got[1] == 0.0 and got[3] == 0.0
    assert torch.equal(ops.frame_stats(td, tc, tgd, tgc), out)
    assert torch.equal(ops.frame_stats(td.double(), tc, tgd, tgc), out)  # render_img's float64 depth is cast with .float()


def test_frame_metrics_against_render_quality_expression():
    from myslam_amd import ops
    H, W = 240, 320
    d, c, gd, gc = _stats_case(H, W, "zeros", seed=5)
    td, tc, tgd, tgc = _gpu(d, c, gd, gc)
    m = ops.frame_metrics(td.double(), tc, tgd, tgc)
    assert set(m) == {"psnr", "ssim", "depth_l1", "n_valid"} and all(isinstance(v, float) for v in m.values())
    # Slam.render_quality's expressions on the same tensors
    valid = tgd > 0
    l1 = float((td.double().float() - tgd)[valid].abs().mean())
    mse = float(((tc - tgc) ** 2).mean())
    psnr = float(-10.0 * torch.log10(torch.tensor(mse)))
    print(f"psnr {m['psnr']:.6f} vs {psnr:.6f}; depth L1 {m['depth_l1']:.8f} vs {l1:.8f}; ssim {m['ssim']:.6f}")
    assert abs(m["psnr"] - psnr) <= 1e-3
    assert abs(m["depth_l1"] - l1) <= 1e-5 * l1                          # (torch's mean is a float32 pairwise sum)
    assert m["n_valid"] == float(valid.sum())
    assert m["ssim"] == float(ops.ssim(tc, tgc)) and abs(m["ssim"] - vr.ssim64(c, gc)[1]) <= vr.ssim_tolerance(*_tiles())
    none = ops.frame_metrics(td, tc, torch.zeros_like(tgd), tgc)
    assert none["n_valid"] == 0.0 and math.isnan(none["depth_l1"]) and none["psnr"] == m["psnr"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_stats(td.cpu(), tc, tgd, tgc)
    with pytest.raises(RuntimeError, match=r"\[H,W,3\]"):
        ops.frame_stats(td, tc[:, :, :2], tgd, tgc)


# ---- the panel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vr.panel_cases(), ids=[c[0] for c in vr.panel_cases()])
def test_vis_panel_bit_for_bit(case):
    from myslam_amd import ops
    name, d, c, gd, gc = case
    want = vr.panel32(d, c, gd, gc, _lut())
    td, tc, tgd, tgc = _gpu(d, c, gd, gc)
    got = ops.vis_panel(td, tc, tgd, tgc)
    assert got.device == DEV and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    diff = got.cpu().numpy() != want
    assert not diff.any(), f"{name}: {int(diff.sum())} bytes differ, first at {np.argwhere(diff)[:4].tolist()}"
    stats = ops.frame_stats(torch.nan_to_num(td, nan=0.0), tc, tgd, tgc)
    assert torch.equal(ops.vis_panel(td.double(), tc, tgd, tgc, stats=stats), got)
    with pytest.raises(RuntimeError, match="stats"):
        ops.vis_panel(td, tc, tgd, tgc, stats=stats.float())


class _FixedRenderer:
    """render_img returns a fixed frame (depth as float64, like Renderer.render_img)."""

    def __init__(self, depth, color):
        self.depth, self.color, self.calls = depth, color, []

    def render_img(self, all_planes, decoders, c2w, truncation, device, gt_depth=None):
        self.calls.append((tuple(c2w.shape), float(truncation), tuple(gt_depth.shape)))
        return self.depth.double(), self.color


def test_save_imgs_writes_the_panel(tmp_path):
    from PIL import Image
    from myslam_amd import ops
    from myslam_amd.src.utils.Frame_Visualizer import Frame_Visualizer
    name, d, c, gd, gc = vr.panel_cases()[2]                             # 37 x 45
    H, W = gd.shape
    d = np.nan_to_num(d, nan=2.0)
    td, tc, tgd, tgc = _gpu(d, c, gd, gc)
    want = ops.vis_panel(td, tc, tgd, tgc).cpu().numpy()
    pose7 = torch.tensor([[1.0, 0, 0, 0, 0.1, 0.2, 0.3]], device=DEV)
    for titles in (True, False):
        r = _FixedRenderer(td, tc)
        vis = Frame_Visualizer(4, 2, str(tmp_path / f"png{titles}"), r, 0.06, False, device=DEV, fmt="png", titles=titles)
        assert vis.save_imgs(3, 2, tgd, tgc, pose7, None, None) is None and r.calls == []
        m = vis.save_imgs(8, 6, tgd[None], tgc[None], pose7, None, None)      # a [1,7] pose goes through cam_pose_to_matrix
        assert r.calls == [((4, 4), 0.06, (H, W))]
        assert os.listdir(tmp_path / f"png{titles}") == ["00008_0006.png"]
        img = np.asarray(Image.open(tmp_path / f"png{titles}" / "00008_0006.png"))
        r0, r1 = vis.panel_rows(H)
        assert img.shape == ((2 * H + 28, 3 * W, 3) if titles else (2 * H, 3 * W, 3))
        assert np.array_equal(img[r0], want[:H]) and np.array_equal(img[r1], want[H:])
        if titles:
            assert (img[:r0.start] != 255).any() and (img[r0.stop:r1.start] != 255).any()      # something was drawn
        assert m == ops.frame_metrics(td, tc, tgd, tgc) and 0.0 < m["ssim"] <= 1.0
    vis = Frame_Visualizer(1, 1, str(tmp_path / "jpg"), _FixedRenderer(td, tc), 0.06, False, device=DEV)
    vis.save_imgs(0, 0, tgd, tgc, torch.eye(4, device=DEV), None, None)
    with Image.open(tmp_path / "jpg" / "00000_0000.jpg") as im:
        assert im.format == "JPEG" and im.size == (3 * W, 2 * H + 28)
        im.load()


# ---- the system ----------------------------------------------------------------------------------------------------------
N_FRAMES = 9


@pytest.fixture(scope="module")
def toy_sequence(tmp_path_factory):
    from tests.test_gpu_frames import _write_toy_sequence
    root = tmp_path_factory.mktemp("vis_seq")
    _write_toy_sequence(root / "seq", N_FRAMES)
    return root / "seq"


def _names(folder):
    return sorted(os.path.splitext(f)[0] for f in os.listdir(folder))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_eslam_writes_panels_and_render_eval(toy_sequence, tmp_path, graph):
    from PIL import Image
    from myslam_amd.src.ESLAM import ESLAM
    from tests.test_gpu_frames import _toy_cfg
    out = tmp_path / "out"
    cfg = _toy_cfg(toy_sequence, out)
    cfg["tracking"].update(vis_freq=4, vis_inside_freq=4, no_vis_on_first_frame=False)
    cfg["mapping"].update(vis_freq=4, vis_inside_freq=50, no_vis_on_first_frame=False)
    cfg["render_eval"] = dict(every=4)
    eslam = ESLAM(cfg, SimpleNamespace(input_folder=None, output=None, graph=graph))
    stats = eslam.run()
    assert stats["tracking_iters"] == 8 * (N_FRAMES - 1) and stats["mapping_iters"] == 100 + 10 * 2
    # the reference's gate: idx % freq == 0 and iter % inside_freq == 0 (Tracker.py:276-302, Mapper.py:308-310)
    assert _names(out / "tracking_vis") == ["00000_0000", "00004_0000", "00004_0004", "00008_0000", "00008_0004"]
    assert _names(out / "mapping_vis") == ["00000_0000", "00000_0050", "00004_0000", "00008_0000"]
    for folder in ("tracking_vis", "mapping_vis"):
        for f in os.listdir(out / folder):
            with Image.open(out / folder / f) as im:
                assert im.format == "JPEG" and im.size == (3 * 320, 2 * 240 + 28)
    with open(out / "render_eval.json") as fh:
        rep = json.load(fh)
    rows = rep["frames"]
    assert [r["idx"] for r in rows] == [0, 4, 8] and rep["every"] == 4
    for k in ("psnr", "ssim", "depth_l1"):
        assert abs(rep[k] - sum(r[k] for r in rows) / 3) <= 1e-12 * abs(rep[k])
    for r in rows:
        assert 0.0 < r["ssim"] <= 1.0 and math.isfinite(r["psnr"]) and math.isfinite(r["depth_l1"]) and r["depth_l1"] >= 0.0
    assert eslam.render_eval == rep and (out / "ate.json").exists()
    print(f"\ngraph={graph}: render eval {dict((k, rep[k]) for k in ('psnr', 'ssim', 'depth_l1'))}, {stats}")


def test_eslam_with_the_shipped_defaults_writes_nothing_new(toy_sequence, tmp_path):
    """configs/ESLAM.yaml's vis_freq: 4000 with no_vis_on_first_frame: True never fires on a short sequence: no hook is set,
    no image and no render_eval.json are written, and the loop runs the iterations it runs without the keys."""
    from myslam_amd.src.ESLAM import ESLAM
    from tests.test_gpu_frames import _toy_cfg
    out = tmp_path / "out"
    cfg = _toy_cfg(toy_sequence, out)
    for sec in ("tracking", "mapping"):
        cfg[sec].update(vis_freq=4000, vis_inside_freq=400, no_vis_on_first_frame=True)
    eslam = ESLAM(cfg, SimpleNamespace(input_folder=None, output=None))
    stats = eslam.run()
    assert eslam.slam.on_iter is None and eslam.render_eval is None
    assert stats["tracking_iters"] == 8 * (N_FRAMES - 1) and stats["mapping_iters"] == 100 + 10 * 2
    for folder in ("tracking_vis", "mapping_vis"):
        assert not (out / folder).exists() or os.listdir(out / folder) == []
    assert not (out / "render_eval.json").exists() and (out / "ate.json").exists()
