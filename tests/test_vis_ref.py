"""CPU tests of the render metrics' and the visualiser panel's numpy models (tests/vis_ref.py) and of the acceptance
criterion the GPU tests hold the kernels to: it must accept the float32 model in the kernel's operation order and reject
every listed mutation of the definition, well above the tolerance.  Also the host-side pieces: the committed colour table,
the visualiser's gate, the loop's on_iter hook (on the oracle backend).  Seconds."""
import os

import numpy as np
import pytest
import torch

from tests import vis_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiles():
    from myslam_amd import _hip
    return _hip.SSIM_TILE_H, _hip.SSIM_TILE_W


def _lut():
    from myslam_amd import ops
    return ops.load_plasma_lut()


def test_tile_constants_match_the_header():
    import re
    from myslam_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "eslam_hip.h")).read()
    for name, val in (("ESLAM_SSIM_TILE_H", _hip.SSIM_TILE_H), ("ESLAM_SSIM_TILE_W", _hip.SSIM_TILE_W),
                      ("ESLAM_STATS_BLOCK_PIXELS", _hip.STATS_BLOCK_PIXELS)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == val


def test_committed_lut_is_matplotlibs_plasma():
    matplotlib = pytest.importorskip("matplotlib")
    lut = _lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert np.array_equal(lut, matplotlib.colormaps["plasma"](np.arange(256), bytes=True)[:, :3])


def test_no_matplotlib_import_in_the_package():
    import glob
    for path in glob.glob(os.path.join(ROOT, "myslam_amd", "**", "*.py"), recursive=True):
        src = open(path).read()
        assert "import matplotlib" not in src and "from matplotlib" not in src, path


def test_ssim_of_an_image_with_itself_is_exactly_one():
    for H, W, C in ((11, 11, 1), (37, 45, 3)):
        for kind, a, b in vr.ssim_inputs(H, W, C):
            m, mean = vr.ssim64(a, a)
            assert m.shape == (H - 10, W - 10, C) and np.all(m == 1.0) and mean == 1.0, kind
            m32, mean32 = vr.ssim32(a, a, *_tiles())
            assert np.all(m32 == 1.0) and mean32 == 1.0, kind


def test_window_and_a_hand_computed_value():
    w = vr.window()
    assert w.dtype == np.float32 and abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-7 and np.array_equal(w, w[::-1])
    assert abs(float(w[5]) - 0.26601172) < 1e-7                          # 1 / sum_k exp(-k^2 / 4.5)
    # two constant images p and q: no variance, ssim = (2 p q + C1) / (p^2 + q^2 + C1).  The float32-rounded weights sum to
    # 1 + d with |d| < 1e-7, which leaves "variances" of order d q^2 = 6e-8 against C2 = 9e-4: within 1e-4 relative
    a, b = np.full((11, 11), 0.25, dtype=np.float32), np.full((11, 11), 0.75, dtype=np.float32)
    m, mean = vr.ssim64(a, b)
    want = (2 * 0.25 * 0.75 + 1e-4) / (0.25 ** 2 + 0.75 ** 2 + 1e-4)
    assert m.shape == (1, 1, 1) and abs(mean - want) < 1e-4 * want


def test_float32_model_error_scale_and_the_criterion_accepts_it():
    """A float32 variance is a difference of two numbers each carrying about a dozen roundings of 2^-24 relative; after the
    per-tile shift those numbers are at most 0.6^2 (the smooth image's swing inside a tile), so the variance is off by some
    1e-7 absolute, and against denominators of at least C2 = 9e-4 the SSIM by up to some 1e-4.  Without the shift the flat
    0.7 image alone would be off by 2e-4."""
    th, tw = _tiles()
    err = vr.model_error(th, tw)
    print(f"\nfloat32 model vs float64 model: {err:.3e}; tolerance {vr.ssim_tolerance(th, tw):.3e}")
    assert 0.0 < err < 2e-4
    ok, worst = vr.ssim_accepts(lambda a, b: vr.ssim32(a, b, th, tw), th, tw)
    assert ok and worst == err


@pytest.mark.parametrize("name", list(vr.SSIM_MUTATIONS))
def test_criterion_rejects_ssim_mutation(name):
    th, tw = _tiles()
    kw = vr.SSIM_MUTATIONS[name]
    ok, worst = vr.ssim_accepts(lambda a, b: vr.ssim64(a, b, **kw), th, tw)
    tol = vr.ssim_tolerance(th, tw)
    print(f"\n{name}: deviation {worst:.3e}, tolerance {tol:.3e}")
    assert not ok and worst > 10.0 * tol


@pytest.mark.parametrize("kw", [dict(unmasked_residual=True), dict(round_index=True)], ids=["unmasked_residual", "rounded_lut_index"])
def test_criterion_rejects_panel_mutation(kw):
    """The panel's criterion is bit equality with panel32: each mutation must change bytes of some case."""
    lut = _lut()
    changed = [int((vr.panel32(*case[1:], lut, **kw) != vr.panel32(*case[1:], lut)).sum()) for case in vr.panel_cases()]
    assert max(changed) > 0
    if "unmasked_residual" in kw:
        assert all(c > 0 for c in changed)                               # every case has holes with a residual in them


def test_panel_model_layout_and_special_values():
    lut = _lut()
    name, d, c, gd, gc = vr.panel_cases()[0]
    p = vr.panel32(d, c, gd, gc, lut)
    H, W = gd.shape
    assert p.shape == (2 * H, 3 * W, 3) and p.dtype == np.uint8
    assert np.array_equal(p[0, 0], lut[0]) and np.array_equal(p[0, 2 * W], lut[0])           # a hole: depth 0, residual 0
    assert np.array_equal(p[H // 2, W + W // 2], lut[0])                                     # NaN depth -> index 0
    assert np.array_equal(p[H - 1, W], lut[255]) and np.array_equal(p[H - 1, 2 * W - 1], lut[0])   # beyond vmax; negative
    y, x = np.unravel_index(np.argmax(gd), gd.shape)
    assert np.array_equal(p[y, x], lut[255])                                                 # t == 1 -> min(255, 256)
    assert np.array_equal(p[H + 1, 1], [0, 255, 128])                                        # clipped, 0.5 * 255 + 0.5 -> 128
    assert np.array_equal(p[H, 2 * W], [0, 0, 0])                                            # colour residual in a hole
    # vmax == 0: every depth panel divides by 1
    name, d, c, gd, gc = vr.panel_cases()[1]
    p0 = vr.panel32(d, c, gd, gc, lut)
    assert np.array_equal(p0[0, 0], lut[0]) and (p0[:H, 2 * W:] == lut[0]).all() and (p0[H:, 2 * W:] == 0).all()


def test_stats_model():
    name, d, c, gd, gc = vr.panel_cases()[2]
    d = np.nan_to_num(d, nan=1.0)
    n, s_abs, s_sq, mx = vr.stats64(d, c, gd, gc)
    assert n == float((gd > 0).sum()) and mx == float(gd.max())
    assert abs(s_abs - float(np.abs(d.astype(np.float64) - gd)[gd > 0].sum())) < 1e-3 * s_abs
    assert abs(s_sq - float(((c.astype(np.float64) - gc) ** 2).sum())) < 1e-5 * s_sq


class _RaisingRenderer:
    def render_img(self, *a, **k):
        raise AssertionError("the renderer was called with a false gate")


def test_save_imgs_with_a_false_gate_touches_nothing(tmp_path, monkeypatch):
    from myslam_amd import ops
    from myslam_amd.src.utils.Frame_Visualizer import Frame_Visualizer

    def boom(*a, **k):
        raise AssertionError("the GPU path was called with a false gate")
    for fn in ("frame_stats", "vis_panel", "frame_metrics", "ssim"):
        monkeypatch.setattr(ops, fn, boom)
    was_up = torch.cuda.is_initialized()
    vis = Frame_Visualizer(4, 5, str(tmp_path / "vis"), _RaisingRenderer(), 0.06, False, device="cuda:0", fmt="png")
    assert os.path.isdir(tmp_path / "vis")
    gd, gc, pose = torch.ones(4, 4), torch.ones(4, 4, 3), torch.eye(4)
    for idx, it in ((1, 0), (4, 1), (3, 5), (7, 9)):
        assert vis.save_imgs(idx, it, gd, gc, pose, None, None) is None
    assert os.listdir(tmp_path / "vis") == [] and torch.cuda.is_initialized() == was_up
    with pytest.raises(AssertionError, match="renderer"):
        vis.save_imgs(8, 10, gd, gc, pose, None, None)                   # a true gate does reach the renderer
    with pytest.raises(ValueError):
        Frame_Visualizer(1, 1, str(tmp_path / "vis"), None, 0.06, False, fmt="bmp")


def test_on_iter_sees_every_iteration_on_the_oracle_backend():
    """Slam.on_iter: frame 0's single tracking call with the ground-truth pose, then every tracking iteration with its [1,7]
    pose and every mapping iteration with the c2w the mapper was given; unset, the loop's counts are what they were."""
    from myslam_amd import scene as scn, slam, synthscene
    from tests.oracle_backend import OracleBackend
    sc = scn.make_scene("toy")
    cfg = slam.SlamConfig(tracking_pixels=40, tracking_iters=2, ignore_edge_H=10, ignore_edge_W=10, mapping_pixels=60,
                          iters_first=3, iters=2, every_frame=2, keyframe_every=2, mapping_window_size=4)
    frames = synthscene.make_sequence(sc, 3)
    torch.manual_seed(0)
    s = slam.Slam(sc, cfg, device="cpu", backend=OracleBackend(sc))
    assert s.on_iter is None
    calls = []

    def on_iter(stage, idx, it, gt_depth, gt_color, pose):
        assert gt_depth.shape == (sc.H, sc.W) and gt_color.shape == (sc.H, sc.W, 3)
        calls.append((stage, idx, it, tuple(pose.shape)))
    s.on_iter = on_iter
    s.run(frames)
    assert calls == ([("tracking", 0, 0, (4, 4))] + [("mapping", 0, k, (4, 4)) for k in range(3)]
                     + [("tracking", 1, k, (1, 7)) for k in range(2)] + [("tracking", 2, k, (1, 7)) for k in range(2)]
                     + [("mapping", 2, k, (4, 4)) for k in range(2)])
    assert s.stats["tracking_iters"] == 4 and s.stats["mapping_iters"] == 5
    assert callable(s.render_report)


def test_run_takes_render_eval(monkeypatch):
    from myslam_amd import run
    seen = {}

    class Stub:
        def __init__(self, cfg, args):
            seen["cfg"] = cfg

        def run(self):
            pass
    monkeypatch.setattr(run, "ESLAM", Stub)
    monkeypatch.setattr(run.config, "load_config", lambda a, b: {})
    monkeypatch.setattr(run, "default_config_for", lambda p: p)
    run.main(["x.yaml", "--render_eval", "5"])
    assert seen["cfg"]["render_eval"] == {"every": 5}
    run.main(["x.yaml"])
    assert "render_eval" not in seen["cfg"]
