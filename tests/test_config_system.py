"""The config system without a GPU: src/config.load_config on copies of the reference's settings files against the
reference's own merged result (tests/golden/configs_merged.json, written by tests/golden/make_config_golden.py), and the
objects the loop takes built from a config: scene.scene_from_config, slam.SlamConfig.from_config, Mesher."""
import json
import os

import pytest
import torch
import yaml  # noqa: F401  (load_config needs it: without it this suite fails, it does not skip)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LEAVES = {"Replica/room0.yaml": "room0", "ScanNet/scene0000.yaml": "scene0000", "TUM_RGBD/freiburg1_desk.yaml": "freiburg1_desk"}


@pytest.fixture(scope="module")
def merged():
    with open(os.path.join(GOLDEN, "configs_merged.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def configs(tmp_path_factory):
    """The three leaf configs loaded from a working directory that is not the config root."""
    from myslam_amd.src.config import load_config
    cwd = os.getcwd()
    os.chdir(tmp_path_factory.mktemp("elsewhere"))
    try:
        root = os.path.join(GOLDEN, "configs")
        return {leaf: load_config(os.path.join(root, leaf), os.path.join(root, "ESLAM.yaml")) for leaf in LEAVES}
    finally:
        os.chdir(cwd)


@pytest.mark.parametrize("leaf", list(LEAVES))
def test_load_config_equals_the_reference(configs, merged, leaf):
    assert configs[leaf] == merged[leaf]
    assert json.loads(json.dumps(configs[leaf])) == merged[leaf]          # value types included (int stays int)


def test_inherit_from_as_written_wins_and_update_recursive(tmp_path, monkeypatch):
    from myslam_amd.src.config import load_config, update_recursive
    (tmp_path / "configs").mkdir()
    (tmp_path / "configs" / "base.yaml").write_text("a: {x: 1, y: 2}\nb: 3\n")
    (tmp_path / "configs" / "leaf.yaml").write_text("inherit_from: configs/base.yaml\na: {y: 5}\nc: {d: 6}\n")
    (tmp_path / "default.yaml").write_text("b: 0\nz: 9\n")
    monkeypatch.chdir(tmp_path)                       # the reference's way: the path as written, from the working directory
    want = {"a": {"x": 1, "y": 5}, "b": 3, "c": {"d": 6}, "z": 9, "inherit_from": "configs/base.yaml"}
    assert load_config("configs/leaf.yaml", "default.yaml") == want
    monkeypatch.chdir(tmp_path / "configs")           # elsewhere: found against an ancestor of the config file
    assert load_config("leaf.yaml", str(tmp_path / "default.yaml")) == want
    d = {"k": {"n": 1}}
    update_recursive(d, {"k": {"o": 2}, "m": {}})     # the reference's rule: a new key starts as a fresh dict
    assert d == {"k": {"n": 1, "o": 2}, "m": {}}
    with pytest.raises(FileNotFoundError):
        load_config("leaf.yaml", "no_such_default.yaml")


@pytest.mark.parametrize("leaf", list(LEAVES))
def test_scene_from_config_equals_make_scene(configs, leaf):
    from myslam_amd import scene as scn
    a, b = scn.scene_from_config(configs[leaf]), scn.make_scene(LEAVES[leaf])
    for k in ("H", "W", "fx", "fy", "cx", "cy", "n_stratified", "n_importance", "learnable_beta", "truncation", "scale"):
        assert getattr(a, k) == getattr(b, k), k
    assert a.bound.dtype == torch.float32 and torch.equal(a.bound, b.bound)
    assert a.plane_shapes == b.plane_shapes
    assert a.cfg() == b.cfg()


def test_slam_config_from_config(configs):
    from myslam_amd.slam import SlamConfig
    assert SlamConfig.from_config(configs["Replica/room0.yaml"]) == SlamConfig()
    t = SlamConfig.from_config(configs["TUM_RGBD/freiburg1_desk.yaml"])
    assert (t.tracking_pixels, t.tracking_iters, t.iters, t.every_frame, t.keyframe_every) == (5000, 200, 60, 1, 1)
    assert (t.mapping_pixels, t.lr_T, t.lr_R, t.ignore_edge_H, t.ignore_edge_W) == (5000, 0.01, 0.002, 20, 20)
    assert t.tracking_w == (10.0, 200.0, 50.0, 1.0, 5.0) and t.mapping_w == (5.0, 200.0, 10.0, 0.1, 5.0)
    assert not t.mixed_precision
    assert SlamConfig.from_config(dict(configs["Replica/room0.yaml"], mixed_precision=True)).mixed_precision


def test_mesher_class_carries_what_the_functions_read(configs):
    from types import SimpleNamespace
    from myslam_amd import scene as scn
    from myslam_amd.src.utils import Mesher as M
    cfg = configs["TUM_RGBD/freiburg1_desk.yaml"]
    sc = scn.scene_from_config(cfg)
    m = M.Mesher(cfg, SimpleNamespace(), sc)
    assert (m.points_batch_size, m.ray_batch_size, m.scale, m.resolution, m.level_set, m.mesh_bound_scale) == \
        (500000, 100000, 1, 0.01, 0, 1.02)
    assert m.bound is sc.bound and (m.H, m.W, m.fx, m.cy) == (sc.H, sc.W, sc.fx, sc.cy)
    assert m.marching_cubes_bound.dtype == torch.float64 and m.marching_cubes_bound.tolist() == cfg["mapping"]["marching_cubes_bound"]
    for name in ("eval_points", "get_bound_from_frames", "get_bound_from_frames_tsdf", "get_mesh", "extract_mesh"):
        assert getattr(M.Mesher, name) is getattr(M, name)          # the free functions stay, the class binds them
    assert [len(a) for a in M.grid_axes(m.marching_cubes_bound, 0.1)] == [38, 31, 31]


def test_cull_mesh_load_config_unchanged(configs):
    from myslam_amd.src.tools import cull_mesh
    root = os.path.join(GOLDEN, "configs")
    assert cull_mesh.load_config(os.path.join(root, "ESLAM.yaml"), "no_such_file.yaml")["cam"]["H"] == 680
