"""The mesh clean-up on the GPU (eslam_meshclean.hip through ops.weld_vertices / mesh_components / component_face_counts,
src/tools/clean_mesh.py and its hooks) against the numpy model of tests/meshclean_ref.py: every comparison is bit for bit,
and every kernel call runs twice with equal results."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from myslam_amd import ops
from myslam_amd.src.tools import clean_mesh as cm
from myslam_amd.src.tools import cull_mesh as cu
from myslam_amd.src.utils.Mesher import read_ply, write_ply
from tests import meshclean_ref as mr
from tests.test_meshclean_ref import same_mesh

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def twice(fn, *args):
    """fn's int32 result as numpy, after checking that a second call gives the same bits."""
    a, b = fn(*args), fn(*args)
    assert a.dtype == torch.int32 and a.device == DEV and torch.equal(a, b)
    return a.cpu().numpy()


def gpu_weld(v):
    return twice(ops.weld_vertices, torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).to(DEV))


def gpu_components(f, n):
    return twice(ops.mesh_components, torch.as_tensor(np.asarray(f)).to(DEV), n)


def gpu_counts(f, lab):
    return twice(ops.component_face_counts, torch.as_tensor(np.asarray(f)).to(DEV), torch.as_tensor(lab).to(DEV))


def equal_i32(got, want):
    assert got.dtype == np.int32 and want.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} entries differ"


# ---------------------------------------------------------------------------------------------------------------------
# weld
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 65])
def test_weld_small_sizes(n):
    rng = np.random.default_rng(n)
    v = rng.integers(0, 3, (n, 3)).astype(np.float32)                # 27 positions: duplicates across the wave boundary
    equal_i32(gpu_weld(v), mr.weld(v))


def test_weld_restores_the_soup_of_a_grid():
    rng = np.random.default_rng(1)
    v, f = mr.grid_mesh(64)
    sv, sf = mr.soup(v, f, rng)
    rep = gpu_weld(sv)
    equal_i32(rep, mr.weld(sv))
    assert len(np.unique(rep)) == len(v) == 65 * 65 and np.array_equal(sv[rep[sf]], v[f])


def test_weld_one_position_4096_times():
    v = np.tile(np.array([[0.3, -1.7, 2.5]], dtype=np.float32), (4096, 1))
    equal_i32(gpu_weld(v), np.zeros(4096, dtype=np.int32))


def test_weld_distinct_positions():
    rng = np.random.default_rng(2)
    v = np.unique(rng.random((50_400, 3), dtype=np.float32), axis=0)[:50_000]
    v = v[rng.permutation(len(v))]
    assert len(v) == 50_000
    equal_i32(gpu_weld(v), np.arange(50_000, dtype=np.int32))


def test_weld_special_values():
    rng = np.random.default_rng(4)
    one, tiny = np.float32(1.0), np.float32(1e-40)
    vals = np.array([0.0, -0.0, one, np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0)), tiny, -tiny,
                     np.nextafter(tiny, one), np.float32(1.1754944e-38), np.nan, np.inf, -np.inf, -one, 3.0e38],
                    dtype=np.float32)
    v = vals[rng.integers(0, len(vals), (3000, 3))]
    v[::7] = rng.random((len(v[::7]), 3), dtype=np.float32)           # ordinary rows in between
    want = mr.weld(v)
    assert (want < 0).sum() > 500 and (want[want >= 0] != np.nonzero(want >= 0)[0]).sum() > 200
    equal_i32(gpu_weld(v), want)


# ---------------------------------------------------------------------------------------------------------------------
# components
# ---------------------------------------------------------------------------------------------------------------------
def test_components_without_faces():
    equal_i32(gpu_components(np.zeros((0, 3), dtype=np.int64), 70), np.arange(70, dtype=np.int32))
    equal_i32(gpu_components(np.zeros((0, 3), dtype=np.int64), 0), np.zeros(0, dtype=np.int32))


def test_components_permuted_strip():
    rng = np.random.default_rng(6)
    f, perm = mr.permuted(mr.strip(100_000), 100_002, rng)
    got = gpu_components(f, 100_002)
    equal_i32(got, mr.components(f, 100_002))
    assert (got == 0).all()


def test_components_blobs_and_loose_vertices():
    rng = np.random.default_rng(7)
    f, n, sizes = mr.blobs(rng)
    got = gpu_components(f, n)
    want = mr.components(f, n)
    equal_i32(got, want)
    assert len(np.unique(got)) == 37 + 50
    counts = gpu_counts(f, got)
    equal_i32(counts, mr.face_counts(f, want))
    assert sorted(counts[counts > 0].tolist()) == sorted(sizes.tolist())


def test_components_fans_touching_at_one_vertex():
    hub = 40
    a = np.stack([np.full(19, hub), np.arange(0, 19), np.arange(1, 20)], axis=1)          # around the hub: 0 .. 19
    b = np.stack([np.full(19, hub), np.arange(20, 39), np.arange(21, 40)], axis=1)        # and 20 .. 39
    f = np.concatenate([a, b, [[41, 42, 43]]])
    got = gpu_components(f, 45)
    equal_i32(got, mr.components(f, 45))
    assert got.tolist() == [0] * 41 + [41, 41, 41, 44]


def test_components_repeated_indices_and_the_last_vertex():
    f = np.array([[7, 7, 3], [3, 9, 9], [5, 5, 5], [1, 8, 6], [99, 99, 99], [98, 2, 98]])
    got = gpu_components(f, 100)
    equal_i32(got, mr.components(f, 100))
    assert got[[7, 9, 5, 8, 99, 98]].tolist() == [3, 3, 5, 1, 99, 2]
    f = np.array([[0, 1, 64], [64, 65, 129]])                                              # V - 1 in another wave
    equal_i32(gpu_components(f, 130), mr.components(f, 130))


@pytest.mark.parametrize("bad", [4, -1])
def test_an_index_out_of_range_raises(bad):
    f = torch.tensor([[0, 1, 2], [1, bad, 3]], device=DEV)
    with pytest.raises(ValueError):
        ops.mesh_components(f, 4)
    with pytest.raises(ValueError):
        ops.component_face_counts(f, torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        cm.clean_mesh_arrays(np.zeros((4, 3), np.float32), f.cpu().numpy(), None)


# ---------------------------------------------------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------------------------------------------------
def test_counts_one_large_component_among_floaters():
    big = mr.strip(60_000)
    small = 60_002 + 3 * np.arange(500)[:, None] + np.arange(3)[None, :]
    n = 60_002 + 1500
    f = np.empty((60_500, 3), dtype=np.int64)
    at = np.arange(500) * 121 + 17                                     # a floater every 121 faces: waves hold mixed labels
    mask = np.zeros(60_500, dtype=bool)
    mask[at] = True
    f[mask], f[~mask] = small, big
    lab = gpu_components(f, n)
    equal_i32(lab, mr.components(f, n))
    got = gpu_counts(f, lab)
    equal_i32(got, np.bincount(lab[f[:, 0]], minlength=n).astype(np.int32))
    assert got[0] == 60_000 and (got[60_002::3] == 1).all() and got.sum() == 60_500


def test_counts_all_faces_in_one_component():
    f = mr.strip(10_001)
    lab = np.zeros(10_003, dtype=np.int32)
    got = gpu_counts(f, lab)
    assert got[0] == 10_001 and got.sum() == 10_001
    equal_i32(got, mr.face_counts(f, lab))


def test_counts_every_face_its_own_component():
    f = 3 * np.arange(5_003)[:, None] + np.arange(3)[None, :]
    lab = gpu_components(f, 3 * 5_003)
    got = gpu_counts(f, lab)
    equal_i32(got, mr.face_counts(f, lab))
    assert (got[::3] == 1).all() and got.sum() == 5_003
    equal_i32(gpu_counts(np.zeros((0, 3), dtype=np.int64), lab), np.zeros(3 * 5_003, dtype=np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
BIG = ((18.3, 18.6, 18.9), 14.0)
SMALL = [((39.0, 39.0, 38.7), 3.5), ((39.0, 8.5, 8.2), 3.0), ((8.4, 38.8, 8.6), 4.0), ((8.5, 8.3, 39.0), 3.2),
         ((39.0, 38.7, 8.4), 3.7)]


@pytest.fixture(scope="module")
def spheres():
    """(vertices, faces int64, colours) of the level set of six spheres on a 48^3 grid (voxel 1, origin 0): one of radius
    14 and five of radius 3 to 4, all at least 4 voxels from each other and from the border."""
    g = torch.arange(48, dtype=torch.float32, device=DEV)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    sdf = None
    for (cx, cy, cz), r in [BIG] + SMALL:
        d = torch.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r
        sdf = d if sdf is None else torch.minimum(sdf, d)
    v, f = ops.marching_cubes(sdf.contiguous(), 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    v, f = v.cpu().numpy(), f.cpu().numpy().astype(np.int64)
    col = np.random.default_rng(9).random((len(v), 3)).astype(np.float32)
    return v, f, col


def _on_big(v):
    return np.abs(np.linalg.norm(v.astype(np.float64) - np.array(BIG[0]), axis=1) - BIG[1]) <= 1.0


def test_the_model_finds_six_components(spheres):
    v, f, _ = spheres
    fc = mr.face_counts(f, mr.components(f, len(v)))
    assert (fc > 0).sum() == 6 and np.array_equal(mr.weld(v), np.arange(len(v)))
    assert fc.max() > 10 * np.sort(fc)[-2]


@pytest.mark.parametrize("kw", [dict(min_faces=1000), dict(keep_largest=True), dict(min_fraction=0.5), dict()])
def test_clean_mesh_arrays_equals_the_model(spheres, kw):
    v, f, col = spheres
    out = cm.clean_mesh_arrays(v, f, col, **kw)
    again = cm.clean_mesh_arrays(v, f, col, **kw)
    want = mr.clean(v, f, col, **kw)
    same_mesh(out, want)
    same_mesh(out, again)
    assert out[3]["components"] == 6 and out[3]["components_kept"] == (1 if kw else 6)
    assert len(out[1]) > 0 and out[1].max() == len(out[0]) - 1
    if kw:
        assert _on_big(out[0]).all() and len(out[0]) == int(_on_big(v).sum())


def test_clean_mesh_arrays_on_the_soup(spheres):
    v, f, col = spheres
    sv, sf = mr.soup(v, f, np.random.default_rng(10))
    sc = np.random.default_rng(12).random((len(sv), 3)).astype(np.float32)
    out = cm.clean_mesh_arrays(sv, sf, sc, min_faces=1000)
    same_mesh(out, mr.clean(sv, sf, sc, min_faces=1000))
    assert out[3]["vertices_merged"] == len(sv) - len(v) and out[3]["components"] == 6 and _on_big(out[0]).all()
    soup_only = cm.clean_mesh_arrays(sv, sf, sc, merge_vertices=False, min_faces=2)
    assert soup_only[3]["components"] == len(sf) and len(soup_only[1]) == 0          # a soup: a component per triangle


def _frames():
    """One camera at (24, 24, 80) looking along -z, 100 x 100 pixels and a narrow lens: it sees a part of most spheres."""
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([24.0, 24.0, 80.0])
    return [(0, None, torch.zeros(100, 100), c2w)], dict(H=100, W=100, fx=250.0, fy=250.0, cx=50.0, cy=50.0)


def test_cull_mesh_arrays_with_and_without_the_merge(spheres):
    v, f, col = spheres
    sv, sf = mr.soup(v, f, np.random.default_rng(13))
    sc = np.random.default_rng(14).random((len(sv), 3)).astype(np.float32)
    frames, cam = _frames()
    seen = ops.cull_vertices(torch.as_tensor(sv).to(DEV), ((fr[2], fr[3]) for fr in frames),
                             (cam["fx"], cam["fy"], cam["cx"], cam["cy"]), cam["H"], cam["W"], 0.06, False).cpu().numpy()
    assert 0 < seen.sum() < len(seen)
    today = cu.compact(sv, sf, sc, seen)
    args = (cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], 0.06, False)
    same_mesh(cu.cull_mesh_arrays(sv, sf, sc, frames, *args), today)
    merged = cu.cull_mesh_arrays(sv, sf, sc, frames, *args, merge_vertices=True)
    assert len(merged) == 3
    same_mesh(merged, mr.clean(*today)[:3])
    assert len(merged[0]) < len(today[0]) and len(merged[1]) == len(today[1])


def test_cli_writes_the_clean_mesh(spheres, tmp_path):
    v, f, col = spheres
    path = tmp_path / "some.mesh.ply"
    write_ply(path, v, f, col)
    r = subprocess.run([sys.executable, "-m", "myslam_amd.src.tools.clean_mesh", "--input_mesh", str(path), "--min_faces", "1000"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "'components': 6" in r.stdout and "'components_kept': 1" in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["some.mesh.ply", "some.mesh_clean.ply"]
    want = mr.clean(*read_ply(path), min_faces=1000)
    write_ply(tmp_path / "want.ply", *want[:3])
    same_mesh(read_ply(tmp_path / "some.mesh_clean.ply"), read_ply(tmp_path / "want.ply"))


def test_eslam_writes_the_clean_mesh_when_asked(tmp_path):
    from myslam_amd.src.ESLAM import ESLAM
    from tests.test_gpu_frames import _toy_cfg, _write_toy_sequence
    n_frames, min_faces = 5, 300
    _write_toy_sequence(tmp_path / "seq", n_frames)
    files = {}
    for name, key in (("with", True), ("without", False)):
        cfg = _toy_cfg(tmp_path / "seq", tmp_path / name)
        if key:
            cfg["meshing"]["clean_min_faces"] = min_faces
        ESLAM(cfg, SimpleNamespace(input_folder=None, output=None)).run()
        files[name] = sorted(os.listdir(tmp_path / name / "mesh"))
    assert files["without"] == ["final_mesh.ply", "final_mesh_culled.ply"]
    assert files["with"] == ["final_mesh.ply", "final_mesh_culled.ply", "final_mesh_culled_clean.ply"]
    culled = read_ply(tmp_path / "with" / "mesh" / "final_mesh_culled.ply")
    clean = read_ply(tmp_path / "with" / "mesh" / "final_mesh_culled_clean.ply")
    assert 0 < len(clean[1]) <= len(culled[1])
    fc = mr.face_counts(clean[1], mr.components(clean[1], len(clean[0])))
    assert (fc[fc > 0] >= min_faces).all()
    want = mr.clean(*culled, min_faces=min_faces)
    write_ply(tmp_path / "want.ply", *want[:3])
    same_mesh(clean, read_ply(tmp_path / "want.ply"))
