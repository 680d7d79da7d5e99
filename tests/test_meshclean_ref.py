"""The mesh clean-up without a GPU: the numpy model (tests/meshclean_ref.py) pinned on hand-built cases and against scipy,
the host pipeline of src/tools/clean_mesh.py driven by the model, the hooks' defaults, and the new ABI symbols."""
import inspect

import numpy as np
import pytest
import torch

from myslam_amd import _hip
from myslam_amd.src.tools import clean_mesh as cm
from myslam_amd.src.tools import cull_mesh as cu
from tests import meshclean_ref as mr


def _t(fn):
    """A model function as clean_tensors wants it: tensors in, tensor out."""
    return lambda *a: torch.as_tensor(fn(*[x.numpy() if torch.is_tensor(x) else x for x in a]))


def host_clean(vertices, faces, colors, **kw):
    """clean_mesh_arrays with the three graph steps taken from the model instead of the GPU."""
    v = torch.as_tensor(np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3))
    f = torch.as_tensor(np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3))
    used, f, info = cm.clean_tensors(v, f, _t(mr.weld), _t(mr.components), _t(mr.face_counts), **kw)
    used = used.numpy()
    return np.asarray(vertices)[used], f.numpy(), None if colors is None else np.asarray(colors)[used], info


def same_mesh(a, b):
    assert a[0].dtype == b[0].dtype and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert a[1].dtype == b[1].dtype and np.array_equal(a[1], b[1])
    assert (a[2] is None) == (b[2] is None) and (a[2] is None or np.array_equal(a[2], b[2]))
    if len(a) > 3:
        assert a[3] == b[3]


# ---------------------------------------------------------------------------------------------------------------------
# the model on hand-built cases
# ---------------------------------------------------------------------------------------------------------------------
def test_components_two_triangles_sharing_one_vertex_are_one():
    f = np.array([[0, 1, 2], [2, 3, 4], [6, 7, 8]])
    assert mr.components(f, 10).tolist() == [0, 0, 0, 0, 0, 5, 6, 6, 6, 9]          # 5 and 9 are loose
    assert mr.face_counts(f, mr.components(f, 10)).tolist() == [2, 0, 0, 0, 0, 0, 1, 0, 0, 0]


def test_components_label_is_the_smallest_index_and_repeats_are_legal():
    f = np.array([[7, 7, 3], [3, 9, 9], [5, 5, 5], [1, 8, 6]])
    assert mr.components(f, 10).tolist() == [0, 1, 2, 3, 4, 5, 1, 3, 1, 3]
    assert mr.components(np.zeros((0, 3), dtype=np.int64), 3).tolist() == [0, 1, 2]


def test_weld_equality_rules():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    tiny = np.float32(1e-40)                                                        # a denormal
    v = np.array([[0.0, 1.0, 2.0], [-0.0, 1.0, 2.0], [one, one, one], [one, one, up], [np.nan, 0, 0], [0, np.inf, 0],
                  [0, 0, -np.inf], [tiny, 0, 0], [tiny, -0.0, 0], [-tiny, 0, 0], [one, one, one], [0.0, 1.0, 2.0]],
                 dtype=np.float32)
    assert tiny > 0 and tiny < np.finfo(np.float32).tiny
    assert mr.weld(v).tolist() == [0, 0, 2, 3, -1, -1, -1, 7, 7, 9, 2, 0]
    assert mr.weld(np.zeros((0, 3), dtype=np.float32)).tolist() == []


def test_weld_restores_a_shuffled_soup():
    rng = np.random.default_rng(3)
    v, f = mr.grid_mesh(12)
    sv, sf = mr.soup(v, f, rng)
    rep = mr.weld(sv)
    assert len(np.unique(rep)) == len(v)
    assert np.array_equal(sv[rep], sv) and np.all(rep <= np.arange(len(sv)))
    assert np.array_equal(sv[rep[sf]], v[f])


def test_model_against_scipy():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(5)
    cases = [mr.blobs(rng)[:2], (mr.permuted(mr.strip(100_000), 100_002, rng)[0], 100_002)]
    for f, n in cases:
        rounds = []
        lab = mr.components(f, n, rounds)
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]]])
        g = sparse.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
        n_comp, ids = csgraph.connected_components(g, directed=False)
        assert len(np.unique(lab)) == n_comp
        first = np.full(n_comp, n, dtype=np.int64)
        np.minimum.at(first, ids, np.arange(n))
        assert np.array_equal(lab, first[ids])
        assert rounds[0] < 64


# ---------------------------------------------------------------------------------------------------------------------
# the host pipeline
# ---------------------------------------------------------------------------------------------------------------------
def _pieces():
    """Three pieces of 4, 2 and 4 faces over 20 vertices (10 .. 13 unused)."""
    f = np.concatenate([mr.strip(4, 0), mr.strip(2, 6), mr.strip(4, 14)])
    v = (np.arange(60, dtype=np.float32).reshape(20, 3) * 0.5) - 7.0
    c = np.arange(60, dtype=np.float32).reshape(20, 3) / 64.0
    return v, f, c


def test_pipeline_keeps_order_and_drops_unreferenced():
    v, f, c = _pieces()
    out = host_clean(v, f, c)
    keep = np.r_[0:10, 14:20]
    assert np.array_equal(out[0], v[keep]) and np.array_equal(out[2], c[keep])
    assert np.array_equal(out[1], np.concatenate([mr.strip(4, 0), mr.strip(2, 6), mr.strip(4, 10)]))
    assert out[3] == dict(vertices_merged=0, nonfinite_vertices=0, components=3, components_kept=3, face_counts=[4, 4, 2])
    same_mesh(out, mr.clean(v, f, c))


def test_pipeline_colours_follow_representatives():
    v, f, c = _pieces()
    v2, c2 = np.concatenate([v, v[::-1]]), np.concatenate([c, c[::-1] + 1.0])      # vertex 39 - k is a copy of k
    f2 = f.copy()
    f2[::2] = 39 - f2[::2]                                                          # every other face uses the copies
    out = host_clean(v2, f2, c2)
    ref = host_clean(v, f, c)
    same_mesh(out[:3], ref[:3])                                                     # the first of each pair stays, with its colour
    assert out[3]["vertices_merged"] == 20 and out[3]["components"] == 3
    same_mesh(out, mr.clean(v2, f2, c2))
    unmerged = host_clean(v2, f2, c2, merge_vertices=False)
    assert unmerged[3]["components"] == 6 and unmerged[3]["vertices_merged"] == 0
    same_mesh(unmerged, mr.clean(v2, f2, c2, merge_vertices=False))


def test_pipeline_nonfinite_vertices_take_their_faces():
    v, f, c = _pieces()
    v = v.copy()
    v[7, 1] = np.nan
    v[19, 0] = np.inf
    out = host_clean(v, f, c)
    assert out[3]["nonfinite_vertices"] == 2 and out[3]["face_counts"] == [4, 3]
    assert np.isfinite(out[0]).all()
    same_mesh(out, mr.clean(v, f, c))


@pytest.mark.parametrize("kw, kept", [
    (dict(min_faces=2), [4, 2, 4]), (dict(min_faces=3), [4, 4]), (dict(min_faces=5), []),
    (dict(min_fraction=0.5), [4, 2, 4]), (dict(min_fraction=0.51), [4, 4]), (dict(min_fraction=1.0), [4, 4]),
    (dict(keep_largest=True), [4]), (dict(keep_largest=True, min_faces=5), []),
])
def test_pipeline_filters(kw, kept):
    v, f, c = _pieces()
    out = host_clean(v, f, c, **kw)
    assert len(out[1]) == sum(kept) and out[3]["components_kept"] == len(kept)
    if kw.get("keep_largest") and kept:
        assert np.array_equal(out[0], v[:6])                                        # the tie goes to the smaller label
    same_mesh(out, mr.clean(v, f, c, **kw))


def test_pipeline_drop_degenerate():
    v, f, c = _pieces()
    v = v.copy()
    v[1] = v[0]                                                                     # face (0, 1, 2) collapses to (0, 0, 2)
    kept = host_clean(v, f, c)
    assert kept[3]["face_counts"] == [4, 4, 2] and (kept[1][0, 0] == kept[1][0, 1])
    out = host_clean(v, f, c, drop_degenerate=True)
    assert out[3]["face_counts"] == [4, 3, 2] and len(out[1]) == 9
    same_mesh(out, mr.clean(v, f, c, drop_degenerate=True))
    same_mesh(kept, mr.clean(v, f, c))
    rep = np.array([[3, 3, 4], [0, 1, 2]])
    assert cm.weld_faces(torch.as_tensor(rep), None, True).tolist() == [[0, 1, 2]]  # without the merge too


def test_pipeline_on_an_empty_mesh():
    out = host_clean(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), None)
    assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[3]["components"] == 0
    out = host_clean(np.ones((4, 3), np.float32), np.zeros((0, 3), np.int64), None, keep_largest=True)
    assert out[0].shape == (0, 3) and out[3]["face_counts"] == []


# ---------------------------------------------------------------------------------------------------------------------
# hooks and ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_compact_then_merge_equals_the_model():
    rng = np.random.default_rng(11)
    v, f = mr.grid_mesh(10)
    sv, sf = mr.soup(v, f, rng)
    col = rng.random((len(sv), 3)).astype(np.float32)
    seen = sv[:, 0] < 0.7
    culled = cu.compact(sv, sf, col, seen)
    out = host_clean(*culled)
    same_mesh(out, mr.clean(*culled))
    assert out[3]["components"] == 1 and len(out[1]) == len(culled[1])
    assert len(out[0]) == len(np.unique(culled[0], axis=0))


def test_hook_defaults_leave_the_old_calls_alone():
    p = list(inspect.signature(cu.cull_mesh_arrays).parameters.values())
    assert [q.name for q in p] == ["vertices", "faces", "colors", "frames", "H", "W", "fx", "fy", "cx", "cy", "truncation",
                                   "eval_rec", "device", "chunk", "merge_vertices"]
    assert p[-1].default is False and p[-2].default == 32 and p[-3].default == "cuda:0"
    p = list(inspect.signature(cu.cull_mesh).parameters.values())
    assert [q.name for q in p] == ["mesh_file", "cfg", "args", "device", "estimate_c2w_list", "merge_vertices"]
    assert p[-1].default is False and p[-2].default is None
    d = inspect.signature(cm.clean_mesh_arrays).parameters
    assert [d[k].default for k in ("merge_vertices", "min_faces", "min_fraction", "keep_largest", "drop_degenerate", "device")] \
        == [True, 0, 0.0, False, False, "cuda:0"]
    assert cm.clean_path("a/b.c/final_mesh_culled.ply") == "a/b.c/final_mesh_culled_clean.ply"


def test_new_symbols_have_prototypes():
    for name in ("eslam_mesh_weld_workspace_bytes", "eslam_mesh_weld", "eslam_mesh_components", "eslam_mesh_component_sizes"):
        assert name in _hip.SIGNATURES
    assert _hip.ABI_VERSION == 5
    lib = _hip.load_library()
    assert lib.eslam_mesh_weld_workspace_bytes(65) == 4 * 256
    assert lib.eslam_mesh_weld_workspace_bytes(_hip.MESH_MAX_COUNT + 1) == -1
    assert lib.eslam_mesh_components(None, -1, 4, None, None) != 0 and b"faces" in lib.eslam_last_error()


def test_ops_refuse_cpu_tensors():
    from myslam_amd import ops
    with pytest.raises(RuntimeError):
        ops.weld_vertices(torch.zeros(4, 3))
    with pytest.raises(RuntimeError):
        ops.mesh_components(torch.zeros(2, 3, dtype=torch.int64), 4)
    with pytest.raises(RuntimeError):
        ops.component_face_counts(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(4, dtype=torch.int32))
