"""CPU-side checks of mesh culling and the reconstruction metrics: the PLY reader, face / vertex compaction, the rigid
solve from ICP moments, surface sampling and the nearest-neighbour grid rule (no GPU needed)."""
import ctypes

import numpy as np
import pytest
import torch


# ----------------------------------------------------------------------------------------------
# PLY
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_colour", [True, False])
def test_ply_round_trip(tmp_path, with_colour):
    from myslam_amd.src.utils.Mesher import read_ply, write_ply
    rng = np.random.default_rng(1)
    v = rng.normal(size=(31, 3)).astype(np.float32)
    f = rng.integers(0, 31, size=(20, 3)).astype(np.int32)
    c = rng.uniform(0, 1, size=(31, 3)).astype(np.float32) if with_colour else None
    p = tmp_path / "a.ply"
    write_ply(str(p), v, f, c)
    v2, f2, c2 = read_ply(str(p))
    assert v2.dtype == np.float32 and np.array_equal(v2, v)
    assert np.array_equal(f2, f)
    if with_colour:
        assert np.array_equal(np.round(c2 * 255), np.round(c * 255))
        q = tmp_path / "b.ply"
        write_ply(str(q), v2, f2, c2)                      # and back: the same bytes
        assert q.read_bytes() == p.read_bytes()
    else:
        assert c2 is None


def test_ply_ascii_quad_and_extra_properties(tmp_path):
    from myslam_amd.src.utils.Mesher import read_ply
    text = "\n".join([
        "ply", "format ascii 1.0", "comment made by hand", "element vertex 5",
        "property double x", "property double y", "property double z",
        "property float nx", "property float ny", "property float nz", "property uchar red", "property uchar green",
        "property uchar blue", "property int label",
        "element face 2", "property list uchar uint vertex_indices", "property uchar flags",
        "element edge 1", "property int vertex1", "property int vertex2",
        "end_header",
        "0 0 0 0 0 1 255 0 0 7", "1 0 0 0 0 1 0 255 0 7", "1 1 0 0 0 1 0 0 255 7", "0 1 0 0 0 1 10 20 30 7",
        "0.5 0.5 1.25 0 0 1 0 0 0 3",
        "4 0 1 2 3 9", "3 0 1 4 9",
        "0 1", ""])
    p = tmp_path / "q.ply"
    p.write_text(text)
    v, f, c = read_ply(str(p))
    assert v.shape == (5, 3) and v.dtype == np.float32
    assert np.allclose(v[4], [0.5, 0.5, 1.25])
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4]]           # the quad fanned from its first vertex
    assert np.allclose(c[3] * 255, [10, 20, 30])


def test_ply_binary_mixed_polygons_and_types(tmp_path):
    from myslam_amd.src.utils.Mesher import read_ply
    head = "\n".join(["ply", "format binary_big_endian 1.0", "element vertex 4", "property float x", "property float y",
                      "property float z", "property short extra", "element face 2",
                      "property list int ushort vertex_index", "end_header", ""]).encode()
    verts = np.array([(0, 0, 0, 1), (1, 0, 0, 2), (1, 1, 0, 3), (0, 1, 0, 4)],
                     dtype=[("x", ">f4"), ("y", ">f4"), ("z", ">f4"), ("e", ">i2")])
    body = verts.tobytes() + np.array([4, 0, 1, 2, 3], ">i4")[:1].tobytes() + np.array([0, 1, 2, 3], ">u2").tobytes()
    body += np.array([3], ">i4").tobytes() + np.array([3, 2, 1], ">u2").tobytes()
    p = tmp_path / "b.ply"
    p.write_bytes(head + body)
    v, f, c = read_ply(str(p))
    assert np.array_equal(v, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]) and c is None
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [3, 2, 1]]


# ----------------------------------------------------------------------------------------------
# culling: compaction
# ----------------------------------------------------------------------------------------------
def test_compact_keeps_order():
    from myslam_amd.src.tools.cull_mesh import compact, culled_path
    v = np.arange(8 * 3, dtype=np.float32).reshape(8, 3)
    c = np.arange(8 * 3, dtype=np.float32).reshape(8, 3) / 100
    f = np.array([[0, 1, 2], [2, 3, 4], [5, 6, 7], [7, 6, 1], [3, 3, 5]])
    seen = np.array([0, 0, 0, 0, 1, 0, 0, 1], dtype=bool)
    v2, f2, c2 = compact(v, f, c, seen)
    # faces kept: [2,3,4] (4 seen), [5,6,7] (7 seen), [7,6,1] (7 seen); vertex 0 is no longer referenced
    assert np.array_equal(v2, v[[1, 2, 3, 4, 5, 6, 7]]) and np.array_equal(c2, c[[1, 2, 3, 4, 5, 6, 7]])
    assert f2.tolist() == [[1, 2, 3], [4, 5, 6], [6, 5, 0]]
    v3, f3, c3 = compact(v, f, None, np.zeros(8, dtype=bool))
    assert v3.shape == (0, 3) and f3.shape == (0, 3) and c3 is None
    assert culled_path("out/mesh/00010_mesh.ply") == "out/mesh/00010_mesh_culled.ply"
    assert culled_path("a.b/final.mesh.ply") == "a.b/final.mesh_culled.ply"


# ----------------------------------------------------------------------------------------------
# ICP: the rigid solve from moments
# ----------------------------------------------------------------------------------------------
def _moments(s, t):
    d = np.linalg.norm(s - t, axis=1)
    return np.concatenate([[len(s), (d * d).sum()], s.sum(0), t.sum(0), (s[:, :, None] * t[:, None, :]).sum(0).reshape(-1)])


def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    th = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


@pytest.mark.parametrize("planar", [False, True])
def test_umeyama_from_moments(planar):
    from myslam_amd.src.tools.eval_recon import umeyama_from_moments
    rng = np.random.default_rng(3)
    s = rng.normal(size=(500, 3)) + [2.0, -1.0, 0.5]
    if planar:                         # coplanar points: H has a zero singular value, the plain SVD may reflect
        s[:, 2] = 0.5
    R = _rot([0.3, -0.5, 0.8], 37.0)
    t = np.array([0.4, -0.2, 1.1])
    T = umeyama_from_moments(_moments(s, s @ R.T + t))
    assert abs(np.linalg.det(T[:3, :3]) - 1) < 1e-9
    assert np.abs(T[:3, :3] - R).max() < 1e-9 and np.abs(T[:3, 3] - t).max() < 1e-9
    # an exact mirror image: the best proper rotation, never a reflection
    M = np.diag([1.0, 1.0, -1.0])
    T2 = umeyama_from_moments(_moments(s, s @ M.T))
    assert abs(np.linalg.det(T2[:3, :3]) - 1) < 1e-9
    assert np.array_equal(umeyama_from_moments(np.zeros(17)), np.eye(4))


# ----------------------------------------------------------------------------------------------
# surface sampling
# ----------------------------------------------------------------------------------------------
def test_sample_surface_on_faces_and_by_area():
    from myslam_amd import ops
    rng = np.random.default_rng(5)
    v = torch.from_numpy(rng.normal(size=(40, 3)).astype(np.float32))
    f = torch.from_numpy(rng.choice(40, size=(25, 3), replace=True))
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    n = 200000
    pts, fi = ops.sample_surface(v, f, n, seed=11)
    assert pts.shape == (n, 3) and pts.dtype == torch.float64 and fi.shape == (n,)
    vd = v.double()
    v0, v1, v2 = vd[f[fi, 0]], vd[f[fi, 1]], vd[f[fi, 2]]
    # on the picked face: barycentric coordinates in [0, 1] that reproduce the point
    e1, e2, r = v1 - v0, v2 - v0, pts - v0
    G = torch.stack([torch.stack([(e1 * e1).sum(1), (e1 * e2).sum(1)], 1), torch.stack([(e1 * e2).sum(1), (e2 * e2).sum(1)], 1)], 1)
    b = torch.linalg.solve(G, torch.stack([(r * e1).sum(1), (r * e2).sum(1)], 1))
    assert float((v0 + b[:, :1] * e1 + b[:, 1:] * e2 - pts).abs().max()) < 1e-9
    assert float(b.min()) > -1e-9 and float(b.sum(1).max()) < 1 + 1e-9
    # face counts follow area: chi-squared against the expected counts (p = 1e-4 bound for F - 1 degrees of freedom)
    area = 0.5 * torch.linalg.cross(vd[f[:, 1]] - vd[f[:, 0]], vd[f[:, 2]] - vd[f[:, 0]]).norm(dim=1)
    expect = (area / area.sum() * n).numpy()
    count = np.bincount(fi.numpy(), minlength=f.shape[0])
    chi2 = float(((count - expect) ** 2 / expect).sum())
    dof = f.shape[0] - 1
    assert chi2 < dof + 4.0 * np.sqrt(2 * dof) + 10, (chi2, dof)
    # deterministic for a seed, different across seeds
    assert torch.equal(ops.sample_surface(v, f, n, seed=11)[0], pts)
    assert not torch.equal(ops.sample_surface(v, f, n, seed=12)[0], pts)


# ----------------------------------------------------------------------------------------------
# the nearest-neighbour grid rule (eslam_nn_grid_plan: host code)
# ----------------------------------------------------------------------------------------------
def _plan(n, bbox):
    from myslam_amd import _hip
    g = _hip.NnGrid()
    rc = _hip.lib().eslam_nn_grid_plan(n, (ctypes.c_float * 6)(*bbox), ctypes.byref(g))
    return rc, g


def test_nn_grid_rule():
    from myslam_amd import _hip
    lib = _hip.lib()
    rc, g = _plan(1, [1.5, 1.5, -2, -2, 3, 3])              # one point (or all points equal): one cell
    assert rc == 0 and list(g.dims) == [1, 1, 1] and g.cell == 1.0 and list(g.lo) == [1.5, -2, 3]
    rc, g = _plan(10000, [0, 4, 0, 2, 1, 1])                 # a flat cloud: one cell across the flat axis
    assert rc == 0 and g.dims[2] == 1
    h = np.sqrt(8.0 / (2 * 10000))                           # h = (P / (2 N))^(1/m), m = 2
    assert abs(g.cell - h) <= 1e-6 * h
    assert g.dims[0] == int(np.ceil(4 / np.float64(g.cell))) and g.dims[1] == int(np.ceil(2 / np.float64(g.cell)))
    rc, g = _plan(5000, [0, 1e-8, 0, 1, 0, 1e-9])            # a line: flat axes are at most 1e-6 of the longest
    assert rc == 0 and g.dims[0] == 1 and g.dims[2] == 1 and g.dims[1] == 10000
    rc, g = _plan(450000, [-1, 5, -2, 3, 0, 3])              # a volume: about 2 cells per point, every extent covered
    cells = g.dims[0] * g.dims[1] * g.dims[2]
    assert rc == 0 and 900000 <= cells <= 900000 * 1.1
    for d, ext in enumerate((6, 5, 3)):
        assert g.dims[d] * np.float64(g.cell) >= ext
    rc, g = _plan(2 ** 31 - 1, [0, 1, 0, 1, 0, 1])           # the cell count is bounded: workspace too
    assert rc == 0 and g.dims[0] * g.dims[1] * g.dims[2] <= _hip.NN_MAX_CELLS
    ws = lib.eslam_nn_workspace_bytes(ctypes.byref(g), 1000)
    assert 0 < ws <= 4 * (_hip.NN_MAX_CELLS + 1) + 4 * (_hip.NN_MAX_CELLS // 4096 + 1) + 1000 * 24 + 5 * 256
    assert _plan(0, [0] * 6)[0] != 0 and _plan(5, [0, -1, 0, 0, 0, 0])[0] != 0
    assert _plan(5, [0, float("nan"), 0, 0, 0, 0])[0] != 0
