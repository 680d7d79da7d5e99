"""Host-side parts of mesh extraction: the marching-cubes tables, the grid axes, the PLY writer, the frame hull's
half-spaces and the workspace query.  No GPU needed."""
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

from tests import mesh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", os.path.join(ROOT, "tools", "gen_mc_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _corner(k):
    return np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1])


def _edge_ends(e):
    (dx, dy, dz), axis = mesh_ref.edge_owner(e)
    lo = np.array([dx, dy, dz])
    hi = lo.copy()
    hi[axis] = 1
    return lo, hi


def _crossing_edges(case):
    out = set()
    for e in range(12):
        lo, hi = _edge_ends(e)
        kl, kh = int(lo @ [1, 2, 4]), int(hi @ [1, 2, 4])
        if ((case >> kl) & 1) != ((case >> kh) & 1):
            out.add(e)
    return out


def _case_tris(case):
    ntri, tri, _ = mesh_ref.load_tables()
    return [tuple(int(e) for e in tri[case, 3 * t:3 * t + 3]) for t in range(ntri[case])]


def _boundary(tris):
    """Directed edges of the triangle set whose reverse is not in it (the polygon outlines on the cube's faces)."""
    de = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
    s = set(de)
    return [(a, b) for a, b in de if (b, a) not in s]


def test_generator_reproduces_committed_header():
    gen = _gen()
    with open(gen.HEADER) as f:
        assert f.read() == gen.render_header()


def test_tables_use_exactly_the_crossing_edges():
    ntri, tri, max_tris = mesh_ref.load_tables()
    assert ntri[0] == 0 and ntri[255] == 0
    for case in range(256):
        used = {e for t in _case_tris(case) for e in t}
        assert used == _crossing_edges(case), case
        assert (tri[case, 3 * ntri[case]:] == -1).all()


def test_case_polygons_are_closed():
    for case in range(1, 255):
        b = _boundary(_case_tris(case))
        outs = {}
        ins = {}
        for a, c in b:
            outs[a] = outs.get(a, 0) + 1
            ins[c] = ins.get(c, 0) + 1
        assert outs == ins, case                       # every outline vertex is entered and left once: closed loops
        assert set(outs) == _crossing_edges(case), case
        for a, c in b:                                 # every outline segment lies on one face of the cube
            pa = sum(_edge_ends(a)) / 2.0
            pc = sum(_edge_ends(c)) / 2.0
            assert any(pa[ax] == pc[ax] and pa[ax] in (0.0, 1.0) for ax in range(3)), (case, a, c)


def _face_segments(case, axis, side):
    """Outline segments of the case on face (axis, side), as pairs of edge-midpoint coordinates."""
    out = set()
    for a, c in _boundary(_case_tris(case)):
        pa = sum(_edge_ends(a)) / 2.0
        pc = sum(_edge_ends(c)) / 2.0
        if pa[axis] == side and pc[axis] == side:
            out.add((tuple(pa), tuple(pc)))
    return out


def test_neighbouring_cubes_emit_matching_face_segments():
    for case in range(256):
        for axis in range(3):
            # the neighbour across face (axis, 1): its corners with coordinate 0 on `axis` are ours with 1
            shared = [k for k in range(8) if _corner(k)[axis] == 1]
            mine = _face_segments(case, axis, 1)
            for free in range(16):
                nb = 0
                for k in shared:
                    if (case >> k) & 1:
                        nb |= 1 << (k - (1 << axis))
                free_corners = [k for k in range(8) if _corner(k)[axis] == 1]
                for bit, k in enumerate(free_corners):
                    if (free >> bit) & 1:
                        nb |= 1 << k
                theirs = _face_segments(nb, axis, 0)
                shifted = set()
                for pa, pc in theirs:
                    qa, qc = list(pa), list(pc)
                    qa[axis] += 1.0
                    qc[axis] += 1.0
                    shifted.add((tuple(qc), tuple(qa)))     # reversed: the shared face seen from the other side
                assert shifted == mine, (case, axis, free)


def _ref_nsteps(lo, hi, res):
    return int(round((hi - lo + 0.1) / res))


@pytest.mark.parametrize("bound,expect", [
    ([[-1.9, 7.9], [-2.2, 4.5], [-2.5, 2.3]], [990, 680, 490]),          # room0
    ([[-4.5, 4.9], [-5.7, 4.4], [-3.7, 4.3]], [950, 1020, 810]),         # office0
    ([[-2.6, 1.1], [-1.5, 1.5], [-0.6, 2.4]], [380, 310, 310]),          # freiburg1_desk
])
def test_grid_axes_match_reference_formula(bound, expect):
    from myslam_amd.src.utils.Mesher import grid_axes
    b = np.array(bound) * 1.0
    axes = grid_axes(torch.from_numpy(b), 0.01)
    assert [len(a) for a in axes] == expect
    for k in range(3):
        assert _ref_nsteps(b[k][0], b[k][1], 0.01) == expect[k]
        assert np.array_equal(axes[k], np.linspace(b[k][0] - 0.05, b[k][1] + 0.05, expect[k]))


def _read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    nf = int([h for h in head if h.startswith("element face")][0].split()[-1])
    vt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("a", "u1")])
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    v = np.frombuffer(data, dtype=vt, count=nv, offset=end)
    f = np.frombuffer(data, dtype=ft, count=nf, offset=end + nv * vt.itemsize)
    assert end + nv * vt.itemsize + nf * ft.itemsize == len(data)
    return head, v, f


def test_ply_round_trip(tmp_path):
    from myslam_amd.src.utils.Mesher import write_ply
    rng = np.random.default_rng(0)
    verts = rng.normal(size=(17, 3)).astype(np.float32)
    faces = rng.integers(0, 17, size=(9, 3)).astype(np.int32)
    cols = rng.uniform(-0.1, 1.1, size=(17, 3)).astype(np.float32)
    p = tmp_path / "m.ply"
    write_ply(str(p), verts, faces, cols)
    head, v, f = _read_ply(p)
    assert head == ["ply", "format binary_little_endian 1.0", "element vertex 17", "property float x", "property float y",
                    "property float z", "property uchar red", "property uchar green", "property uchar blue",
                    "property uchar alpha", "element face 9", "property list uchar int vertex_indices", "end_header"]
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), verts)
    assert np.array_equal(np.stack([v["r"], v["g"], v["b"]], 1), np.clip(np.round(255.0 * cols.astype(np.float64)), 0, 255))
    assert (v["a"] == 255).all()
    assert (f["n"] == 3).all() and np.array_equal(f["v"], faces)


def _excess(points, hs):
    """max over the hull's vertices... of the polytope's excess: largest distance of a polytope vertex to the exact hull,
    measured along the exact hull's facet normals, as a share of the bounding-box diagonal."""
    spatial = pytest.importorskip("scipy.spatial")
    p = points.double().numpy()
    hull = spatial.ConvexHull(p)
    # polytope vertices: intersect the half-spaces (an interior point: the mean of the points)
    hsi = spatial.HalfspaceIntersection(hs.numpy(), p.mean(0))
    poly = hsi.intersections
    eq = hull.equations                                    # n.x + d <= 0 inside, unit n
    dist = (poly @ eq[:, :3].T + eq[:, 3]).max(axis=1)     # > 0 outside the exact hull (a lower bound of the distance)
    diag = np.linalg.norm(p.max(0) - p.min(0))
    return float(max(dist.max(), 0.0) / diag)


def _contains_all(points, hs):
    p = points.double()
    return bool(((p @ hs[:, :3].T + hs[:, 3]) <= 0).all())


def test_halfspaces_box_cloud_is_exact():
    from myslam_amd.src.utils.Mesher import halfspaces_from_points
    g = torch.Generator().manual_seed(1)
    pts = torch.rand(20000, 3, generator=g, dtype=torch.float64) * torch.tensor([3.0, 2.0, 1.5]) - 1.0
    corners = torch.tensor(list(itertools.product((0.0, 1.0), repeat=3)), dtype=torch.float64) * torch.tensor([3.0, 2.0, 1.5]) - 1.0
    pts = torch.cat([pts, corners]).float()
    hs = halfspaces_from_points(pts, 1.0)
    assert hs.shape == (1024, 4)
    assert _contains_all(pts, hs)
    ex = _excess(pts, hs)
    print(f"\nbox cloud: excess {ex:.2e} of the diagonal")
    assert ex <= 1e-6


def test_halfspaces_rotated_ellipsoid_cloud():
    from myslam_amd.src.utils.Mesher import halfspaces_from_points
    g = torch.Generator().manual_seed(2)
    u = torch.randn(30000, 3, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=1, keepdim=True)
    a, b = 0.7, 0.4
    R = torch.tensor([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=torch.float64) @ \
        torch.tensor([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]], dtype=torch.float64)
    pts = ((u * torch.tensor([2.0, 1.2, 0.6], dtype=torch.float64)) @ R.T + torch.tensor([0.3, -0.2, 1.0])).float()
    hs = halfspaces_from_points(pts, 1.0)
    assert _contains_all(pts, hs)
    ex = _excess(pts, hs)
    print(f"\nrotated ellipsoid: excess {ex:.2e} of the diagonal")
    assert ex <= 5e-3


def _synthetic_keyframe_points():
    from myslam_amd import scene as scn, synthscene
    from oracle import eslam_oracle as orc
    sc = scn.make_scene("toy")
    frames = synthscene.make_sequence(sc, 13)
    pts = []
    cams = []
    for idx, color, depth, c2w in frames[::4]:
        ro, rd = orc.rays_full_image(sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy, c2w)
        d = depth.reshape(-1)
        ok = d > 0
        pts.append(ro.reshape(-1, 3)[ok] + rd.reshape(-1, 3)[ok] * d[ok, None])
        cams.append(c2w[:3, 3][None])
    return torch.cat(pts + cams).float()


def test_halfspaces_synthetic_keyframes_and_scale():
    from myslam_amd.src.utils.Mesher import halfspaces_from_points, support_directions
    pts = _synthetic_keyframe_points()
    hs = halfspaces_from_points(pts, 1.0)
    assert _contains_all(pts, hs)
    ex = _excess(pts, hs)
    print(f"\nsynthetic keyframe points: excess {ex:.2e} of the diagonal")
    assert ex <= 2e-2
    # mesh_bound_scale grows it as h' = s h + (1 - s) d.c, c the mean of the distinct support points
    hs2 = halfspaces_from_points(pts, 1.02)
    assert _contains_all(pts, hs2)
    d = support_directions()
    arg = (pts.double() @ d.T).argmax(dim=0)
    c = pts.double()[torch.unique(arg)].mean(0)
    h = -hs[:, 3]
    assert torch.allclose(-hs2[:, 3], 1.02 * h - 0.02 * (d @ c), rtol=0, atol=1e-12)
    assert torch.equal(hs2[:, :3], d)
    assert (-hs2[:, 3] >= h).all()


def test_mc_workspace_query():
    from myslam_amd import _hip
    lib = _hip.load_library()
    N = 1400 ** 3
    align = lambda b: (b + 255) // 256 * 256
    expect = align(16 * ((N + 4095) // 4096)) + align(4 * N) + 2 * align(N)
    got = lib.eslam_mc_workspace_bytes(1400, 1400, 1400)
    assert got == expect and got > 2 ** 31
    assert lib.eslam_mc_workspace_bytes(0, 5, 5) == -1
