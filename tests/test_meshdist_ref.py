"""No GPU: the float32 model of the point-to-mesh distance (tests/meshdist_ref.py, what the kernel must reproduce bit for
bit) against a float64 truth reached by another route, hand cases for the seven regions, degenerate and sliver faces, the
mutants the comparison must reject, the pure metric functions of eval_recon, and the header's declarations.

The bars: the worst |float32 model - float64 truth| over the seeded soup is 4.95e-8 in the unit cube and 8.02e-6 moved by
+100 on every axis (coordinates of magnitude 100 carry 7.6e-6 of float32 spacing); each case is pinned at 4 x its figure."""
import os
import re

import numpy as np
import pytest
import torch

from tests import meshdist_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOUP_SEED = 7
MEASURED = {0.0: 4.95e-8, 100.0: 8.02e-6}          # worst |model - truth| on soup(300, 1000, SOUP_SEED, shift)
BAR = {k: 4.0 * v for k, v in MEASURED.items()}


@pytest.fixture(scope="module", params=[0.0, 100.0])
def soup_case(request):
    shift = request.param
    v, f, q = mr.soup(300, 1000, SOUP_SEED, shift=shift)
    return shift, v, f, q, mr.truth_f64(v, f, q)


def test_model_against_truth_on_soup(soup_case):
    shift, v, f, q, truth = soup_case
    d, face, near = mr.model_query(v, f, q)
    err = np.abs(d.astype(np.float64) - truth).max()
    print(f"shift {shift}: worst |float32 model - float64 truth| = {err:.3e} (bar {BAR[shift]:.3e})")
    assert err <= BAR[shift]
    assert err >= 0.25 * MEASURED[shift], "the figure in the docstring and DESIGN.md no longer describes the model"
    # the returned face is one whose own float64 distance is the minimum, to the bar; the closest point lies on it
    tri = v[f[face]].astype(np.float64)
    own = mr.pair_truth_f64(tri[:, 0], tri[:, 1], tri[:, 2], q.astype(np.float64))
    assert np.abs(own - truth).max() <= BAR[shift]
    on = mr.pair_truth_f64(tri[:, 0], tri[:, 1], tri[:, 2], near.astype(np.float64))
    assert on.max() <= BAR[shift]
    # every region decides some pair of the soup
    region = mr.closest_f32(v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None], q[:, None, :])[1]
    assert (np.bincount(region.ravel(), minlength=7) > 0).all()
    assert (np.bincount(region[np.arange(len(q)), face], minlength=7) > 0).all()


# the triangle (0,0,0) (2,0,0) (0,2,0): one query per region, closest point in closed form
HAND = [
    ("vertex A", (-1.0, -1.0, 0.5), (0.0, 0.0, 0.0), 0),
    ("vertex B", (3.0, -0.5, 0.5), (2.0, 0.0, 0.0), 1),
    ("edge AB", (1.0, -1.0, 0.5), (1.0, 0.0, 0.0), 2),
    ("vertex C", (-0.5, 3.0, 0.5), (0.0, 2.0, 0.0), 3),
    ("edge AC", (-1.0, 1.0, 0.5), (0.0, 1.0, 0.0), 4),
    ("edge BC", (2.0, 2.0, 0.5), (1.0, 1.0, 0.0), 5),
    ("interior", (0.5, 0.75, 0.5), (0.5, 0.75, 0.0), 6),
]


@pytest.mark.parametrize("name,q,expect,region", HAND, ids=[h[0] for h in HAND])
def test_hand_cases(name, q, expect, region):
    a, b, c = np.float32([0, 0, 0]), np.float32([2, 0, 0]), np.float32([0, 2, 0])
    p, r = mr.closest_f32(a, b, c, np.float32(q))
    assert int(r) == region
    assert np.array_equal(p, np.float32(expect))
    d = np.sqrt(mr.pair_d2_f32(np.float32(q), p))
    assert abs(float(d) - np.linalg.norm(np.float64(q) - np.float64(expect))) <= BAR[0.0]
    assert abs(float(mr.pair_truth_f64(a, b, c, q)) - np.linalg.norm(np.float64(q) - np.float64(expect))) <= 1e-15


def degenerate_faces():
    """(name, a, b, c) float32: zero-area faces, and slivers of aspect 1 : 10^4 short enough that the face and its edge
    segments are the same set to well below the bar (length 1e-3, width 1e-7)."""
    f = np.float32
    return [
        ("A = B", f([0.2, 0.3, 0.4]), f([0.2, 0.3, 0.4]), f([0.7, 0.5, 0.6])),
        ("A = C", f([0.2, 0.3, 0.4]), f([0.7, 0.5, 0.6]), f([0.2, 0.3, 0.4])),
        ("B = C", f([0.2, 0.3, 0.4]), f([0.7, 0.5, 0.6]), f([0.7, 0.5, 0.6])),
        ("A = B = C", f([0.5, 0.5, 0.5]), f([0.5, 0.5, 0.5]), f([0.5, 0.5, 0.5])),
        ("collinear, C between", f([0.0, 0.0, 0.0]), f([1.0, 1.0, 1.0]), f([0.5, 0.5, 0.5])),
        ("collinear, C beyond", f([0.25, 0.5, 0.75]), f([0.5, 0.5, 0.5]), f([1.0, 0.5, 0.0])),
        ("sliver along x", f([0.5, 0.5, 0.5]), f([0.501, 0.5, 0.5]), f([0.5005, 0.5000001, 0.5])),
        ("sliver, long edge last", f([0.5, 0.5, 0.5]), f([0.5005, 0.5, 0.5000001]), f([0.501, 0.5, 0.5])),
    ]


def degenerate_queries():
    rng = np.random.default_rng(3)
    return rng.uniform(0.0, 1.0, (400, 3)).astype(np.float32)


@pytest.mark.parametrize("case", degenerate_faces(), ids=[c[0] for c in degenerate_faces()])
def test_degenerate_and_sliver_faces(case):
    _, a, b, c = case
    q = degenerate_queries()
    p, region = mr.closest_f32(a, b, c, q)
    d = np.sqrt(mr.pair_d2_f32(q, p))
    assert np.isfinite(p).all() and np.isfinite(d).all()
    seg = mr.segments_f64(a, b, c, q)
    assert np.abs(d.astype(np.float64) - seg).max() <= BAR[0.0]
    assert np.abs(mr.pair_truth_f64(a, b, c, q) - seg).max() <= 1e-6          # (the truth agrees that they are thin)


def test_overflow_is_never_selected():
    """Coordinates whose dot products overflow float32 give no NaN in the result: such a pair is never the minimum."""
    v = np.float32([[1e30, 0, 0], [0, 1e30, 0], [0, 0, 1e30], [0, 0, 0], [1, 0, 0], [0, 1, 0]])
    f = np.int32([[0, 1, 2], [3, 4, 5]])
    d, face, near = mr.model_query(v, f, np.float32([[0.25, 0.25, 1.0], [1e30, 1e30, 1e30]]))
    assert not np.isnan(d).any() and face[0] == 1 and d[0] == 1.0


# ---------------------------------------------------------------------------------------------------------
# mutants: each must be told apart from the truth by the comparison above
# ---------------------------------------------------------------------------------------------------------
def _vertices_only(a, b, c, q):
    cands = np.stack(np.broadcast_arrays(a + 0 * q, b + 0 * q, c + 0 * q))
    d2 = ((q[None] - cands) ** 2).sum(-1)
    return np.take_along_axis(cands, d2.argmin(0)[None, ..., None], 0)[0].astype(np.float32)


def _unclamped_plane(a, b, c, q):
    n = np.cross(b - a, c - a)
    h = ((q - a) * n).sum(-1, keepdims=True) / np.maximum((n * n).sum(-1, keepdims=True), 1e-30)
    return (q - n * h).astype(np.float32)


def _no_edges(a, b, c, q):
    return mr.closest_f32(a, b, c, q, drop_edges=True)[0]


@pytest.mark.parametrize("pair", [_vertices_only, _unclamped_plane, _no_edges], ids=["vertices", "plane", "no_edges"])
def test_mutants_are_rejected(soup_case, pair):
    shift, v, f, q, truth = soup_case
    with np.errstate(all="ignore"):
        d = mr.model_query(v, f, q, pair=pair)[0]
    err = np.abs(d.astype(np.float64) - truth)
    assert np.nanmax(err) > 100 * BAR[shift] or np.isnan(err).any()


def test_tie_mutant_is_rejected():
    """Two faces mirrored in the plane x = 0.5 and a query on it: equal d2 bit for bit, the smaller index wins; the mutant
    that keeps the larger index differs in `face`."""
    v = np.float32([[0.25, 0, 0], [0.25, 1, 0], [0.25, 0, 1], [0.75, 0, 0], [0.75, 1, 0], [0.75, 0, 1]])
    f = np.int32([[3, 4, 5], [0, 1, 2]])
    q = np.float32([[0.5, 0.25, 0.25]])
    d, face, _ = mr.model_query(v, f, q)
    assert face[0] == 0 and d[0] == np.float32(0.25)
    assert mr.model_query(v, f, q, ties="larger")[1][0] == 1


def test_max_dist_and_non_finite_rows():
    v, f, q = mr.soup(50, 200, 5)
    d, face, near = mr.model_query(v, f, q)
    cut = float(np.median(d))
    d2, face2, near2 = mr.model_query(v, f, q, max_dist=cut)
    far = d >= np.float32(cut)
    assert far.any() and (~far).any()
    assert np.isinf(d2[far]).all() and (face2[far] == -1).all() and np.isnan(near2[far]).all()
    assert np.array_equal(d2[~far], d[~far]) and np.array_equal(face2[~far], face[~far])
    v[f[0, 1], 2] = np.nan
    q[0, 0] = np.inf
    d3, face3, _ = mr.model_query(v, f, q)
    assert np.isinf(d3[0]) and face3[0] == -1 and not (face3 == 0).any() and not np.isnan(d3).any()


def test_icosphere():
    for s, n in ((2, 320), (3, 1280)):
        v, f = mr.icosphere(s, radius=1.5)
        assert f.shape == (n, 3) and v.shape == (n // 2 + 2, 3)
        assert np.allclose(np.linalg.norm(v, axis=1), 1.5, atol=1e-12)
        nrm = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        assert ((nrm * v[f].mean(1)).sum(1) > 0).all()                 # outward, every face
        assert abs(0.5 * np.linalg.norm(nrm, axis=1).sum() / (4 * np.pi * 1.5 ** 2) - 1.0) < 0.02


# ---------------------------------------------------------------------------------------------------------
# the pure metric functions (any device: here the CPU)
# ---------------------------------------------------------------------------------------------------------
def test_f_score():
    from myslam_amd.src.tools import eval_recon as er
    th = 0.05
    below = float(np.nextafter(np.float32(th), np.float32(0)))
    a = torch.tensor([below, th, 0.2, 0.0])                             # exactly at the threshold does not count
    b = torch.tensor([0.01, 0.3])
    p, r, f = er.f_score(a, b, th)
    assert (p, r) == (0.5, 0.5) and f == 0.5
    assert er.f_score(a, torch.zeros(0), th) == (0.5, 0.0, 0.0)         # an empty side
    assert er.f_score(torch.tensor([1.0]), torch.tensor([2.0]), th) == (0.0, 0.0, 0.0)      # f = 0, no division
    p, r, f = er.f_score(np.float32([0.0, 0.0, 1.0, 1.0]), np.float32([0.0]), th)
    assert (p, r) == (0.5, 1.0) and abs(f - 2 * 0.5 / 1.5) < 1e-15


def test_normal_consistency_and_face_normals():
    from myslam_amd.src.tools import eval_recon as er
    a = torch.tensor([[0.0, 0, 2], [0, 0, 1], [1, 0, 0], [0, 0, 0], [0, 1, 0]])
    b = torch.tensor([[0.0, 0, -3], [0, 1, 0], [1, 1, 0], [0, 0, 1], [0, 0, 0]])
    nc, used = er.normal_consistency(a, b)
    assert used == 3 and abs(nc - (1.0 + 0.0 + 2 ** -0.5) / 3) < 1e-15
    nc, used = er.normal_consistency(torch.zeros(4, 3), torch.ones(4, 3))
    assert used == 0 and nc != nc
    v = torch.tensor([[0.0, 0, 0], [2, 0, 0], [0, 3, 0], [1, 0, 0]])
    n = er.face_normals(v, torch.tensor([[0, 1, 2], [0, 2, 1], [0, 3, 1], [1, 1, 1]]))
    assert n.dtype == torch.float64
    assert torch.equal(n, torch.tensor([[0.0, 0, 1], [0, 0, -1], [0, 0, 0], [0, 0, 0]], dtype=torch.float64))


def test_error_colour_rule():
    from myslam_amd import ops
    from myslam_amd.src.tools import eval_recon as er
    lut = ops.load_plasma_lut()
    e = 0.05
    d = torch.tensor([0.0, e, 2 * e, float("inf"), e * 127.4 / 255, e * 127.6 / 255], dtype=torch.float32)
    c = er.error_colors(d, e).numpy()
    assert c.dtype == np.uint8
    assert np.array_equal(c, lut[[0, 255, 255, 255, 127, 128]])
    ramp = torch.linspace(0, 2 * e, 1001, dtype=torch.float32)
    idx = np.floor(np.minimum(ramp.numpy().astype(np.float64) / e, 1.0) * 255 + 0.5).astype(np.int64)
    assert np.array_equal(er.error_colors(ramp, e).numpy(), lut[idx])


def test_header_declares_the_entries():
    from myslam_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "eslam_hip.h")).read()
    for name in ("eslam_tri_grid_plan", "eslam_tri_count", "eslam_tri_workspace_bytes", "eslam_tri_build",
                 "eslam_tri_query_workspace_bytes", "eslam_tri_query"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _hip.SIGNATURES
    assert int(re.search(r"#define ESLAM_ABI_VERSION (\d+)", hdr).group(1)) == _hip.ABI_VERSION == 5
    assert int(re.search(r"#define ESLAM_PROF_KERNELS (\d+)", hdr).group(1)) == _hip.PROF_KERNELS == 13
    assert int(re.search(r"#define ESLAM_TRI_INPUT_ORDER (\d+)", hdr).group(1)) == _hip.TRI_INPUT_ORDER
    assert int(re.search(r"#define ESLAM_TRI_CELL_PER_EXTENT (\d+)", hdr).group(1)) == _hip.TRI_CELL_PER_EXTENT
    lib = _hip.load_library()
    g = _hip.TriGrid()
    import ctypes
    assert ctypes.sizeof(g) == 40
    box = (ctypes.c_float * 6)(0, 7, 0, 5, 0, 3)
    assert lib.eslam_tri_grid_plan(1000, box, 0.5, ctypes.byref(g)) == 0 and tuple(g.dims) == (7, 5, 3) and g.entries == 0
    g.entries = 2 ** 31
    assert lib.eslam_tri_workspace_bytes(ctypes.byref(g)) == -1
    assert b"2147483648" in lib.eslam_last_error()
