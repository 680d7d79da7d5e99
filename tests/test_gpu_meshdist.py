"""ops.MeshDistance (csrc/eslam_meshdist.hip) against the float32 numpy model of tests/meshdist_ref.py - bit for bit in
`dist`, exact in `face`, every row - and the metrics, error maps and command line built on it (eval_recon).  The shapes
are the smallest at which the kernel can still go wrong: a wave boundary, several cells and rings, faces in many cells,
queries outside the grid, degenerate faces."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import meshdist_ref as mr
from tests.test_meshdist_ref import BAR, degenerate_faces, degenerate_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _build(v, f, dev):
    from myslam_amd import ops
    return ops.MeshDistance(torch.as_tensor(v, dtype=torch.float32).to(dev), torch.as_tensor(f).to(dev))


def _query(md, q, **kw):
    out = md.query(torch.as_tensor(q, dtype=torch.float32).to(md.device), closest=True, **kw)
    return tuple(t.cpu().numpy() for t in out)


def _check(md, v, f, q, max_dist=None, **kw):
    """Every row: dist's bits and face equal the model's; q - closest, squared and summed in the header's order, gives
    dist's bits; rows without a face are (inf, -1, NaN).  Returns the kernel's (dist, face, closest)."""
    d, face, near = _query(md, q, max_dist=max_dist, **kw)
    rd, rface, rnear = mr.model_query(v, f, q, max_dist=max_dist)
    assert d.dtype == np.float32 and face.dtype == np.int32 and near.shape == (len(d), 3)
    assert np.array_equal(face, rface), f"{int((face != rface).sum())} of {len(face)} faces differ"
    assert np.array_equal(_bits(d), _bits(rd)), f"{int((_bits(d) != _bits(rd)).sum())} of {len(d)} distances differ"
    hit = face >= 0
    q = np.asarray(q, dtype=np.float32).reshape(-1, 3)
    assert np.array_equal(_bits(np.sqrt(mr.pair_d2_f32(q[hit], near[hit]))), _bits(d[hit]))
    assert np.array_equal(near[hit], rnear[hit])
    assert np.isinf(d[~hit]).all() and np.isnan(near[~hit]).all() and not np.isnan(d).any()
    return d, face, near


ONE_FACE = (np.float32([[0.1, 0.2, 0.3], [0.9, 0.1, 0.4], [0.3, 0.8, 0.7]]), np.int32([[0, 1, 2]]))


@pytest.mark.parametrize("nq", [0, 1, 64, 65, 257])
def test_sizes_against_one_face(dev, nq):
    v, f = ONE_FACE
    md = _build(v, f, dev)
    assert md.entries == 1 and md.dims == (1, 1, 1)
    q = np.random.default_rng(nq).uniform(-0.5, 1.5, (nq, 3)).astype(np.float32)
    d, face, near = _check(md, v, f, q)
    assert d.shape == (nq,) and (face == 0).all()
    d2, face2 = md.query(torch.from_numpy(q).to(dev))
    assert d2.shape == (nq,) and face2.shape == (nq,) and np.array_equal(_bits(d2.cpu().numpy()), _bits(d))


def test_no_faces(dev):
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    for verts in (v, np.zeros((0, 3), np.float32)):
        md = _build(verts, np.zeros((0, 3), np.int32), dev)
        assert md.entries == 0
        d, face, near = _query(md, np.float32([[0.1, 0.2, 0.3], [5, 5, 5]]))
        assert np.isinf(d).all() and (face == -1).all() and np.isnan(near).all()
        d, face, near = _query(md, np.zeros((0, 3), np.float32))
        assert d.shape == (0,) and face.shape == (0,) and near.shape == (0, 3)


@pytest.mark.parametrize("shift", [0.0, 100.0])
def test_seeded_soup(dev, shift):
    v, f, q = mr.soup(500, 2000, 11, size=0.03, shift=shift)
    md = _build(v, f, dev)
    assert int(np.prod(md.dims)) >= 500 and md.entries > 500, (md.dims, md.entries)     # many cells, faces in several
    first = _check(md, v, f, q)
    again = _check(md, v, f, q)
    unsorted = _check(md, v, f, q, sort=False)
    for a, b, c in zip(first, again, unsorted):
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)
    # large faces, few cells: the other end of the plan
    v, f, q = mr.soup(500, 2000, 12, size=0.15, shift=shift)
    _check(_build(v, f, dev), v, f, q)


def _far_face_scene():
    """200 small faces 0.65 .. 0.8 from (0.3, 0.3, 0.6) along the four upward diagonals, and LAST one face in the plane
    z = 0 that spans the box: for queries near that centre the big face is the nearest (0.6 below, about 9 cells), while
    the small faces, farther away, lie in nearer rings of cells (a diagonal's Chebyshev distance is 1 / sqrt(3) of it)."""
    rng = np.random.default_rng(21)
    centre = np.float64([0.3, 0.3, 0.6])
    u = np.float64([[1, 1, 1], [1, -1, 1], [-1, 1, 1], [-1, -1, 1]])[rng.integers(0, 4, 200)] + 0.1 * rng.normal(size=(200, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    c = centre + u * rng.uniform(0.65, 0.8, (200, 1))
    small = (c[:, None, :] + rng.uniform(-0.01, 0.01, (200, 3, 3))).reshape(-1, 3)
    big = np.float64([[-1.0, -1.0, 0.0], [3.0, -1.0, 0.0], [-1.0, 3.0, 0.0]])
    v = np.concatenate([small, big]).astype(np.float32)
    f = np.arange(603, dtype=np.int32).reshape(-1, 3)
    return v, f, centre


def test_early_termination_far_face(dev):
    v, f, centre = _far_face_scene()
    md = _build(v, f, dev)
    rng = np.random.default_rng(22)
    q = (centre + rng.uniform(-0.02, 0.02, (64, 3))).astype(np.float32)
    d, face, near = _check(md, v, f, q)
    assert (face == 200).all()
    # the scene does what it is for: some small face sits in a nearer ring than the big face's closest point
    cell = md.grid.cell
    lo = np.float64(list(md.grid.lo))
    ring = lambda p: np.abs(np.floor((p - lo) / cell) - np.floor((q[0].astype(np.float64) - lo) / cell)).max(axis=-1)
    assert ring(v[:600].reshape(200, 3, 3).astype(np.float64)).max(axis=1).min() + 1 < ring(near[0].astype(np.float64))
    # a face shared by many cells, the query in each of them: points just above the big face, all over it
    assert md.entries > 1000
    g = np.stack(np.meshgrid(np.linspace(-0.9, 1.9, 23), np.linspace(-0.9, 1.9, 23), [1e-3, 0.0]), -1).reshape(-1, 3)
    g = g[g[:, 0] + g[:, 1] < 1.9].astype(np.float32)
    d, face, near = _check(md, v, f, g)
    assert (face == 200).all() and np.abs(d - g[:, 2]).max() < 1e-6
    _check(md, v, f, rng.uniform(-1.0, 3.0, (500, 3)).astype(np.float32))


def test_queries_outside_the_box(dev):
    v, f, _ = mr.soup(300, 1, 31, size=0.03)
    md = _build(v, f, dev)
    rng = np.random.default_rng(32)
    qs = []
    for off in (0.05, 0.5, 5.0, 100.0):
        for axis in range(3):
            for sign in (-1.0, 1.0):
                p = rng.uniform(0.0, 1.0, (6, 3))
                p[:, axis] = (1.0 + off) if sign > 0 else -off
                qs.append(p)
        corner = rng.integers(0, 2, (8, 3)) * (1.0 + 2 * off) - off      # beyond a corner, on all three axes
        qs.append(corner)
    _check(md, v, f, np.concatenate(qs).astype(np.float32))


def test_equidistant_faces_give_the_smaller_index(dev):
    left = [[0.25, 0, 0], [0.25, 1, 0], [0.25, 0, 1]]
    right = [[0.75, 0, 0], [0.75, 1, 0], [0.75, 0, 1]]
    q = np.float32([[0.5, 0.25, 0.25], [0.5, 0.1, 0.6], [0.5, 0.5, 0.25]])
    for v in (np.float32(left + right), np.float32(right + left)):
        f = np.int32([[0, 1, 2], [3, 4, 5]])
        d, face, near = _check(_build(v, f, dev), v, f, q)
        assert (face == 0).all() and np.abs(d - 0.25).max() < 1e-6
    # the same face twice: the copy with the smaller index
    v = np.float32(left)
    f = np.int32([[0, 1, 2], [0, 1, 2], [0, 1, 2]])
    assert (_check(_build(v, f, dev), v, f, q)[1] == 0).all()


def test_degenerate_sliver_and_nan_faces(dev):
    q = degenerate_queries()
    cases = degenerate_faces()
    for name, a, b, c in cases:
        v, f = np.stack([a, b, c]), np.int32([[0, 1, 2]])
        d, face, near = _check(_build(v, f, dev), v, f, q)
        assert np.isfinite(d).all() and (face == 0).all(), name
        assert np.abs(d.astype(np.float64) - mr.segments_f64(a, b, c, q)).max() <= BAR[0.0], name
    # all of them in one mesh, among ordinary faces, with a face that has a NaN vertex FIRST: it is never returned
    sv, sf, _ = mr.soup(100, 1, 41, size=0.05)
    dv = np.concatenate([np.stack([a, b, c]) for _, a, b, c in cases])
    nanface = np.float32([[0.4, 0.4, 0.4], [0.6, np.nan, 0.4], [0.4, 0.6, 0.6]])
    v = np.concatenate([nanface, dv, sv])
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    md = _build(v, f, dev)
    assert md.faces_entered == len(f) - 1
    d, face, near = _check(md, v, f, q)
    assert (face > 0).all() and np.isfinite(d).all()
    bad = np.float32([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [0.5, 0.5, 0.5]])
    d, face, near = _check(md, v, f, bad)
    assert np.isinf(d[:3]).all() and (face[:3] == -1).all() and face[3] > 0
    # nothing but non-finite faces: as no faces
    md = _build(nanface, np.int32([[0, 1, 2]]), dev)
    assert md.entries == 0 and (_query(md, q[:5])[1] == -1).all()


def test_marching_cubes_sphere(dev):
    from myslam_amd import ops
    n = 24
    ax = torch.arange(n, dtype=torch.float64, device=dev) / (n - 1) * 2.0 - 1.0
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sqrt(x * x + y * y + z * z) - 0.7).float().contiguous()
    v, f = ops.marching_cubes(vol, 0.0, (-1.0, -1.0, -1.0), (2.0 / (n - 1),) * 3)
    assert v.shape[0] > 1000 and f.shape[0] > 2000
    md = ops.MeshDistance(v, f)
    d, face = md.query(v)
    assert (d == 0).all() and (face >= 0).all()                        # a vertex lies on its own faces, exactly
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    pushed = (vn.astype(np.float64) * (1.0 + 0.01 / np.linalg.norm(vn.astype(np.float64), axis=1, keepdims=True))).astype(np.float32)
    d, face, near = _check(md, vn, fn, pushed)
    assert np.abs(d - 0.01).max() < 2e-3                               # (the facets' sagitta)
    print(f"marching-cubes sphere: V={len(vn)} F={len(fn)} dims={md.dims} entries per face={md.entries / len(fn):.2f}")


def test_max_dist(dev):
    v, f, q = mr.soup(300, 1000, 51, size=0.03)
    md = _build(v, f, dev)
    full = _check(md, v, f, q)
    cut = float(np.sort(full[0])[300])                                  # an attained distance: `at` the limit is out
    d, face, near = _check(md, v, f, q, max_dist=cut)
    far = full[0] >= np.float32(cut)
    assert far.sum() == 700 and (face[far] == -1).all() and np.isinf(d[far]).all()
    assert np.array_equal(_bits(d[~far]), _bits(full[0][~far])) and np.array_equal(face[~far], full[1][~far])
    assert np.array_equal(near[~far], full[2][~far])
    _check(md, v, f, q, max_dist=cut, sort=False)
    d, face, near = _check(md, v, f, q, max_dist=0.0)
    assert (face == -1).all()


def test_bad_arguments(dev):
    from myslam_amd import ops
    v, f = (torch.from_numpy(x) for x in ONE_FACE)
    with pytest.raises(RuntimeError):
        ops.MeshDistance(v, f.to(dev))                                  # vertices on the CPU
    with pytest.raises(RuntimeError):
        ops.MeshDistance(v.to(dev), f)                                  # faces on the CPU
    with pytest.raises(ValueError):
        ops.MeshDistance(v.to(dev), torch.tensor([[0, 1, 3]], device=dev))
    with pytest.raises(ValueError):
        ops.MeshDistance(v.to(dev), torch.tensor([[0, -1, 2]], device=dev))
    with pytest.raises(RuntimeError):
        ops.MeshDistance(v.to(dev).reshape(-1)[:8], f.to(dev))          # not [V,3]
    with pytest.raises(RuntimeError):
        ops.MeshDistance(v.to(dev), torch.tensor([[0, 1, 2, 0]], device=dev))       # not [F,3]
    md = ops.MeshDistance(v.to(dev), f.to(dev))
    with pytest.raises(RuntimeError):
        md.query(torch.zeros(4, 2, device=dev))
    with pytest.raises(ValueError):
        md.query(torch.zeros(4, 3, device=dev), max_dist=float("nan"))


# ---------------------------------------------------------------------------------------------------------
# metrics, error maps, the command line
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spheres():
    (v1, f1), (v2, f2) = mr.icosphere(3, 1.0), mr.icosphere(3, 1.02)
    assert len(f1) == len(f2) == 1280
    return v1, f1, v2, f2


def _sagitta_and_cos(v, f, radius):
    """(radius minus the smallest distance of a face's plane to the centre; the smallest cosine between a face's normal
    and the radius through one of its corners - the farthest from the normal)."""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    plane = np.abs((n * a).sum(1))
    cos = np.stack([(n * p).sum(1) / np.linalg.norm(p, axis=1) for p in (a, b, c)]).min()
    return radius - plane.min(), cos


def test_metrics_on_concentric_icospheres(dev, spheres):
    from myslam_amd.src.tools import eval_recon as er
    v1, f1, v2, f2 = spheres
    (s1, c1), (s2, c2) = _sagitta_and_cos(v1, f1, 1.0), _sagitta_and_cos(v2, f2, 1.02)
    s = max(s1, s2)
    kw = dict(align=False, num_points=2000)
    ex = er.recon_report(v1, f1, v2, f2, exact=True, **kw)
    sa = er.recon_report(v1, f1, v2, f2, exact=False, **kw)
    print(f"icospheres: sagitta {s:.5f}; exact {ex}; sampled {sa}")
    assert ex["exact"] is True and sa["exact"] is False
    for key in ("accuracy", "completion"):
        assert (0.02 - s) * 100 <= ex[key] <= (0.02 + s) * 100
        assert ex[key] <= sa[key] + BAR[0.0] * 100                      # a sample lies on its mesh
    assert ex["chamfer"] == 0.5 * (ex["accuracy"] + ex["completion"])
    assert ex["precision"] == ex["recall"] == ex["f_score"] == 100.0 and ex["completion_ratio"] == 100.0
    low = er.recon_report(v1, f1, v2, f2, exact=True, f_threshold=0.01, **kw)
    assert low["precision"] == low["recall"] == low["f_score"] == 0.0
    # the cosine of the largest angle between a face normal and the radius through its farthest corner
    worst = min(c1, c2)
    assert 0.9 < worst < 1.0
    assert ex["normal_consistency"] > worst and sa["normal_consistency"] > worst
    assert ex["normal_consistency"] <= 1.0 and ex["normals_skipped"] == 0
    # exact=False: the same samples and queries as recon_metrics, the same floats
    rm = er.recon_metrics(v1, f1, v2, f2, **kw)
    for key in ("accuracy", "completion", "completion_ratio"):
        assert sa[key] == rm[key]


def test_error_meshes(dev):
    from myslam_amd import ops
    from myslam_amd.src.tools import eval_recon as er
    v1, f1 = mr.icosphere(2, 1.0)
    v2, f2 = mr.icosphere(1, 1.03)
    v2 = v2 + np.float64([0.01, 0.02, 0.0])                             # off centre, coarser: the distances vary
    e = er.error_meshes(v1, f1, v2, f2, max_err=0.04, align=False)
    lut = ops.load_plasma_lut()
    for dist, col, (qv, mv, mf) in ((e["rec_dist"], e["rec_colors"], (v1, v2, f2)), (e["gt_dist"], e["gt_colors"], (v2, v1, f1))):
        rd = mr.model_query(mv.astype(np.float32), mf, qv.astype(np.float32))[0]
        assert np.array_equal(_bits(dist.cpu().numpy()), _bits(rd))
        idx = np.floor(np.minimum(rd.astype(np.float64) / 0.04, 1.0) * 255 + 0.5).astype(np.int64)
        assert len(np.unique(idx)) > 5 and idx.max() == 255 and idx.min() < 128       # a range, the top of the scale in it
        assert col.dtype == torch.uint8 and np.array_equal(col.cpu().numpy(), lut[idx])
    assert torch.equal(e["rec_vertices"].cpu(), torch.from_numpy(v1))


def test_command_line(dev, tmp_path):
    from myslam_amd import ops
    from myslam_amd.src.tools import eval_recon as er
    from myslam_amd.src.utils.Mesher import read_ply, write_ply
    v1, f1 = mr.icosphere(1, 1.0)
    v2, f2 = mr.icosphere(1, 1.02)
    rec, gt = str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply")
    write_ply(rec, v1, f1)
    write_ply(gt, v2, f2)
    prefix = str(tmp_path / "err")
    p = subprocess.run([sys.executable, "-m", "myslam_amd.src.tools.eval_recon", "--rec_mesh", rec, "--gt_mesh", gt, "--report",
                        "--exact", "--f_threshold", "0.06", "--error_mesh", prefix, "--error_max", "0.1", "-3d"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    report = dict(ln.split(": ", 1) for ln in lines[:10])
    assert list(report) == ["accuracy", "completion", "completion_ratio", "chamfer", "precision", "recall", "f_score",
                            "normal_consistency", "normals_skipped", "exact"]
    assert report["exact"] == "True" and int(report["normals_skipped"]) == 0
    for key in list(report)[:8]:
        assert np.isfinite(float(report[key]))
    rv, rf, _ = read_ply(rec)
    gv, gf, _ = read_ply(gt)
    same = er.recon_report(rv, rf, gv, gf, exact=True, f_threshold=0.06)
    assert float(report["accuracy"]) == same["accuracy"] and float(report["f_score"]) == same["f_score"]
    # -3d prints what calc_3d_metric prints, after the report
    r3 = er.recon_metrics(rv, rf, gv, gf)
    assert lines[10:] == ["accuracy:  %s" % r3["accuracy"], "completion:  %s" % r3["completion"],
                          "completion ratio:  %s" % r3["completion_ratio"]]
    # the two error meshes: the geometry of each side, colours by the rule
    e = er.error_meshes(rv, rf, gv, gf, max_err=0.1)
    lut = ops.load_plasma_lut()
    for path, geom, faces, col in ((prefix + "_accuracy.ply", e["rec_vertices"].cpu().numpy(), rf, e["rec_colors"]),
                                   (prefix + "_completion.ply", gv, gf, e["gt_colors"])):
        pv, pf, pc = read_ply(path)
        assert np.array_equal(pv, geom.astype(np.float32)) and np.array_equal(pf, faces)
        assert np.array_equal(np.round(pc * 255).astype(np.uint8), col.cpu().numpy())
        assert (col.cpu().numpy()[:, None, :] == lut[None]).all(-1).any(1).all()
