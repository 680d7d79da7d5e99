"""CPU side of the SDF-gradient / normals feature: the criteria of tests/sdf_normals_ref.py accept the float32 oracle and
reject three mutants of the model; normals in PLY files; the numpy model of the shading rule.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import sdf_normals_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def models():
    pts, planes, params, sc = ref.fixture_model()
    s64, g64 = ref.model(pts, planes(torch.float64), params(torch.float64), sc.bound)
    s32, g32 = ref.model(pts, planes(torch.float32), params(torch.float32), sc.bound, dtype=torch.float32)
    return dict(pts=pts, planes=planes, params=params, sc=sc, s64=s64, g64=g64, s32=s32, g32=g32,
                clamped=ref.clamped_components(pts.numpy(), sc.bound.numpy()))


def test_float32_oracle_meets_every_criterion(models):
    """Measured when the criteria were written: float32 against float64 8.3e-6 on the gradient (helpers.rel_err; a 12 x margin
    under the 1e-4 bar), 4.4e-7 on the sdf; 997 clamped components, all exactly zero; 13 zero rows; unit normals differ by at
    most 6.3e-5, at rows with |grad| of 1e-3 against a median of 2.3e-2."""
    m = models
    assert m["pts"].shape == (2000, 3) and m["g32"].dtype == np.float32
    assert int(m["clamped"].sum()) == 997
    assert int((~m["g64"].any(-1)).sum()) == 13
    assert (m["g64"][m["clamped"]] == 0.0).all()
    fig = ref.gradient_figures(m["g32"], m["g64"], m["clamped"])
    assert ref.gradient_ok(fig) and fig["rel_err"] <= ref.GRAD_RTOL / 4, fig
    assert hp.rel_err(m["s32"], m["s64"]) <= 1e-5
    u32 = ref.unit_rows(m["g32"])
    assert np.abs(u32 - ref.unit_rows(m["g64"])).max() <= 2e-4
    nfig = ref.normal_figures(u32.astype(np.float32), m["g64"], m["g32"])
    assert ref.normals_ok(nfig) and nfig["excess"] <= 1.0 / ref.MARGIN + 1e-3, nfig
    # the model itself is the project's: a central difference of the float64 sdf at interior points
    inside = ~m["clamped"].any(-1)
    p = m["pts"][inside][:50].double()
    h = 1e-6
    for k in range(3):
        d = torch.zeros(3, dtype=torch.float64)
        d[k] = h
        sp, _ = ref.model(p + d, m["planes"](torch.float64), m["params"](torch.float64), m["sc"].bound)
        sm, _ = ref.model(p - d, m["planes"](torch.float64), m["params"](torch.float64), m["sc"].bound)
        fd = (sp - sm) / (2 * h)
        g = m["g64"][inside][:50, k]
        ok = np.abs(fd - g) <= 1e-4 * np.abs(m["g64"]).max()          # (a kink of a ReLU or a texel edge inside +-h: not compared)
        assert ok.mean() >= 0.9, (k, ok.mean())


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_criteria_reject_mutants(models, mutant):
    m = models
    _, g = ref.model(m["pts"], m["planes"](torch.float64), m["params"](torch.float64), m["sc"].bound, mutant=mutant)
    fig = ref.gradient_figures(g, m["g64"], m["clamped"])
    assert not ref.gradient_ok(fig), fig
    if mutant == "no_border_gate":
        assert fig["clamped_nonzero"] > 0 and fig["zero_rows_nonzero"] > 0
    if mutant != "no_tanh_factor":          # (a positive factor per row: the direction is unchanged, the gradient bar catches it)
        assert not ref.normals_ok(ref.normal_figures(ref.unit_rows(g), m["g64"], m["g32"]))


def test_unit_rows_keeps_zero_rows_zero():
    g = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 4.0], [1e-30, 0.0, 0.0]])
    u = ref.unit_rows(g)
    assert (u[0] == 0).all() and np.allclose(u[1], [0.6, 0.0, 0.8]) and np.allclose(u[2], [1.0, 0.0, 0.0])
    assert not np.isnan(u).any()


# ----------------------------------------------------------------------------------------------
# PLY
# ----------------------------------------------------------------------------------------------
def _mesh(rng, V=37, F=50):
    v = rng.normal(size=(V, 3)).astype(np.float32)
    f = rng.integers(0, V, size=(F, 3)).astype(np.int32)
    c = (rng.integers(0, 256, size=(V, 3)) / 255.0).astype(np.float32)
    n = rng.normal(size=(V, 3)).astype(np.float32)
    n[3] = 0.0
    n[4] = [np.float32(1e-38), -0.0, np.float32(3e38)]
    return v, f, c, n


@pytest.mark.parametrize("with_colors", [True, False])
def test_ply_normals_round_trip(tmp_path, with_colors):
    from myslam_amd.src.utils.Mesher import read_ply, read_ply_normals, write_ply
    v, f, c, n = _mesh(np.random.default_rng(5))
    c = c if with_colors else None
    a, b = tmp_path / "with.ply", tmp_path / "without.ply"
    write_ply(a, v, f, c, normals=n)
    write_ply(b, v, f, c)
    got = read_ply_normals(a)
    assert got.dtype == np.float32 and got.tobytes() == n.tobytes()           # bit for bit, -0.0 and denormals included
    assert read_ply_normals(b) is None
    head = open(a, "rb").read().split(b"end_header")[0].decode().split("\n")
    k = head.index("property float z")
    assert head[k + 1:k + 4] == ["property float nx", "property float ny", "property float nz"]
    ra, rb = read_ply(a), read_ply(b)
    assert len(ra) == 3
    for x, y in zip(ra, rb):
        assert (x is None and y is None) or (x.dtype == y.dtype and x.tobytes() == y.tobytes())
    assert ra[0].tobytes() == v.tobytes() and (ra[1] == f).all()
    with pytest.raises(ValueError, match="normals"):
        write_ply(a, v, f, c, normals=n[:5])


@pytest.mark.parametrize("with_colors", [True, False])
def test_ply_without_normals_is_byte_identical(tmp_path, with_colors):
    from myslam_amd.src.utils.Mesher import write_ply
    v, f, c, _ = _mesh(np.random.default_rng(6))
    c = c if with_colors else None
    a, b, d = tmp_path / "a.ply", tmp_path / "b.ply", tmp_path / "d.ply"
    write_ply(a, v, f, c)
    write_ply(d, v, f, c, normals=None)
    ref.parent_write_ply(b, v, f, c)
    assert open(a, "rb").read() == open(b, "rb").read() == open(d, "rb").read()


def test_ply_normals_ascii_and_big_endian(tmp_path):
    from myslam_amd.src.utils.Mesher import read_ply_normals
    p = tmp_path / "a.ply"
    p.write_text("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
                 "property float nx\nproperty float ny\nproperty float nz\nelement face 0\n"
                 "property list uchar int vertex_indices\nend_header\n0 0 0 0 0 1\n1 2 3 0.6 0 -0.8\n")
    assert np.array_equal(read_ply_normals(p), np.array([[0, 0, 1], [0.6, 0, -0.8]], dtype=np.float32))
    q = tmp_path / "b.ply"
    head = ("ply\nformat binary_big_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nend_header\n").encode()
    q.write_bytes(head + np.array([1, 2, 3, 0, 1, 0], dtype=">f4").tobytes())
    assert np.array_equal(read_ply_normals(q), np.array([[0, 1, 0]], dtype=np.float32))


# ----------------------------------------------------------------------------------------------
# shading rule
# ----------------------------------------------------------------------------------------------
def test_shading_model():
    v = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 2.0], [0, 0, 0]], dtype=np.float64)
    n = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 0], [0, 3, 4], [0, 0, 1], [1, 0, 0]], dtype=np.float64)
    c = np.array([[100, 200, 255, 7]] * 6, dtype=np.uint8)
    cam = (0.0, 0.0, 2.0)
    k = ref.shade(v, n, c, cam, 0.3)[:, 0] / 100.0
    # facing the light; facing away (ambient only); no normal; oblique (cos = 0.8); the vertex at the light; perpendicular
    assert np.allclose(k, [1.0, 0.3, 1.0, 0.3 + 0.7 * 0.8, 1.0, 0.3])
    u8 = ref.shade_u8(v, n, c, cam, 0.3)
    assert u8.dtype == np.uint8 and (u8[:, 3] == 255).all()
    assert u8[0].tolist() == [100, 200, 255, 255] and u8[1].tolist() == [30, 60, 77, 255]      # floor(76.5 + 0.5) = 77
    assert ref.shade_u8(v, n, None, cam, 0.0)[1].tolist() == [0, 0, 0, 255]
    assert ref.shade_u8(v, n, None, cam, 1.0)[:, :3].tolist() == [[200, 200, 200]] * 6
    # never above the input colour, never below the ambient share
    rng = np.random.default_rng(1)
    v, n = rng.normal(size=(500, 3)), rng.normal(size=(500, 3))
    c = rng.integers(0, 256, size=(500, 3)).astype(np.uint8)
    s = ref.shade(v, n, c, (0.1, -0.2, 0.3), 0.25)
    assert (s <= c + 1e-9).all() and (s >= 0.25 * c - 1e-9).all()


def test_header_declares_the_new_entries():
    from myslam_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "eslam_hip.h")).read()
    assert "#define ESLAM_SDF_GRAD_UNIT 1" in hdr and "#define ESLAM_ABI_VERSION 5" in hdr
    for name in ("eslam_sdf_grad", "eslam_shade_vertices"):
        assert name + "(" in hdr and name in _hip.SIGNATURES
    lib = _hip.load_library()
    assert lib.eslam_profile_name(_hip.PROF_KERNELS - 1).decode() == "sdf_grad_kernel"
    # argument checks that need no GPU: decided before any launch
    assert lib.eslam_sdf_grad(None, None, None, None, -1, 0, None, None, None) != 0
    assert b"eslam_sdf_grad" in lib.eslam_last_error()
    assert lib.eslam_sdf_grad(None, None, None, None, 5, 4, None, None, None) != 0
    assert b"flags" in lib.eslam_last_error()
    assert lib.eslam_sdf_grad(None, None, None, None, 0, 0, None, None, None) == 0          # N = 0 launches nothing
    assert lib.eslam_sdf_grad(None, None, None, None, 5, 1, None, None, None) != 0
    assert b"null" in lib.eslam_last_error()
    assert lib.eslam_shade_vertices(None, None, None, 0, (_hip.ctypes.c_float * 3)(0, 0, 0), 0.3, None, None) == 0
    assert lib.eslam_shade_vertices(None, None, None, 4, (_hip.ctypes.c_float * 3)(0, 0, 0), 0.3, None, None) != 0
    assert b"eslam_shade_vertices" in lib.eslam_last_error()
    assert lib.eslam_shade_vertices(None, None, None, 0, (_hip.ctypes.c_float * 3)(0, 0, 0), 1.5, None, None) != 0
    assert b"ambient" in lib.eslam_last_error()


def test_tools_size_the_profile_buffer_from_the_binding():
    """eslam_profile_read writes ESLAM_PROF_KERNELS floats (13 since sdf_grad_kernel has a slot): a caller's buffer of a literal
    size is a write past its end the next time the count grows."""
    import glob
    import re
    from myslam_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "eslam_hip.h")).read()
    assert int(re.search(r"#define ESLAM_PROF_KERNELS (\d+)", hdr).group(1)) == _hip.PROF_KERNELS == 13
    users = [p for p in glob.glob(os.path.join(ROOT, "tools", "*.py")) + [os.path.join(ROOT, "bench.py")]
             if "eslam_profile_read" in open(p).read()]
    assert len(users) >= 5
    for p in users:
        src = open(p).read()
        assert "PROF_KERNELS" in src and not re.search(r"c_float \* \d+\)\(\)", src), p
