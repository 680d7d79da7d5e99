"""The fused SDF gradient on the GPU (eslam_sdf_grad, ops.sdf_gradient, Decoders.sdf_gradient / sdf_normals), normals in
meshes and PLY files, and the viewer's headlight shading - against the CPU models and criteria of tests/sdf_normals_ref.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import sdf_normals_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda:0")


_cache = {}


def _setup(shapes=None):
    """The fixture's points, decoders and both CPU models (computed once per plane-shape set, shared, never changed)."""
    if shapes not in _cache:
        from myslam_amd import scene as scn
        from myslam_amd.src.networks.decoders import Decoders
        from tests import every_texel as et
        sc = scn.make_scene("room0")
        if shapes is not None:
            sc = et.with_shapes(sc, shapes)
        pts, planes, params, sc = ref.fixture_model(sc)
        fx = hp.load("decoders_room0_points")
        dec = Decoders()
        dec.load_state_dict({k[6:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("param:")})
        dec = dec.to(_dev())
        dec.bound = sc.bound
        for t in dec.parameters():
            t.requires_grad_(False)
        s64, g64 = ref.model(pts, planes(torch.float64), params(torch.float64), sc.bound)
        s32, g32 = ref.model(pts, planes(torch.float32), params(torch.float32), sc.bound, dtype=torch.float32)
        _cache[shapes] = dict(sc=sc, pts=pts, planes=planes, dec=dec, g64=g64, g32=g32, s64=s64,
                              clamped=ref.clamped_components(pts.numpy(), sc.bound.numpy()))
    return _cache[shapes]


def _check_against_model(s, planes, pts_gpu):
    from myslam_amd import ops
    bound6 = ops.bound_to_host(s["sc"].bound)
    sdf, grad = ops.sdf_gradient(pts_gpu, bound6, planes, s["dec"])
    assert sdf.shape == (pts_gpu.shape[0],) and grad.shape == (pts_gpu.shape[0], 3)
    assert torch.equal(sdf, ops.decode_sdf_only(pts_gpu, bound6, planes, s["dec"]))          # bit for bit
    assert hp.rel_err(sdf.cpu().numpy(), s["s64"]) <= 1e-4
    fig = ref.gradient_figures(grad.cpu().numpy(), s["g64"], s["clamped"])
    print("gradient", fig)
    assert ref.gradient_ok(fig), fig
    sdf_u, unit = ops.sdf_gradient(pts_gpu, bound6, planes, s["dec"], unit=True)
    assert torch.equal(sdf_u, sdf)
    nfig = ref.normal_figures(unit.cpu().numpy(), s["g64"], s["g32"])
    print("normals", nfig)
    assert ref.normals_ok(nfig), nfig
    zero = ~s["g64"].any(-1)
    assert not unit.cpu().numpy()[zero].any() and not grad.cpu().numpy()[zero].any()
    return sdf, grad, unit


@pytest.mark.parametrize("channels_last", [True, False])
def test_gradient_and_normals_against_the_model(channels_last):
    s = _setup()
    assert int(s["clamped"].sum()) == 997 and int((~s["g64"].any(-1)).sum()) == 13
    planes = s["planes"](device=_dev(), channels_last=channels_last)
    assert planes[0][0].is_contiguous() != channels_last
    _check_against_model(s, planes, s["pts"].to(_dev()))


@pytest.mark.parametrize("shapes", ["one_cell", "slivers", "levels_swapped"])
@pytest.mark.parametrize("channels_last", [True, False])
def test_planes_no_scene_makes(shapes, channels_last):
    s = _setup(shapes)
    _check_against_model(s, s["planes"](device=_dev(), channels_last=channels_last), s["pts"].to(_dev()))


@pytest.mark.parametrize("channels_last", [True, False])
def test_tile_edges(channels_last):
    """A call on the first N points equals the first N rows of the full call bit for bit: clamped duplicate lanes, partial
    blocks, several workgroups; and one size above the grid cap, where the grid-stride loop runs twice."""
    from myslam_amd import ops
    s = _setup()
    dev = _dev()
    planes = s["planes"](device=dev, channels_last=channels_last)
    bound6 = ops.bound_to_host(s["sc"].bound)
    pts = s["pts"].to(dev)
    for unit in (False, True):
        sdf, grad = ops.sdf_gradient(pts, bound6, planes, s["dec"], unit=unit)
        for n in (1, 15, 16, 17, 63, 64, 65, 257):
            a, b = ops.sdf_gradient(pts[:n], bound6, planes, s["dec"], unit=unit)
            assert torch.equal(a, sdf[:n]) and torch.equal(b, grad[:n]), (n, unit)
    a, b = ops.sdf_gradient(pts[:0], bound6, planes, s["dec"])
    assert a.shape == (0,) and b.shape == (0, 3)
    # any leading shape
    sdf, grad = ops.sdf_gradient(pts, bound6, planes, s["dec"])
    a, b = ops.sdf_gradient(pts.reshape(40, 50, 3), bound6, planes, s["dec"])
    assert a.shape == (40, 50) and b.shape == (40, 50, 3)
    assert torch.equal(a.reshape(-1), sdf) and torch.equal(b.reshape(-1, 3), grad)
    if channels_last:
        hdr = open(os.path.join(ROOT, "include", "eslam_hip.h")).read()
        cap = int(re.search(r"#define ESLAM_SDF_GRAD_MAX_GROUPS (\d+)", hdr).group(1))
        n = cap * 256 + 77
        idx = torch.arange(n, device=dev) % pts.shape[0]
        a, b = ops.sdf_gradient(pts[idx], bound6, planes, s["dec"])
        assert torch.equal(a, sdf[idx]) and torch.equal(b, grad[idx])


def test_agrees_with_the_autograd_route():
    from myslam_amd import ops
    s = _setup()
    dev = _dev()
    planes = s["planes"](device=dev, channels_last=True)
    p = s["pts"].to(dev).requires_grad_(True)
    raw = s["dec"](p, all_planes=planes)
    raw[:, 3].sum().backward()
    sdf, grad = s["dec"].sdf_gradient(p, planes)
    assert not grad.requires_grad
    assert hp.rel_err(grad.cpu().numpy(), p.grad.cpu().numpy()) <= 1e-4
    assert hp.rel_err(sdf.cpu().numpy(), raw[:, 3].detach().cpu().numpy()) <= 1e-6
    n = s["dec"].sdf_normals(p, planes)
    assert torch.equal(n, ops.sdf_gradient(p, ops.bound_to_host(s["sc"].bound), planes, s["dec"], unit=True)[1])


def test_argument_errors():
    from myslam_amd import _hip, ops
    s = _setup()
    dev = _dev()
    planes = s["planes"](device=dev, channels_last=True)
    bound6 = ops.bound_to_host(s["sc"].bound)
    pts = s["pts"].to(dev)
    with pytest.raises(RuntimeError, match="on the GPU"):
        ops.sdf_gradient(s["pts"], bound6, planes, s["dec"])
    with pytest.raises(RuntimeError, match="float32"):
        ops.sdf_gradient(pts.double(), bound6, planes, s["dec"])
    with pytest.raises(RuntimeError, match=r"\[\.\.\.,3\]"):
        ops.sdf_gradient(pts[:, :2], bound6, planes, s["dec"])
    with pytest.raises(RuntimeError, match="float32"):
        ops.sdf_gradient(pts, bound6, tuple([q.half() for q in grp] for grp in planes), s["dec"])
    # the C entry point itself: non-zero and eslam_last_error() set, before any launch
    lib = _hip.lib()
    arr, _ = _hip.make_planes(tuple(planes[:3]) + tuple(planes[:3]))
    dec, keep = _hip.make_decoders(ops.decoder_params(s["dec"]), ops.beta_tensor(10, dev))
    out = torch.full((8, 3), 7.0, device=dev)
    b6 = _hip.make_bound(bound6)
    st = _hip.stream_handle(dev)
    for args, word in (((arr, ctypes.byref(dec), b6, _hip.ptr(pts), 8, 2, None, _hip.ptr(out), st), "flags"),
                       ((arr, ctypes.byref(dec), b6, _hip.ptr(pts), -1, 0, None, _hip.ptr(out), st), "negative"),
                       ((arr, ctypes.byref(dec), b6, None, 8, 0, None, _hip.ptr(out), st), "null"),
                       ((arr, ctypes.byref(dec), b6, _hip.ptr(pts), 8, 0, None, None, st), "null")):
        assert lib.eslam_sdf_grad(*args) != 0
        msg = lib.eslam_last_error().decode()
        assert "eslam_sdf_grad" in msg and word in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # sdf may be NULL
    assert lib.eslam_sdf_grad(arr, ctypes.byref(dec), b6, _hip.ptr(pts), 8, 0, None, _hip.ptr(out), st) == 0
    assert torch.equal(out, ops.sdf_gradient(pts[:8], bound6, planes, s["dec"])[1])


# ----------------------------------------------------------------------------------------------
# meshes
# ----------------------------------------------------------------------------------------------
def test_mesh_normals(tmp_path):
    from myslam_amd.src.utils import Mesher as M
    from tests.test_gpu_mesh import _mesher, _toy_run
    sc, s = _toy_run()
    m = _mesher(sc, resolution=0.04)
    plain = M.extract_mesh(m, s.all_planes, s.decoders, s.keyframe_dict, device="cuda:0")
    full = M.extract_mesh(m, s.all_planes, s.decoders, s.keyframe_dict, device="cuda:0", normals=True)
    assert len(plain) == 3 and len(full) == 4
    for a, b in zip(plain, full):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    v, f, c, n = full
    assert n.dtype == np.float32 and n.shape == v.shape and len(v) > 1000
    length = np.sqrt((n.astype(np.float64) ** 2).sum(-1))
    assert (np.abs(length[length > 0] - 1.0) <= 1e-6).all() and (length > 0).mean() > 0.99
    want = s.decoders.sdf_normals(torch.from_numpy(v).to(_dev()) * m.scale, s.all_planes)
    assert n.tobytes() == want.cpu().numpy().tobytes()
    assert n.tobytes() == M.vertex_normals(m, v, s.all_planes, s.decoders).tobytes()
    # +grad sdf is the side the faces' winding faces: (v1 - v0) x (v2 - v0) points toward values >= level
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).astype(np.float64)
    agree = ((fn * n[f].astype(np.float64).sum(1)).sum(-1) > 0).mean()
    # a test of the SIGN: with the share p of agreeing faces for +grad sdf, -grad sdf would give 1 - p, so one half separates
    # the two whatever the noise of a briefly trained field does to single faces (measured on an MI355X: p = 0.905)
    print(f"faces whose winding agrees with the mean of their vertex normals: {agree:.4f}")
    assert agree > 0.5
    a, b, d = tmp_path / "n.ply", tmp_path / "plain.ply", tmp_path / "parent.ply"
    M.get_mesh(m, str(a), s.all_planes, s.decoders, s.keyframe_dict, device="cuda:0", normals=True)
    assert M.read_ply_normals(a).tobytes() == n.tobytes()
    ra = M.read_ply(a)
    assert ra[0].tobytes() == v.tobytes() and (ra[1] == f).all()
    M.get_mesh(m, str(b), s.all_planes, s.decoders, s.keyframe_dict, device="cuda:0")
    ref.parent_write_ply(d, *plain)
    assert open(b, "rb").read() == open(d, "rb").read()
    assert M.read_ply_normals(b) is None


_CHILD = r"""
import sys
from pathlib import Path
from types import SimpleNamespace
import yaml
from myslam_amd.src.ESLAM import ESLAM
from tests.test_gpu_frames import _toy_cfg, _write_toy_sequence
root, name = Path(sys.argv[1]), sys.argv[2]
if not (root / "seq").exists():
    _write_toy_sequence(root / "seq", 9)
cfg = _toy_cfg(root / "seq", root / name)
cfg["mapping"]["mesh_freq"] = 4
cfg["meshing"]["clean_min_faces"] = 20
if name == "with":
    cfg["meshing"]["normals"] = True
ESLAM(cfg, SimpleNamespace(input_folder=None, output=None)).run()
with open(root / "ESLAM.yaml", "w") as fh:          # the defaults file the visualizer finds above its config
    yaml.safe_dump(cfg, fh)
print("CHILD-OK")
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The tiny sequence of tests/test_gpu_frames.py run twice, each in a fresh child process under its own timeout: with
    meshing.normals: true and without the key, under ESLAM_DETERMINISTIC=1 (reproducible plane gradients: the two runs learn
    the same field from the same seed)."""
    root = tmp_path_factory.mktemp("normals_runs")
    env = dict(os.environ, ESLAM_DETERMINISTIC="1")
    for name in ("with", "without"):
        p = subprocess.run([sys.executable, "-c", _CHILD, str(root), name], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stderr[-3000:]
    return root


def test_eslam_writes_normals_into_every_mesh_file(runs):
    from myslam_amd.src.utils.Mesher import read_ply, read_ply_normals
    names = sorted(os.listdir(runs / "with" / "mesh"))
    assert names == sorted(os.listdir(runs / "without" / "mesh"))
    assert {"final_mesh.ply", "final_mesh_culled.ply", "final_mesh_culled_clean.ply", "00004_mesh.ply", "00004_mesh_culled.ply",
            "00004_mesh_culled_clean.ply"} <= set(names)
    for name in names:
        a, b = runs / "with" / "mesh" / name, runs / "without" / "mesh" / name
        n = read_ply_normals(a)
        va, fa, ca = read_ply(a)
        vb, fb, cb = read_ply(b)
        assert read_ply_normals(b) is None and n is not None and n.shape == va.shape, name
        length = np.sqrt((n.astype(np.float64) ** 2).sum(-1))
        assert (np.abs(length[length > 0] - 1.0) <= 1e-6).all() and (length > 0).mean() > 0.99, name
        assert va.tobytes() == vb.tobytes() and fa.tobytes() == fb.tobytes() and ca.tobytes() == cb.tobytes(), name


# ----------------------------------------------------------------------------------------------
# shading
# ----------------------------------------------------------------------------------------------
def _bumpy(nq):
    """A height field of nq x nq quads (2 nq^2 faces) over [-1, 1]^2 near z = 0 with its analytic normals (towards -z, where
    the cameras stand), a few normals zeroed or scaled; colours from a hash."""
    g = np.linspace(-1.0, 1.0, nq + 1)
    x, y = np.meshgrid(g, g, indexing="xy")
    z = 0.15 * np.sin(2.5 * x) * np.cos(1.7 * y)
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    dzdx, dzdy = 0.15 * 2.5 * np.cos(2.5 * x) * np.cos(1.7 * y), -0.15 * 1.7 * np.sin(2.5 * x) * np.sin(1.7 * y)
    n = np.stack([dzdx, dzdy, -np.ones_like(z)], -1).reshape(-1, 3)
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    n[0] = 0.0
    n[1] *= 3.0
    i = np.arange(nq)
    a = (i[:, None] * (nq + 1) + i[None]).reshape(-1)
    f = np.concatenate([np.stack([a, a + nq + 1, a + 1], 1), np.stack([a + 1, a + nq + 1, a + nq + 2], 1)]).astype(np.int32)
    c = ((np.arange(v.shape[0])[:, None] * np.array([37, 91, 53]) + np.array([11, 140, 200])) % 256).astype(np.uint8)
    return v, f, c, n


def _views():
    out = []
    for tx, ty, tz in ((0.0, 0.0, -3.0), (1.2, -0.4, -2.0), (-0.8, 0.9, -1.5)):
        c2w = np.eye(4)
        c2w[:3, 3] = (tx, ty, tz)
        out.append(c2w)
    return np.stack(out)


@pytest.mark.parametrize("nq", [1, 10])
@pytest.mark.parametrize("colours", [True, False])
def test_shaded_render(nq, colours):
    from myslam_amd import ops
    dev = _dev()
    v, f, c, n = _bumpy(nq)
    assert len(f) == 2 * nq * nq
    tv, tf, tn = (torch.from_numpy(a).to(dev) for a in (v, f, n))
    tc = torch.from_numpy(c).to(dev) if colours else None
    views = _views()
    K, H, W = (90.0, 90.0, 63.5, 47.5), 96, 128
    kw = dict(cull_backfaces=False, chunk=2)
    lit = ops.render_view([(tv, tf, tc, tn)], [], views, K, H, W, shade=True, ambient=0.3, **kw)
    unlit = ops.render_view([(tv, tf, tc)], [], views, K, H, W, **kw)
    assert lit.shape == unlit.shape == (3, H, W, 3)
    worst = 0
    for k in range(len(views)):
        cam = views[k, :3, 3]
        sc = ops.shade_vertices(tv, tn, tc, cam, 0.3)
        assert sc.dtype == torch.uint8 and sc.shape == (len(v), 4) and bool((sc[:, 3] == 255).all())
        model = ref.shade(v, n, c if colours else None, cam.astype(np.float32), 0.3)
        want = np.floor(np.minimum(255.0, model) + 0.5)
        worst = max(worst, int(np.abs(sc[:, :3].cpu().numpy().astype(np.int64) - want.astype(np.int64)).max()))
        assert sc[0, :3].tolist() == ([int(x) for x in c[0]] if colours else [200, 200, 200])         # no normal: k = 1
        one = ops.render_view([(tv, tf, sc)], [], views[k:k + 1], K, H, W, **kw)
        assert torch.equal(lit[k], one[0]), k
    print(f"shaded colours against the float64 model: at most {worst} level(s) off")
    assert worst <= 1
    assert not torch.equal(lit, unlit) and (lit.cpu().numpy().astype(np.int64).sum() < unlit.cpu().numpy().astype(np.int64).sum())
    # shade=False with normals attached, and shade=True without normals: today's image
    assert torch.equal(ops.render_view([(tv, tf, tc, tn)], [], views, K, H, W, **kw), unlit)
    assert torch.equal(ops.render_view([(tv, tf, tc, None)], [], views, K, H, W, shade=True, **kw), unlit)
    assert torch.equal(ops.render_view([(tv, tf, tc)], [], views, K, H, W, shade=True, **kw), unlit)
    with pytest.raises(RuntimeError, match="normal"):
        ops.render_view([(tv, tf, tc, tn[:-1])], [], views, K, H, W, shade=True, **kw)
    with pytest.raises(RuntimeError, match="ambient"):
        ops.shade_vertices(tv, tn, tc, views[0, :3, 3], 1.5)


def test_visualizer_shaded(runs):
    from PIL import Image
    import yaml
    hs, ws = 135, 240
    imgs = {}
    for name in ("with", "without"):
        out = runs / name
        with open(runs / f"{name}_toy.yaml", "w") as fh:
            yaml.safe_dump(dict(data=dict(output=str(out))), fh)
        p = subprocess.run([sys.executable, "-m", "myslam_amd.visualizer", str(runs / f"{name}_toy.yaml"), "--save_rendering",
                            "--every", "8", "--size", str(hs), str(ws), "--shaded", "--ambient", "0.2"], cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        assert ("no vertex normals" in p.stdout) == (name == "without"), p.stdout[-2000:]
        assert sorted(os.listdir(out / "tmp_rendering")) == ["000000.jpg", "000008.jpg"]
        imgs[name] = np.asarray(Image.open(out / "tmp_rendering" / "000008.jpg")).astype(np.int64)
        assert imgs[name].shape == (hs, ws, 3)
    # the same mesh, lit and unlit: the lit picture is darker where the mesh shows
    assert imgs["with"].sum() < imgs["without"].sum()
