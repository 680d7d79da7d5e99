"""Free points on the mixed-precision kernels - ops.mixed_precision(half, points=True): DecodeFn (Decoders.forward), decode_sdf_only,
Mesher.eval_points, ops.sdf_grid and through them Mesher.extract_mesh - against tests/lowp_points_ref.py, the float64 model with
the kernels' rounding points.  tests/test_lowp_points_ref.py pins that model on the CPU and shows that the criteria used here
reject the float32 field and a position derivative taken on the float32 masters.

  1  a step (forward, saved features, g_pts, plane and decoder gradients) at every prefix length and on both states, also
     with frozen decoders and with points that take no gradient
  2  decode_sdf_only and eval_points give the bits of DecodeFn's forward; -1 outside the bound(s)
  3  exact-arithmetic inputs: the plain float64 oracle at the float32 parity bar, features bit for bit
  4  the copies are what is read - and only under points=True
  5  sdf_grid: the bits of eslam_decode_fwd on the materialised points, the hull mask, the model
  6  extract_mesh inside the context = its parts inside the context, and not the float32 mesh
  7  refusals, defaults, a backward behind the context's exit

Prefix lengths (lowp_points_ref.SIZES): one point, partial and full 16-point MFMA blocks (15, 16, 17), partial and full
64-point wave tiles (63, 64, 65), a partial workgroup (255, 257) and many workgroups (all 8000 / 6400 points).
Every test prints the figures it measured before it asserts (pytest -s).
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import lowp_points_ref as P
from tests import lowp_ref as lr

pytestmark = pytest.mark.gpu

CASES = [(name, n) for name in P.STATES for n in P.sizes(name)]


def _dev():
    return torch.device("cuda:0")


def _np(t):
    return None if t is None else t.detach().float().cpu().numpy().astype(np.float64)


def _saved_features(raw):
    """The features ops.DecodeFn saved for the backward of `raw` (its save order: pts, raw, feat, ...); Decoders.forward puts a
    view behind the function's output."""
    fn = raw.grad_fn
    while not hasattr(fn, "saved_tensors"):
        fn = fn.next_functions[0][0]
    return fn.saved_tensors[2]


def _build(name, planes_grad=True, dec_grad=True, channels_last=True):
    from tests.test_gpu_parity import build
    sc, planes, dec, _ = build(P.state(name)["fx"], channels_last=channels_last, planes_grad=planes_grad, dec_grad=dec_grad)
    return planes, dec


def _step(name, n, planes_grad=True, dec_grad=True, pts_grad=True, points=True):
    """Decoders.forward on the first n points of a state inside the context, then L = sum(raw * G) backward.  Returns the
    dict lowp_points_ref's criteria read (float64 numpy; gradients that were not asked for are missing)."""
    from myslam_amd import lowp, ops
    dev = _dev()
    st = P.state(name)
    planes, dec = _build(name, planes_grad, dec_grad)
    half = lowp.HalfPlanes(planes)
    p = st["pts"][:n].to(dev).requires_grad_(pts_grad)
    G = st["G"][:n].to(dev)
    with ops.mixed_precision(half, points=points):
        raw = dec(p, planes)
        feat = _saved_features(raw)
        (raw * G).sum().backward()
    torch.cuda.synchronize()
    out = dict(raw=_np(raw), feat=feat.float().cpu().numpy(), feat_dtype=feat.dtype)
    if pts_grad:
        out["g_pts"] = _np(p.grad)
    if planes_grad:
        out["planes"] = [_np(q.grad) for q in hp.flat_planes(planes)]
    if dec_grad:
        out["dec"] = {k: _np(q.grad) for k, q in dec.named_parameters() if k != "beta"}
    return out


def _hold(label, got, name, ref, f32, which):
    rep = []
    bad = P.forward_failures(got, ref, f32, P.full_set_figures(name)["cap"], rep) + P.feature_failures(got, name, rep)
    bad += P.gradient_failures(got, ref, f32, rep, which)
    print(f"{label}: " + "; ".join(rep))
    for k in ("raw", "g_pts"):
        assert k not in got or np.isfinite(got[k]).all(), (label, k)
    assert not bad, (label, bad)


# ---- 1. a step against the model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES)
def test_step_against_the_model(name, n):
    full = _step(name, n)
    assert full["feat_dtype"] == torch.bfloat16 and full["feat"].shape == (n, 128)
    ref, f32 = P.model_pair(name, n, full["feat"])
    _hold(f"{name} N={n}", full, name, ref, f32, ("g_pts", "planes", "dec"))
    # frozen decoders (g_dec NULL: the kernel without the weight-gradient contractions), and points that take no gradient
    # (no coordinate kernel): the same forward, the remaining gradients under the same bars
    frozen = _step(name, n, dec_grad=False)
    fixed = _step(name, n, pts_grad=False)
    for r, label, which in ((frozen, "frozen decoders", ("g_pts", "planes")), (fixed, "fixed points", ("planes", "dec"))):
        assert np.array_equal(r["raw"], full["raw"]) and np.array_equal(r["feat"], full["feat"]), label
        _hold(f"{name} N={n} {label}", r, name, ref, f32, which)
    # nothing in front of the coordinate kernel has atomics, and its own sums have a fixed order
    assert np.array_equal(frozen["g_pts"], full["g_pts"])


# ---- 2. the other free-point entries give DecodeFn's bits ------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(P.STATES))
def test_sdf_only_and_eval_points_are_the_bits_of_decode(name):
    from myslam_amd import lowp, ops
    from myslam_amd.src.utils.Mesher import eval_points
    dev = _dev()
    st = P.state(name)
    planes, dec = _build(name, False, False)
    half = lowp.HalfPlanes(planes)
    p = st["pts"].to(dev)
    b = st["bound"]
    inside = ((st["pts"] > b[:, 0]) & (st["pts"] < b[:, 1])).all(1)
    small = torch.stack([b[:, 0] + 0.2 * (b[:, 1] - b[:, 0]), b[:, 1] - 0.15 * (b[:, 1] - b[:, 0])], 1)     # a mesher bound of its own
    inside_small = ((st["pts"] > small[:, 0]) & (st["pts"] < small[:, 1])).all(1)
    assert 0 < int((~inside).sum()) and int(inside_small.sum()) < int(inside.sum())
    for n in (65, p.shape[0]):
        with torch.no_grad(), ops.mixed_precision(half, points=True):
            raw = dec(p[:n], planes)
            sdf = ops.decode_sdf_only(p[:n], ops.bound_to_host(dec.bound), planes, dec)
            same = eval_points(SimpleNamespace(points_batch_size=1000, bound=dec.bound), p[:n], planes, dec)
            other = eval_points(SimpleNamespace(points_batch_size=500000, bound=small), p[:n], planes, dec)
            p_nor = ((p[:n] - b[:, 0].to(dev)) / (b[:, 1] - b[:, 0]).to(dev)) * 2 - 1.0
            raw_nor = dec._decode(p_nor, (-1.0, 1.0) * 3, planes)
            sdf_nor = dec.get_raw_sdf(p_nor, planes)
        with torch.no_grad():
            f32 = dec(p[:n], planes)
        torch.cuda.synchronize()
        assert not torch.equal(raw, f32)
        assert torch.equal(sdf, raw[:, 3])
        assert torch.equal(sdf_nor, raw_nor[:, 3])
        minus = torch.full((n,), -1.0, device=dev)
        for out, ins in ((same, inside[:n]), (other, inside_small[:n])):
            assert torch.equal(out[:, :3], raw[:, :3])
            assert torch.equal(out[:, 3], torch.where(ins.to(dev), raw[:, 3], minus))


# ---- 3. exact arithmetic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", lr.EXACT_SHAPES)
def test_exact_arithmetic_points_match_the_plain_oracle(R, S):
    """The points rays_o + rays_d z_vals of lowp_ref.exact_case: nothing that is rounded has anything to round, so the forward
    under points=True is the plain float64 oracle at the float32 parity bar on EVERY point, the saved features bit for bit.
    Forward only: these points sit on texel centres, where the derivative has a kink."""
    from myslam_amd import lowp, ops
    from oracle.eslam_oracle import DECODER_KEYS
    from tests.test_oracle_golden import OUT_RTOL
    dev = _dev()
    c = lr.exact_case(R, S)
    planes = tuple([p.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for p in grp] for grp in c["planes"])
    params = [c["params"][k].to(dev) for k in DECODER_KEYS]
    pts = (c["rays_o"][:, None, :] + c["rays_d"][:, None, :] * c["z_vals"][..., None]).reshape(-1, 3).to(dev)
    with ops.mixed_precision(lowp.HalfPlanes(planes), points=True):
        raw = ops.DecodeFn.apply(pts, ops.bound_to_host(c["bound"]), ops.beta_tensor(10, dev), *hp.flat_planes(planes), *params)
    torch.cuda.synchronize()
    feat = raw.grad_fn.saved_tensors[2]
    o = {k: v.numpy() for k, v in c["oracle"].items()}
    got = feat.float().cpu().numpy()
    assert feat.dtype == torch.bfloat16
    assert np.array_equal(got, o["feat"].astype(np.float32)), f"{int((got != o['feat']).sum())} of {feat.numel()} saved features differ"
    for name, a, want in (("sdf", raw[:, 3], o["sdf"].reshape(-1)), ("raw_rgb", raw[:, :3], o["raw_rgb"].reshape(-1, 3))):
        err = hp.rel_err(_np(a), want)
        ok, info = hp.elementwise_close(_np(a), want, rtol=1e-4, floor=1e-6)
        print(f"exact {R}x{S} points {name}: max-normalised error {err:.2e}, element-wise worst / bar {info[1]:.2e}")
        assert err <= OUT_RTOL, (name, err)
        assert ok, (name, info)


# ---- 4. the copies are what is read ----------------------------------------------------------------------------------------
def test_the_copies_are_read_and_only_when_asked():
    from myslam_amd import lowp, ops
    from myslam_amd.src.utils.Mesher import eval_points
    from oracle import eslam_oracle as orc
    name, n = "trained", 2000
    dev = _dev()
    st = P.state(name)
    planes, dec = _build(name)
    half = lowp.HalfPlanes(planes)                       # copies of A
    with torch.no_grad():
        for q in hp.flat_planes(planes):
            q.mul_(1.5)                                  # the masters move on, no refresh
    p = st["pts"][:n].to(dev)
    mesher = SimpleNamespace(points_batch_size=500000, bound=dec.bound)
    axes = [torch.linspace(float(st["bound"][k, 0]), float(st["bound"][k, 1]), m).to(dev) for k, m in enumerate((9, 7, 70))]
    calls = dict(decode=lambda: dec(p, planes), sdf=lambda: ops.decode_sdf_only(p, ops.bound_to_host(dec.bound), planes, dec),
                 eval=lambda: eval_points(mesher, p, planes, dec), grid=lambda: ops.sdf_grid(planes, dec, axes, dec.bound))
    with torch.no_grad():
        outside = {k: f() for k, f in calls.items()}
        with ops.mixed_precision(half):
            default = {k: f() for k, f in calls.items()}
        with ops.mixed_precision(half, ray_grads=True):
            default_rg = {k: f() for k, f in calls.items()}
        with ops.mixed_precision(half, points=True):
            asked = {k: f() for k, f in calls.items()}
    pg = p.clone().requires_grad_(True)
    with ops.mixed_precision(half, points=True):
        raw = dec(pg, planes)
    feat = _saved_features(raw).float().cpu().numpy()
    with ops.mixed_precision(half):
        raw_default = dec(pg, planes)
    assert _saved_features(raw_default).dtype == torch.float32
    torch.cuda.synchronize()
    for k in calls:
        assert torch.equal(default[k], outside[k]) and torch.equal(default_rg[k], outside[k]), k
        assert not torch.equal(asked[k], outside[k]), k
    assert torch.equal(raw_default, outside["decode"]) and torch.equal(raw.detach(), asked["decode"])
    # outside the context: the float32 field of the SCALED masters
    scaled = tuple([q * 1.5 for q in grp] for grp in st["planes"])
    want = orc.decode(st["pts"][:n], scaled, st["params"], st["bound"])
    assert hp.rel_err(_np(outside["decode"]), want.numpy()) <= 1e-4
    # with points=True: the model on A, whose planes the copies were made from
    got = dict(raw=_np(raw), feat=feat)
    ref, f32 = P.model_pair(name, n, feat, backward=False)
    rep = []
    bad = P.forward_failures(got, ref, f32, P.full_set_figures(name)["cap"], rep) + P.feature_failures(got, name, rep)
    print(f"copies of A, masters x 1.5: " + "; ".join(rep))
    assert not bad, bad


# ---- 5. the grid -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _field():
    from tests.test_gpu_mesh import _field_setup, _ref_points
    from myslam_amd import lowp
    wl, axes = _field_setup()
    _, pts = _ref_points(axes)
    return wl, axes, pts, lowp.HalfPlanes(wl.planes)


def test_sdf_grid_on_the_copies():
    from myslam_amd import _hip, ops
    from myslam_amd.src.utils.Mesher import halfspaces_from_points
    dev = _dev()
    wl, axes, pts, half = _field()
    nx, ny, nz = (len(a) for a in axes)
    assert (nx, ny, nz) == (41, 33, 70)
    gax = [a.to(dev) for a in axes]
    with ops.mixed_precision(half, points=True):
        vol = ops.sdf_grid(wl.planes, wl.decoders, gax, wl.scene.bound)
    f32 = ops.sdf_grid(wl.planes, wl.decoders, gax, wl.scene.bound)
    assert vol.shape == (nx, ny, nz) and not torch.equal(vol, f32)
    # eslam_decode_fwd(SDF_ONLY | MASK_OUTSIDE) with half copies on the materialised points, bit for bit
    lib = _hip.lib()
    p = pts.to(dev)
    geo = tuple(wl.planes[:3]) + tuple(wl.planes[:3])
    arr, _ = _hip.make_planes(tuple([t.detach() for t in g] for g in geo), half=half.flat[:6] + half.flat[:6])
    dec, keep = _hip.make_decoders([t.detach() for t in ops.decoder_params(wl.decoders)], ops.beta_tensor(10, dev))
    raw = torch.empty(p.shape[0], device=dev)
    _hip.check(lib.eslam_decode_fwd(arr, ctypes.byref(dec), _hip.make_bound(ops.bound_to_host(wl.scene.bound)), _hip.ptr(p), p.shape[0], 3,
                                    _hip.ptr(raw), None, _hip.stream_handle(dev)), "eslam_decode_fwd")
    assert torch.equal(vol.reshape(-1), raw)
    b = wl.scene.bound
    inside = ((pts < b[:, 1]) & (pts > b[:, 0])).all(dim=1)
    assert 0.2 < float(inside.float().mean()) < 0.9
    assert torch.equal(vol.reshape(-1).cpu()[~inside], torch.full((int((~inside).sum()),), -1.0))
    # the half-space hull of test_sdf_grid_halfspace_mask: -1 or unchanged on the clear points
    bd = b.double()
    g = torch.Generator().manual_seed(3)
    cloud = (torch.rand(4000, 3, generator=g, dtype=torch.float64) - 0.5) @ torch.tensor(
        [[0.8, 0.5, 0.1], [-0.5, 0.8, 0.2], [0.0, -0.2, 0.9]], dtype=torch.float64)
    cloud = cloud * (bd[:, 1] - bd[:, 0]) * 0.7 + bd.mean(1)
    hs = halfspaces_from_points(cloud, 1.02)
    with ops.mixed_precision(half, points=True):
        cut = ops.sdf_grid(wl.planes, wl.decoders, gax, wl.scene.bound, hs.to(dev)).reshape(-1).cpu()
    plain = vol.reshape(-1).cpu()
    val = pts.double() @ hs[:, :3].T + hs[:, 3]
    outside = (val > 0).any(dim=1)
    clear = (val.abs() > 1e-5).all(dim=1)
    assert 0.1 < float(outside.float().mean()) < 0.9
    assert torch.equal(cut[clear & outside], torch.full((int((clear & outside).sum()),), -1.0))
    assert torch.equal(cut[clear & ~outside], plain[clear & ~outside])
    # the forward sdf criterion against the model, on every fifth point inside the bound (forced with the features DecodeFn
    # saves on them; its sdf is the grid's, bit for bit)
    sel = torch.nonzero(inside).reshape(-1)[::5]
    ps = pts[sel].to(dev).requires_grad_(True)
    with ops.mixed_precision(half, points=True):
        full = wl.decoders(ps, wl.planes)
    torch.cuda.synchronize()
    assert torch.equal(full[:, 3].detach().cpu(), plain[sel])
    feat = _saved_features(full).float().cpu().numpy()
    st = dict(planes=tuple([t.detach().cpu().contiguous() for t in grp] for grp in wl.planes),
              params={k: v.detach().cpu() for k, v in wl.decoders.state_dict().items() if k != "beta"},
              bound=wl.scene.bound.float(), pts=pts[sel], G=torch.zeros(sel.shape[0], 4))
    fig = P.figures(st)
    ref, m32 = P.model_pair(st, None, feat, backward=False)
    rep = []
    bad = [x for x in P.forward_failures(dict(raw=_np(full), feat=feat), ref, m32, fig["cap"], rep) if x.startswith("sdf")]
    print(f"grid, {sel.shape[0]} points: " + "; ".join(r for r in rep if r.startswith("sdf")))
    assert not bad, bad


# ---- 6. the mesh -----------------------------------------------------------------------------------------------------------
def test_extract_mesh_runs_on_the_copies():
    from myslam_amd import ops
    from myslam_amd.src.utils import Mesher as M
    dev = _dev()
    wl, axes, _, half = _field()
    sc = wl.scene
    kf = [dict(est_c2w=wl.c2w.to(dev), depth=torch.full((sc.H, sc.W), 1.6, device=dev))]
    gax = [a.to(dev) for a in axes]
    with ops.mixed_precision(half, points=True):
        vol0 = ops.sdf_grid(wl.planes, wl.decoders, gax, sc.bound)
    level = float(vol0[vol0 > -1].median())               # emit, colours and hull all have work
    m = SimpleNamespace(H=sc.H, W=sc.W, fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy, scale=1.0, resolution=0.1, level_set=level,
                        mesh_bound_scale=1.02, bound=sc.bound, points_batch_size=500000, marching_cubes_bound=sc.bound.double())
    with ops.mixed_precision(half, points=True):
        mesh = M.extract_mesh(m, wl.planes, wl.decoders, kf, device=dev)
        # its parts, issued inside the context
        x, y, z = M.grid_axes(m.marching_cubes_bound, m.resolution)
        ax = [torch.from_numpy(a).float().to(dev) for a in (x, y, z)]
        hull = M.get_bound_from_frames(m, kf, m.scale)
        vol = ops.sdf_grid(wl.planes, wl.decoders, ax, m.bound, hull.halfspaces)
        nohull = ops.sdf_grid(wl.planes, wl.decoders, ax, m.bound)
        verts, faces = ops.marching_cubes(vol, level, (x[0], y[0], z[0]), (x[2] - x[1], y[2] - y[1], z[2] - z[1]))
        colours = M.eval_points(m, verts, wl.planes, wl.decoders)[:, :3]
    mesh32 = M.extract_mesh(m, wl.planes, wl.decoders, kf, device=dev)
    torch.cuda.synchronize()
    assert mesh is not None and mesh32 is not None
    v, f, c = mesh
    print(f"mesh on the copies: V={len(v)} F={len(f)}; float32: V={len(mesh32[0])} F={len(mesh32[1])}")
    assert len(v) > 1000 and len(f) > 1000
    cut = (vol == -1) & (nohull != -1)
    assert 0.05 < float(cut.float().mean()) < 0.95         # the hull took points away, and left some
    assert np.array_equal(v, verts.cpu().numpy()) and np.array_equal(f, faces.cpu().numpy())
    assert np.array_equal(c, colours.cpu().numpy())
    assert mesh32[0].shape != v.shape or not np.array_equal(mesh32[0], v)


# ---- 7. refusals and defaults ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 8000])      # below and above the size at which NCHW planes get per-call scratch copies
def test_nchw_planes_raise(n):
    from myslam_amd import lowp, ops
    from myslam_amd.src.utils.Mesher import eval_points
    dev = _dev()
    st = P.state("trained")
    planes, dec = _build("trained", False, False, channels_last=False)
    half = lowp.HalfPlanes(tuple([q.contiguous(memory_format=torch.channels_last) for q in grp] for grp in planes))
    p = st["pts"][:n].to(dev)
    mesher = SimpleNamespace(points_batch_size=500000, bound=dec.bound)
    axes = [torch.linspace(-1, 1, 5).to(dev)] * 3
    for call in (lambda: dec(p, planes), lambda: dec.get_raw_sdf(p, planes), lambda: dec.get_raw_rgb(p, planes),
                 lambda: ops.decode_sdf_only(p, ops.bound_to_host(dec.bound), planes, dec), lambda: eval_points(mesher, p, planes, dec),
                 lambda: ops.sdf_grid(planes, dec, axes, dec.bound)):
        with torch.no_grad(), ops.mixed_precision(half, points=True):
            with pytest.raises(RuntimeError, match="channels_last"):
                call()
        with torch.no_grad(), ops.mixed_precision(half):
            call()                                           # the default: float32 on the planes as they are
    assert ops._half_planes is None and ops._half_points is False and ops._half_ray_grads is False


def test_flags_are_restored_and_a_late_backward_uses_its_copies():
    from myslam_amd import lowp, ops
    dev = _dev()
    name, n = "trained", 257
    st = P.state(name)
    planes, dec = _build(name, False, False)
    half = lowp.HalfPlanes(planes)
    G = st["G"][:n].to(dev)

    def g_pts(late):
        p = st["pts"][:n].to(dev).requires_grad_(True)
        with ops.mixed_precision(half, points=True):
            assert ops._half_points is True and ops._half_planes is half
            with ops.mixed_precision(half):                  # nested: the inner default switches the points off ...
                assert ops._half_points is False
            assert ops._half_points is True                  # ... and hands the outer state back
            raw = dec(p, planes)
            if not late:
                (raw * G).sum().backward()
        assert ops._half_planes is None and ops._half_points is False and ops._half_ray_grads is False
        if late:
            (raw * G).sum().backward()
        return p.grad.clone()

    inside, late = g_pts(False), g_pts(True)
    p = st["pts"][:n].to(dev).requires_grad_(True)
    (dec(p, planes) * G).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(late, inside)
    assert not torch.equal(late, p.grad)
    try:
        with ops.mixed_precision(half, points=True):
            raise KeyError("leave by an exception")
    except KeyError:
        pass
    assert ops._half_planes is None and ops._half_points is False


def test_slam_backend_asks_for_points():
    from myslam_amd import lowp, ops, scene as scn, slam
    planes, dec = _build("initial", False, False)
    half = lowp.HalfPlanes(planes)
    with slam.HipBackend(scn.make_scene("toy"), _dev()).mixed_precision(half):
        assert ops._half_planes is half and ops._half_points is True and ops._half_ray_grads is True
    assert ops._half_planes is None and ops._half_points is False
