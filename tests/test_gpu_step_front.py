"""eslam_step_front: the front of a training step - the scatter's three ray orders, the clear of the plane-gradient buffer and the
samplers' z_vals - as ONE launch on the step's own stream, where eslam_ray_order_clear (side stream) and eslam_sample_z_all_rng
made two.  1024-thread workgroups in four roles; a depth-less ray is run by one of a workgroup's four 4-wave teams.

Held here: z_vals to eslam_sample_z_all_rng's bits, the orders to eslam_ray_order's keys (the order inside one key's bin is
arbitrary in both), the clear to zero words between intact guards, a whole step through each host glue to the forked front's
results (the `forked_front` keyword selects it), and a process that only ran the new front to having made no side stream.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import helpers as hp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 8192                         # rays ordered by one workgroup (SORT_MAX)
SEG = 1024                           # rays of one segment of the depth-less role (IMP_SEG)
NAN_BITS = 0x7FC00123                # a quiet NaN with a payload: "never written"
PLANES = [(0, 1), (0, 2), (1, 2)]    # axes of orientation 0 (xy), 1 (xz), 2 (yz)
GUARD = 8                            # words in front of and behind the cleared range (32 bytes: the range stays 16-byte aligned)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _leave_the_random_number_state_as_found():
    """This module builds workloads (torch.manual_seed) and keys the in-kernel random numbers (ops.seed): both are process-wide,
    and the in-kernel step counter restarts only when the key changes, so what a LATER test module draws would depend on this
    module having run.  Everything is put back: torch's CPU and GPU generators, the explicit key, the key the counter belongs to,
    the pending flag, and the counter itself."""
    from myslam_amd import ops
    dev = _dev()
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    explicit, key, pending = ops._explicit_seed, dict(ops._rng_key), dict(ops._rng_pending)
    counter = ops._rng_state(dev).clone()
    torch.cuda.synchronize()
    yield
    torch.cuda.synchronize()
    torch.set_rng_state(cpu_state)
    torch.cuda.set_rng_state(gpu_state, dev)
    ops._explicit_seed = explicit
    ops._rng_key.clear()
    ops._rng_key.update(key)
    ops._rng_pending.clear()
    ops._rng_pending.update(pending)
    ops._rng_state(dev).copy_(counter)
    torch.cuda.synchronize()


_workloads = {}


def _workload(channels_last):
    """Planes, decoders and >= 2050 camera rays inside the bound (trained-like state: the importance sampler's weights spread
    over the ray).  Built once per layout and left unchanged."""
    from myslam_amd import harness
    wl = _workloads.get(channels_last)
    if wl is None:
        wl = _workloads[channels_last] = harness.make_workload("room0", 4096, 56, 8, device=_dev(), state="trained",
                                                               channels_last=channels_last)
        assert wl.R >= 2050
    return wl


def _sentinel(shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device=_dev())


def _front(wl, ro, rd, gd, ns, ni, perturb, entry, state, seed=0x1234ABCD5678, offset=0, perm=None, clear=None, clear_bytes=0, z=None):
    """One call of `entry` (eslam_step_front | eslam_sample_z_all_rng) -> (rc, z_vals as int32 bits, perm)."""
    from myslam_amd import _hip, ops
    dev = gd.device
    R = int(gd.shape[0])
    if z is None:
        z = _sentinel((R, ns + ni))
    if perm is None and entry == "eslam_step_front":
        perm = torch.full((_hip.ray_order_words(R),), -1, dtype=torch.int32, device=dev)
    t_free, t_surf = ops.linspace01(ns, dev), ops.linspace01(ni, dev)
    arr, _ = _hip.make_planes(wl.plane_list)
    dec, keep = _hip.make_decoders(ops.decoder_params(wl.decoders), ops.beta_tensor(wl.decoders.beta, dev))
    head = (arr, ctypes.byref(dec), _hip.make_bound(wl.renderer._bound6), _hip.ptr(ro), _hip.ptr(rd), _hip.ptr(gd), R, ns, ni,
            float(wl.truncation), _hip.ptr(t_free), _hip.ptr(t_surf), 1 if perturb else 0, seed, _hip.ptr(state), offset, _hip.ptr(z))
    with _hip.on_device(dev):
        st = _hip.stream_handle(dev)
        if entry == "eslam_step_front":
            rc = _hip.lib().eslam_step_front(*head, _hip.ptr(perm), None if clear is None else ctypes.c_void_p(clear), clear_bytes, st)
        else:
            rc = _hip.lib().eslam_sample_z_all_rng(*head, st)
    torch.cuda.synchronize()
    return rc, z, perm


def _depth_patterns(R, base):
    """name -> gt_depth [R] (host): `base` (all > 0) with depth-less rays (0) placed to load the teams of a workgroup unevenly."""
    g = torch.Generator().manual_seed(4242 + R)
    out = {"none": base.clone(), "all": torch.zeros(R)}
    d = base.clone()
    d[torch.rand(R, generator=g) < 0.10] = 0.0
    out["ten_percent"] = d
    # segments that hold exactly 1 and exactly 5 depth-less rays (one team works while three idle; two trips' worth for one team
    # of a workgroup and one for the next), alternating over the segments
    d = base.clone()
    for s, lo in enumerate(range(0, R, SEG)):
        n = min(SEG, R - lo)
        k = min(n, 1 if s % 2 == 0 else 5)
        d[lo + torch.randperm(n, generator=g)[:k]] = 0.0
    out["one_and_five"] = d
    d = base.clone()
    for s, lo in enumerate(range(0, R, SEG)):
        n = min(SEG, R - lo)
        k = min(n, 5 if s % 2 == 0 else 1)
        d[lo + torch.randperm(n, generator=g)[:k]] = 0.0
    out["five_and_one"] = d
    # all of a segment's depth-less rays at its end
    d = base.clone()
    for lo in range(0, R, SEG):
        hi = min(R, lo + SEG)
        d[max(lo, hi - 37):hi] = 0.0
    out["segment_tail"] = d
    return out


@pytest.mark.parametrize("channels_last", [True, False], ids=["channels_last", "nchw"])
@pytest.mark.parametrize("ns,ni", [(56, 8), (88, 8), (3, 1)])
def test_z_vals_are_the_samplers_bits(ns, ni, channels_last):
    """Every row of z_vals, bit for bit, against eslam_sample_z_all_rng with the same seed, step and ray offset: all R of the
    issue, depth-less shares 0 / 10 % / 100 %, unevenly loaded teams, depth-less rays at a segment's end, a ray whose AABB exit is
    0/0 (its row is NaN in both), jitter on and off, each call made twice."""
    wl = _workload(channels_last)
    dev = wl.device
    state = torch.tensor([5, 0, 0, 0], dtype=torch.int32, device=dev)           # step 5
    b = wl.renderer._bound6
    for R in (1, 15, 16, 17, 1023, 1025, 2050):
        ro, rd = wl.rays_o[:R].detach().clone(), wl.rays_d[:R].detach().clone()
        base = wl.gt_depth[:R].detach().cpu().clone()
        assert bool((base > 0).all())
        pats = _depth_patterns(R, base)
        # the 0/0 exit: ray 7 starts exactly on the x-max face with no x component (tests/hostile_rays.py class 8).  It is
        # depth-less in a pattern of its own and wherever a pattern makes it so; "none" stays without a single depth-less ray
        # (every depth-less workgroup takes its early exit, rows only), and the 1 / 5 counts per segment stay exact
        if R >= 15:
            ro[7] = torch.tensor([b[1], 0.5 * (b[2] + b[3]), 0.5 * (b[4] + b[5])], device=dev)
            rd[7] = torch.tensor([0.0, 0.3, -1.0], device=dev)
            pats["nan_exit"] = base.clone()
            pats["nan_exit"][7] = 0.0
        assert int((pats["none"] <= 0).sum()) == 0
        for lo in range(0, R, SEG):
            n, s = min(SEG, R - lo), lo // SEG
            assert int((pats["one_and_five"][lo:lo + n] <= 0).sum()) == min(n, 1 if s % 2 == 0 else 5)
            assert int((pats["five_and_one"][lo:lo + n] <= 0).sum()) == min(n, 5 if s % 2 == 0 else 1)
        for name, d in pats.items():
            gd = d.to(dev)
            for perturb in (True, False):
                rc0, want, _ = _front(wl, ro, rd, gd, ns, ni, perturb, "eslam_sample_z_all_rng", state, offset=3)
                assert rc0 == 0
                assert not bool((want == NAN_BITS).any()), ("the reference sampler left elements unwritten", R, name)
                for rep in range(2):
                    rc, got, perm = _front(wl, ro, rd, gd, ns, ni, perturb, "eslam_step_front", state, offset=3)
                    assert rc == 0
                    bad = (got != want).any(dim=1).nonzero().flatten()
                    assert bad.numel() == 0, (R, name, perturb, rep, "rows differ", bad[:8].tolist(), "depth-less?", (gd[bad[:8]] <= 0).tolist())
                if R >= 15 and float(d[7]) <= 0:
                    assert bool(torch.isnan(want[7].view(torch.float32)).all()), "the 0/0 ray's row is expected to be NaN"


# ---- orders -------------------------------------------------------------------------------------------------------------------
def _fan(cameras, R, camera_major, seed):
    """A pinhole-like fan of R directions from `cameras` origins -> (rays_o, rays_d on the GPU; origins, directions, camera ids on the host)."""
    g = torch.Generator().manual_seed(seed)
    org = torch.randn(cameras, 3, generator=g)
    cam = torch.randint(cameras, (R,), generator=g)
    if camera_major:
        cam, _ = torch.sort(cam)
    d = torch.randn(R, 3, generator=g) * 0.35
    d[:, 2] = -1.0
    return org[cam].to(_dev()).contiguous(), d.to(_dev()).contiguous(), org[cam], d, cam


def _orders(R, cameras, camera_major, seed):
    """-> (perm of eslam_step_front, perm of eslam_ray_order, origins, directions, camera ids), all on the host."""
    from myslam_amd import _hip
    wl = _workload(True)
    dev = wl.device
    ro, rd, o, d, cam = _fan(cameras, R, camera_major, seed)
    gd = torch.ones(R, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    rc, z, perm = _front(wl, ro, rd, gd, 16, 4, True, "eslam_step_front", state)
    assert rc == 0
    assert not bool((z == NAN_BITS).any())
    perm0 = torch.full((_hip.ray_order_words(R),), -1, dtype=torch.int32, device=dev)
    with _hip.on_device(dev):
        assert _hip.lib().eslam_ray_order(_hip.ptr(ro), _hip.ptr(rd), R, _hip.ptr(perm0), _hip.stream_handle(dev)) == 0
    torch.cuda.synchronize()
    perm, perm0 = perm.cpu(), perm0.cpu()
    for p in (perm, perm0):
        for k in range(3):
            q = p[k * R:(k + 1) * R].long()
            for lo in range(0, R, CHUNK):                        # chunks are ordered independently
                hi = min(R, lo + CHUNK)
                assert torch.equal(torch.sort(q[lo:hi]).values, torch.arange(lo, hi)), (k, lo)
    assert torch.equal(perm[3 * R:3 * R + 3], perm0[3 * R:3 * R + 3]), (perm[3 * R:3 * R + 3].view(torch.float32), perm0[3 * R:3 * R + 3].view(torch.float32))
    return perm.numpy().astype(np.int64), perm0.numpy().astype(np.int64), o.double().numpy(), d.double().numpy(), cam.numpy()


def _azimuth(d, sel, a, b):
    """float64 azimuth, in plane (a, b), of the directions d[sel] about the projected sum of their unit vectors (what the kernel keys on)."""
    u = d[sel] / np.linalg.norm(d[sel], axis=1, keepdims=True)
    m = u.sum(0)
    return np.arctan2(m[a] * u[:, b] - m[b] * u[:, a], m[a] * u[:, a] + m[b] * u[:, b])


@pytest.mark.parametrize("R", [200, 1024, 1025, 4096, 8193])
def test_orders_one_origin(R):
    """Three permutations per chunk from both entries, fan extents bit-equal, and along the two orders the float64 azimuths agree
    element by element to one key bin (extent / 2^key_bits; 12 bits up to 1024 rays in the chunk, else 14)."""
    perm, perm0, _, d, _ = _orders(R, 1, True, 2000 + R)
    for lo in range(0, R, CHUNK):
        hi = min(R, lo + CHUNK)
        n = hi - lo
        key_bits = 12 if min(R, CHUNK) <= 1024 else 14
        for k, (a, b) in enumerate(PLANES):
            ang = np.zeros(R)
            ang[lo:hi] = _azimuth(d, slice(lo, hi), a, b)
            tol = (ang[lo:hi].max() - ang[lo:hi].min()) / 2.0 ** key_bits
            new, old = ang[perm[k * R + lo:k * R + hi]], ang[perm0[k * R + lo:k * R + hi]]
            worst = float(np.abs(new - old).max())
            print(f"order {k} chunk {lo // CHUNK} of R={R}: {n} rays, max |azimuth new - old| = {worst:.3e}, one bin = {tol:.3e}")
            assert worst <= tol, (k, lo, worst, tol)


def test_orders_two_cameras():
    """A camera-major batch of two cameras: key = (camera, azimuth about the camera's own mean direction), 1 + 13 bits."""
    R = 3000
    perm, perm0, _, d, cam = _orders(R, 2, True, 2222)
    abits = 14 - 1
    for k, (a, b) in enumerate(PLANES):
        new, old = perm[k * R:(k + 1) * R], perm0[k * R:(k + 1) * R]
        assert np.array_equal(cam[new], cam[old]), k
        assert bool((np.diff(cam[new]) >= 0).all()), k
        for c in range(2):
            sel = np.nonzero(cam == c)[0]
            ang = np.zeros(R)
            ang[sel] = _azimuth(d, sel, a, b)
            tol = (ang[sel].max() - ang[sel].min()) / 2.0 ** abits
            worst = float(np.abs(ang[new[cam[new] == c]] - ang[old[cam[old] == c]]).max())
            print(f"order {k} camera {c}: max |azimuth new - old| = {worst:.3e}, one bin = {tol:.3e}")
            assert worst <= tol, (k, c, worst, tol)


def test_orders_33_cameras_morton():
    """More cameras than the per-camera key holds (32): a Morton key of the point one metre along the ray (4 bits per axis at 14
    key bits), the same for the three orders.  The keys along the two entries' orders are equal element by element."""
    R = 33 * 40
    perm, perm0, o, d, _ = _orders(R, 33, True, 3333)
    p = (o + d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    lo, hi = p.min(0), p.max(0)
    q = np.minimum(np.maximum((p - lo) * (np.float32(16.0) / np.maximum(hi - lo, np.float32(1e-6))), 0).astype(np.int64), 15)
    key = np.zeros(R, dtype=np.int64)
    for bit in range(4):
        for ax in range(3):
            key |= ((q[:, ax] >> bit) & 1) << (3 * bit + ax)
    for k in range(3):
        new, old = key[perm[k * R:(k + 1) * R]], key[perm0[k * R:(k + 1) * R]]
        assert np.array_equal(new, old), (k, int((new != old).sum()))
        assert int((np.diff(old) < 0).sum()) <= 2, "the model's Morton keys are not those the kernel sorts by"


# ---- clear --------------------------------------------------------------------------------------------------------------------
def _nan_buffer(words):
    return _sentinel((GUARD + words + GUARD,))


def _small_call(clear, clear_bytes, null_rays=False):
    """eslam_step_front on 77 rays (some depth-less) with a buffer to clear; null_rays: rays_o = NULL."""
    wl = _workload(True)
    R = 77
    gd = wl.gt_depth[:R].detach().clone()
    gd[::9] = 0.0
    state = torch.zeros(4, dtype=torch.int32, device=wl.device)
    return _front(wl, None if null_rays else wl.rays_o[:R].detach(), wl.rays_d[:R].detach(), gd, 16, 4, True, "eslam_step_front", state,
                  clear=clear, clear_bytes=clear_bytes)


@pytest.mark.parametrize("clear_bytes", [0, 4, 65540, 3 * 1024 * 1024 + 12])
def test_clear_zeroes_its_range_and_nothing_else(clear_bytes):
    words = clear_bytes // 4
    buf = _nan_buffer(words)
    start = buf.data_ptr() + 4 * GUARD
    assert start % 16 == 0
    rc, z, perm = _small_call(start, clear_bytes)
    assert rc == 0
    assert not bool((z == NAN_BITS).any())
    for k in range(3):
        assert torch.equal(torch.sort(perm[k * 77:(k + 1) * 77].cpu().long()).values, torch.arange(77)), k
    assert bool((buf[GUARD:GUARD + words] == 0).all()), int((buf[GUARD:GUARD + words] != 0).sum())
    assert bool((buf[:GUARD] == NAN_BITS).all()) and bool((buf[GUARD + words:] == NAN_BITS).all()), "guard words changed"


def test_bad_arguments_are_refused_before_anything_is_launched():
    from myslam_amd import _hip
    buf = _nan_buffer(64)
    start = buf.data_ptr() + 4 * GUARD
    before = buf.clone()
    cases = ((start + 4, 64, False, "misaligned pointer"), (start, -16, False, "negative length"), (start, 64, True, "null rays"))
    for ptr, nbytes, null_rays, why in cases:
        rc, z, perm = _small_call(ptr, nbytes, null_rays=null_rays)
        assert rc != 0, why
        msg = _hip.lib().eslam_last_error()
        assert msg and b"eslam_step_front" in msg, (why, msg)
        assert torch.equal(buf, before), (why, "the clear ran although the call failed")
        assert bool((perm == -1).all()), (why, "the order ran although the call failed")
        assert bool((z == NAN_BITS).all()), (why, "the sampler ran although the call failed")


# ---- a whole step through each host glue ---------------------------------------------------------------------------------------
def _poison_gradient_memory(wl):
    """Fill the memory the next step's gradient buffer comes from with NaN: the buffers the Python glue keeps for reuse, and a
    block of the buffer's size handed back to the caching allocator (what the next allocation of that size is then given)."""
    from myslam_amd import ops
    for flat, _ in ops._grad_reuse.values():
        flat.fill_(float("nan"))
    total = sum(p.numel() for p in wl.plane_list)
    junk = torch.full((total,), float("nan"), device=wl.device)
    del junk


def _step(wl, R, forked, seed=77):
    from myslam_amd import losses, ops
    dev = wl.device
    for p in wl.params():
        p.grad = None
    _poison_gradient_memory(wl)
    ops.seed(seed)
    try:
        sl = slice(0, R)
        gd, gc = wl.gt_depth[sl], wl.gt_color[sl]
        d, c, s, z, pre = wl.renderer.render_batch_ray_with_loss(wl.planes, wl.decoders, wl.rays_d[sl], wl.rays_o[sl], dev, wl.truncation,
                                                                 gd, gc, losses.MAPPING_W, forked_front=forked)
        loss = losses.mapping_loss(d, c, s, z, gd, gc, wl.truncation, precomputed=pre)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.seed(None)
    cp = lambda t: t.detach().cpu().clone()
    out = dict(depth=cp(d), rgb=cp(c), sdf=cp(s), z=cp(z), loss=cp(loss), planes=[cp(p.grad) for p in wl.plane_list],
               dec={k: cp(t.grad) for k, t in wl.decoders.named_parameters() if t.grad is not None})
    for p in wl.params():
        p.grad = None
    return out


def _spread(a, b):
    return max(hp.rel_err(x.double().numpy(), y.double().numpy()) for x, y in zip(a["planes"], b["planes"]))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _compare_fronts(wl, R, glue):
    """Old front twice, new front once, on NaN-filled gradient memory.  -> nothing; asserts."""
    old0, old1, new = _step(wl, R, True), _step(wl, R, True), _step(wl, R, False)
    for r in (old0, new):
        assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in r["planes"]), (glue, "plane gradients")
    for k in ("depth", "rgb", "sdf", "z"):
        assert torch.equal(_bits(new[k]), _bits(old0[k])), (glue, k)
    assert set(new["dec"]) == set(old0["dec"]) and "beta" in new["dec"]
    bad = [k for k in new["dec"] if not torch.equal(_bits(new["dec"][k]), _bits(old0["dec"][k]))]
    assert not bad, (glue, "decoder / beta gradients differ between the fronts", bad)
    # the loss: float32 sums over the rays formed with atomics in the forward's epilogue, so held to the forked front's own run
    # to run difference with a floor of a few float32 roundings (1e-6 relative)
    l0, l1, ln = float(old0["loss"]), float(old1["loss"]), float(new["loss"])
    lbar = max(4.0 * abs(l1 - l0), 1e-6 * abs(l0))
    print(f"margin step front {R} rays ({glue}): loss old {l0:.9g} / {l1:.9g}, new {ln:.9g} (bar {lbar:.1e})")
    assert abs(ln - l0) <= lbar, (glue, ln, l0, lbar)
    x = _spread(old0, old1)
    bar = max(1e-5, 4.0 * x)
    e = _spread(new, old0)
    print(f"margin step front {R} rays ({glue}): old front run to run x = {x:.3e}, new against old {e:.3e} (bar {bar:.1e})")
    assert e <= bar, (glue, e, bar, x)


@pytest.mark.parametrize("R,ns,ni", [(256, 16, 4), (1024, 56, 8)])
def test_step_through_both_glues_new_front_against_old(R, ns, ni, monkeypatch):
    """depth, rgb, sdf, z_vals, the loss, decoder and beta gradients: the forked front's bits.  Plane gradients (float atomics in
    the scatter; the order inside a key's bin is arbitrary): within max(1e-5, 4 x) of the forked front's, x = what two runs of the
    FORKED front differ by (max-normalised) - tests/test_gpu_ray_order_clear.py's bound."""
    from myslam_amd import harness, ops
    ext = ops.torch_ext()
    assert ext is not None, "eslam_torch_ext is not built"
    wl = harness.make_workload("room0", 4 * R, ns, ni, device=_dev(), state="trained", zero_frac=0.1)
    assert wl.R >= R
    assert int((wl.gt_depth[:R] <= 0).sum()) > 0, "the step is meant to hold depth-less rays"
    for glue, mod in (("python", None), ("compiled", ext)):
        monkeypatch.setattr(ops, "_ext_mod", mod)
        _compare_fronts(wl, R, glue)


_CHILD_DET = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from myslam_amd import harness, ops
from tests.test_gpu_step_front import _step
ext = ops.torch_ext()
assert ext is not None
wl = harness.make_workload("room0", 1024, 16, 4, device=torch.device("cuda:0"), state="trained", zero_frac=0.1)
R = 256
for glue, mod in (("python", None), ("compiled", ext)):
    ops._ext_mod = mod
    old, new = _step(wl, R, True), _step(wl, R, False)
    for i, (a, b) in enumerate(zip(old["planes"], new["planes"])):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, (glue, i)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (glue, "plane", i, float((a - b).abs().max()))
print("DET-OK")
"""

_CHILD_NO_SIDE = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from myslam_amd import harness, ops
ext = ops.torch_ext()
assert ext is not None
wl = harness.make_workload("room0", 1024, 16, 4, device=torch.device("cuda:0"), state="trained", zero_frac=0.1)
for mod in (None, ext):
    ops._ext_mod = mod
    for _ in range(2):
        wl.step()
    torch.cuda.synchronize()
    g = harness.GraphedStep(wl.step, wl.params())
    for _ in range(3):
        g()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in wl.plane_list)
    del g
assert ops._side_streams == {}, ops._side_streams
assert ext.side_streams_created() == 0, ext.side_streams_created()
print("NO-SIDE-OK")
"""


def _child(code, env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-c", code, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_deterministic_mode_plane_gradients_are_bit_equal():
    """A fresh process in deterministic mode (fixed-point sums in the scatter: neither the order inside a bin nor the order of the
    atomics can change a bit): the plane gradients of the new front are the forked front's, through both glues."""
    assert "DET-OK" in _child(_CHILD_DET, {"ESLAM_DETERMINISTIC": "1"})


def test_new_front_creates_no_side_stream():
    """A fresh process that only runs new-front steps, eager and replayed from a captured graph, through both glues: the Python
    glue holds no side stream afterwards and the compiled glue reports that it created none."""
    assert "NO-SIDE-OK" in _child(_CHILD_NO_SIDE, {})
