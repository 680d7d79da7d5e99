"""eslam_ray_order_clear: the ray orders of the backward's scatter and the clear of the iteration's plane-gradient buffer as ONE
launch (ordering workgroups in front, clearing workgroups behind them), which both host glues call at the head of the side
stream instead of eslam_zero_async followed by eslam_ray_order.

The orders are held to the properties tests/test_gpu_callers.py::test_ray_order_is_a_permutation_and_groups_neighbours holds
eslam_ray_order to (the order inside one key's cell is arbitrary, so two launches need not agree element by element), the fan
extents to eslam_ray_order's own bits, the clear to zero words between intact guards, and a whole step through each glue to its
own run-to-run spread.
"""
import ctypes

import pytest
import torch

from tests import helpers as hp

pytestmark = pytest.mark.gpu
CHUNK = 8192                         # rays ordered by one workgroup (SORT_MAX in csrc/eslam_ray_order_dev.h)
NAN_BITS = 0x7FC00123                # a quiet NaN with a payload: what an uncleared gradient buffer is filled with here
PLANES = [(0, 1), (0, 2), (1, 2)]    # axes of orientation 0 (xy), 1 (xz), 2 (yz)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _rays(cameras, R, camera_major, seed):
    """A pinhole-like fan of R directions from `cameras` origins -> (rays_o, rays_d on the GPU, directions and camera ids on the host)."""
    g = torch.Generator().manual_seed(seed)
    org = torch.randn(cameras, 3, generator=g)
    cam = torch.randint(cameras, (R,), generator=g)
    if camera_major:
        cam, _ = torch.sort(cam)
    d = torch.randn(R, 3, generator=g) * 0.35
    d[:, 2] = -1.0
    return org[cam].to(_dev()).contiguous(), d.to(_dev()).contiguous(), d, cam


def _call(ro, rd, clear=None, clear_bytes=0, perm=None, entry="eslam_ray_order_clear"):
    """-> (return code, perm).  clear: an integer address or None."""
    from myslam_amd import _hip
    dev = ro.device
    R = int(ro.shape[0])
    if perm is None:
        perm = torch.full((_hip.ray_order_words(R),), -1, dtype=torch.int32, device=dev)
    with _hip.on_device(dev):
        st = _hip.stream_handle(dev)
        if entry == "eslam_ray_order":
            rc = _hip.lib().eslam_ray_order(_hip.ptr(ro), _hip.ptr(rd), R, _hip.ptr(perm), st)
        else:
            rc = _hip.lib().eslam_ray_order_clear(_hip.ptr(ro), _hip.ptr(rd), R, _hip.ptr(perm),
                                                  None if clear is None else ctypes.c_void_p(clear), clear_bytes, st)
    torch.cuda.synchronize()
    return rc, perm


def _check_permutations(perm, R):
    for o in range(3):
        p = perm[o * R:(o + 1) * R].cpu().long()
        for lo in range(0, R, CHUNK):                            # chunks are ordered independently
            hi = min(R, lo + CHUNK)
            assert torch.equal(torch.sort(p[lo:hi]).values, torch.arange(lo, hi)), (o, lo)


@pytest.mark.parametrize("R", [1, 63, 77, 1025, 4096, 8192, 8193])
def test_one_origin_orders_by_azimuth(R):
    """Three permutations per chunk; within the first chunk the azimuth in the order's plane is non-decreasing up to the key's
    quantisation with at most one seam; the fan extents are the bits eslam_ray_order writes for the same rays."""
    ro, rd, d, _ = _rays(1, R, True, 1000 + R)
    rc, perm = _call(ro, rd)
    assert rc == 0
    assert perm.numel() == 3 * R + 4
    _check_permutations(perm, R)
    rc0, perm0 = _call(ro, rd, entry="eslam_ray_order")
    assert rc0 == 0
    _check_permutations(perm0, R)
    fan, fan0 = perm[3 * R:3 * R + 3].cpu(), perm0[3 * R:3 * R + 3].cpu()
    assert torch.equal(fan, fan0), (fan.view(torch.float32), fan0.view(torch.float32))
    fanf = fan.view(torch.float32)
    if R >= 1000:
        assert bool((fanf > 0.1).all()) and bool((fanf < 6.3).all())
    n1 = min(R, CHUNK)
    m = torch.nn.functional.normalize(d[:n1], dim=1).sum(0)      # the first chunk's own mean direction
    for o, (a, b) in enumerate(PLANES):
        p = perm[o * R:o * R + n1].cpu().long()
        ang = torch.atan2(m[a] * d[:, b] - m[b] * d[:, a], m[a] * d[:, a] + m[b] * d[:, b])
        if n1 >= 2:
            assert int(((ang[p[1:]] - ang[p[:-1]]) < -2e-3).sum()) <= 1, o
        if n1 >= 1000:
            step_sorted = (ang[p[1:]] - ang[p[:-1]]).abs().mean()
            step_given = (ang[1:n1] - ang[:n1 - 1]).abs().mean()
            assert float(step_sorted) < 0.02 * float(step_given), o


def test_camera_major_origins_stay_together_and_random_origins_are_permuted():
    cameras, R = 3, 3000
    ro, rd, d, cam = _rays(cameras, R, True, 3003)
    rc, perm = _call(ro, rd)
    assert rc == 0
    _check_permutations(perm, R)
    assert float(perm[3 * R:3 * R + 3].view(torch.float32).abs().max()) == 0.0       # several origins: no single fan
    dn = torch.nn.functional.normalize(d, dim=1)
    for o, (a, b) in enumerate(PLANES):
        p = perm[o * R:(o + 1) * R].cpu().long()
        assert bool((cam[p][1:] >= cam[p][:-1]).all())                              # cameras stay together, in their order
        for c in range(cameras):
            sel = p[cam[p] == c]
            assert len(sel) >= 50
            m = dn[cam == c].sum(0)
            ang = torch.atan2(m[a] * d[sel, b] - m[b] * d[sel, a], m[a] * d[sel, a] + m[b] * d[sel, b])
            assert int(((ang[1:] - ang[:-1]) < -0.05).sum()) <= 1                   # sorted up to the key's quantisation, one wrap at most
    # origins in random order: a Morton order, the same for the three planes up to the order inside a key's cell
    ro, rd, _, _ = _rays(cameras, R, False, 3004)
    rc, perm = _call(ro, rd)
    assert rc == 0
    _check_permutations(perm, R)
    assert float(perm[3 * R:3 * R + 3].view(torch.float32).abs().max()) == 0.0
    rc0, perm0 = _call(ro, rd, entry="eslam_ray_order")
    assert rc0 == 0 and torch.equal(perm[3 * R:3 * R + 3], perm0[3 * R:3 * R + 3])


GUARD = 8                            # words in front of and behind the cleared range (32 bytes: the range stays 16-byte aligned)


def _nan_buffer(words):
    bits = NAN_BITS - (1 << 32) if NAN_BITS >= (1 << 31) else NAN_BITS
    return torch.full((GUARD + words + GUARD,), bits, dtype=torch.int32, device=_dev())


@pytest.mark.parametrize("clear_bytes", [0, 4, 60, 64, 4 * 1024 * 1024 + 4])
def test_clear_zeroes_its_range_and_nothing_else(clear_bytes):
    words = clear_bytes // 4
    ro, rd, _, _ = _rays(1, 77, True, 5)
    buf = _nan_buffer(words)
    start = buf.data_ptr() + 4 * GUARD
    assert start % 16 == 0
    rc, perm = _call(ro, rd, clear=start, clear_bytes=clear_bytes)
    assert rc == 0
    _check_permutations(perm, 77)
    assert bool((buf[GUARD:GUARD + words] == 0).all()), int((buf[GUARD:GUARD + words] != 0).sum())
    assert bool((buf[:GUARD] == buf[0]).all()) and bool((buf[GUARD + words:] == buf[0]).all()) and int(buf[0]) != 0, "guard words changed"
    assert bool(torch.isnan(buf[:GUARD].view(torch.float32)).all())


def test_null_pointer_orders_only_and_bad_clear_arguments_launch_nothing():
    from myslam_amd import _hip
    ro, rd, _, _ = _rays(1, 77, True, 6)
    rc, perm = _call(ro, rd, clear=None, clear_bytes=0)
    assert rc == 0
    _check_permutations(perm, 77)
    buf = _nan_buffer(64)
    start = buf.data_ptr() + 4 * GUARD
    before = buf.clone()
    for ptr, nbytes, why in ((start + 4, 64, "misaligned pointer"), (start, 6, "bytes not a multiple of 4"), (None, 64, "null pointer with bytes")):
        rc, perm = _call(ro, rd, clear=ptr, clear_bytes=nbytes)
        assert rc != 0, why
        msg = _hip.lib().eslam_last_error()
        assert msg and b"eslam_ray_order_clear" in msg, (why, msg)
        assert torch.equal(buf, before), why
        assert bool((perm == -1).all()), (why, "the order ran although the call failed")


# ---- a whole step through each host glue ---------------------------------------------------------------------------------------
def _poison_gradient_memory(wl):
    """Fill the memory the next step's gradient buffer comes from with NaN: the buffers the Python glue keeps for reuse, and a
    block of the buffer's size handed back to the caching allocator (what the compiled glue's allocation is then given)."""
    from myslam_amd import ops
    for flat, _ in ops._grad_reuse.values():
        flat.fill_(float("nan"))
    total = sum(p.numel() for p in wl.plane_list)
    junk = torch.full((total,), float("nan"), device=wl.device)
    del junk


def _step(wl, R, seed=77):
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
                                                                 gd, gc, losses.MAPPING_W)
        loss = losses.mapping_loss(d, c, s, z, gd, gc, wl.truncation, precomputed=pre)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.seed(None)
    cp = lambda t: t.detach().cpu().clone()
    out = dict(z=cp(z), planes=[cp(p.grad) for p in wl.plane_list], dec={k: cp(t.grad) for k, t in wl.decoders.named_parameters()})
    for p in wl.params():
        p.grad = None
    return out


def _spread(a, b):
    return max(hp.rel_err(x.double().numpy(), y.double().numpy()) for x, y in zip(a["planes"], b["planes"]))


@pytest.mark.parametrize("state", ["initial", "trained"])
def test_step_through_both_glues(state, monkeypatch):
    """512 x 32.  Each glue, run three times on gradient memory filled with NaN beforehand: every plane gradient is finite and
    non-zero, and the third run is within max(1e-5, 4 x) of the first, x = what the first two runs differ by (max-normalised; the
    scatter's float atomics).  The compiled glue's run is within the Python glue's bar of the Python glue's, z_vals are equal, and
    the decoder gradients of the two glues are equal bit for bit."""
    from myslam_amd import harness, ops
    ext = ops.torch_ext()
    assert ext is not None, "eslam_torch_ext is not built"
    R, ns, ni = 512, 24, 8
    wl = harness.make_workload("room0", 4 * R, ns, ni, device=_dev(), state=state)
    assert wl.R >= R
    runs = {}
    for glue, mod in (("python", None), ("compiled", ext)):
        monkeypatch.setattr(ops, "_ext_mod", mod)
        r0, r1, r2 = _step(wl, R), _step(wl, R), _step(wl, R)
        for r in (r0, r1, r2):
            assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in r["planes"]), (glue, "plane gradients")
            assert all(bool(torch.isfinite(g).all()) for g in r["dec"].values()), glue
        x = _spread(r0, r1)
        bar = max(1e-5, 4.0 * x)
        e = _spread(r2, r0)
        print(f"margin ray order + clear {state} ({glue}): x = {x:.3e}, third run {e:.3e} (bar {bar:.1e})")
        assert e <= bar, (glue, e, bar, x)
        assert torch.equal(r0["z"], r2["z"])
        runs[glue] = (r0, bar)
    (py, bar), (cx, _) = runs["python"], runs["compiled"]
    e = _spread(cx, py)
    print(f"margin ray order + clear {state}: compiled against python {e:.3e} (bar {bar:.1e})")
    assert e <= bar, (e, bar)
    assert torch.equal(py["z"], cx["z"])
    bad = [k for k in py["dec"] if not torch.equal(py["dec"][k], cx["dec"][k])]
    assert not bad, ("decoder gradients differ between the glues", bad)
