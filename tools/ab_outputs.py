"""A/B check of two builds of the library on identical inputs: dump outputs + gradients of a list of configurations
(python tools/ab_outputs.py dump out.npz, once per build via ESLAM_HIP_LIB), then `compare a.npz b.npz` (relative difference
beyond 1e-5), `compare a.npz b.npz exact` (every array whose bytes differ: what two ESLAM_DETERMINISTIC=1 dumps must not have) or
`compare a.npz b.npz strict` (bytes for everything that does not pass through float atomics - outputs, z, decoder, beta, ray and
point gradients, the dispatch flags - and 1e-5 for the plane gradients and the loss values).

The first nine configurations are whole workloads (float32 rays, trainable decoders).  The small ones behind them walk the
decoder backward's dispatch: across a default and a deterministic dump every one of the 24 mlp_bwd_kernel instantiations runs at
least once - frozen decoders, rays that take gradients, no saved hidden layer, the unfused loss, mixed precision, free points -
and each dumps eslam_last_backward_rank16 / _saved_hidden, so that a change of dispatch shows up as a difference."""
import re, sys, os, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIGS = [("toy", 999, 32, 8, 0.0), ("toy", 497, 32, 8, 0.0), ("toy", 333, 32, 8, 0.1), ("toy", 1000, 16, 8, 0.0),
           ("room0", 200, 24, 8, 0.0), ("room0", 1001, 56, 8, 0.0), ("room0", 301, 88, 8, 0.1), ("room0", 77, 8, 4, 0.0),
           ("room0", 130, 120, 8, 0.0)]
# rays: R = 5 with S = 20 (one chunk whose second block is a quarter full) and S = 72 (two chunks, the second partial)
RAY_SHAPES = ((5, 12, 8), (5, 64, 8))
# (precision, loss, frozen decoders, rays take gradients, saved hidden layer); default mode runs the float32 ones without ray
# gradients on the rank-16 pair, deterministic mode on full-width rows
RAY_VARIANTS = [("f32", loss, frozen, False, saved) for loss in ("fused", "separate") for frozen in (False, True) for saved in (True, False)]
RAY_VARIANTS += [("f32", "fused", False, True, True), ("f32", "separate", True, True, False)]
RAY_VARIANTS += [("lowp", loss, frozen, False, True) for loss in ("fused", "separate") for frozen in (False, True)]
RAY_VARIANTS += [("lowp", "fused", False, True, True), ("lowp", "separate", True, True, True)]
# free points: N = 70 (two tiles, the second with 6 points)
POINT_VARIANTS = [(prec, frozen) for prec in ("f32", "lowp") for frozen in (False, True)]
SMALL = [("rays",) + s + v for v in RAY_VARIANTS for s in RAY_SHAPES] + [("points", 70) + v for v in POINT_VARIANTS]
ALL = CONFIGS + SMALL


def _flags(out, tag):
    from myslam_amd import _hip
    lib = _hip.lib()
    out[f"{tag}_flag_rank16"] = np.array(lib.eslam_last_backward_rank16())
    out[f"{tag}_flag_saved_hidden"] = np.array(lib.eslam_last_backward_saved_hidden())


def _small_workload(dev, R, ns, ni, rays_grad, frozen):
    import torch
    from myslam_amd import harness
    wl = harness.Workload("room0", 4 * R, ns, ni, dev, planes="synth", state="trained", rays_grad=rays_grad)      # (the AABB pre-filter drops some rays)
    assert wl.R >= R, (wl.R, R)
    for p in wl.decoders.parameters():
        p.requires_grad_(not frozen)
    return wl


def _dump_grads(out, tag, wl):
    for j, p in enumerate(wl.plane_list):
        out[f"{tag}_pg{j}"] = p.grad.cpu().numpy()
    for k, p in wl.decoders.named_parameters():
        if p.grad is not None:
            out[f"{tag}_dg_{k}"] = p.grad.cpu().numpy()


def dump_rays(out, tag, dev, R, ns, ni, prec, loss_kind, frozen, rays_grad, saved):
    import contextlib
    import torch
    from myslam_amd import losses, lowp, ops
    wl = _small_workload(dev, R, ns, ni, rays_grad, frozen)
    sl = slice(0, R)
    ro, rd, gd, gc = wl.rays_o[sl], wl.rays_d[sl], wl.gt_depth[sl], wl.gt_color[sl]
    rand = tuple(t[sl] for t in wl._rand)
    ctx = ops.mixed_precision(lowp.HalfPlanes(wl.planes), ray_grads=rays_grad) if prec == "lowp" else contextlib.nullcontext()
    with ctx:
        if loss_kind == "fused":
            depth, color, sdf, z, pre = wl.renderer.render_batch_ray_with_loss(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gd, gc,
                                                                              losses.MAPPING_W, _rand=rand, saved_hidden=saved)
            loss = losses.mapping_loss(depth, color, sdf, z, gd, gc, wl.truncation, precomputed=pre)
        else:
            depth, color, sdf, z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd, _rand=rand,
                                                                saved_hidden=saved)
            loss = losses.mapping_loss(depth, color, sdf, z, gd, gc, wl.truncation)
        loss.backward()
    torch.cuda.synchronize()
    _flags(out, tag)
    for k, t in (("depth", depth), ("rgb", color), ("sdf", sdf), ("z", z), ("loss", loss)):
        out[f"{tag}_{k}"] = t.detach().cpu().numpy()
    _dump_grads(out, tag, wl)
    if rays_grad:
        out[f"{tag}_g_rays_o"] = wl.rays_o.grad[sl].cpu().numpy()
        out[f"{tag}_g_rays_d"] = wl.rays_d.grad[sl].cpu().numpy()


def dump_points(out, tag, dev, N, prec, frozen):
    import contextlib
    import torch
    from myslam_amd import lowp, ops, synth
    wl = _small_workload(dev, 5, 12, 8, False, frozen)
    b = wl.scene.bound.to(dev).float()
    u = torch.from_numpy(synth.hash_uniform((N, 3), 95_000)).to(dev)
    pts = (b[:, 0] + u * (b[:, 1] - b[:, 0])).requires_grad_(True)
    G = torch.from_numpy(synth.hash_uniform((N, 4), 95_001)).to(dev) - 0.5
    ctx = ops.mixed_precision(lowp.HalfPlanes(wl.planes), points=True) if prec == "lowp" else contextlib.nullcontext()
    with ctx:
        raw = wl.decoders(pts, wl.planes)            # DecodeFn
        (raw * G).sum().backward()
    torch.cuda.synchronize()
    _flags(out, tag)
    out[f"{tag}_raw"] = raw.detach().float().cpu().numpy()
    out[f"{tag}_g_pts"] = pts.grad.cpu().numpy()
    _dump_grads(out, tag, wl)


if sys.argv[1] == "dump":
    import torch
    from myslam_amd import harness
    dev = torch.device("cuda:0")
    out = {}
    for i, (sc, R, ns, ni, zf) in enumerate(CONFIGS):
        wl = harness.make_workload(sc, R, ns, ni, device=dev, zero_frac=zf)
        o = wl.forward()
        g = wl.backward_with(o)
        _flags(out, f"{i}_bwd")
        for k, t in zip(("depth", "rgb", "sdf", "z"), o):
            out[f"{i}_{k}"] = t.detach().cpu().numpy()
        for j, t in enumerate(g):
            out[f"{i}_g{j}"] = t.cpu().numpy()
        with torch.no_grad():
            o2 = wl.forward()
        out[f"{i}_nograd_depth"] = o2[0].cpu().numpy()
        out[f"{i}_nograd_rgb"] = o2[1].cpu().numpy()
        torch.manual_seed(0)
        from myslam_amd import ops
        ops._rng_state(dev).zero_()           # same jitter in both builds
        loss = wl.step()                      # fused loss path (eslam_render_fwd_loss / eslam_render_bwd_loss), in-kernel jitter
        _flags(out, f"{i}_step")
        out[f"{i}_step_loss"] = loss.detach().cpu().numpy()
        for j, p_ in enumerate(wl.params()):
            out[f"{i}_sg{j}"] = p_.grad.cpu().numpy()
    for i, cfg in enumerate(SMALL, len(CONFIGS)):
        if cfg[0] == "rays":
            dump_rays(out, str(i), dev, *cfg[1:])
        else:
            dump_points(out, str(i), dev, *cfg[1:])
    np.savez(sys.argv[2], **out)
else:
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    mode = sys.argv[4] if len(sys.argv) > 4 else ""
    assert mode in ("", "exact", "strict"), mode
    assert sorted(a.files) == sorted(b.files), sorted(set(a.files) ^ set(b.files))

    def atomics(k):      # plane gradients (the first 12 of a workload's parameters) and loss values
        m = re.search(r"_(g|sg|pg)(\d+)$", k)
        return (m is not None and int(m.group(2)) < 12) or k.endswith("loss")
    n_exact = 0
    for k in a.files:
        x, y = a[k], b[k]
        if mode == "exact" or (mode == "strict" and not atomics(k)):
            n_exact += 1
            if x.shape != y.shape or x.tobytes() != y.tobytes():
                print("BYTES DIFFER", k, ALL[int(k.split('_')[0])], int((x != y).sum()) if x.shape == y.shape else "shape", "elements")
            continue
        err = float(np.abs(x - y).max() / (np.abs(y).max() + 1e-30))
        if not err <= 1e-5:
            print("DIFF", k, ALL[int(k.split('_')[0])], err)
    print("compared", len(a.files), "arrays,", n_exact, "of them byte for byte", f"({mode})" if mode else "")
