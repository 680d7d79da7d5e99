"""One mixed-precision render call with ray (pose) gradients on a fixture's inputs: shared by tests/test_gpu_lowp_pose.py and
its child process (python -m tests.lowp_pose_gpu, the bitwise comparison under ESLAM_DETERMINISTIC=1).  Test-only."""
import json
import sys

import numpy as np
import torch

from tests import helpers as hp


def _np(t):
    return None if t is None else t.detach().float().cpu().numpy()


def step(fx, form, grad_o=True, grad_d=True, ray_grads=True, dec_grad=None):
    """form: "tracking" = planes and decoders frozen, losses.tracking_loss; "separate" / "fused" = a mapping step with the
    loss formed outside / inside the kernels, planes and decoders trained.  grad_o / grad_d: which of rays_o / rays_d require
    grad.  dec_grad=False: a mapping step with the decoders frozen (their gradients come back as None).
    Returns numpy arrays: depth, color, sdf, z, feat (the saved bf16 features), g_o, g_d (None where not asked for),
    and for a mapping step planes (12), dec {name}, beta."""
    from myslam_amd import lowp, losses, ops
    from tests.test_gpu_parity import _dev, build
    dev = _dev()
    train = form != "tracking"
    sc, planes, dec, renderer = build(fx, planes_grad=train, dec_grad=train if dec_grad is None else dec_grad)
    rand = tuple(None if t is None else t.to(dev) for t in hp.rand_inputs(fx))
    ro = torch.from_numpy(fx["rays_o"]).to(dev).requires_grad_(grad_o)
    rd = torch.from_numpy(fx["rays_d"]).to(dev).requires_grad_(grad_d)
    gd, gc = (torch.from_numpy(fx[k]).to(dev) for k in ("gt_depth", "gt_color"))
    tr = float(fx["truncation"])
    half = lowp.HalfPlanes(planes)
    ctx = ops.mixed_precision(half, ray_grads=True) if ray_grads else ops.mixed_precision(half)
    with ctx:
        if form == "fused":
            depth, color, sdf, z, pre = renderer.render_batch_ray_with_loss(planes, dec, rd, ro, dev, tr, gd, gc, losses.MAPPING_W,
                                                                            _rand=rand)
            loss = pre.loss
        else:
            depth, color, sdf, z = renderer.render_batch_ray(planes, dec, rd, ro, dev, tr, gt_depth=gd, _rand=rand)
            loss = (losses.mapping_loss if train else losses.tracking_loss)(depth, color, sdf, z, gd, gc, tr)
        feat = sdf.grad_fn.saved_tensors[5] if sdf.grad_fn is not None else None      # ops.RenderFn.forward's save order
        if loss.requires_grad:
            loss.backward()
    torch.cuda.synchronize()
    out = dict(depth=_np(depth), color=_np(color), sdf=_np(sdf), z=_np(z), feat=_np(feat), g_o=_np(ro.grad), g_d=_np(rd.grad),
               loss=float(loss.detach()))
    if train:
        out["planes"] = [_np(p.grad) for p in hp.flat_planes(planes)]
        out["dec"] = {k: _np(p.grad) for k, p in dec.named_parameters()}
    return out


def sliced(fx, z, n):
    """The first n rays through ops.RenderFn.apply on the given z_vals (rows of a full run), planes and decoders frozen,
    losses.tracking_loss of that batch.  Returns g_o, g_d, feat as numpy."""
    from myslam_amd import lowp, losses, ops
    from tests.test_gpu_parity import _dev, build
    dev = _dev()
    sc, planes, dec, renderer = build(fx, planes_grad=False, dec_grad=False)
    ro = torch.from_numpy(fx["rays_o"][:n]).to(dev).requires_grad_(True)
    rd = torch.from_numpy(fx["rays_d"][:n]).to(dev).requires_grad_(True)
    gd, gc = (torch.from_numpy(fx[k][:n]).to(dev) for k in ("gt_depth", "gt_color"))
    zz = torch.from_numpy(np.ascontiguousarray(z[:n])).to(dev)
    with ops.mixed_precision(lowp.HalfPlanes(planes), ray_grads=True):
        depth, color, sdf = ops.RenderFn.apply(ro, rd, zz, ops.bound_to_host(dec.bound), ops.beta_tensor(dec.beta, dev), None, None,
                                               *hp.flat_planes(planes), *ops.decoder_params(dec))
        feat = sdf.grad_fn.saved_tensors[5]
        losses.tracking_loss(depth, color, sdf, zz, gd, gc, float(fx["truncation"])).backward()
    torch.cuda.synchronize()
    return _np(ro.grad), _np(rd.grad), _np(feat)


def _same(a, b):
    return bool(np.array_equal(a, b))


def main():
    """Child process (ESLAM_DETERMINISTIC=1, where the plane-gradient scatter is reproducible bit for bit): per fixture and loss
    form, are the plane / decoder gradients of a step WITH ray gradients the bits of the same step without?"""
    from myslam_amd import _hip
    out = {"det": int(_hip.lib().eslam_deterministic())}
    for case in sys.argv[1:]:
        fx = hp.load(case)
        for form in ("separate", "fused"):
            base = step(fx, form, False, False, ray_grads=False)
            for tag, (go, gd) in (("both", (True, True)), ("o", (True, False)), ("d", (False, True))):
                r = step(fx, form, go, gd)
                out[f"{case} {form} {tag}"] = dict(
                    forward=all(_same(r[k], base[k]) for k in ("depth", "color", "sdf", "z", "feat")),
                    planes=[_same(a, b) for a, b in zip(r["planes"], base["planes"])],
                    dec={k: _same(r["dec"][k], base["dec"][k]) for k in base["dec"]})
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
