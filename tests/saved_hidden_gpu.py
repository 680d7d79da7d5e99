"""GPU side of tests/test_gpu_saved_hidden.py, shared with its child process (python -m tests.saved_hidden_gpu, the bitwise
comparison of the plane gradients under ESLAM_DETERMINISTIC=1, which is read once per process).  Test-only.

A case is one mapping iteration on the first R rays of a harness workload (room0, synth planes, trained-like state); run() renders
it, takes the mapping loss and back-propagates, with the keyword that selects the backward's source of the first hidden layer."""
import json
import sys

import numpy as np
import torch

BASE = dict(R=37, ns=56, ni=8, loss="fused", frozen=False, rays_grad=False, channels_last=True, mask=False, zero_frac=0.0)
# on top of the first, each later case varies one property (see the test file's docstring)
CASES = {
    "base_37x64": {},
    "s56_half_block": dict(ns=48),
    "s96_two_chunks": dict(ns=88),
    "s40": dict(ns=32),
    "r1100x32_second_ray": dict(R=1100, ns=24),
    "separate_loss": dict(loss="separate"),
    "frozen_decoders": dict(frozen=True),
    "ray_gradients": dict(rays_grad=True),
    "nchw": dict(channels_last=False),
    "masked_and_depthless": dict(mask=True, zero_frac=0.1),
    "frozen_separate_5x72": dict(R=5, ns=64, loss="separate", frozen=True),
}


def spec(case):
    return dict(BASE, **CASES[case])


def workload(case, dev):
    from myslam_amd import harness
    sp = spec(case)
    R = sp["R"]
    # (the AABB pre-filter drops some of the rays asked for)
    wl = harness.Workload("room0", R * 4 if R < 1000 else R + R // 2, sp["ns"], sp["ni"], dev, zero_frac=sp["zero_frac"],
                          channels_last=sp["channels_last"], rays_grad=sp["rays_grad"], planes="synth", state="trained")
    assert wl.R >= R, (wl.R, R)
    if sp["frozen"]:
        for p in wl.decoders.parameters():
            p.requires_grad_(False)
    wl.case = sp
    wl.mask = None
    if sp["mask"]:
        wl.mask = (torch.arange(R, device=dev) % 3) != 1          # a third of the rays masked
        n0 = int((wl.gt_depth[:R] == 0).sum())
        assert 0 < n0 < R // 3, n0
    return wl


def run(wl, saved, glue="python", seed=1234):
    """One iteration; returns loss, forward outputs, z_vals and every gradient as CPU tensors (None where not requested)."""
    from myslam_amd import _hip, losses, ops
    sp, dev = wl.case, wl.device
    R = sp["R"]
    sl = slice(0, R)
    for p in wl.params():
        p.grad = None
    wl.rays_o.grad = wl.rays_d.grad = None
    ro, rd, gd, gc = wl.rays_o[sl], wl.rays_d[sl], wl.gt_depth[sl], wl.gt_color[sl]
    rand = None
    if glue == "python":
        rand = tuple(t[sl] for t in wl._rand)          # injected numbers: a call the compiled glue does not take
    else:
        assert ops.torch_ext() is not None, "eslam_torch_ext is not built"
        ops.seed(seed)                                  # the same in-kernel numbers in every run (the counter restarts)
    try:
        if sp["loss"] == "fused":
            depth, color, sdf, z, pre = wl.renderer.render_batch_ray_with_loss(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gd, gc,
                                                                              losses.MAPPING_W, ray_mask=wl.mask, _rand=rand,
                                                                              saved_hidden=saved)
            loss = losses.mapping_loss(depth, color, sdf, z, gd, gc, wl.truncation, precomputed=pre)
        else:
            depth, color, sdf, z = wl.renderer.render_batch_ray(wl.planes, wl.decoders, rd, ro, dev, wl.truncation, gt_depth=gd,
                                                                _rand=rand, saved_hidden=saved)
            loss = losses.mapping_loss(depth, color, sdf, z, gd, gc, wl.truncation, ray_mask=wl.mask)
        python_node = "RenderFn" in type(sdf.grad_fn).__name__
        assert python_node == (glue == "python"), (glue, type(sdf.grad_fn).__name__)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        if glue != "python":
            ops.seed(None)
    lib = _hip.lib()
    assert lib.eslam_last_backward_saved_hidden() == int(bool(saved)), "the library dispatched the other decoder backward"
    c = lambda t: None if t is None else t.detach().cpu().clone()
    out = dict(loss=c(loss), depth=c(depth), color=c(color), sdf=c(sdf), z=c(z), planes=[c(p.grad) for p in wl.plane_list],
               dec={k: c(t.grad) for k, t in wl.decoders.named_parameters()}, rank16=lib.eslam_last_backward_rank16(),
               ro=None if wl.rays_o.grad is None else c(wl.rays_o.grad[sl]), rd=None if wl.rays_d.grad is None else c(wl.rays_d.grad[sl]))
    assert all(g is not None for g in out["planes"])
    return out


def exact_names(a, loss=True):
    """What must agree bit for bit between the two paths: everything but the plane gradients.  loss=False: not the loss value
    either - outside deterministic mode the forward pass sums it with unordered float atomics (loss_finalize), so two runs of
    ONE path need not agree in its last bit; the caller holds it to that path's own spread."""
    names = (["loss"] if loss else []) + ["depth", "color", "sdf", "z"] + [k for k in ("ro", "rd") if a[k] is not None]
    return names + ["dec:" + k for k, v in a["dec"].items() if v is not None]


def get(a, name):
    return a["dec"][name[4:]] if name.startswith("dec:") else a[name]


def unequal(a, b, loss=True):
    """Names of the bit-exact quantities that differ between two runs (and how many elements)."""
    assert exact_names(a) == exact_names(b)
    return [(n, int((get(a, n) != get(b, n)).sum())) for n in exact_names(a, loss) if not torch.equal(get(a, n), get(b, n))]


def main():
    """Child: deterministic mode, every case, recompute against saved, every quantity bit for bit - the loss (fixed-order sums
    there) and the plane gradients (fixed point there) included."""
    from myslam_amd import _hip
    dev = torch.device("cuda:0")
    res = dict(det=int(_hip.lib().eslam_deterministic()), cases={})
    for case in sys.argv[1:] or list(CASES):
        wl = workload(case, dev)
        off, on = run(wl, False), run(wl, True)
        res["cases"][case] = dict(rank16=[off["rank16"], on["rank16"]], unequal=unequal(off, on),
                                  planes=[bool(torch.equal(a, b)) for a, b in zip(off["planes"], on["planes"])],
                                  nonzero=[bool(np.abs(a.numpy()).max() > 0) for a in on["planes"]])
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    sys.exit(main())
