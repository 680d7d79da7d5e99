"""GPU side of tests/test_gpu_loss_direct.py: every launch the test makes, in one function.  run() is called in-process (default
mode) and by a child process, `python -m tests.loss_direct_gpu OUT.npz`, under ESLAM_DETERMINISTIC=1 (read once per process),
where the sums go through loss_finalize_det instead of float atomics.  Nothing is judged here against the reference: run() returns
what the kernels wrote, and the differences between two kernels' outputs, as a flat dict of numpy arrays; the parent holds
them against tests/loss_ref.py on the host.  Test-only.

Keys: "<case>/<name>" for the direct entries (cases()), "reuse/<k>/...", "halves/<case>/acc", "err/<name>/...", and
"ik/<tag>/..." for the forms inside the render kernels (IN_KERNEL).
"""
import ctypes
import sys

import numpy as np
import torch

from tests import loss_ref as lf

SHAPES = [(1, 1), (3, 5), (4, 64), (5, 65), (7, 256), (1023, 8), (1025, 8), (4099, 33)]
BORDER_S = (29, 77)
SENTINEL = -7.25
UPSTREAM = 0.37
W5 = lf.MAPPING_W5
REUSE = ("shape_5x65", "shape_4099x33", "shape_1x1")          # one scratch, three batch sizes
HALVES = ("shape_1025x8", "plain_9x77_t0.06")
IK_R = 37
IN_KERNEL = [(S, variant) for S in BORDER_S for variant in ("plain", "depthless_masked")]
# (ray gradients requested, upstream, further upstream gradients on the outputs)
IK_CONFIGS = [(True, None, False), (False, None, False), (True, UPSTREAM, True), (False, UPSTREAM, True)]


def cases():
    """name -> (R, S, truncation, variant, stream) of the direct entries' batches."""
    out = {}
    for k, (R, S) in enumerate(SHAPES):
        out[f"shape_{R}x{S}"] = (R, S, lf.TRUNCATIONS[k % 2], "depthless_masked", 10 + k)
    for variant in lf.VARIANTS:
        for S in BORDER_S:
            for t in lf.TRUNCATIONS:
                out[f"{variant}_9x{S}_t{t}"] = (9, S, t, variant, 0)
    return out


def batch_of(spec):
    R, S, t, variant, stream = spec
    return lf.border_batch(R, S, t, variant, stream)


def workgroups(R):
    """Workgroups of eslam_loss_reduce / eslam_loss_value: four rays each, at most 256 (the grid-stride wraps from ray 1025)."""
    return min((R + 3) // 4, 256)


def forward_workgroups(R):
    """Workgroups of the render forward below its persistent size: four rays each, rounded up to a multiple of eight."""
    return ((R + 3) // 4 + 7) // 8 * 8


def ik_tag(S, variant):
    return f"{IK_R}x{S}_{variant}"


def ik_batch(S, variant):
    return lf.border_batch(IK_R, S, 0.06, variant, stream=40 + S)


def ik_config_tag(cfg):
    rays, up, extra = cfg
    return f"{'full' if rays else 'rank16'}_{'up' if up is not None else 'one'}{'_extra' if extra else ''}"


class _Entries:
    """The argument plumbing of the five loss entries on one uploaded batch."""

    def __init__(self, dev, b, truncation):
        from myslam_amd import _hip
        self.h, self.dev, self.t = _hip, dev, float(truncation)
        self.lib = _hip.lib()
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.x = {k: up(v) for k, v in b.items()}
        self.R, self.S = b["z"].shape
        self.w5 = (ctypes.c_float * 5)(*W5)

    def inputs(self, lo=0, hi=None):
        p = self.h.ptr
        hi = self.R if hi is None else hi
        return [p(self.x[k][lo:hi]) for k in ("depth", "rgb", "sdf", "z", "gt_depth", "gt_color")]

    def mask(self, lo=0, hi=None):
        m = self.x["ray_mask"]
        return None if m is None else self.h.ptr(m[lo:self.R if hi is None else hi])

    def stream(self):
        return self.h.stream_handle(self.dev)

    def full(self, *shape):
        return torch.full(shape, SENTINEL, device=self.dev)

    def grads(self):
        return self.full(self.R), self.full(self.R, 3), self.full(self.R, self.S)

    def reduce(self, acc, lo=0, hi=None, R=None):
        n = (self.R if hi is None else hi) - lo
        return self.lib.eslam_loss_reduce(*self.inputs(lo, hi), n if R is None else R, self.S, self.t, self.mask(lo, hi), self.h.ptr(acc),
                                          self.stream())

    def value(self, scratch, acc, loss, R=None):
        p = self.h.ptr
        return self.lib.eslam_loss_value(*self.inputs(), self.R if R is None else R, self.S, self.t, self.w5, self.mask(), p(scratch), p(acc),
                                         p(loss), self.stream())

    def grad(self, acc, loss, g, upstream=None, R=None):
        p = self.h.ptr
        return self.lib.eslam_loss_grad(*self.inputs(), self.R if R is None else R, self.S, self.t, self.w5, self.mask(), p(acc), p(loss),
                                        p(g[0]), p(g[1]), p(g[2]), p(upstream), self.stream())

    def mapping(self, loss, g, scratch, R=None):
        p = self.h.ptr
        return self.lib.eslam_mapping_loss(*self.inputs(), self.R if R is None else R, self.S, self.t, self.w5, self.mask(), p(loss), p(g[0]),
                                           p(g[1]), p(g[2]), p(scratch), self.stream())

    def ok(self, rc, what):
        self.h.check(rc, what)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _nonzero_words(t):
    return int((t.view(torch.int32) != 0).sum())


def _garbage(dev, n=16):
    return torch.tensor([0x7FC12345, 0x4B000001, -1, 0x3F800000] * (n // 4), dtype=torch.int32, device=dev).view(torch.float32)


def _direct(out, dev):
    from myslam_amd import ops
    up = torch.tensor([UPSTREAM], device=dev)
    all_cases = cases()
    for name, spec in all_cases.items():
        b = batch_of(spec)
        e = _Entries(dev, b, spec[2])
        x = e.x
        # (a) eslam_loss_reduce into a zeroed acc, eslam_loss_grad: value and gradients
        acc = ops.loss_reduce(x["depth"], x["rgb"], x["sdf"], x["z"], x["gt_depth"], x["gt_color"], e.t, ray_mask=x["ray_mask"])
        loss, g = e.full(1), e.grads()
        e.ok(e.grad(acc, loss, g), "eslam_loss_grad")
        for k, v in (("a/acc", acc), ("a/loss", loss), ("a/g_depth", g[0]), ("a/g_rgb", g[1]), ("a/g_sdf", g[2])):
            out[f"{name}/{k}"] = _np(v)
        # (b) eslam_loss_value on a scratch of its own, eslam_loss_grad with an upstream gradient and loss = NULL, then with
        # loss alone
        scratch = torch.zeros(int(e.lib.eslam_loss_scratch_floats(e.R)), device=dev)
        acc_v, loss_v, g_u, loss_only = e.full(16), e.full(1), e.grads(), e.full(1)
        e.ok(e.value(scratch, acc_v, loss_v), "eslam_loss_value")
        e.ok(e.grad(acc_v, None, g_u, upstream=up), "eslam_loss_grad(upstream)")
        e.ok(e.grad(acc_v, loss_only, (None, None, None)), "eslam_loss_grad(value)")
        out[f"{name}/b/scratch_nonzero"] = np.asarray([_nonzero_words(scratch), _nonzero_words(scratch[:32])])
        for k, v in (("b/acc", acc_v), ("b/loss", loss_v), ("b/loss_only", loss_only), ("b/g_depth", g_u[0]), ("b/g_rgb", g_u[1]),
                     ("b/g_sdf", g_u[2])):
            out[f"{name}/{k}"] = _np(v)
        # (c) eslam_mapping_loss, its 64 bytes of scratch holding anything
        loss_c, g_c, scr = e.full(1), e.grads(), _garbage(dev)
        e.ok(e.mapping(loss_c, g_c, scr), "eslam_mapping_loss")
        for k, v in (("c/acc", scr), ("c/loss", loss_c), ("c/g_depth", g_c[0]), ("c/g_rgb", g_c[1]), ("c/g_sdf", g_c[2])):
            out[f"{name}/{k}"] = _np(v)
        if name in HALVES:                       # two halves of the batch into one acc
            acc2 = torch.zeros(16, device=dev)
            half = e.R // 2
            e.ok(e.reduce(acc2, 0, half), "eslam_loss_reduce(first half)")
            e.ok(e.reduce(acc2, half, e.R), "eslam_loss_reduce(second half)")
            out[f"halves/{name}/acc"] = _np(acc2)
    # one scratch, three batch sizes
    from myslam_amd import _hip
    scratch = torch.zeros(int(_hip.lib().eslam_loss_scratch_floats(max(all_cases[n][0] for n in REUSE))), device=dev)
    for k, name in enumerate(REUSE):
        spec = all_cases[name]
        e = _Entries(dev, batch_of(spec), spec[2])
        acc_v, loss_v = e.full(16), e.full(1)
        e.ok(e.value(scratch, acc_v, loss_v), "eslam_loss_value(reuse)")
        out[f"reuse/{k}/acc"], out[f"reuse/{k}/loss"] = _np(acc_v), _np(loss_v)
        out[f"reuse/{k}/scratch_nonzero"] = np.asarray([_nonzero_words(scratch), _nonzero_words(scratch[:32])])


def _errors(out, dev):
    """Calls that must be refused before anything is launched: return code, message, and whether every output buffer still holds
    what it held."""
    spec = cases()["shape_3x5"]
    e = _Entries(dev, batch_of(spec), spec[2])
    acc, loss, g, scratch = e.full(16), e.full(1), e.grads(), e.full(int(e.lib.eslam_loss_scratch_floats(e.R)))
    none3 = (None, None, None)
    calls = {
        "reduce_no_rays": lambda: e.reduce(acc, R=0),
        "value_no_rays": lambda: e.value(scratch, acc, loss, R=0),
        "grad_no_rays": lambda: e.grad(acc, loss, g, R=0),
        "mapping_no_rays": lambda: e.mapping(loss, g, acc, R=0),
        "reduce_null_acc": lambda: e.reduce(None),
        "value_null_acc": lambda: e.value(scratch, None, loss),
        "grad_null_acc": lambda: e.grad(None, loss, g),
        "value_null_scratch": lambda: e.value(None, acc, loss),
        "mapping_null_scratch": lambda: e.mapping(loss, g, None),
        "grad_depth_without_sdf": lambda: e.grad(acc, loss, (g[0], g[1], None)),
        "grad_depth_alone": lambda: e.grad(acc, None, (g[0], None, None)),
        "grad_nothing_asked": lambda: e.grad(acc, None, none3),
    }
    for name, call in calls.items():
        acc.fill_(SENTINEL)
        rc = int(call())
        msg = e.lib.eslam_last_error()
        torch.cuda.synchronize()
        # (eslam_mapping_loss clears the 64 bytes it was given - acc here - before it looks at the batch: a memset, no launch)
        bufs = [loss, scratch, *g] + ([] if name == "mapping_no_rays" else [acc])
        out[f"err/{name}/rc"] = np.asarray(rc)
        out[f"err/{name}/message"] = np.asarray(msg.decode() if msg else "")
        out[f"err/{name}/untouched"] = np.asarray(all(bool((t == SENTINEL).all()) for t in bufs))


def _max_rel(a, b):
    return lf.max_rel(_np(a).astype(np.float64), _np(b).astype(np.float64))


def _in_kernel(out, dev):
    """The border rows as z_vals of eslam_render_fwd_loss / eslam_render_bwd_loss on room0 (synthetic planes, trained-like state)."""
    from myslam_amd import _hip, harness, ops, synth
    lib, p = _hip.lib(), _hip.ptr
    wl = harness.Workload("room0", IK_R * 4, 21, 8, dev, planes="synth", state="trained")
    assert wl.R >= IK_R, wl.R
    R = IK_R
    ro, rd = wl.rays_o.detach()[:R].contiguous(), wl.rays_d.detach()[:R].contiguous()
    dec, _keep_dec = _hip.make_decoders(ops.decoder_params(wl.decoders), ops.beta_tensor(wl.decoders.beta, dev))
    bound = _hip.make_bound(wl.renderer._bound6)
    planes = [q.detach() for q in wl.plane_list]
    st = _hip.stream_handle(dev)
    up_t = torch.tensor([UPSTREAM], device=dev)
    for S, variant in IN_KERNEL:
        tag = "ik/" + ik_tag(S, variant)
        e = _Entries(dev, ik_batch(S, variant), 0.06)
        x = e.x
        z, gd, gc, mask = x["z"], x["gt_depth"], x["gt_color"], x["ray_mask"]
        depth, rgb, sdf = e.full(R), e.full(R, 3), e.full(R, S)
        raw_rgb, feat = e.full(R, S, 3), e.full(R * S, 128)
        scratch = torch.zeros(int(lib.eslam_loss_scratch_floats(R)), device=dev)
        acc, loss = e.full(16), e.full(1)
        arr, _keep = _hip.make_planes(planes)
        _hip.check(lib.eslam_render_fwd_loss(arr, ctypes.byref(dec), bound, p(ro), p(rd), p(z), R, S, p(depth), p(rgb), p(sdf), p(raw_rgb),
                                             p(feat), None, p(gd), p(gc), e.t, e.w5, p(mask), p(scratch), p(acc), p(loss), None, st),
                   "eslam_render_fwd_loss")
        # the separate entries on the kernel's own outputs
        x["depth"], x["rgb"], x["sdf"] = depth, rgb, sdf
        acc_v, loss_v = e.full(16), e.full(1)
        e.ok(e.value(scratch, acc_v, loss_v), "eslam_loss_value")
        for k, v in (("depth", depth), ("rgb", rgb), ("sdf", sdf), ("acc", acc), ("loss", loss), ("acc_value", acc_v), ("loss_value", loss_v)):
            out[f"{tag}/{k}"] = _np(v)
        out[f"{tag}/scratch_nonzero"] = np.asarray([_nonzero_words(scratch), _nonzero_words(scratch[:32])])
        extra = tuple((torch.from_numpy(synth.hash_uniform(shape, 760_000 + k)).to(dev) - 0.5) * s
                      for k, (shape, s) in enumerate((((R,), 0.2), ((R, 3), 0.2), ((R, S), 0.05))))

        def backward(fused, rays, upstream, further):
            grads = [torch.zeros_like(q) for q in planes]
            arr_g, _k = _hip.make_planes(planes, grads)
            g_dec, g_beta = e.full(_hip.N_DEC_PARAMS), e.full(1)
            g_ro, g_rd = (e.full(R, 3), e.full(R, 3)) if rays else (None, None)
            ws = torch.empty(int(lib.eslam_bwd_workspace_bytes(R * S)), dtype=torch.uint8, device=dev)
            up = None if upstream is None else up_t
            loss_out = None
            if fused:
                loss_out = e.full(1)
                ex = further or (None, None, None)
                _hip.check(lib.eslam_render_bwd_loss(arr_g, ctypes.byref(dec), bound, p(ro), p(rd), p(z), R, S, p(sdf), p(raw_rgb), p(feat),
                                                     p(depth), p(rgb), p(gd), p(gc), e.t, e.w5, p(mask), p(acc), p(up), p(loss_out), p(ex[0]),
                                                     p(ex[1]), p(ex[2]), p(g_dec), p(g_beta), p(g_ro), p(g_rd), None, p(ws), st),
                           "eslam_render_bwd_loss")
            else:
                g = e.grads()
                e.ok(e.grad(acc, None, g, upstream=up), "eslam_loss_grad")
                if further:
                    g = tuple(a + b for a, b in zip(g, further))
                _hip.check(lib.eslam_render_bwd(arr_g, ctypes.byref(dec), bound, p(ro), p(rd), p(z), R, S, p(sdf), p(raw_rgb), p(feat), p(g[0]),
                                                p(g[1]), p(g[2]), p(g_dec), p(g_beta), p(g_ro), p(g_rd), None, p(ws), st), "eslam_render_bwd")
            torch.cuda.synchronize()
            return dict(planes=grads, dec=g_dec, beta=g_beta, ro=g_ro, rd=g_rd, loss_out=loss_out, rank16=int(lib.eslam_last_backward_rank16()))

        loss_from_acc = e.full(1)
        e.ok(e.grad(acc, loss_from_acc, (None, None, None)), "eslam_loss_grad(value)")
        out[f"{tag}/loss_from_acc"] = _np(loss_from_acc)
        for cfg in IK_CONFIGS:
            rays, upstream, further = cfg
            ex = extra if further else None
            a, a2, f = backward(False, rays, upstream, ex), backward(False, rays, upstream, ex), backward(True, rays, upstream, ex)
            pl = lambda u, v: max(_max_rel(s, t) for s, t in zip(u["planes"], v["planes"]))
            m = dict(x=pl(a2, a), planes=pl(f, a), dec=_max_rel(f["dec"], a["dec"]), beta=_max_rel(f["beta"], a["beta"]),
                     rays=max(_max_rel(f["ro"], a["ro"]), _max_rel(f["rd"], a["rd"])) if rays else 0.0,
                     rank16_separate=a["rank16"], rank16_fused=f["rank16"], loss_out=float(f["loss_out"][0]),
                     nonzero=float(min(float(q.abs().max()) for q in f["planes"] + [f["dec"], f["beta"]])),
                     rays_nonzero=float(min(float(f["ro"].abs().max()), float(f["rd"].abs().max()))) if rays else 1.0,
                     finite=float(all(bool(torch.isfinite(q).all()) for q in f["planes"] + [f["dec"], f["beta"]])))
            for k, v in m.items():
                out[f"{tag}/{ik_config_tag(cfg)}/{k}"] = np.asarray(v, dtype=np.float64)


def run(dev=None):
    from myslam_amd import _hip
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dev = torch.device("cuda:0") if dev is None else dev
    out = {"det": np.asarray(int(_hip.lib().eslam_deterministic()))}
    _direct(out, dev)
    _errors(out, dev)
    _in_kernel(out, dev)
    torch.cuda.synchronize()
    return out


def main():
    np.savez(sys.argv[1], **run())
    print("RESULT written", sys.argv[1])


if __name__ == "__main__":
    sys.exit(main())
