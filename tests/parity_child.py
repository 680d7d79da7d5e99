"""Child program of tests/test_gpu_deterministic_parity.py: every GPU run of that module, in ONE process per mode
(ESLAM_DETERMINISTIC is read once per process).  `python -m tests.parity_child OUTDIR` from the repository root.

It asserts nothing about results: each case's arrays go to OUTDIR/<case>.npz as soon as the case is done (written under
a temporary name and renamed, so a file that exists is complete), and the parent compares them with the float64 oracle
on the CPU.  The only assertion made here is the host-side one in front of every fused-loss launch: the scratch slot
handed out holds at least eslam_loss_scratch_floats(R) floats.  Bitwise comparisons between two GPU runs are made here
on the device (count of elements whose 32 bits differ); the second run's arrays are written only when that count is
not zero.  Any exception ends the child at once: nothing more is started on the GPU after a failed step."""
import json
import os
import sys
import time

import numpy as np
import torch

RENDER_CASES = ["room0_200x32", "room0_200x40_zero15", "room0_200x40_trained_zero15", "room0_4096x64_trained_zero10",
                "scene0000_8192x96_zero10"]
NCHW_CASES = RENDER_CASES[:3]
LAYOUTS = {"cl": None, "nchw_strided": -1, "nchw_relayout": 0}      # ops._RELAYOUT_MIN_POINTS of the run (None: as it is)
SCRATCH_SEQUENCE = ["room0_200x40_zero15", "scene0000_8192x96_zero10", "room0_200x40_zero15"]     # 200, 8192, 200 rays
DECODE_NS = [1, 63, 64, 65, 2000, 32768, 32769, 40000 + 37]
CONTENTION_K = 64
BIG_SCALE = 2.0 ** 50


def ray_mask_of(R):
    """The ray_mask of the masked-loss checks: two rays of three."""
    return np.arange(R) % 3 != 1


def decode_points(N, sc):
    """N points for the decode cases: uniform over the AABB grown by 10 % a side (42 % outside: border clamp), the first
    N // 8 of them within 1 mm of one point (one texel of every plane is 30 mm or more: contention)."""
    from myslam_amd import synth
    lo, hi = sc.bound[:, 0].numpy(), sc.bound[:, 1].numpy()
    u = synth.hash_uniform((N, 3), 77_000 + N)
    p = lo - 0.1 * (hi - lo) + u * 1.2 * (hi - lo)
    nc = N // 8
    centre = lo + (hi - lo) * np.array([100.5 / 327, 45.5 / 222, 70.5 / 167])
    p[:nc] = centre + (u[:nc] - 0.5) * 1e-3
    return p.astype(np.float32)


def main(out_dir):
    from myslam_amd import _hip, harness, losses, ops, scene as scn
    from tests import helpers as hp
    from tests.test_gpu_parity import build, check_against_fixture, run_hip

    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    det = int(lib.eslam_deterministic())
    t_start = time.time()

    def save(name, **arrays):
        tmp = os.path.join(out_dir, "." + name + ".tmp.npz")
        np.savez_compressed(tmp, **arrays)
        os.replace(tmp, os.path.join(out_dir, name + ".npz"))
        with open(os.path.join(out_dir, "progress.log"), "a") as f:
            f.write(f"{time.time() - t_start:8.1f} s  {name}\n")

    def cpu(t):
        return np.ascontiguousarray(t.detach().cpu().numpy())           # logical (NCHW) order whatever the strides

    def ndiff(a, b):
        """Elements whose bits differ, in logical order."""
        a, b = a.detach().contiguous(), b.detach().contiguous()
        return int((a.view(torch.int32) != b.view(torch.int32)).sum())

    def fixture_check(fx, r):
        try:
            check_against_fixture(fx, r)
            return ""
        except AssertionError as e:
            return "check_against_fixture: " + (str(e) or repr(e))[:500]

    # ---- the host-side check in front of every fused-loss launch -------------------------------------------------------
    scratch_log = []
    loss_scratch = ops._loss_scratch

    def checked_loss_scratch(d, n_rays=0):
        t = loss_scratch(d, n_rays)
        need = int(lib.eslam_loss_scratch_floats(int(n_rays)))
        scratch_log.append((int(n_rays), need, int(t.numel())))
        assert t.numel() >= need, f"loss scratch: {t.numel()} floats handed out, {n_rays} rays need {need}"
        return t
    ops._loss_scratch = checked_loss_scratch

    def fused_losses(fx, kinds):
        """The loss of a fixture from the fused formulations; every launch must have asked for the scratch of R rays."""
        R = int(fx["rays_o"].shape[0])
        out = {}
        for kind in kinds:
            mark = len(scratch_log)
            r = run_hip(fx, fused_loss=kind)
            calls = scratch_log[mark:]
            assert calls and all(c[0] == R for c in calls), (kind, R, calls)
            name = "fwd" if kind == "forward" else "sep"
            out["loss_" + name] = np.float64(float(r["loss"]))
            out["fixture_" + name] = fixture_check(fx, r)
            out["scratch_" + name] = np.array(calls, dtype=np.int64)
            last = r
        return out, last

    # ---- (0) loss scratch across growing batches: 200, 8192, 200 rays on one stream, first thing in the process -------------
    first_grads = None
    for step, case in enumerate(SCRATCH_SEQUENCE):
        fx = hp.load(case)
        out, r = fused_losses(fx, ["forward", True])
        if first_grads is None:        # the child's first case: kept on the device for the shadow-hygiene repeat at the end
            first_grads = [p.grad.detach().clone() for p in hp.flat_planes(run_hip(fx)["planes"])]
        save(f"scratch_{step}", case=case, **out)

    # ---- (1) render cases ----------------------------------------------------------------------------------------------
    relayout_default = ops._RELAYOUT_MIN_POINTS
    for case in RENDER_CASES:
        fx = hp.load(case)
        for layout, relayout in LAYOUTS.items():
            if layout != "cl" and case not in NCHW_CASES:
                continue
            ops._RELAYOUT_MIN_POINTS = relayout_default if relayout is None else relayout
            r = run_hip(fx, channels_last=(layout == "cl"))
            ops._RELAYOUT_MIN_POINTS = relayout_default
            arrays = dict(depth=cpu(r["depth"]), color=cpu(r["color"]), sdf=cpu(r["sdf"]), z=cpu(r["z"]),
                          loss=np.float64(float(r["loss"])), g_ro=cpu(r["ro"].grad), g_rd=cpu(r["rd"].grad),
                          fixture=fixture_check(fx, r))
            for k, p in enumerate(hp.flat_planes(r["planes"])):
                arrays[f"pg{k}"] = cpu(p.grad)
                arrays[f"pg{k}_strides_kept"] = np.bool_(p.grad.stride() == p.stride())
            for k, p in r["dec"].named_parameters():
                arrays["dg:" + k] = cpu(p.grad)
            if layout == "cl":
                out, _ = fused_losses(fx, ["forward", True])
                arrays.update(out)
                # ... and with a ray_mask (forward only: the values), both formulations
                sc, planes, dec, renderer = build(fx)
                rand = tuple(None if t is None else t.to(dev) for t in hp.rand_inputs(fx))
                ro, rd = torch.from_numpy(fx["rays_o"]).to(dev), torch.from_numpy(fx["rays_d"]).to(dev)
                gd, gc = torch.from_numpy(fx["gt_depth"]).to(dev), torch.from_numpy(fx["gt_color"]).to(dev)
                tr = float(fx["truncation"])
                mask = torch.from_numpy(ray_mask_of(ro.shape[0])).to(dev)
                depth, color, sdf, z, pre = renderer.render_batch_ray_with_loss(planes, dec, rd, ro, dev, tr, gd, gc,
                                                                                losses.MAPPING_W, ray_mask=mask, _rand=rand)
                arrays["loss_fwd_masked"] = np.float64(float(pre.loss))
                arrays["loss_sep_masked"] = np.float64(float(losses.mapping_loss(depth.detach(), color.detach(), sdf.detach(),
                                                                                 z, gd, gc, tr, ray_mask=mask)))
                arrays["masked_depth"], arrays["masked_color"], arrays["masked_sdf"], arrays["masked_z"] = (
                    cpu(depth), cpu(color), cpu(sdf), cpu(z))
            save(f"render_{case}_{layout}", **arrays)
            del r, arrays
    fx = hp.load("room0_200x40_tracking")
    out, r = fused_losses(fx, [True])
    save("tracking", depth=cpu(r["depth"]), **out)
    del r

    # ---- (2) properties of the fixed-point scatter --------------------------------------------------------------------------
    def reindex(wl, idx):
        """The workload's batch <- its rays `idx` (a permutation, a slice, a repetition), with their depths, colours,
        random numbers and cotangents."""
        for name in ("rays_o", "rays_d", "gt_depth", "gt_color"):
            setattr(wl, name, getattr(wl, name).detach()[idx].contiguous())
        wl._rand = tuple(t[idx].contiguous() for t in wl._rand)
        wl._cot = tuple(t[idx].contiguous() for t in wl._cot)
        wl.R = int(idx.shape[0])

    def run_wl(wl):
        out = wl.forward()
        grads = wl.backward_with(out)
        torch.cuda.synchronize()
        return [t.detach().clone() for t in out], grads

    def batch_arrays(wl, out, grads, prefix=""):
        a = {prefix + "rays_o": cpu(wl.rays_o), prefix + "rays_d": cpu(wl.rays_d), prefix + "gt_depth": cpu(wl.gt_depth),
             prefix + "cot_depth": cpu(wl._cot[0]), prefix + "cot_color": cpu(wl._cot[1]), prefix + "cot_sdf": cpu(wl._cot[2])}
        for n, t in zip(("depth", "color", "sdf", "z"), out):
            a[prefix + n] = cpu(t)
        for k, v in wl.decoders.state_dict().items():
            a["param:" + k] = cpu(v)
        a["beta"] = np.float64(float(wl.decoders.beta))
        for k, g in enumerate(grads):
            a[f"{prefix}g{k}"] = cpu(g)
        return a

    def compare(out_a, grads_a, out_b, grads_b, arrays, tag, inv=None, scale_b=1.0):
        """Bit differences of run b against run a (rays of b taken back to a's order by `inv`; a's gradients times scale_b)."""
        for n, a, b in zip(("depth", "color", "sdf", "z"), out_a, out_b):
            arrays[f"{tag}_ndiff_{n}"] = np.int64(ndiff(a, b if inv is None else b[inv]))
        for k, (a, b) in enumerate(zip(grads_a, grads_b)):
            nd = ndiff(a * scale_b, b)
            arrays[f"{tag}_ndiff_g{k}"] = np.int64(nd)
            arrays[f"{tag}_relerr_g{k}"] = np.float64(float((a.double() * scale_b - b.double()).abs().max() /
                                                            ((a.double() * scale_b).abs().max() + 1e-30)))
            if nd and k < 12:
                arrays[f"{tag}_g{k}"] = cpu(b)

    # ray permutation (10 % of the rays without depth, trained-like state)
    wl = harness.make_workload("room0", 1500, 24, 8, device=dev, zero_frac=0.1, planes="synth", state="trained")
    out_a, grads_a = run_wl(wl)
    arrays = batch_arrays(wl, out_a, grads_a)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(wl.R)).to(dev)
    inv = torch.argsort(perm)
    reindex(wl, perm)
    out_b, grads_b = run_wl(wl)
    compare(out_a, grads_a, out_b, grads_b, arrays, "perm", inv=inv)
    save("prop_permutation", n_params=np.int64(len(grads_a)), **arrays)
    del wl

    # contention: 128 rays, and the same 128 rays 64 times over
    for state in ("initial", "trained"):
        wl = harness.make_workload("room0", 400, 24, 8, device=dev, planes="synth", state=state)
        assert wl.R >= 128, wl.R
        reindex(wl, torch.arange(128, device=dev))
        out_a, grads_a = run_wl(wl)
        arrays = batch_arrays(wl, out_a, grads_a)
        rep = torch.arange(128, device=dev).repeat(CONTENTION_K)
        reindex(wl, rep)
        out_b, grads_b = run_wl(wl)
        tiled = [t.repeat(CONTENTION_K, *([1] * (t.dim() - 1))) for t in out_a]       # every copy of a ray against the single batch
        compare(tiled, grads_a, out_b, grads_b, arrays, "rep", scale_b=float(CONTENTION_K))
        save(f"prop_contention_{state}", n_params=np.int64(len(grads_a)), **arrays)
        del wl

    # layout: channels-last against NCHW planes, strided kernels and relayout path
    runs = {}
    for layout, relayout in LAYOUTS.items():
        ops._RELAYOUT_MIN_POINTS = relayout_default if relayout is None else relayout
        wl = harness.make_workload("room0", 1000, 24, 8, device=dev, zero_frac=0.1, planes="synth", state="trained",
                                   channels_last=(layout == "cl"))
        runs[layout] = run_wl(wl)
        ops._RELAYOUT_MIN_POINTS = relayout_default
        if layout == "cl":
            arrays = batch_arrays(wl, *runs[layout])
        else:
            compare(*runs["cl"], *runs[layout], arrays, layout)
        del wl
    save("prop_layout", n_params=np.int64(len(runs["cl"][1])), **arrays)
    del runs

    # out-of-range contributions: one ray's cotangent x 2^50, then inf; baseline = that ray's cotangent zero
    wl = harness.make_workload("room0", 300, 24, 8, device=dev, planes="synth", state="trained")
    j = wl.R // 2
    cot = wl._cot

    def with_ray(factor):
        new = tuple(t.clone() for t in cot)
        for t in new:
            if factor == float("inf"):
                t[j] = factor
            else:
                t[j] *= factor
        wl._cot = new
        return run_wl(wl)
    out_a, grads_a = with_ray(0.0)
    arrays = batch_arrays(wl, out_a, grads_a)
    arrays["ray"] = np.int64(j)
    arrays["ray_cot_depth"], arrays["ray_cot_color"], arrays["ray_cot_sdf"] = cpu(cot[0][j]), cpu(cot[1][j]), cpu(cot[2][j])
    for tag, factor in (("big", BIG_SCALE), ("inf", float("inf")), ("clean", 0.0)):
        _, grads_b = with_ray(factor)
        for k in range(12):
            a, b = grads_a[k].contiguous().view(-1), grads_b[k].contiguous().view(-1)
            idx = torch.nonzero(a.view(torch.int32) != b.view(torch.int32)).view(-1)
            arrays[f"{tag}_idx{k}"] = cpu(idx)                  # flat positions (logical NCHW) whose bits differ from the baseline
            arrays[f"{tag}_val{k}"] = cpu(b[idx])
    save("prop_out_of_range", **arrays)
    del wl

    # ---- (3) decode mode ---------------------------------------------------------------------------------------------------
    from myslam_amd.src.networks.decoders import Decoders
    fxd = hp.load("decoders_room0_points")
    sc = scn.make_scene("room0")

    def decode_run(pts, wts):
        planes = tuple([p.requires_grad_(True) for p in grp] for grp in scn.synth_planes(sc, device=dev))
        dec = Decoders()
        dec.load_state_dict({k[6:]: torch.from_numpy(fxd[k]) for k in fxd.files if k.startswith("param:")})
        dec = dec.to(dev)
        dec.bound = sc.bound
        p = torch.from_numpy(pts).to(dev).requires_grad_(True)
        raw = dec(p, all_planes=planes)
        (raw * torch.from_numpy(wts).to(dev)).sum().backward()
        torch.cuda.synchronize()
        return raw.detach(), p.grad, [q.grad for q in hp.flat_planes(planes)], {k: t.grad for k, t in dec.named_parameters() if k != "beta"}

    for N in DECODE_NS:
        pts = decode_points(N, sc)
        wts = np.linspace(0.5, 1.5, N * 4, dtype=np.float32).reshape(N, 4)
        raw, g_pts, pg, dg = decode_run(pts, wts)
        arrays = dict(points=pts, wts=wts, raw=cpu(raw), g_points=cpu(g_pts),
                      bundle_samples=np.int64(lib.eslam_scatter_bundle_samples(N, 0, 0)))
        for k, g in enumerate(pg):
            arrays[f"pg{k}"] = cpu(g)
        for k, g in dg.items():
            arrays["dg:" + k] = cpu(g)
        if N == DECODE_NS[-1]:          # the permutation property for points
            perm = np.random.default_rng(6).permutation(N)
            raw_b, _, pg_b, _ = decode_run(pts[perm], wts[perm])
            arrays["perm_ndiff_raw"] = np.int64(ndiff(raw[torch.from_numpy(perm).to(dev)], raw_b))
            for k, (a, b) in enumerate(zip(pg, pg_b)):
                arrays[f"perm_ndiff_pg{k}"] = np.int64(ndiff(a, b))
                arrays[f"perm_relerr_pg{k}"] = np.float64(float((a.double() - b.double()).abs().max() / (a.double().abs().max() + 1e-30)))
        save(f"decode_{N}", **arrays)

    # ---- shadow hygiene: the child's first case once more, after everything above -------------------------------------------
    again = [p.grad for p in hp.flat_planes(run_hip(hp.load(SCRATCH_SEQUENCE[0]))["planes"])]
    arrays = {}
    for k, (a, b) in enumerate(zip(first_grads, again)):
        arrays[f"ndiff_pg{k}"] = np.int64(ndiff(a, b))
        arrays[f"relerr_pg{k}"] = np.float64(float((a.double() - b.double()).abs().max() / (a.double().abs().max() + 1e-30)))
    save("hygiene", **arrays)

    with open(os.path.join(out_dir, "done.json"), "w") as f:
        json.dump({"det": det, "seconds": time.time() - t_start, "scratch_calls": len(scratch_log)}, f)


if __name__ == "__main__":
    main(sys.argv[1])
