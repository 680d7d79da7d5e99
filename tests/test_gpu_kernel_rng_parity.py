"""The default path - the sampler that draws its own uniform numbers (eslam_sample_z_all_rng), the compiled host glue that
calls it, and the step bench.py times (harness.Workload.step under harness.GraphedStep) - against the float64 oracle.

The in-kernel numbers are a counter-based hash of (key, device step counter, stream, global ray index, element);
tests/rng_ref.py regenerates them on the host exactly (tests/test_rng_ref.py pins that replica without a GPU).  So:

  1. the in-kernel entry must equal the injected entry (`_rand=`, eslam_sample_z_all) fed the replica's numbers BIT FOR BIT -
     z_vals of all rays and the rendered depth / colour / sdf (same kernel instantiation, same arithmetic, no atomics in the
     forward) - over sizes, shares of depth-less rays, consecutive steps, keys, perturb on / off, ray offsets up to the
     ABI's limit, both host glues and both plane layouts; and z_vals must match orc.sample_z in float64 on the same numbers
     at the bars of test_gpu_parity.test_edge_shapes_against_oracle;
  2. every step and every graph replay must match loss and all gradients of autograd over the oracle AT ITS OWN STEP of the
     counter, at the bars test_gpu_parity.test_whole_gradient_tensors_at_full_size holds the injected path to;
  3. what `bench.py --dump-outputs` writes must be those oracle-checked tensors.

No tolerance of its own: everything is exact equality or a bar the suite already holds for injected numbers.

Run time, measured on an MI355X: 70 s for the module, 39 s of it the float64 / float32 oracle of the 8192 x 96 batch and
25 s the oracle of the other steps, on the host; the GPU work is a few seconds.  The one child process (bench.py) has a
time limit of its own.
"""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import rng_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4
BENCH_CHILD_TIMEOUT = 600           # seconds, as tests/test_gpu_callers.py::test_bench_plain_line_and_dumped_outputs

SIZES = [(1, 24, 8), (7, 3, 1), (130, 100, 28), (33, 16, 0), (1500, 24, 8), (4096, 56, 8)]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _workload(R, ns, ni, zero_frac, scene="room0", **kw):
    """A harness workload with exactly R rays (the AABB pre-filter drops some of those asked for)."""
    from myslam_amd import harness
    wl = harness.make_workload(scene, max(R, 8) * 4 if R < 1000 else R + R // 2, ns, ni, device=_dev(), zero_frac=zero_frac, **kw)
    assert wl.R >= R, (wl.R, R)
    wl.sl = slice(0, R)
    return wl


def _key_and_step(dev, explicit=None):
    """(key, step) the NEXT sampler call draws with: the library's key - which must be the replica's independent statement of
    it - and the device counter read after the key is settled (a new key restarts the counter when it is first used)."""
    from myslam_amd import ops
    key = ops._rng_seed(dev)
    assert key == rng_ref.key_for(dev, explicit), (key, rng_ref.key_for(dev, explicit))
    return key, int(ops._rng_state(dev)[0])


def _numbers(key, step, R, ns, ni, dev, lo=0, perturb=True):
    t_rand, t_uni, u = (torch.from_numpy(a).to(dev) for a in rng_ref.sampler_numbers(key, step, R, ns, ni, ray_offset=lo))
    return (t_rand, t_uni, u) if perturb else (None, None, u)


def _render(wl, rand=None, sl=None, grad=True):
    """depth, colour, sdf, z_vals of one render call, detached.  grad=True: as a training call renders (the forward kernel that
    also saves what the backward needs); grad=False: under torch.no_grad()."""
    sl = wl.sl if sl is None else sl
    with torch.set_grad_enabled(grad):
        out = wl.renderer.render_batch_ray(wl.planes, wl.decoders, wl.rays_d[sl], wl.rays_o[sl], wl.device, wl.truncation,
                                           gt_depth=wl.gt_depth[sl], _rand=rand)
    return tuple(t.detach() for t in out)


def _assert_bit_equal(a, b, what):
    bad = [(name, int((x != y).sum()), float((x - y).abs().max())) for name, x, y in zip(("depth", "colour", "sdf", "z_vals"), a, b)
           if x.shape != y.shape or not torch.equal(x, y)]
    assert not bad, (what, bad)


def _glues(monkeypatch):
    """(name, switch) of the two host paths of a render call: the compiled glue (eslam_torch_ext, the default) and the Python /
    ctypes glue (the switch test_gpu_parity.test_compiled_host_glue_equals_python_path uses)."""
    from myslam_amd import ops
    ext = ops.torch_ext()
    assert ext is not None, "eslam_torch_ext is not built: the default path cannot be tested"
    return [("compiled", lambda: monkeypatch.setattr(ops, "_ext_mod", ext)), ("python", lambda: monkeypatch.setattr(ops, "_ext_mod", None))]


# ---- 1. the in-kernel entry against the injected entry ----------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
@pytest.mark.parametrize("R,ns,ni", SIZES)
def test_in_kernel_entry_equals_injected_entry_bit_for_bit(R, ns, ni, layout, monkeypatch):
    """Three consecutive renders per configuration without re-seeding: the counter reads k, k + 1, k + 2 and each render
    equals the injected entry fed the replica's numbers of its own step - z_vals of every ray (with depth: stream 0; without:
    streams 1 and 2) and the rendered outputs, bit for bit.  zero_frac 0 / 0.3 / 1 exercises the streams alone and together;
    n_strat, S and n_imp differ, so a row stride taken from the wrong count shows from row 1 on."""
    from myslam_amd import ops
    dev = _dev()
    glues = _glues(monkeypatch)
    try:
        for zero_frac in (0.0, 0.3, 1.0):
            wl = _workload(R, ns, ni, zero_frac, channels_last=(layout == "channels_last"), state="trained")
            n_zero = int((wl.gt_depth[wl.sl] == 0).sum())
            assert n_zero == 0 if zero_frac == 0.0 else n_zero == R if zero_frac == 1.0 else (0 < n_zero < R or R < 33)
            for glue, switch in glues:
                switch()
                seed = 1000 * R + 10 * ns + int(zero_frac * 10) + (glue == "python")
                ops.seed(seed)
                key, k0 = _key_and_step(dev, seed)
                assert k0 == 0
                prev = None
                for k in range(3):
                    assert int(ops._rng_state(dev)[0]) == k
                    mine = _render(wl)
                    assert int(ops._rng_state(dev)[0]) == k + 1, "one advance of the step counter per rendered batch"
                    ref = _render(wl, _numbers(key, k, R, ns, ni, dev))
                    assert int(ops._rng_state(dev)[0]) == k + 1, "a render with injected numbers leaves the counter alone"
                    _assert_bit_equal(mine, ref, (zero_frac, glue, "step", k))
                    assert mine[3].shape == (R, ns + ni) and bool((mine[3][:, 1:] >= mine[3][:, :-1]).all())
                    if prev is not None:
                        assert not torch.equal(prev, mine[3]), "fresh numbers every step"
                    prev = mine[3]
                # Under torch.no_grad() the compiled glue launches the forward kernel that saves nothing, the Python glue (every
                # call with injected numbers) the one that saves features and raw colour: with strided NCHW planes the two
                # instantiations round the last bit of some sdf / colour values differently (measured: <= 1.5e-7 absolute on
                # 16 % of the sdf values of 33 x 16 trained-like rays; none with channels-last planes).  z_vals stay bit-equal;
                # the rendered outputs are held to 1e-6 there.
                key, k = _key_and_step(dev, seed)
                mine, ref = _render(wl, grad=False), _render(wl, _numbers(key, k, R, ns, ni, dev), grad=False)
                assert torch.equal(mine[3], ref[3]), (zero_frac, glue, "no_grad z_vals")
                for name, a, b in zip(("depth", "colour", "sdf"), mine, ref):
                    assert hp.rel_err(a.cpu().numpy(), b.cpu().numpy()) <= 1e-6, (zero_frac, glue, "no_grad", name)
    finally:
        ops.seed(None)


@pytest.mark.parametrize("R,ns,ni,zero_frac,state", [(1, 24, 8, 0.0, "initial"), (7, 3, 1, 1.0, "trained"), (130, 100, 28, 0.3, "trained"),
                                                     (33, 16, 0, 0.3, "initial"), (1500, 24, 8, 0.3, "trained"), (4096, 56, 8, 0.3, "initial")])
def test_in_kernel_z_vals_against_the_float64_oracle_sampler(R, ns, ni, zero_frac, state):
    """z_vals of the DEFAULT entry against orc.sample_z in float64 fed the replica's numbers, at a step other than 0: ties the
    in-kernel entry to the reference's sampler (Renderer.py:85-134), not only to its sibling entry.  Bars of
    test_edge_shapes_against_oracle: rays with depth equal after rounding to float32 or within 1e-6, depth-less rays 1e-4."""
    from oracle import eslam_oracle as orc
    from myslam_amd import ops
    dev = _dev()
    wl = _workload(R, ns, ni, zero_frac, planes="synth", state=state)
    seed = (0x5EED << 32) | (R * 131 + ns)
    try:
        ops.seed(seed)
        _render(wl)
        _render(wl)
        key, step = _key_and_step(dev, seed)
        assert step == 2
        z = _render(wl)[3].cpu()
    finally:
        ops.seed(None)
    cv = lambda t: t.detach().cpu().double()
    planes = tuple([cv(p).contiguous() for p in grp] for grp in wl.planes)
    params = {k: cv(v) for k, v in wl.decoders.state_dict().items() if k != "beta"}
    gd = cv(wl.gt_depth[wl.sl])
    nums = [torch.from_numpy(a).double() for a in rng_ref.sampler_numbers(key, step, R, ns, ni)]
    zo = orc.sample_z(cv(wl.rays_o[wl.sl]), cv(wl.rays_d[wl.sl]), gd, planes, params, cv(wl.decoders.beta), wl.scene.bound.double(),
                      wl.truncation, ns, ni, *nums)
    has = gd > 0
    if zero_frac > 0 and R >= 33:
        assert has.any() and (~has).any()
    if has.any():
        e = hp.rel_err(z[has].numpy(), zo[has].numpy())
        print(f"z_vals vs float64 oracle, rays with depth: {e:.2e}")
        assert torch.equal(z[has], zo.float()[has]) or e <= 1e-6, e
    if (~has).any():
        e = hp.rel_err(z[~has].numpy(), zo[~has].numpy())
        print(f"z_vals vs float64 oracle, depth-less rays: {e:.2e}")
        assert e <= RTOL, e


def test_keys_perturb_off_and_unconsumed_samples(monkeypatch):
    """Keys: ops.seed below 2^32, with only high bits, with both (k1 = key_hi + ... matters), and the default key folded from
    torch.manual_seed and torch.cuda.manual_seed - each equals the replica's own statement of the folding and gives its own
    samples.  perturb=False: only the importance draw is used.  Samples never consumed by a forward (ops.sample_z alone) are
    followed by a render one step on, and the counter ends one past that."""
    from myslam_amd import ops
    dev = _dev()
    R, ns, ni = 1500, 24, 8
    wl = _workload(R, ns, ni, 0.3, state="trained")
    try:
        for glue, switch in _glues(monkeypatch):
            switch()
            seen = []
            for seed in (5, 0xABCD << 40, 0xDEADBEEF12345678, None):
                ops.seed(seed)
                if seed is None:
                    torch.manual_seed(1234)
                    torch.cuda.manual_seed(5)
                    assert rng_ref.key_for(dev) == (1234 * 0x9E3779B97F4A7C15 + 5) % (1 << 64)
                key, step = _key_and_step(dev, seed)
                assert step == 0
                mine = _render(wl)
                _assert_bit_equal(mine, _render(wl, _numbers(key, 0, R, ns, ni, dev)), (glue, "key", seed))
                mine = _render(wl)
                _assert_bit_equal(mine, _render(wl, _numbers(key, 1, R, ns, ni, dev)), (glue, "key", seed, "step 1"))
                assert all(not torch.equal(mine[3], z) for z in seen)
                seen.append(mine[3])
            # perturb off: no jitter on either kind of ray, the importance draw as ever
            ops.seed(31)
            key, _ = _key_and_step(dev, 31)
            wl.renderer.perturb = False
            try:
                for k in range(2):
                    mine = _render(wl)
                    _assert_bit_equal(mine, _render(wl, _numbers(key, k, R, ns, ni, dev, perturb=False)), (glue, "perturb off", k))
                with_jitter = _render(wl, _numbers(key, 1, R, ns, ni, dev))
                assert not torch.equal(mine[3], with_jitter[3])
            finally:
                wl.renderer.perturb = True
            # samples that no forward consumes: each later draw is one step on
            ops.seed(63)
            key, _ = _key_and_step(dev, 63)
            _render(wl)                                                    # step 0, consumed
            sl = wl.sl
            args = (wl.rays_o[sl], wl.rays_d[sl], wl.gt_depth[sl], wl.planes, wl.decoders, wl.renderer._bound6, wl.truncation, ns, ni, True)
            z_a = ops.sample_z(*args)                                      # step 1, never rendered
            assert int(ops._rng_state(dev)[0]) == 1
            z_b = ops.sample_z(*args)                                      # step 2, never rendered
            assert int(ops._rng_state(dev)[0]) == 2
            assert int(ops.rng_step_snapshot(dev)[0]) == 3                 # what the next call will draw with
            mine = _render(wl)                                             # step 3
            assert int(ops._rng_state(dev)[0]) == 4
            for k, z in ((1, z_a), (2, z_b), (3, mine[3])):
                assert torch.equal(z, ops.sample_z(*args, rand=_numbers(key, k, R, ns, ni, dev))), (glue, "unconsumed", k)
            _assert_bit_equal(mine, _render(wl, _numbers(key, 3, R, ns, ni, dev)), (glue, "after unconsumed samples"))
    finally:
        ops.seed(None)


@pytest.mark.parametrize("R,ns,ni", [(7, 3, 1), (130, 100, 28)])
def test_ray_offset_up_to_the_abi_limit(R, ns, ni, monkeypatch):
    """A slice rendered under ops.ray_offset(lo) draws rows lo .. lo + R of the whole batch's numbers, up to the last offset
    the ABI admits ((lo + R) * S just under 2^32, eslam_sample_z_all_rng); one ray further the call fails with the ABI's
    error instead of returning samples from wrapped indices."""
    from myslam_amd import ops
    dev = _dev()
    S = ns + ni
    lo = (1 << 32) // S - 1 - R
    assert (lo + R) * S < (1 << 32) <= (lo + 1 + R) * S
    wl = _workload(R, ns, ni, 0.3, state="trained")
    try:
        for glue, switch in _glues(monkeypatch):
            switch()
            for off in (500, lo):
                ops.seed(4321)
                key, step = _key_and_step(dev, 4321)
                with ops.ray_offset(off):
                    mine = _render(wl)
                assert int(ops._rng_state(dev)[0]) == step + 1
                _assert_bit_equal(mine, _render(wl, _numbers(key, step, R, ns, ni, dev, lo=off)), (glue, "offset", off))
                if off == 500:
                    assert not torch.equal(mine[3], _render(wl, _numbers(key, step, R, ns, ni, dev))[3])
            with pytest.raises(RuntimeError, match="out of range"):
                with ops.ray_offset(lo + 1):
                    _render(wl)
            torch.cuda.synchronize()
    finally:
        ops.seed(None)


def test_loss_set_sizes_equal_the_counts_of_replica_fed_samples():
    """eslam_loss_set_sizes with in-kernel numbers: its five counts equal parallel.set_sizes_from_z, on the host, of the z_vals
    the injected entry forms from the replica's numbers of the same key and step - one unmasked and one masked batch."""
    from myslam_amd import ops, parallel
    dev = _dev()
    R, ns, ni = 1500, 24, 8
    wl = _workload(R, ns, ni, 0.1)
    sl = wl.sl
    gd = wl.gt_depth[sl]
    g = torch.Generator().manual_seed(1)
    keep = (torch.rand(R, generator=g) > 0.3).to(dev)
    cs = list(parallel._ACC_COUNT_SLOTS)
    try:
        ops.seed(808)
        _render(wl)                                                        # (a step other than 0)
        for mask in (None, keep):
            key, step = _key_and_step(dev, 808)
            acc = ops.loss_set_sizes(gd, mask, ns, ni, wl.truncation, True).cpu()
            assert int(ops._rng_state(dev)[0]) == step, "counting draws no step"
            z = _render(wl, _numbers(key, step, R, ns, ni, dev))[3]
            want = parallel.set_sizes_from_z(z.cpu(), gd.cpu(), wl.truncation, None if mask is None else mask.cpu())
            assert torch.equal(acc[cs], want[cs]), (acc[cs], want[cs])
            assert float(acc[cs].min()) > 0
            _render(wl)                                                    # the masked batch counts at the next step
    finally:
        ops.seed(None)


# ---- 2. the benchmarked step against the float64 oracle -----------------------------------------------------------------------
def _oracle_step(wl, z, dtype):
    """Loss and every parameter gradient of one mapping iteration on the CPU: orc.render_batch_ray on the given z_vals +
    orc.mapping_loss + autograd.  Gradients in the order of wl.params()."""
    from oracle import eslam_oracle as orc
    cv = lambda t: t.detach().cpu().to(dtype)
    planes = tuple([cv(p).contiguous().requires_grad_(True) for p in grp] for grp in wl.planes)
    named = [(k, cv(v).requires_grad_(True)) for k, v in wl.decoders.named_parameters()]
    params = {k: v for k, v in named if k != "beta"}
    beta = dict(named)["beta"] if "beta" in dict(named) else float(wl.decoders.beta)
    gd, gc = cv(wl.gt_depth), cv(wl.gt_color)
    d, c, s, zz = orc.render_batch_ray(planes, params, beta, wl.scene.bound, cv(wl.rays_d), cv(wl.rays_o), wl.truncation, gd,
                                       wl.n_strat, wl.n_imp, z_vals=cv(z))
    loss = orc.mapping_loss(d, c, s, zz, gd, gc, wl.truncation)
    loss.backward()
    return dict(loss=float(loss), planes=planes, params=params, plane_grads=[p.grad.numpy() for p in hp.flat_planes(planes)],
                dec_grads=[(k, v.grad.numpy()) for k, v in named])


def _check_step_against_oracle(wl, key, step, loss, grads, tag, margins=None):
    """What a step left behind - loss (float) and the gradients in the order of wl.params() - against the oracle at `step`:
    loss to 1e-4 relative (check_against_fixture's bar), the 12 plane gradients whole through helpers.plane_grads_close with
    helpers.ambiguous_samples and the cap on their share, decoder and beta gradients through helpers.elementwise_vs_oracles
    with the floor test_whole_gradient_tensors_at_full_size uses."""
    from oracle import eslam_oracle as orc
    from myslam_amd import ops
    dev = wl.device
    # z_vals from the injected entry on the replica's numbers (section 1 shows it bit-equal to what the step drew itself)
    z = ops.sample_z(wl.rays_o, wl.rays_d, wl.gt_depth, wl.planes, wl.decoders, wl.renderer._bound6, wl.truncation, wl.n_strat,
                     wl.n_imp, True, rand=_numbers(key, step, wl.R, wl.n_strat, wl.n_imp, dev)).cpu()
    o64 = _oracle_step(wl, z, torch.float64)
    o32 = _oracle_step(wl, z, torch.float32)
    e = abs(loss - o64["loss"]) / abs(o64["loss"])
    print(f"[{tag}] step {step}: loss {loss:.8f} oracle {o64['loss']:.8f} ratio {e / RTOL:.3f}")
    if margins is not None:
        margins.append(("loss", e / RTOL))
    assert e <= RTOL, (tag, step, loss, o64["loss"])
    pts = (wl.rays_o.detach().cpu().double()[:, None, :] + wl.rays_d.detach().cpu().double()[:, None, :] * z.double()[..., None]).reshape(-1, 3)
    pn = orc.normalize_points(pts, wl.scene.bound.double())
    amb = hp.ambiguous_samples(pn, tuple([p.detach() for p in grp] for grp in o64["planes"]), {k: v.detach() for k, v in o64["params"].items()})
    print(f"[{tag}] step {step}: ambiguous samples {int(amb.sum())} of {amb.numel()} (cap {2e-3 * amb.numel():.0f})")
    report = []
    ok, msg = hp.plane_grads_close([g.cpu().numpy() for g in grads[:12]], o32["plane_grads"], o64["plane_grads"], pn, amb,
                                   wl.scene.plane_shapes, RTOL, report=report)
    for k, r in report:
        print(f"[{tag}] step {step}: plane {k:2d} ratio {r:.3f}")
        if margins is not None:
            margins.append((f"plane {k}", r))
    assert ok, (tag, step, msg, int(amb.sum()))
    assert int(amb.sum()) <= 2e-3 * amb.numel()               # the exclusion stays an exception
    names = [k for k, _ in wl.decoders.named_parameters()]
    assert len(grads) == 12 + len(names)
    for (k, g32), (_, g64), g in zip(o32["dec_grads"], o64["dec_grads"], grads[12:]):
        r = hp.elementwise_vs_oracles(k, g.cpu().numpy(), g32, g64, 3e-5, RTOL)
        print(f"[{tag}] step {step}: {k} ratio {r:.3f}")
        if margins is not None:
            margins.append((k, r))


def _fresh_counter(dev):
    """Forget the key the library last used, so that the next sampler call restarts the step counter at 0 as a new process
    would, whatever ran before in this one."""
    from myslam_amd import ops
    ops.seed(None)
    ops._rng_seed(dev)
    assert int(ops._rng_state(dev)[0]) == 0


# Image / pixel seed of the reduced (1024-ray) workloads.  The share of ReLU-ambiguous samples is a property of the oracle
# and the inputs alone: in the trained-like state it is 1.5e-3 - 2.3e-3 per step at 1024 rays (98 - 151 of 65536 samples, measured
# with the oracle for seeds 0 - 5 at steps 0 - 8), around the 2e-3 cap, and seed 0 exceeds the cap at step 3 (135 > 131).
# Seed 1 stays below it at every step these tests look at (step 0: 119; steps 3 - 6: 104, 116, 121, 117).
# What one such sample does where nothing sets it aside, measured at seed 0, step 0 (117 ambiguous samples): the gradient of
# c_linears.0.weight is 6.90e-4 (of its largest element) from the float64 oracle, all of it in the row of ONE hidden unit -
# and so, to three digits and in the same row, is the float32 oracle evaluated with torch on the GPU; the float32 oracle
# on the CPU puts that unit on the other side of its ReLU and sits 2.78e-4 away.  The decoder comparator's bound, 1.5 x the
# distance between the CPU's two oracles, is then 4.2e-4 and is missed by a correct float32 evaluation.  The step with
# in-kernel numbers and the step with the same numbers injected give bit-identical decoder gradients there.
REDUCED_SEED = {"initial": 0, "trained": 1}


def _bench_workload(cfg, R=None, seed=0, **kw):
    from myslam_amd import harness
    return harness.make_workload(cfg["scene"], cfg["rays"] if R is None else R, cfg["n_strat"], cfg["n_imp"], device=_dev(),
                                 zero_frac=cfg["zero_frac"], seed=seed, **kw)


def _graphed_replays(wl, n_replays, until=None):
    """harness.GraphedStep over wl.step as bench.py builds it; replays it n_replays times (or until the counter reads `until`)
    and returns (key, [(step the replay drew with, loss, gradients copied)]): the counter must advance by exactly one per replay."""
    from myslam_amd import harness, ops
    dev = wl.device
    _fresh_counter(dev)
    warm = inspect.signature(harness.GraphedStep.__init__).parameters["warmup"].default
    step = harness.GraphedStep(wl.step, wl.params())
    key, c = _key_and_step(dev)
    assert c == warm, "each eager warm-up step advances the counter by one, the capture itself by none"
    out = []
    while len(out) < n_replays if until is None else c < until:
        loss = step()
        torch.cuda.synchronize()
        c1 = int(ops._rng_state(dev)[0])
        assert c1 == c + 1, "one advance of the step counter per replay"
        assert all(p.grad is not None for p in wl.params())
        out.append((c, float(loss), [p.grad.detach().clone() for p in wl.params()]))
        c = c1
    return key, out


@pytest.mark.parametrize("state", ["initial", "trained"])
def test_graph_replays_match_the_oracle_each_at_its_own_step(state):
    """bench.py's scene and sample counts at 1024 rays, captured as bench.py captures it, four replays: each replay's loss and
    whole gradient tensors match the oracle on the numbers of ITS step - not if gradients accumulate in the static p.grad
    buffers, the counter is baked into the graph, or a replay repeats the captured numbers.  "trained": the state in which
    later samples of a ray carry compositing weight (harness.Workload)."""
    import bench
    wl = _bench_workload(bench.SINGLE, R=1024, state=state, seed=REDUCED_SEED[state])
    key, reps = _graphed_replays(wl, 4)
    losses = [l for _, l, _ in reps]
    assert len(set(losses)) == 4, losses
    for c, loss, grads in reps:
        _check_step_against_oracle(wl, key, c, loss, grads, f"graph 1024 {state}")


def test_eager_step_matches_the_oracle():
    """The same comparison once for wl.step() issued eagerly (no graph), in the trained-like state."""
    import bench
    from myslam_amd import ops
    wl = _bench_workload(bench.SINGLE, R=1024, state="trained", seed=REDUCED_SEED["trained"])
    dev = wl.device
    _fresh_counter(dev)
    key, c = _key_and_step(dev)
    assert c == 0
    loss = wl.step()
    torch.cuda.synchronize()
    assert int(ops._rng_state(dev)[0]) == 1
    _check_step_against_oracle(wl, key, c, float(loss), [p.grad.detach().clone() for p in wl.params()], "eager 1024 trained")


def test_eager_step_at_the_strong_scaling_shape_matches_the_oracle():
    """bench.STRONG's batch (scene0000, 8192 x 96, 10 % depth-less rays: the importance stream at scale) through wl.step
    unsharded, one step at a step other than 0."""
    import bench
    from myslam_amd import ops
    wl = _bench_workload(bench.STRONG)
    dev = wl.device
    assert int((wl.gt_depth == 0).sum()) > 0.05 * wl.R
    _fresh_counter(dev)
    wl.step()
    key, c = _key_and_step(dev)
    assert c == 1
    loss = wl.step()
    torch.cuda.synchronize()
    assert int(ops._rng_state(dev)[0]) == 2
    _check_step_against_oracle(wl, key, c, float(loss), [p.grad.detach().clone() for p in wl.params()], "eager 8192x96")


# ---- 3. the full-size step as bench.py runs it, and the CLI's dump ----------------------------------------------------------------
BENCH_ARGS = {"--steps": 3, "--warmup": 2}


@pytest.fixture(scope="module")
def full_size_run():
    """bench.SINGLE (4096 x 64) under GraphedStep, replayed until the counter reads what a `bench.py --warmup 2 --steps 3`
    process reaches: GraphedStep's own warm-up steps + --warmup + --steps, each advancing the counter by one (asserted in
    _graphed_replays, not assumed).  Returns the workload, key and the LAST replay - the one bench.py dumps."""
    import bench
    from myslam_amd import harness
    wl = _bench_workload(bench.SINGLE)
    warm = inspect.signature(harness.GraphedStep.__init__).parameters["warmup"].default
    target = warm + BENCH_ARGS["--warmup"] + BENCH_ARGS["--steps"]
    key, reps = _graphed_replays(wl, None, until=target)
    assert len(reps) == BENCH_ARGS["--warmup"] + BENCH_ARGS["--steps"] >= 4 and reps[-1][0] == target - 1
    assert len(set(l for _, l, _ in reps)) == len(reps)
    return wl, key, reps[-1]


def test_full_size_graph_replay_matches_the_oracle(full_size_run):
    """The workload bench.py times, in its own state, the last of five replays: loss and whole gradient tensors against the
    oracle at that replay's step.  Prints value / bar per tensor (profiles/parity_margins_kernel_rng.txt records a run)."""
    wl, key, (c, loss, grads) = full_size_run
    assert wl.R * wl.S > 200_000
    margins = []
    _check_step_against_oracle(wl, key, c, loss, grads, "graph 4096x64", margins)
    for name, r in margins:
        print(f"margin 4096x64 replay at step {c}: {name:24s} {r:.3f}")


def test_bench_cli_dumps_the_oracle_checked_step(full_size_run, tmp_path):
    """`bench.py --steps 3 --warmup 2 --dump-outputs DIR` in a child process: the loss and gradients it writes equal those of
    the replay at the same counter value in this process (checked against the oracle above) to the order of the float
    atomics - the promise of --dump-outputs that inputs and seeds are fixed, across processes."""
    import bench
    wl, key, (c, loss, grads) = full_size_run
    assert key == 0, "harness.Workload seeds both of torch's generators with model_seed = 0, so every process folds the same key"
    child_dir, mine_dir = str(tmp_path / "child"), str(tmp_path / "mine")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")]
    for k, v in BENCH_ARGS.items():
        cmd += [k, str(v)]
    out = subprocess.run(cmd + ["--dump-outputs", child_dir], capture_output=True, text=True, timeout=BENCH_CHILD_TIMEOUT, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "capture failed" not in out.stderr, out.stderr[-2000:]          # (an eager run would stand at another step)
    outs = bench.step_outputs(torch.tensor(loss, dtype=torch.float32), wl.planes, wl.decoders, wl.params(), grads)
    bench.dump_outputs(outs, mine_dir)
    files = sorted(os.listdir(child_dir))
    assert files == sorted(os.listdir(mine_dir)) and "loss.npy" in files and len(files) == 1 + len(wl.params())
    for f in files:
        a, b = np.load(os.path.join(child_dir, f)), np.load(os.path.join(mine_dir, f))
        assert a.shape == b.shape and np.abs(b).max() > 0, f
        assert hp.rel_err(a, b) <= 1e-5, (f, hp.rel_err(a, b))
