"""torch.autograd glue around the C-ABI kernels.  PyTorch is plumbing here (device memory, streams, the
autograd graph the reference's Mapper/Tracker call .backward() on); all arithmetic is in the HIP library.

Nothing in this file computes on the CPU: tensors that are not on a GPU raise.
"""
import ctypes
import math
import os
import sys

import torch

from . import _hip

_const_cache = {}


def _cached(key, make):
    t = _const_cache.get(key)
    if t is None:
        t = make()
        _const_cache[key] = t
    return t


def beta_tensor(beta, device):
    """decoders.beta is an nn.Parameter or the Python int 10 (reference decoders.py:59-62)."""
    if torch.is_tensor(beta):
        return beta
    dev = torch.device(device)
    return _cached(("beta", float(beta), dev.index), lambda: torch.full((1,), float(beta), device=dev))


def linspace01(n, device):
    dev = torch.device(device)
    return _cached(("lin", n, dev.index), lambda: torch.linspace(0.0, 1.0, steps=n, device=dev))


def decoder_params(decoders):
    """The 12 tensors in C-ABI order from our Decoders or the reference's (same attribute names).  Walking the
    ModuleLists costs ~12 us; the list is remembered on the module and checked by identity of its first and last
    entries (nn.Module.to() / _apply replace the Parameter objects, load_state_dict copies in place)."""
    hit = decoders.__dict__.get("_eslam_param_list")
    if hit is not None and hit[0] is decoders.linears[0].weight and hit[11] is decoders.c_output_linear.bias:
        return hit
    lst = _decoder_params_slow(decoders)
    decoders.__dict__["_eslam_param_list"] = lst
    return lst


def _decoder_params_slow(decoders):
    return [decoders.linears[0].weight, decoders.linears[0].bias, decoders.linears[1].weight,
            decoders.linears[1].bias, decoders.output_linear.weight, decoders.output_linear.bias,
            decoders.c_linears[0].weight, decoders.c_linears[0].bias, decoders.c_linears[1].weight,
            decoders.c_linears[1].bias, decoders.c_output_linear.weight, decoders.c_output_linear.bias]


_bound_last = None


def bound_to_host(bound):
    """[3,2] tensor (the reference keeps decoders.bound on the CPU, ESLAM.py:173) -> 6 floats.  The last tensor's values are
    remembered (same object, same version counter: a render call asks twice per iteration)."""
    global _bound_last
    if torch.is_tensor(bound):
        last = _bound_last
        if last is not None and last[0] is bound and last[1] == bound._version:
            return last[2]
        vals = tuple(float(v) for v in bound.detach().reshape(-1).tolist())
        _bound_last = (bound, bound._version, vals)
        return vals
    return tuple(float(v) for v in bound)


def _c(t):
    return t if t is None or t.is_contiguous() else t.contiguous()


def _split_planes(flat12):
    return tuple([flat12[2 * g], flat12[2 * g + 1]] for g in range(6))


_grad_sink = None


class grad_sink:
    """Context manager: RenderFn.backward writes plane / decoder / beta gradients into the views of a
    parallel.FlatGrads (params = 12 planes, 12 decoder tensors, [beta]) instead of fresh buffers, so a data-parallel
    caller can all-reduce one flat buffer with no copy in between.  Enter it around the backward pass; the FORWARD pass of
    that call must have run inside this context or inside ops.keep_layout() (either keeps the render call on the Python
    glue, whose backward looks the sink up - the compiled glue, eslam_torch_ext, hands its gradients to autograd)."""

    def __init__(self, flat_grads):
        self.fg = flat_grads

    def __enter__(self):
        global _grad_sink
        self._prev, _grad_sink = _grad_sink, self.fg
        return self.fg

    def __exit__(self, *a):
        global _grad_sink
        _grad_sink = self._prev


_grad_layout_cache = {}
_grad_reuse = {}


def _alloc_plane_grads(planes, zero=True):
    """One flat zero buffer, 12 views with the planes' own strides (so autograd can adopt them without a copy
    and a multi-GPU caller can all-reduce the flat buffer).  zero=False: uninitialised (the caller clears it)."""
    key = tuple((tuple(p.shape), p.stride()) for p in planes)
    layout = _grad_layout_cache.get(key)
    if layout is None:
        off, layout = 0, []
        for p in planes:
            if not (p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last)):
                raise RuntimeError("planes must be dense (contiguous or channels_last)")
            layout.append((tuple(p.shape), p.stride(), off))
            off += p.numel()
        layout = _grad_layout_cache[key] = (layout, off)
    entries, total = layout
    dev = planes[0].device
    # The previous call's buffer and its 12 views are handed out again when NOBODY else holds them any more (the caller dropped
    # the gradients: optimizer.zero_grad(set_to_none=True), p.grad = None): 13 tensor constructions (~30 us of host time per
    # iteration) become 12 reference-count reads.  A view that is still somebody's .grad keeps its count up, and a fresh
    # buffer is built.
    ck = (key, dev.index)
    old = _grad_reuse.get(ck)
    if old is not None and not torch.cuda.is_current_stream_capturing():
        flat, views = old
        # the LIST is what an autograd node of a forward pass without its backward yet holds on to (ctx.pregrads); the ELEMENTS
        # are what became somebody's .grad.  Counts: cache tuple + local + argument (list); list + loop variable + argument (views)
        if sys.getrefcount(views) == 3 and all(sys.getrefcount(v) == 3 for v in views):
            if zero:
                flat.zero_()
            return flat, views
    flat = (torch.zeros if zero else torch.empty)(total, device=dev, dtype=torch.float32)
    views = [torch.as_strided(flat, shp, st, off) for shp, st, off in entries]
    if not torch.cuda.is_current_stream_capturing():
        _grad_reuse[ck] = (flat, views)
    return flat, views


def _flat_views(planes, memory_format):
    """One uninitialised flat buffer + 12 views of the planes' shapes in `memory_format` (dense)."""
    dev = planes[0].device
    total = sum(p.numel() for p in planes)
    flat = torch.empty(total, device=dev, dtype=torch.float32)
    views, off = [], 0
    for p in planes:
        n, c, h, w = p.shape
        st = (c * h * w, 1, c * w, c) if memory_format == torch.channels_last else (c * h * w, h * w, w, 1)
        views.append(torch.as_strided(flat, tuple(p.shape), st, off))
        off += p.numel()
    return flat, views


def _relayout(src, dst, field):
    """eslam_planes_relayout between two lists of 12 tensors (field 0: values; field 1: the tensors are gradients)."""
    dev = src[0].device
    a, _ = _hip.make_planes(_split_planes(src), src if field else None, remember=False)
    b, _ = _hip.make_planes(_split_planes(dst), dst if field else None, remember=False)
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_planes_relayout(a, b, int(field), _hip.stream_handle(dev)), "eslam_planes_relayout")


class ChannelsLastFn(torch.autograd.Function):
    """12 channels-last scratch copies = ChannelsLastFn.apply(*12 planes in the reference's NCHW layout, ESLAM.py:199-210).

    Forward: one launch (eslam_planes_relayout).  Backward: the gradients the render kernels scattered into channels-last
    buffers go back to the planes' own layout in one launch, so `p.grad.stride() == p.stride()` for the caller's optimiser.
    Nothing is kept across calls: the mapper swaps the plane Parameters every frame (Mapper.py:254-266)."""

    @staticmethod
    def forward(ctx, *planes):
        for k, p in enumerate(planes):
            _hip.require_gpu_f32(f"plane {k}", p)
            if not p.is_contiguous():
                raise RuntimeError("planes must be dense (contiguous or channels_last)")
        src = [p.detach() for p in planes]
        _, views = _flat_views(src, torch.channels_last)
        _relayout(src, views, 0)
        ctx.shapes = [tuple(p.shape) for p in planes]
        ctx.device = planes[0].device
        return tuple(views)

    @staticmethod
    def backward(ctx, *grads):
        if all(g is None for g in grads):
            return (None,) * 12
        if any(g is None for g in grads):           # (the render backward produces all 12 or none)
            grads = [g if g is not None else torch.zeros(shp, device=ctx.device).contiguous(memory_format=torch.channels_last)
                     for g, shp in zip(grads, ctx.shapes)]
        grads = [g if g.is_contiguous(memory_format=torch.channels_last) else g.contiguous(memory_format=torch.channels_last)
                 for g in grads]
        _, out = _flat_views(grads, torch.contiguous_format)
        _relayout(list(grads), out, 1)
        return tuple(out)


# Planes in the reference's NCHW layout are copied to channels-last scratch per call when the batch has at least this many
# points (below, the direct strided kernels are cheaper than moving 2 x 27-70 MB); ESLAM_NCHW_RELAYOUT_MIN=-1 disables it
_RELAYOUT_MIN_POINTS = int(os.environ.get("ESLAM_NCHW_RELAYOUT_MIN", "4096"))


_keep_layout = 0


class keep_layout:
    """Context manager: no per-call layout change inside (a caller that hands the kernels gradient buffers in the planes' own
    strides - parallel.ShardedMapper's flat exchange buffer - needs the kernels to see the planes as they are)."""

    def __enter__(self):
        global _keep_layout
        _keep_layout += 1

    def __exit__(self, *a):
        global _keep_layout
        _keep_layout -= 1


def wants_relayout(all_planes, n_points):
    """Whether this call should run on per-call channels-last copies of the planes: they are in the reference's NCHW layout
    and the batch is large enough to pay for the copies."""
    flat = [p for grp in all_planes for p in grp]
    if _keep_layout or _RELAYOUT_MIN_POINTS < 0 or n_points < _RELAYOUT_MIN_POINTS or len(flat) != 12:
        return False
    if all(p.dim() == 4 and p.shape[2] * p.shape[3] > 1 and p.is_contiguous(memory_format=torch.channels_last) for p in flat):
        return False
    # (anything else: let the kernels' own validation speak)
    return all(p.is_cuda and p.dtype == torch.float32 and p.dim() == 4 and p.is_contiguous() for p in flat)


def planes_for_kernels(all_planes, n_points):
    """all_planes as the kernels should see them: unchanged when channels-last (or the batch is small), else per-call
    channels-last scratch copies that carry the gradient back to the caller's planes (ChannelsLastFn)."""
    if not wants_relayout(all_planes, n_points):
        return all_planes
    return _split_planes(ChannelsLastFn.apply(*[p for grp in all_planes for p in grp]))


_DEC_SIZES = [16 * 64, 16, 16 * 16, 16, 16, 1, 16 * 64, 16, 16 * 16, 16, 48, 3]


def _split_dec_grads(g_dec):
    parts = g_dec.split(_DEC_SIZES)
    return [t.view(shape) if len(shape) > 1 else t for t, (_, _, shape) in zip(parts, _hip.DEC_FIELDS)]


_dec_param_cache = {}


_side_streams = {}


def ray_order_async(rays_o, rays_d, grad_planes=None):
    """Launch eslam_ray_order_clear on a side stream (the order depends only on the rays, so it overlaps the samplers; the
    gradient buffer's clear is a second role of the same launch).
    Returns (perm int32 [3 R + 4]: one order per plane orientation + the fan's extent, stream to join before the order is used[, gradient views]).
    grad_planes: the 12 planes when the coming backward pass will need their gradient buffer: it is allocated here and
    cleared at the HEAD of the side stream, beside the samplers (27 - 70 MB: 6 - 15 us in front of the backward pass
    otherwise; beside the forward kernel the memset's writes slowed the forward down by more than that)."""
    _hip.require_gpu_f32("rays_o", rays_o)
    _hip.require_gpu_f32("rays_d", rays_d)
    dev = rays_o.device
    ro, rd = _c(rays_o.detach()), _c(rays_d.detach())
    R = ro.shape[0]
    side = _side_streams.get(dev.index)
    if side is None:
        side = _side_streams[dev.index] = torch.cuda.Stream(device=dev)
    perm = torch.empty(_hip.ray_order_words(R), dtype=torch.int32, device=dev)      # one order per plane orientation (+ the fan's extent)
    pre = None
    if grad_planes is not None and _grad_sink is None and not _keep_layout:      # (keep_layout: a sink will take the gradients)
        pre = _alloc_plane_grads(grad_planes, zero=False)      # on the caller's stream: its allocator's memory
    _hip.stream_wait(dev, side, None)           # the rays - and any earlier use of that memory - come from work on the caller's stream
    with _hip.on_device(dev):
        # one launch: the order's workgroups in front, the gradient buffer's clear behind them
        _hip.check(_hip.lib().eslam_ray_order_clear(_hip.ptr(ro), _hip.ptr(rd), R, _hip.ptr(perm),
                                                    None if pre is None else _hip.ptr(pre[0]),
                                                    0 if pre is None else pre[0].numel() * 4,
                                                    ctypes.c_void_p(side.cuda_stream)), "eslam_ray_order_clear")
    perm.record_stream(side)
    for t, src in ((ro, rays_o), (rd, rays_d)):
        if t.data_ptr() != src.data_ptr():
            t.record_stream(side)        # a contiguous copy made on the current stream and read on the side stream
    return (perm, side) if pre is None else (perm, side, pre[1])


def step_front_ok(n_strat, rand):
    """Whether a training call may take the one-launch front: the sampler draws its own random numbers (as ext_render_ok asks),
    and nobody else owns the gradient buffer or the random-number step (the ray-sharded mapper keeps its own prologue)."""
    return (rand is None and _USE_KERNEL_RNG and n_strat >= 3 and _grad_sink is None and not _keep_layout and
            _rng_override is None)


def step_front(rays_o, rays_d, gt_depth, flat_planes, decoders, bound6, truncation, n_strat, n_imp, perturb):
    """The front of a training step as ONE launch on the current stream (eslam_step_front): the three ray orders, the clear of
    the plane-gradient buffer (allocated here) and the samplers' z_vals - what ray_order_async + sample_z do in two launches
    on two streams.  Nothing is forked, so nothing has to be joined.
    Returns (z_vals [R, S], perm int32 [3 R + 4], the 12 pre-cleared gradient views)."""
    _hip.require_gpu_f32("rays_o", rays_o)
    _hip.require_gpu_f32("rays_d", rays_d)
    _hip.require_gpu_f32("gt_depth", gt_depth)
    if not step_front_ok(n_strat, None):
        raise RuntimeError("ops.step_front: needs the in-kernel random numbers, n_stratified >= 3 and no gradient sink; use "
                           "ray_order_async + sample_z")
    dev = rays_o.device
    ro, rd, gd = _c(rays_o.detach()), _c(rays_d.detach()), _c(gt_depth.detach().reshape(-1))
    R = gd.shape[0]
    z = torch.empty(R, n_strat + n_imp, device=dev)
    perm = torch.empty(_hip.ray_order_words(R), dtype=torch.int32, device=dev)
    pre = _alloc_plane_grads(flat_planes, zero=False)
    t_free, t_surf = linspace01(n_strat, dev), linspace01(n_imp, dev)
    seed_v = _rng_seed(dev)
    state = _rng_state(dev)
    if _rng_pending.get(dev.index, False):
        state[0] += 1                  # the previous samples were never rendered: advance the step here
    arr, _ = _hip.make_planes(flat_planes)
    dec, keep = _hip.make_decoders(decoder_params(decoders), beta_tensor(decoders.beta, dev))
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_step_front(arr, ctypes.byref(dec), _hip.make_bound(bound6), _hip.ptr(ro), _hip.ptr(rd),
                                               _hip.ptr(gd), R, n_strat, n_imp, float(truncation), _hip.ptr(t_free),
                                               _hip.ptr(t_surf), 1 if perturb else 0, seed_v, _hip.ptr(state), _ray_offset,
                                               _hip.ptr(z), _hip.ptr(perm), _hip.ptr(pre[0]), pre[0].numel() * 4,
                                               _hip.stream_handle(dev)), "eslam_step_front")
    _rng_pending[dev.index] = True
    return z, perm, pre[1]


_fused_loss = None

# A float32 render call that will be back-propagated also saves the decoders' first hidden layer (128 bytes per sample beside
# the 512 of the features), and its backward reads it instead of rebuilding it from the features: same bits, 16 of the
# decoder backward's 52 MFMAs per 16 samples less.  The renderer's saved_hidden keyword (a plain argument all the way down to
# RenderFn.apply and the compiled render()) gives a call the recompute kernels; the mixed-precision and free-point paths never
# save it.  `with ops.saved_hidden(False):` changes what a call WITHOUT the keyword does - a process-wide default, for code
# that cannot reach the call (not for threads that want different settings: pass the keyword there).
SAVED_HIDDEN_DEFAULT = True
_saved_hidden = None


class saved_hidden:
    """Context manager: the default of render calls inside that give no saved_hidden keyword; None = SAVED_HIDDEN_DEFAULT."""

    def __init__(self, on):
        self.on = None if on is None else bool(on)

    def __enter__(self):
        global _saved_hidden
        self.prev, _saved_hidden = _saved_hidden, self.on
        return self

    def __exit__(self, *exc):
        global _saved_hidden
        _saved_hidden = self.prev
        return False


def saved_hidden_on():
    return SAVED_HIDDEN_DEFAULT if _saved_hidden is None else _saved_hidden


def saved_hidden_floats(R, S):
    """Floats of the saved first hidden layer of an [R, S] render call: 2 * R * ceil(S / 16) * 256."""
    return int(_hip.lib().eslam_saved_hidden_floats(int(R), int(S)))


def require_saved_hidden(hid, R, S):
    """The backward of a call that saved its hidden layer: refuse a missing or short buffer before anything is launched."""
    want = saved_hidden_floats(R, S)
    if hid is None:
        raise RuntimeError(f"saved hidden layer: the forward pass left no buffer ({want} floats for {R} x {S} samples expected)")
    if hid.dtype != torch.float32 or not hid.is_contiguous() or hid.numel() < want:
        raise RuntimeError(f"saved hidden layer: {hid.numel()} {hid.dtype} elements, {want} contiguous float32 needed for "
                           f"{R} x {S} samples")
    return hid


# The compiled host glue of a render call (myslam_amd/csrc/eslam_torch_ext.cpp, `make torch_ext`): optional - the Python code below
# is the general path and does the same through ctypes.  ESLAM_TORCH_EXT=0 switches it off.
_EXT_WANTED = os.environ.get("ESLAM_TORCH_EXT", "1") != "0"
_ext_mod = False


def torch_ext():
    """The eslam_torch_ext module, or None when it is switched off or not built."""
    global _ext_mod
    if _ext_mod is False:
        _ext_mod = None
        path = os.path.join(os.path.dirname(_hip.LIB_PATH), "eslam_torch_ext.so")
        if _EXT_WANTED and os.path.exists(path) and not os.environ.get("ESLAM_HIP_LIB"):
            import importlib.util
            _hip.load_library()                      # (the module links against libeslam_hip.so: resolve it from the same file)
            spec = importlib.util.spec_from_file_location("eslam_torch_ext", path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            if mod.abi_version() != _hip.ABI_VERSION:
                raise RuntimeError(f"eslam_torch_ext was built against ABI {mod.abi_version()}, the binding expects {_hip.ABI_VERSION}: "
                                   "run `make -C myslam_amd/csrc torch_ext`")
            _ext_mod = mod
    return _ext_mod


def ext_render_ok(rays_o, n_strat, rand):
    """Whether a render call may take the compiled path: the common case only (see eslam_torch_ext.cpp's header)."""
    return (rand is None and _USE_KERNEL_RNG and n_strat >= 3 and _half_planes is None and _grad_sink is None and not _keep_layout and
            _rng_override is None and rays_o.is_cuda and torch_ext() is not None)


def ext_render(cfg, rays_o, rays_d, gt_depth, beta, flat_planes, dec_params, n_strat, n_imp, fl, relayout=False, saved_hidden=None,
               forked_front=False):
    """One compiled call: [planes -> channels-last scratch when `relayout`,] the front (ray order, gradient clear and sampler as
    one launch; forked_front: order + clear on a side stream, joined behind the forward), forward (+ the loss's sums).  fl: the active ops.fused_loss context or None.  Returns depth, rgb, sdf, z_vals."""
    dev = rays_o.device
    seed_v = _rng_seed(dev)
    state = _rng_state(dev)
    if _rng_pending.get(dev.index, False):
        state[0] += 1                  # samples drawn earlier were never rendered
        _rng_pending[dev.index] = False
    ext = torch_ext()
    keep_h = saved_hidden_on() if saved_hidden is None else bool(saved_hidden)
    with _hip.on_device(dev):
        if fl is None:
            outs = ext.render(cfg, rays_o, rays_d, gt_depth, beta, flat_planes, dec_params, linspace01(n_strat, dev), linspace01(n_imp, dev),
                              state, seed_v, _ray_offset, relayout=relayout, saved_hidden=keep_h, forked_front=bool(forked_front))
        else:
            mask = fl.ray_mask
            if mask is not None:
                mask = _c(mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8))
            outs = ext.render(cfg, rays_o, rays_d, gt_depth, beta, flat_planes, dec_params, linspace01(n_strat, dev), linspace01(n_imp, dev),
                              state, seed_v, _ray_offset, fl.gt_color, mask, _loss_scratch(dev, rays_o.shape[0]), fl.acc_out,
                              list(fl.state.weights5), relayout, keep_h, bool(forked_front))
            fl.loss, fl.acc = outs[4], outs[5]
            fl.value = outs[4].detach()
    return outs[0], outs[1], outs[2], outs[3]


class _LossState:
    __slots__ = ("truncation", "weights5", "rewrite_value", "gt_depth", "gt_color", "ray_mask", "acc", "value", "acc_global")

    def __init__(self, truncation, weights5, rewrite_value):
        self.truncation, self.weights5, self.rewrite_value = float(truncation), tuple(float(v) for v in weights5), rewrite_value
        self.gt_depth = self.gt_color = self.ray_mask = self.acc = self.value = self.acc_global = None


class fused_loss:
    """Context manager: the next Renderer.render_batch_ray renders WITH the callers' loss: the forward kernel forms the
    loss's sums in its epilogue (eslam_render_fwd_loss) and the backward kernel forms the loss's gradients itself
    (eslam_render_bwd_loss) - no loss launches at all, and depth / rgb / sdf gradients never touch memory.
    After the call `.acc` [16], `.value` [1] and `.loss` (a 0-d tensor connected to the autograd graph: call
    .backward() on it, or pass the context as losses.mapping_loss(..., precomputed=ctx), which returns it) are set.
    A ray-sharded caller all-reduces `.acc` in place before the backward; the backward then also rewrites `.value` with
    the global loss.  Mapping-style loss only (the tracker's outlier mask depends on the rendered depth itself)."""

    def __init__(self, gt_depth, gt_color, truncation, weights5, ray_mask=None, rewrite_value=False, acc_out=None):
        self.gt_depth, self.gt_color, self.truncation, self.weights5, self.ray_mask = gt_depth, gt_color, truncation, weights5, ray_mask
        self.acc = self.value = self.loss = None
        self.acc_out = acc_out          # optional float32 [16] the forward kernel writes the sums and set sizes into
        # what the backward needs, in an object of its own: the autograd node keeps THIS alive, not the context, which
        # holds .loss and would otherwise close a reference cycle around the saved activations (134 MB at 4096 x 64)
        self.state = _LossState(truncation, weights5, rewrite_value)

    @property
    def acc_global(self):
        return self.state.acc_global

    @acc_global.setter
    def acc_global(self, t):
        self.state.acc_global = t

    def __enter__(self):
        global _fused_loss
        self._prev, _fused_loss = _fused_loss, self
        return self

    def __exit__(self, *a):
        global _fused_loss
        _fused_loss = self._prev


def current_fused_loss():
    return _fused_loss


_half_planes = None
_half_ray_grads = False
_half_points = False


class mixed_precision:
    """Context manager: Renderer.render_batch_ray calls issued inside run the mixed-precision kernels (BASELINE.json
    configs[4]: texels gathered from float16 copies of the planes, decoders on bf16 MFMA forward and backward, float32
    accumulation everywhere, plane gradients accumulated in float32 for the float32 masters).  half: a lowp.HalfPlanes (or any
    object with `.flat`, the 12 float16 channels_last copies in all_planes order) - refresh it after every optimiser step.
    ray_grads=True: rays that require grad (pose optimisation: tracking, joint mapping) get their gradients from the half
    copies as well (coord_bwd_lowp_kernel) - the derivative of what the forward pass interpolated.  The default refuses such
    rays, as before this was built: a caller that did not ask keeps its error.
    points=True: the free-point calls issued inside run on the copies too - DecodeFn (Decoders.forward, get_raw_sdf,
    get_raw_rgb; saved features bf16, backward with gradients for points, planes and decoders), decode_sdf_only,
    Mesher.eval_points and sdf_grid, and through them Mesher.extract_mesh / get_mesh: the mesh is that of the field that was
    trained and rendered.  The default leaves those calls on the float32 masters, bit for bit as outside the context.
    Planes that are not channels-last raise (the per-call scratch copies of planes_for_kernels have no half counterpart)."""

    def __init__(self, half, ray_grads=False, points=False):
        self.half = half
        self.ray_grads = bool(ray_grads)
        self.points = bool(points)

    def __enter__(self):
        global _half_planes, _half_ray_grads, _half_points
        self._prev, _half_planes = (_half_planes, _half_ray_grads, _half_points), self.half
        _half_ray_grads, _half_points = self.ray_grads, self.points
        return self.half

    def __exit__(self, *a):
        global _half_planes, _half_ray_grads, _half_points
        _half_planes, _half_ray_grads, _half_points = self._prev


def points_half(geometry_only=False):
    """The float16 copies a free-point call issued now runs on (the 12 in all_planes order; geometry_only: the six geometry
    planes twice, as the SDF-only entries take them), or None: outside ops.mixed_precision(half, points=True)."""
    if _half_planes is None or not _half_points:
        return None
    flat = list(_half_planes.flat)
    return flat[:6] + flat[:6] if geometry_only else flat


def join_ray_order(device):
    """Make the current stream wait for the ray-ordering side stream.  RenderFn joins it in its backward; a caller that
    captures forward and backward into SEPARATE hipGraphs must join inside the forward's capture (parallel.py)."""
    side = _side_streams.get(torch.device(device).index)
    if side is not None:
        _hip.stream_wait(torch.device(device), None, side)


# In-kernel random numbers of the samplers (eslam_sample_z_all_rng): a step counter per device, read by the sampler and
# advanced by the forward kernel that consumes its samples.  ESLAM_TORCH_RAND=1 restores the torch.rand pool.
_USE_KERNEL_RNG = os.environ.get("ESLAM_TORCH_RAND", "0") != "1"
_rng_pending = {}


def _rng_state(dev):
    return _cached(("rng_state", dev.index), lambda: torch.zeros(4, dtype=torch.int32, device=dev))


# Reproducibility contract of the in-kernel random numbers (the jitter of Renderer.py:59 and the importance draw of
# common.py:59 when nobody injects them): U = hash(key, step, stream, GLOBAL ray index, element).
#   key   ops.seed(s) if called, else torch's seeds: the CPU generator's (torch.manual_seed) folded with the device
#         generator's (torch.cuda.manual_seed) - re-seeding either gives a new key;
#   step  a device counter the forward kernel advances; it restarts at 0 whenever the key changes, so seeding twice with
#         the same value reproduces the same samples (a captured graph bakes the key in: re-seed before capturing);
#   ray   ops.ray_offset(lo) + local index: the ranks of a ray-sharded iteration draw what the unsharded batch draws.
_explicit_seed = None
_rng_key = {}
_ray_offset = 0


def seed(value):
    """Key the in-kernel random numbers explicitly (None: back to torch's seeds).  The step counter restarts."""
    global _explicit_seed
    _explicit_seed = None if value is None else int(value) & 0xFFFFFFFFFFFFFFFF
    _rng_key.clear()


def _rng_seed(dev):
    if _explicit_seed is not None:
        key = _explicit_seed
    else:
        gen = torch.cuda.default_generators[dev.index]
        key = (torch.initial_seed() * 0x9E3779B97F4A7C15 + gen.initial_seed()) & 0xFFFFFFFFFFFFFFFF
    if _rng_key.get(dev.index) != key:
        if not torch.cuda.is_current_stream_capturing():      # (a fill captured into a graph would restart the counter per replay)
            _rng_key[dev.index] = key
            _rng_state(dev).zero_()
            _rng_pending.pop(dev.index, None)
    return key


_rng_override = None


class rng_step:
    """Context manager: sampler calls issued inside read the random-number step from `state` (int32 [4], element 0) instead of
    the device's own counter, and the forward kernel does NOT advance it: the caller does (parallel.ShardedMapper advances it
    with the last launch of its iteration - its set-size replay reads the same step on another stream)."""

    def __init__(self, state):
        self.state = state

    def __enter__(self):
        global _rng_override
        self._prev, _rng_override = _rng_override, self.state

    def __exit__(self, *a):
        global _rng_override
        _rng_override = self._prev


class ray_offset:
    """Context manager: the rays of render / sampler calls issued inside are rays lo, lo + 1, ... of the iteration's whole
    batch (a ray-sharded rank rendering its slice): the in-kernel random numbers are keyed on the global index."""

    def __init__(self, lo):
        self.lo = int(lo)

    def __enter__(self):
        global _ray_offset
        self._prev, _ray_offset = _ray_offset, self.lo

    def __exit__(self, *a):
        global _ray_offset
        _ray_offset = self._prev


def rng_step_snapshot(dev, out=None):
    """A copy of the device step counter the NEXT sampler call will draw with (int32 [4]): lets loss_set_sizes run on another
    stream beside the forward kernel, which advances the live counter."""
    state = _rng_state(dev)
    if _rng_pending.get(dev.index, False):
        state[0] += 1                  # samples drawn earlier were never rendered: what the next sampler call would do
        _rng_pending[dev.index] = False
    _rng_seed(dev)                     # (a new seed restarts the counter: settle that before the copy)
    if out is None:
        return state.clone()
    out.copy_(state)
    return out


def loss_set_sizes(gt_depth, ray_mask, n_strat, n_imp, truncation, perturb, t_rand=None, out=None, state=None):
    """acc [16] with the mapping loss's five set sizes over ALL rays given (eslam_loss_set_sizes): what a ray-sharded rank
    computes for the iteration's whole batch instead of all-reducing its shard's counts.  t_rand [R,S]: injected jitter
    numbers (tests); None = the in-kernel numbers the sampler will draw for the same seed / step / global ray index - call
    it BEFORE the forward kernel that consumes the samples (that kernel advances the step), or hand it a rng_step_snapshot
    taken before as `state`."""
    _hip.require_gpu_f32("gt_depth", gt_depth)
    dev = gt_depth.device
    gd = _c(gt_depth.detach().reshape(-1))
    R = gd.shape[0]
    if ray_mask is not None:
        ray_mask = _c(ray_mask.view(torch.uint8) if ray_mask.dtype == torch.bool else ray_mask.to(torch.uint8))
    # ticket + five counters, zeroed once and left zeroed by the kernel: a slot per (device, stream) out of the pre-zeroed pool
    # the fused loss's scratch comes from (a buffer created inside a graph capture would be re-zeroed by a captured fill)
    scratch = _pooled_scratch(dev, 7 * 32, "set_sizes")
    acc = torch.empty(16, device=dev) if out is None else out
    seed_v = 0 if t_rand is not None else _rng_seed(dev)
    if state is None:
        state = _rng_state(dev)
        if t_rand is None and _rng_pending.get(dev.index, False):
            state[0] += 1              # samples drawn earlier were never rendered: the sampler below will advance the step, too
            _rng_pending[dev.index] = False
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_loss_set_sizes(_hip.ptr(gd), _hip.ptr(ray_mask), R, n_strat, n_imp, float(truncation),
                                                  _hip.ptr(linspace01(n_strat, dev)), _hip.ptr(linspace01(n_imp, dev)),
                                                  _hip.ptr(None if t_rand is None else _c(t_rand)), 1 if perturb else 0, seed_v,
                                                  _hip.ptr(state), _hip.ptr(scratch), _hip.ptr(acc), _hip.stream_handle(dev)),
                   "eslam_loss_set_sizes")
    return acc


def _take_rng_bump(dev):
    """Pointer for the forward kernel's rng_bump if the samples it renders came from the in-kernel generator."""
    if _rng_pending.pop(dev.index, False):
        return _hip.ptr(_rng_state(dev))
    return None


class RenderFn(torch.autograd.Function):
    """depth, rgb, sdf[, loss] = RenderFn.apply(rays_o, rays_d, z_vals, bound6, beta, order, lossctx, *12 planes,
                                                *12 decoder params[, saved_hidden])
    saved_hidden (optional, a bool behind the 24 tensors): whether a float32 call that will be back-propagated saves the
    decoders' first hidden layer for its backward; not given = ops.saved_hidden_on().

    Forward = eslam_render_fwd, backward = eslam_render_bwd (reference: Renderer.py:136-147 and its autograd).
    order = (perm, stream[, pre-cleared gradient views]) from ray_order_async, (perm, None, views) from step_front - made on
    this stream, nothing to join - or None.
    lossctx = an ops.fused_loss context or None.  With it the forward is eslam_render_fwd_loss, a fourth output `loss`
    (0-d) is returned, and the gradient arriving on it is turned into the rendered outputs' gradients inside the backward
    kernel (eslam_render_bwd_loss); gradients arriving on depth / rgb / sdf themselves are added as usual."""

    N_LEAD = 7           # inputs before the planes

    @staticmethod
    def forward(ctx, rays_o, rays_d, z_vals, bound6, beta, order_in, lossctx, *tensors):
        planes, params = tensors[:12], tensors[12:24]
        for n, t in (("rays_o", rays_o), ("rays_d", rays_d), ("z_vals", z_vals)):
            _hip.require_gpu_f32(n, t)
        rays_o, rays_d, z_vals = _c(rays_o.detach()), _c(rays_d.detach()), _c(z_vals.detach())
        R, S = z_vals.shape
        dev = rays_o.device
        lib = _hip.lib()
        half = None if _half_planes is None else list(_half_planes.flat)
        ctx.half = half
        arr, _ = _hip.make_planes(planes, half=half)
        dec, keep = _hip.make_decoders(params, beta)
        needs = any(ctx.needs_input_grad)
        if half is not None and not _half_ray_grads and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            raise RuntimeError("mixed precision: gradients with respect to the rays (pose) are off; ask for them with "
                               "ops.mixed_precision(half, ray_grads=True) or detach the rays")
        depth = torch.empty(R, device=dev)
        rgb = torch.empty(R, 3, device=dev)
        sdf = torch.empty(R, S, device=dev)
        raw_rgb = torch.empty(R, S, 3, device=dev) if needs else None
        # saved features: float32, or (mixed precision) the bf16 values the decoders consumed - half the bytes
        feat = torch.empty(R * S, 128, device=dev, dtype=torch.float32 if half is None else torch.bfloat16) if needs else None
        # the first hidden layer of both decoders as the forward kernel holds it (float32 planes): the backward reads it back
        ctx.extra_inputs = len(tensors) - 24
        keep_h = bool(tensors[24]) if ctx.extra_inputs else saved_hidden_on()
        ctx.saved_hidden = bool(needs and half is None and R > 0 and keep_h)
        hid = torch.empty(saved_hidden_floats(R, S), device=dev) if ctx.saved_hidden else None
        order = None
        ctx.pregrads = None
        if order_in is not None:
            order, side = order_in[0], order_in[1]
            if len(order_in) > 2 and needs:
                ctx.pregrads = order_in[2]          # cleared on the side stream (ray_order_async), joined below
            # only the backward needs the order: the forward kernel runs on the rays as given and starts as soon as the
            # samplers are done (in the order of the backward it measured slower: 119 vs 123-125 us at 4096x64 - sorted
            # neighbours hit the same L2 channels)
        fl = lossctx
        ctx.set_materialize_grads(False)
        ctx.lossctx = None
        with _hip.on_device(dev):
            if fl is None:
                _hip.check(lib.eslam_render_fwd_h(arr, ctypes.byref(dec), _hip.make_bound(bound6), _hip.ptr(rays_o),
                                                  _hip.ptr(rays_d), _hip.ptr(z_vals), R, S, _hip.ptr(depth), _hip.ptr(rgb),
                                                  _hip.ptr(sdf), _hip.ptr(raw_rgb), _hip.ptr(feat),
                                                  None, _take_rng_bump(dev), _hip.ptr(hid),
                                                  _hip.stream_handle(dev)), "eslam_render_fwd")
            else:
                _hip.require_gpu_f32("gt_depth", fl.gt_depth)
                _hip.require_gpu_f32("gt_color", fl.gt_color)
                mask = fl.ray_mask
                if mask is not None:
                    mask = _c(mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8))
                fl.acc = torch.empty(16, device=dev) if getattr(fl, "acc_out", None) is None else fl.acc_out
                fl.value = torch.empty((), device=dev)
                st = fl.state
                st.gt_depth, st.gt_color, st.ray_mask, st.acc, st.value = _c(fl.gt_depth), _c(fl.gt_color), mask, fl.acc, fl.value
                w5 = (ctypes.c_float * 5)(*st.weights5)
                _hip.check(lib.eslam_render_fwd_loss_h(arr, ctypes.byref(dec), _hip.make_bound(bound6), _hip.ptr(rays_o),
                                                       _hip.ptr(rays_d), _hip.ptr(z_vals), R, S, _hip.ptr(depth),
                                                       _hip.ptr(rgb), _hip.ptr(sdf), _hip.ptr(raw_rgb), _hip.ptr(feat),
                                                       None,
                                                       _hip.ptr(st.gt_depth), _hip.ptr(st.gt_color),
                                                       st.truncation, w5, _hip.ptr(mask),
                                                       _hip.ptr(_loss_scratch(dev, R)), _hip.ptr(fl.acc), _hip.ptr(fl.value),
                                                       _take_rng_bump(dev), _hip.ptr(hid), _hip.stream_handle(dev)),
                           "eslam_render_fwd_loss")
                ctx.lossctx = st
        if order_in is not None and side is not None:
            # join the side stream (ray order, gradient clear) BEHIND the forward kernel: the work beside it has overlapped,
            # and no fork is left dangling if this forward is never followed by a backward (or sits in a graph of its own)
            _hip.stream_wait(dev, None, side)
        if needs:
            ctx.bound6 = bound6
            ctx.order_stream = None
            ctx.save_for_backward(rays_o, rays_d, z_vals, sdf, raw_rgb, feat, order, beta, depth, rgb, *planes, *params,
                                  *(() if hid is None else (hid,)))
        if fl is not None:
            return depth, rgb, sdf, fl.value.detach()     # an alias: the state must not hold the output object itself
        return depth, rgb, sdf

    @staticmethod
    def backward(ctx, g_depth, g_rgb, g_sdf, g_loss=None):
        saved = ctx.saved_tensors
        rays_o, rays_d, z_vals, sdf, raw_rgb, feat, order, beta, depth, rgb = saved[:10]
        planes, params = saved[10:22], saved[22:34]
        R, S = z_vals.shape
        hid = None
        if ctx.saved_hidden:
            hid = require_saved_hidden(saved[34] if len(saved) > 34 else None, R, S)
        dev = rays_o.device
        lib = _hip.lib()
        if getattr(ctx, "order_stream", None) is not None:
            _hip.stream_wait(dev, None, ctx.order_stream)      # join the ordering kernel
            ctx.order_stream = None
        need = ctx.needs_input_grad
        L = RenderFn.N_LEAD
        need_planes = any(need[L:L + 12])
        need_rays = need[0] or need[1]
        grads = None
        sink = _grad_sink
        if sink is not None:
            sink.zero_()
            grads = sink.views[:12]
        elif need_planes:
            grads = getattr(ctx, "pregrads", None)
            ctx.pregrads = None
            if grads is None:
                _, grads = _alloc_plane_grads(planes)
        arr, _ = _hip.make_planes(planes, grads, half=ctx.half)
        dec, keep = _hip.make_decoders(params, beta)
        if sink is not None:
            # the 12 decoder tensors follow the planes in the flat buffer in C-ABI order = the layout of g_dec
            o = sink.offsets[12]
            g_dec = sink.flat[o:o + _hip.N_DEC_PARAMS]
            g_beta = sink.flat[sink.offsets[24]:sink.offsets[24] + 1] if len(sink.views) > 24 else \
                torch.empty(1, device=dev)
        else:
            need_dec = any(need[L + 12:L + 24])
            g_dec = torch.empty(_hip.N_DEC_PARAMS, device=dev) if need_dec else None
            g_beta = torch.empty(1, device=dev) if need[4] else None
        g_ro = torch.empty(R, 3, device=dev) if need_rays else None
        g_rd = torch.empty(R, 3, device=dev) if need_rays else None
        if R == 0:        # the C entry returns at once for an empty batch: the gradient of nothing is zero, not uninitialised
            for t in (g_dec, g_beta):
                if t is not None:
                    t.zero_()
        ws = torch.empty(lib.eslam_bwd_workspace_bytes(R * S), dtype=torch.uint8, device=dev)
        g_depth, g_rgb, g_sdf = _c(g_depth), _c(g_rgb), _c(g_sdf)
        fl = ctx.lossctx                 # a _LossState
        with _hip.on_device(dev):
            if fl is not None and g_loss is not None:
                # the loss's gradients are formed inside the backward kernel from the set sizes in acc (a ray-sharded caller
                # has put the global ones into acc_global by now)
                up = _c(g_loss.detach().reshape(1).to(torch.float32))
                w5 = (ctypes.c_float * 5)(*fl.weights5)
                _hip.check(lib.eslam_render_bwd_loss_h(
                    arr, ctypes.byref(dec), _hip.make_bound(ctx.bound6), _hip.ptr(rays_o), _hip.ptr(rays_d),
                    _hip.ptr(z_vals), R, S, _hip.ptr(sdf), _hip.ptr(raw_rgb), _hip.ptr(feat), _hip.ptr(depth), _hip.ptr(rgb),
                    _hip.ptr(fl.gt_depth), _hip.ptr(fl.gt_color), fl.truncation, w5, _hip.ptr(fl.ray_mask),
                    _hip.ptr(fl.acc if fl.acc_global is None else fl.acc_global), _hip.ptr(up), _hip.ptr(fl.value) if fl.rewrite_value else None, _hip.ptr(g_depth),
                    _hip.ptr(g_rgb), _hip.ptr(g_sdf), _hip.ptr(g_dec), _hip.ptr(g_beta), _hip.ptr(g_ro), _hip.ptr(g_rd),
                    _hip.ptr(order), _hip.ptr(ws), _hip.ptr(hid), _hip.stream_handle(dev)), "eslam_render_bwd_loss")
            else:
                _hip.check(lib.eslam_render_bwd_h(arr, ctypes.byref(dec), _hip.make_bound(ctx.bound6), _hip.ptr(rays_o),
                                                  _hip.ptr(rays_d), _hip.ptr(z_vals), R, S, _hip.ptr(sdf), _hip.ptr(raw_rgb),
                                                  _hip.ptr(feat), _hip.ptr(g_depth), _hip.ptr(g_rgb), _hip.ptr(g_sdf),
                                                  _hip.ptr(g_dec), _hip.ptr(g_beta), _hip.ptr(g_ro), _hip.ptr(g_rd),
                                                  _hip.ptr(order), _hip.ptr(ws), _hip.ptr(hid), _hip.stream_handle(dev)),
                           "eslam_render_bwd")
        if sink is not None:
            # the data-parallel caller owns .grad assignment (FlatGrads.assign): hand autograd nothing to accumulate
            return (g_ro if need[0] else None, g_rd if need[1] else None) + (None,) * (L - 2 + 24 + ctx.extra_inputs)
        dec_grads = _split_dec_grads(g_dec) if g_dec is not None else [None] * 12
        out = [g_ro if need[0] else None, g_rd if need[1] else None, None, None, g_beta if need[4] else None, None, None]
        out += [grads[i] if (need_planes and need[L + i]) else None for i in range(12)]
        out += [dec_grads[i] if need[L + 12 + i] else None for i in range(12)]
        out += [None] * ctx.extra_inputs
        return tuple(out)


class DecodeFn(torch.autograd.Function):
    """raw[N,4] = DecodeFn.apply(pts[N,3], bound6, *12 planes, *12 decoder params)   (decoders.py:127-146)"""

    @staticmethod
    def forward(ctx, pts, bound6, dummy_beta, *tensors):
        planes, params = tensors[:12], tensors[12:24]
        _hip.require_gpu_f32("p", pts)
        pts = _c(pts.detach())
        N = pts.shape[0]
        dev = pts.device
        lib = _hip.lib()
        half = points_half()
        ctx.half = half
        arr, _ = _hip.make_planes(planes, half=half)
        dec, keep = _hip.make_decoders(params, dummy_beta)
        needs = any(ctx.needs_input_grad)
        raw = torch.empty(N, 4, device=dev)
        # saved features: float32, or (mixed precision) the bf16 values the decoders consumed, as in RenderFn
        feat = torch.empty(N, 128, device=dev, dtype=torch.float32 if half is None else torch.bfloat16) if needs else None
        with _hip.on_device(dev):
            _hip.check(lib.eslam_decode_fwd(arr, ctypes.byref(dec), _hip.make_bound(bound6), _hip.ptr(pts), N, 0,
                                            _hip.ptr(raw), _hip.ptr(feat), _hip.stream_handle(dev)), "eslam_decode_fwd")
        if needs:
            ctx.bound6 = bound6
            ctx.save_for_backward(pts, raw, feat, dummy_beta, *planes, *params)
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        saved = ctx.saved_tensors
        pts, raw, feat, dummy_beta = saved[:4]
        planes, params = saved[4:16], saved[16:28]
        N = pts.shape[0]
        dev = pts.device
        lib = _hip.lib()
        need = ctx.needs_input_grad
        need_planes = any(need[3:15])
        grads = None
        if need_planes:
            _, grads = _alloc_plane_grads(planes)
        arr, _ = _hip.make_planes(planes, grads, half=ctx.half)       # the copies the forward pass read
        dec, keep = _hip.make_decoders(params, dummy_beta)
        # (frozen decoders: NULL, and the kernel skips their gradient work - as RenderFn)
        g_dec = torch.empty(_hip.N_DEC_PARAMS, device=dev) if any(need[15:27]) else None
        g_pts = torch.empty(N, 3, device=dev) if need[0] else None
        ws = torch.empty(lib.eslam_bwd_workspace_bytes(N), dtype=torch.uint8, device=dev)
        g_raw = _c(g_raw)
        with _hip.on_device(dev):
            _hip.check(lib.eslam_decode_bwd(arr, ctypes.byref(dec), _hip.make_bound(ctx.bound6), _hip.ptr(pts), N,
                                            _hip.ptr(raw), _hip.ptr(feat), _hip.ptr(g_raw), _hip.ptr(g_dec),
                                            _hip.ptr(g_pts), _hip.ptr(ws), _hip.stream_handle(dev)), "eslam_decode_bwd")
        dec_grads = _split_dec_grads(g_dec) if g_dec is not None else [None] * 12
        out = [g_pts, None, None]
        out += [grads[i] if (need_planes and need[3 + i]) else None for i in range(12)]
        out += [dec_grads[i] if need[15 + i] else None for i in range(12)]
        return tuple(out)


def decode_sdf_only(pts, bound6, all_planes, decoders):
    """Geometry planes + SDF decoder only, no autograd (reference decoders.py:87-105 under no_grad)."""
    _hip.require_gpu_f32("p", pts)
    pts = _c(pts.detach())
    N = pts.shape[0]
    dev = pts.device
    lib = _hip.lib()
    geo = tuple(all_planes[:3]) + tuple(all_planes[:3])
    arr, _ = _hip.make_planes(geo, half=points_half(geometry_only=True))
    dec, keep = _hip.make_decoders(decoder_params(decoders), beta_tensor(10, dev))
    out = torch.empty(N, device=dev)
    with _hip.on_device(dev):
        _hip.check(lib.eslam_decode_fwd(arr, ctypes.byref(dec), _hip.make_bound(bound6), _hip.ptr(pts), N, 1,
                                        _hip.ptr(out), None, _hip.stream_handle(dev)), "eslam_decode_fwd(sdf)")
    return out


def sdf_gradient(pts, bound6, all_planes, decoders, unit=False):
    """(sdf [...], grad [...,3]) of pts [...,3] world coordinates: the SDF and its gradient with respect to the point in one
    launch (eslam_sdf_grad), no autograd.  sdf is decode_sdf_only's bit for bit; grad is what autograd of that sdf gives.
    unit: rows divided by their length, zero rows kept zero.  Geometry planes + SDF decoder only, float32 (with half copies
    around, the float32 masters are read)."""
    _hip.require_gpu_f32("p", pts)
    if pts.dim() < 1 or pts.shape[-1] != 3:
        raise RuntimeError(f"p: expected points [...,3], got {tuple(pts.shape)}")
    shape = pts.shape[:-1]
    pts = _c(pts.detach().reshape(-1, 3))
    N = pts.shape[0]
    dev = pts.device
    lib = _hip.lib()
    geo = tuple(all_planes[:3]) + tuple(all_planes[:3])
    arr, _ = _hip.make_planes(geo)
    dec, keep = _hip.make_decoders(decoder_params(decoders), beta_tensor(10, dev))
    sdf = torch.empty(N, device=dev)
    grad = torch.empty(N, 3, device=dev)
    with _hip.on_device(dev):
        _hip.check(lib.eslam_sdf_grad(arr, ctypes.byref(dec), _hip.make_bound(bound6), _hip.ptr(pts), N, 1 if unit else 0,
                                      _hip.ptr(sdf), _hip.ptr(grad), _hip.stream_handle(dev)), "eslam_sdf_grad")
    return sdf.reshape(shape), grad.reshape(*shape, 3)


class SampleRaysFn(torch.autograd.Function):
    """rays_o, rays_d, depth, color = SampleRaysFn.apply(c2ws, indices, depths, colors, geom)   (common.py:87-153)"""

    @staticmethod
    def forward(ctx, c2ws, indices, depths, colors, geom):
        H0, H1, W0, W1, n, H, W, fx, fy, cx, cy = geom
        _hip.require_gpu_f32("c2ws", c2ws)
        _hip.require_gpu_f32("depths", depths)
        _hip.require_gpu_f32("colors", colors)
        c2 = _c(c2ws.detach())
        b = c2.shape[0]
        dev = c2.device
        depths, colors, indices = _c(depths), _c(colors), _c(indices)
        if depths.shape != (b, H, W) or colors.shape != (b, H, W, 3):
            raise RuntimeError(f"get_samples: depths {tuple(depths.shape)} / colors {tuple(colors.shape)} do not match "
                               f"b={b}, H={H}, W={W}")
        if indices.dtype != torch.int64 or indices.numel() != b * n:
            raise RuntimeError("get_samples: indices must be int64 [b*n]")
        ro = torch.empty(b * n, 3, device=dev)
        rd = torch.empty(b * n, 3, device=dev)
        d = torch.empty(b * n, device=dev)
        c = torch.empty(b * n, 3, device=dev)
        with _hip.on_device(dev):
            _hip.check(_hip.lib().eslam_sample_rays(_hip.ptr(indices), b, n, H0, H1, W0, W1, H, W, fx, fy, cx, cy,
                                                    _hip.ptr(c2), _hip.ptr(depths), _hip.ptr(colors), _hip.ptr(ro),
                                                    _hip.ptr(rd), _hip.ptr(d), _hip.ptr(c), _hip.stream_handle(dev)),
                       "eslam_sample_rays")
        ctx.geom = geom
        ctx.b = b
        ctx.save_for_backward(indices)
        ctx.mark_non_differentiable(d, c)
        return ro, rd, d, c

    @staticmethod
    def backward(ctx, g_ro, g_rd, _gd, _gc):
        (indices,) = ctx.saved_tensors
        H0, H1, W0, W1, n, H, W, fx, fy, cx, cy = ctx.geom
        dev = indices.device
        g = torch.empty(ctx.b, 4, 4, device=dev)
        g_ro, g_rd = _c(g_ro), _c(g_rd)
        with _hip.on_device(dev):
            _hip.check(_hip.lib().eslam_sample_rays_bwd(_hip.ptr(indices), ctx.b, n, H0, W0, W1, fx, fy, cx, cy,
                                                        _hip.ptr(g_ro), _hip.ptr(g_rd), _hip.ptr(g),
                                                        _hip.stream_handle(dev)), "eslam_sample_rays_bwd")
        return g, None, None, None, None


def image_rays(H, W, fx, fy, cx, cy, c2w):
    _hip.require_gpu_f32("c2w", c2w)
    c2 = _c(c2w.detach())
    dev = c2.device
    ro = torch.empty(H * W, 3, device=dev)
    rd = torch.empty(H * W, 3, device=dev)
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_image_rays(H, W, fx, fy, cx, cy, _hip.ptr(c2), _hip.ptr(ro), _hip.ptr(rd),
                                               _hip.stream_handle(dev)), "eslam_image_rays")
    return ro, rd


def aabb_exit(rays_o, rays_d, bound6):
    _hip.require_gpu_f32("rays_o", rays_o)
    ro, rd = _c(rays_o.detach()), _c(rays_d.detach())
    R = ro.shape[0]
    t = torch.empty(R, device=ro.device)
    with _hip.on_device(ro.device):
        _hip.check(_hip.lib().eslam_aabb_exit(_hip.ptr(ro), _hip.ptr(rd), R, _hip.make_bound(bound6), _hip.ptr(t),
                                              _hip.stream_handle(ro.device)), "eslam_aabb_exit")
    return t


def prefilter(rays_o, rays_d, gt_depth, bound6, need_depth):
    """bool [R]: the callers' AABB (+ depth) pre-filter as a mask (Mapper.py:322-328 / Tracker.py:175-182), one launch."""
    _hip.require_gpu_f32("rays_o", rays_o)
    ro, rd, gd = _c(rays_o.detach()), _c(rays_d.detach()), _c(gt_depth)
    R = ro.shape[0]
    keep = torch.empty(R, dtype=torch.uint8, device=ro.device)
    with _hip.on_device(ro.device):
        _hip.check(_hip.lib().eslam_prefilter(_hip.ptr(ro), _hip.ptr(rd), _hip.ptr(gd), R, _hip.make_bound(bound6),
                                              1 if need_depth else 0, _hip.ptr(keep), _hip.stream_handle(ro.device)),
                   "eslam_prefilter")
    return keep.view(torch.bool)


TRACKING_MASK_MAX = 8192        # ESLAM_TRACKING_MASK_MAX


def tracking_mask(depth, gt_depth, keep=None, factor=10.0):
    """bool [R]: Tracker.py:192-195, |gt_depth - depth| < factor * median over the kept rays, one launch."""
    _hip.require_gpu_f32("depth", depth)
    d, gd = _c(depth.detach()), _c(gt_depth)
    R = d.shape[0]
    if keep is not None:
        keep = _c(keep.view(torch.uint8) if keep.dtype == torch.bool else keep.to(torch.uint8))
    mask = torch.empty(R, dtype=torch.uint8, device=d.device)
    with _hip.on_device(d.device):
        _hip.check(_hip.lib().eslam_tracking_mask(_hip.ptr(d), _hip.ptr(gd), _hip.ptr(keep), R, float(factor),
                                                  _hip.ptr(mask), _hip.stream_handle(d.device)), "eslam_tracking_mask")
    return mask.view(torch.bool)


def keep_best(loss, pose, best, best_pose):
    """In place: if loss < best, best = loss and best_pose = pose (Tracker.py:304-307), without a host round trip."""
    _hip.require_gpu_f32("loss", loss)
    pose = _c(pose.detach())
    with _hip.on_device(loss.device):
        _hip.check(_hip.lib().eslam_keep_best(_hip.ptr(loss.detach()), _hip.ptr(pose), pose.numel(), _hip.ptr(best),
                                              _hip.ptr(best_pose), _hip.stream_handle(loss.device)), "eslam_keep_best")


class PoseToMatrixFn(torch.autograd.Function):
    """c2ws [b,4,4] = PoseToMatrixFn.apply(poses [b,7])   (common.py:169-181, quaternion real-first then translation)"""

    @staticmethod
    def forward(ctx, poses):
        _hip.require_gpu_f32("batch_poses", poses)
        p = _c(poses.detach())
        b = p.shape[0]
        out = torch.empty(b, 4, 4, device=p.device)
        with _hip.on_device(p.device):
            _hip.check(_hip.lib().eslam_pose_to_c2w(_hip.ptr(p), b, _hip.ptr(out), _hip.stream_handle(p.device)),
                       "eslam_pose_to_c2w")
        ctx.save_for_backward(p)
        return out

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        g = _c(g)
        gp = torch.empty_like(p)
        with _hip.on_device(p.device):
            _hip.check(_hip.lib().eslam_pose_to_c2w_bwd(_hip.ptr(p), _hip.ptr(g), p.shape[0], _hip.ptr(gp),
                                                        _hip.stream_handle(p.device)), "eslam_pose_to_c2w_bwd")
        return gp


def sample_z(rays_o, rays_d, gt_depth, all_planes, decoders, bound6, truncation, n_strat, n_imp, perturb,
             rand=None):
    """z_vals [R,S] of reference Renderer.py:85-134, sync-free: both samplers run over all rays and each skips
    the rays that belong to the other.  rand = (t_rand [R,S], t_rand_uni [R,n_strat], u [R,n_imp]) or None to
    draw them with torch.rand."""
    _hip.require_gpu_f32("gt_depth", gt_depth)
    dev = rays_o.device
    gd = _c(gt_depth.detach().reshape(-1))
    R = gd.shape[0]
    S = n_strat + n_imp
    lib = _hip.lib()
    if rand is None and _USE_KERNEL_RNG and n_strat >= 3:
        # the uniform numbers are drawn inside the sampler kernel, keyed on torch's seed and a device step counter
        z = torch.empty(R, S, device=dev)
        t_free, t_surf = linspace01(n_strat, dev), linspace01(n_imp, dev)
        seed_v = _rng_seed(dev)
        state = _rng_state(dev) if _rng_override is None else _rng_override
        if _rng_override is None and _rng_pending.get(dev.index, False):
            state[0] += 1              # the previous samples were never rendered: advance the step here
        ro, rd = _c(rays_o.detach()), _c(rays_d.detach())
        arr, _ = _hip.make_planes(all_planes)
        dec, keep = _hip.make_decoders(decoder_params(decoders), beta_tensor(decoders.beta, dev))
        with _hip.on_device(dev):
            _hip.check(lib.eslam_sample_z_all_rng(arr, ctypes.byref(dec), _hip.make_bound(bound6), _hip.ptr(ro), _hip.ptr(rd),
                                                  _hip.ptr(gd), R, n_strat, n_imp, float(truncation), _hip.ptr(t_free),
                                                  _hip.ptr(t_surf), 1 if perturb else 0, seed_v, _hip.ptr(state),
                                                  _ray_offset, _hip.ptr(z), _hip.stream_handle(dev)), "eslam_sample_z_all_rng")
        _rng_pending[dev.index] = _rng_override is None
        return z
    if rand is None:
        # one draw, three row-major blocks (the reference draws them in three calls, Renderer.py:59, common.py:59)
        n1, n2 = (R * S, R * n_strat) if perturb else (0, 0)
        pool = torch.rand(n1 + n2 + R * n_imp, device=dev)
        t_rand = pool[:n1].view(R, S) if perturb else None
        t_uni = pool[n1:n1 + n2].view(R, n_strat) if perturb else None
        u = pool[n1 + n2:].view(R, n_imp)
    else:
        t_rand, t_uni, u = (None if t is None else _c(t) for t in rand)
    z = torch.empty(R, S, device=dev)
    t_free, t_surf = linspace01(n_strat, dev), linspace01(n_imp, dev)
    with _hip.on_device(dev):
        st = _hip.stream_handle(dev)
        if u is not None and n_strat >= 3:
            # both samplers in one launch (each wave takes the rule its ray needs)
            ro, rd = _c(rays_o.detach()), _c(rays_d.detach())
            arr, _ = _hip.make_planes(all_planes)
            dec, keep = _hip.make_decoders(decoder_params(decoders), beta_tensor(decoders.beta, dev))
            _hip.check(lib.eslam_sample_z_all(arr, ctypes.byref(dec), _hip.make_bound(bound6), _hip.ptr(ro), _hip.ptr(rd),
                                              _hip.ptr(gd), R, n_strat, n_imp, float(truncation), _hip.ptr(t_free),
                                              _hip.ptr(t_surf), _hip.ptr(t_rand), _hip.ptr(t_uni), _hip.ptr(u),
                                              _hip.ptr(z), st), "eslam_sample_z_all")
        else:
            _hip.check(lib.eslam_sample_z(_hip.ptr(gd), R, n_strat, n_imp, float(truncation), _hip.ptr(t_free),
                                          _hip.ptr(t_surf), _hip.ptr(t_rand), _hip.ptr(z), st), "eslam_sample_z")
            if u is not None:        # fewer than 3 stratified samples: the importance sampler reports it as unsupported
                ro, rd = _c(rays_o.detach()), _c(rays_d.detach())
                arr, _ = _hip.make_planes(all_planes)
                dec, keep = _hip.make_decoders(decoder_params(decoders), beta_tensor(decoders.beta, dev))
                _hip.check(lib.eslam_importance_z(arr, ctypes.byref(dec), _hip.make_bound(bound6), _hip.ptr(ro),
                                                  _hip.ptr(rd), _hip.ptr(gd), R, n_strat, n_imp, _hip.ptr(t_free),
                                                  _hip.ptr(t_uni), _hip.ptr(u), _hip.ptr(z), st), "eslam_importance_z")
    return z


def loss_reduce(depth, rgb, sdf, z_vals, gt_depth, gt_color, truncation, ray_mask=None, acc=None):
    """Phase 1 of the fused loss (eslam_loss_reduce): set sizes and squared-error sums of this rank's rays accumulated
    into acc [16] (zeroed here unless given)."""
    for n, t in (("depth", depth), ("rgb", rgb), ("sdf", sdf), ("z_vals", z_vals), ("gt_depth", gt_depth),
                 ("gt_color", gt_color)):
        _hip.require_gpu_f32(n, t)
    dev = depth.device
    R, S = sdf.shape
    args = [_c(t.detach()) for t in (depth, rgb, sdf, z_vals, gt_depth, gt_color)]
    if acc is None:
        acc = torch.zeros(16, device=dev)
    else:
        acc.zero_()
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_loss_reduce(*[_hip.ptr(t) for t in args], R, S, float(truncation), _hip.ptr(ray_mask),
                                                _hip.ptr(acc), _hip.stream_handle(dev)), "eslam_loss_reduce")
    return acc


_scratch_slots = {}           # (device index, stream handle) -> scratch tensor
_scratch_pool = {}            # device index -> [pre-zeroed pool tensor, floats handed out]
_DEBUG_SCRATCH = os.environ.get("ESLAM_DEBUG_SCRATCH", "0") == "1"
_SCRATCH_POOL_FLOATS = 1 << 20        # 4 MB per device: 8 streams of 32 768-ray deterministic scratch, or ~1900 plain ones


def _loss_scratch(dev, n_rays=0):
    """The scratch of the fused loss's ticket scheme (eslam_loss_value / eslam_render_fwd_loss): zeroed once, then owned by
    the kernels, which leave it zeroed again.  ONE PER (device, stream): two streams of a process evaluating losses at the
    same time must not share the running sums.  Slots come out of a pool that is zeroed when it is created - outside any
    graph capture, by the warm-up iterations - because a buffer created inside a capture would be re-zeroed by a captured
    fill on every replay.  (torch captures every graph on one shared capture stream: graphs that are to REPLAY concurrently
    on different streams need their own slot - capture them under ops.fresh_loss_scratch().)
    ESLAM_DEBUG_SCRATCH=1 checks on the host that the ticket counter is 0 before every use (a graph aborted between the
    adds and the last ticket leaves it non-zero): one sync per loss, for debugging only."""
    t = _pooled_scratch(dev, int(_hip.lib().eslam_loss_scratch_floats(int(n_rays))), "loss")
    if _DEBUG_SCRATCH and not torch.cuda.is_current_stream_capturing():
        if int(t[:1].view(torch.int32).item()) != 0:
            reset_loss_scratch(dev)
            raise RuntimeError("loss scratch: the ticket counter was not 0 on entry - a previous loss evaluation on this stream "
                               "did not finish (aborted graph?) or two streams shared a scratch; it has been reset")
    return t


def _pooled_scratch(dev, need, tag):
    """`need` floats of scratch that were zero when handed out for the first time, one slot per (device, stream, tag)."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, _scratch_epoch, tag)
    t = _scratch_slots.get(key)
    if t is None or t.numel() < need:
        pool = _scratch_pool.get(dev.index)
        if pool is None or pool[1] + need > pool[0].numel():
            pool = _scratch_pool[dev.index] = [torch.zeros(max(_SCRATCH_POOL_FLOATS, need), device=dev), 0]
        t = pool[0][pool[1]:pool[1] + need]
        pool[1] += (need + 31) // 32 * 32
        _scratch_slots[key] = t
    return t


_scratch_epoch = 0


class fresh_loss_scratch:
    """Context manager: loss evaluations issued inside get scratch slots of their own (for a graph that will replay
    concurrently with other graphs captured on torch's shared capture stream)."""

    def __enter__(self):
        global _scratch_epoch
        self._prev = _scratch_epoch
        _scratch_epoch = fresh_loss_scratch._next = getattr(fresh_loss_scratch, "_next", 0) + 1
        return self

    def __exit__(self, *a):
        global _scratch_epoch
        _scratch_epoch = self._prev


def reset_loss_scratch(device=None):
    """eslam_loss_scratch_reset on every scratch slot (of one device): back to the freshly zeroed state."""
    for (di, _, _, tag), t in _scratch_slots.items():
        if tag == "loss" and (device is None or torch.device(device).index == di):
            with _hip.on_device(t.device):
                _hip.check(_hip.lib().eslam_loss_scratch_reset(_hip.ptr(t), t.numel(), _hip.stream_handle(t.device)),
                           "eslam_loss_scratch_reset")


class MappingLossFn(torch.autograd.Function):
    """loss = MappingLossFn.apply(depth, rgb, sdf, z_vals, gt_depth, gt_color, truncation, weights5, ray_mask, group, acc)

    Fused restatement of Mapper.py:110-144,337-346 (ray_mask None) / Tracker.py:114-148,197-204 (ray_mask given).
    forward = eslam_loss_reduce (+ the loss value); backward = eslam_loss_grad scaled by the upstream gradient inside the
    kernel.  `group`: a torch.distributed process group (or True for the default group) makes the set sizes and error
    sums global with one 16-float all-reduce, for ray-sharded data parallelism (myslam_amd/parallel.py).
    `acc`: accumulators that are already reduced (loss_reduce + the caller's own all-reduce); skips phase 1."""

    @staticmethod
    def forward(ctx, depth, rgb, sdf, z_vals, gt_depth, gt_color, truncation, weights5, ray_mask, group, acc):
        if ray_mask is not None:
            ray_mask = _c(ray_mask.view(torch.uint8) if ray_mask.dtype == torch.bool else ray_mask.to(torch.uint8))
        for n, t in (("depth", depth), ("rgb", rgb), ("sdf", sdf), ("z_vals", z_vals), ("gt_depth", gt_depth),
                     ("gt_color", gt_color)):
            _hip.require_gpu_f32(n, t)
        dev = depth.device
        R, S = sdf.shape
        args = [_c(t.detach()) for t in (depth, rgb, sdf, z_vals, gt_depth, gt_color)]
        loss = torch.empty(1, device=dev)
        w = (ctypes.c_float * 5)(*[float(v) for v in weights5])
        if isinstance(acc, tuple):
            acc, value = acc                     # both already formed by the forward kernel (ops.fused_loss)
            loss = value
        elif acc is None and group is None:
            # single GPU: sums, set sizes and the value in one launch, no pre-zeroed accumulator
            acc = torch.empty(16, device=dev)
            with _hip.on_device(dev):
                _hip.check(_hip.lib().eslam_loss_value(*[_hip.ptr(t) for t in args], R, S, float(truncation), w,
                                                       _hip.ptr(ray_mask), _hip.ptr(_loss_scratch(dev, R)), _hip.ptr(acc),
                                                       _hip.ptr(loss), _hip.stream_handle(dev)), "eslam_loss_value")
        else:
            if acc is None:
                acc = loss_reduce(depth, rgb, sdf, z_vals, gt_depth, gt_color, truncation, ray_mask)
                import torch.distributed as dist
                dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=None if group is True else group)
            with _hip.on_device(dev):
                _hip.check(_hip.lib().eslam_loss_grad(*[_hip.ptr(t) for t in args], R, S, float(truncation), w,
                                                      _hip.ptr(ray_mask), _hip.ptr(acc), _hip.ptr(loss), None, None, None,
                                                      None, _hip.stream_handle(dev)), "eslam_loss_grad(value)")
        ctx.save_for_backward(*args, acc)
        ctx.ray_mask = ray_mask
        ctx.consts = (float(truncation), tuple(float(v) for v in weights5))
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        *args, acc = ctx.saved_tensors
        dev = acc.device
        R, S = args[2].shape
        truncation, weights5 = ctx.consts
        g_depth = torch.empty(R, device=dev)
        g_rgb = torch.empty(R, 3, device=dev)
        g_sdf = torch.empty(R, S, device=dev)
        w = (ctypes.c_float * 5)(*weights5)
        g = _c(g.detach().reshape(1).to(torch.float32))
        with _hip.on_device(dev):
            _hip.check(_hip.lib().eslam_loss_grad(*[_hip.ptr(t) for t in args], R, S, truncation, w,
                                                  _hip.ptr(ctx.ray_mask), _hip.ptr(acc), None, _hip.ptr(g_depth),
                                                  _hip.ptr(g_rgb), _hip.ptr(g_sdf), _hip.ptr(g),
                                                  _hip.stream_handle(dev)), "eslam_loss_grad")
        return g_depth, g_rgb, g_sdf, None, None, None, None, None, None, None, None


# ----------------------------------------------------------------------------------------------
# meshing (reference src/utils/Mesher.py:188-262): the SDF on the marching-cubes grid, then marching cubes
# ----------------------------------------------------------------------------------------------
def sdf_grid(all_planes, decoders, axes, bound, halfspaces=None):
    """vol [nx,ny,nz] float32 on the planes' device: the SDF at (xs[ix], ys[iy], zs[iz]), -1 where the point is not
    strictly inside `bound` ([3,2]) and -1 outside the half-spaces [K,4] (n.p + d <= 0 inside).  axes: three ascending
    float32 1-D tensors (np.linspace cast to float32, Mesher.py:170-180).  The reference's volume after its
    reshape(ny, nx, nz).transpose(1, 0, 2) (Mesher.py:224-226)."""
    dev = all_planes[0][0].device
    xs, ys, zs = (_c(a.detach().to(dev, torch.float32).reshape(-1)) for a in axes)
    for n, a in zip("xyz", (xs, ys, zs)):
        _hip.require_gpu_f32(n + "s", a)
    nx, ny, nz = xs.numel(), ys.numel(), zs.numel()
    dec_bound6 = bound_to_host(decoders.bound)
    bound6 = bound_to_host(bound)
    same_bound = dec_bound6 == bound6
    hs = None
    if halfspaces is not None and halfspaces.shape[0] > 0:
        hs = _c(halfspaces.detach().to(dev, torch.float32).reshape(-1, 4))
    geo = tuple(all_planes[:3]) + tuple(all_planes[:3])
    arr, _ = _hip.make_planes(tuple([t.detach() for t in grp] for grp in geo), half=points_half(geometry_only=True))
    dec, keep = _hip.make_decoders([t.detach() for t in decoder_params(decoders)], beta_tensor(10, dev))
    vol = torch.empty(nx, ny, nz, device=dev)
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_sdf_grid(arr, ctypes.byref(dec), _hip.make_bound(dec_bound6), _hip.ptr(xs), _hip.ptr(ys),
                                             _hip.ptr(zs), nx, ny, nz, _hip.ptr(hs), 0 if hs is None else hs.shape[0],
                                             2 if same_bound else 0, _hip.ptr(vol), _hip.stream_handle(dev)),
                   "eslam_sdf_grid")
    if not same_bound:       # a mesher bound that differs from the decoders' normalisation bound (as eval_points)
        b = [(float(bound6[2 * k]), float(bound6[2 * k + 1])) for k in range(3)]
        ins = [(a > lo) & (a < hi) for a, (lo, hi) in zip((xs, ys, zs), b)]
        inside = ins[0][:, None, None] & ins[1][None, :, None] & ins[2][None, None, :]
        vol.masked_fill_(~inside, -1.0)
    return vol


def mc_workspace_bytes(shape):
    return int(_hip.lib().eslam_mc_workspace_bytes(*[int(n) for n in shape]))


def mc_count(vol, level):
    """Count phase of marching_cubes: (workspace, counts [2] int64 on the device) - nothing is synchronised."""
    _hip.require_gpu_f32("vol", vol)
    if vol.dim() != 3 or not vol.is_contiguous():
        raise RuntimeError(f"marching_cubes: vol must be a contiguous [nx,ny,nz] tensor, got {tuple(vol.shape)}")
    dev = vol.device
    ws = torch.empty(mc_workspace_bytes(vol.shape), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_mc_count(_hip.ptr(vol), *vol.shape, float(level), _hip.ptr(ws), _hip.ptr(counts),
                                             _hip.stream_handle(dev)), "eslam_mc_count")
    return ws, counts


def mc_emit(vol, level, origin, spacing, ws, n_verts, n_faces):
    dev = vol.device
    verts = torch.empty(n_verts, 3, device=dev)
    faces = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
    o3 = (ctypes.c_double * 3)(*[float(v) for v in origin])
    s3 = (ctypes.c_double * 3)(*[float(v) for v in spacing])
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_mc_emit(_hip.ptr(vol), *vol.shape, float(level), o3, s3, _hip.ptr(ws), n_verts, n_faces,
                                            _hip.ptr(verts), _hip.ptr(faces), _hip.stream_handle(dev)), "eslam_mc_emit")
    return verts, faces


def marching_cubes(vol, level, origin, spacing):
    """(verts float32 [V,3], faces int32 [F,3]) on vol's device; vol a float32 [nx,ny,nz] GPU tensor.  One vertex per
    crossing grid edge (welded), vertex = origin + (index + t) * spacing (float64 origin / spacing), faces wound so that
    (v1 - v0) x (v2 - v0) points toward values >= level.  One host sync: reading (V, F) between the two phases."""
    ws, counts = mc_count(vol, level)
    n_verts, n_faces = (int(v) for v in counts.tolist())
    return mc_emit(vol, level, origin, spacing, ws, n_verts, n_faces)


def mc_count_masked(vol, weight, level):
    """mc_count for a partly observed volume (eslam_mc_count_masked): grid points with weight > 0 are valid, a cube emits
    faces only when its eight corners are, an edge its vertex only when a fully valid cube touches it."""
    _hip.require_gpu_f32("vol", vol)
    _hip.require_gpu_f32("weight", weight)
    if vol.dim() != 3 or not vol.is_contiguous() or weight.shape != vol.shape or not weight.is_contiguous() or \
            weight.device != vol.device:
        raise RuntimeError(f"marching_cubes: vol and weight must be contiguous [nx,ny,nz] tensors of one shape on one device, "
                           f"got {tuple(vol.shape)} and {tuple(weight.shape)}")
    dev = vol.device
    ws = torch.empty(mc_workspace_bytes(vol.shape), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_mc_count_masked(_hip.ptr(vol), _hip.ptr(weight), *vol.shape, float(level), _hip.ptr(ws),
                                                    _hip.ptr(counts), _hip.stream_handle(dev)), "eslam_mc_count_masked")
    return ws, counts


def marching_cubes_masked(vol, weight, level, origin, spacing):
    """marching_cubes over the observed part of a volume (weight > 0): same vertex and face order; with every weight
    positive the result is marching_cubes' bit for bit."""
    ws, counts = mc_count_masked(vol, weight, level)
    n_verts, n_faces = (int(v) for v in counts.tolist())
    return mc_emit(vol, level, origin, spacing, ws, n_verts, n_faces)


# ----------------------------------------------------------------------------------------------
# TSDF fusion of RGB-D frames (reference src/utils/Mesher.py:63-128, open3d's ScalableTSDFVolume): DESIGN.md section 17
# ----------------------------------------------------------------------------------------------
class TSDFVolume:
    """A dense TSDF volume over the box `bound` ([3,2]): dims = ceil((hi - lo) / voxel) voxels per axis, voxel (i, j, k)
    centred at origin + (index + 0.5) voxel, origin = lo.  tsdf and weight [nx,ny,nz] float32 (weight = the number of
    observations), color [nx,ny,nz,3] float32 or None, all zero at first, on the GPU (eslam_tsdf_integrate has no CPU
    fallback).  Raises RuntimeError, with the byte count, when the device has less memory free than the arrays need."""

    def __init__(self, bound, voxel, trunc, color=True, device=None):
        b = torch.as_tensor(bound).detach().to("cpu", torch.float64).reshape(3, 2)
        self.voxel = float(torch.tensor(float(voxel), dtype=torch.float32))        # what the kernel sees
        self.trunc = float(torch.tensor(float(trunc), dtype=torch.float32))
        if not (self.voxel > 0 and self.trunc > 0):
            raise RuntimeError(f"TSDFVolume: voxel {voxel} and trunc {trunc} must be positive")
        self.dims = tuple(int(math.ceil(float(b[k, 1] - b[k, 0]) / float(voxel))) for k in range(3))
        if min(self.dims) < 1:
            raise RuntimeError(f"TSDFVolume: empty bound {b.tolist()}")
        self.origin = tuple(float(v) for v in b[:, 0].to(torch.float32))
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"TSDFVolume: expected a GPU device (got {dev}); TSDF fusion has no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        n = self.dims[0] * self.dims[1] * self.dims[2]
        need = 4 * n * (5 if color else 2)
        free, _ = torch.cuda.mem_get_info(dev)
        if free < need:
            raise RuntimeError(f"TSDFVolume: {self.dims[0]} x {self.dims[1]} x {self.dims[2]} voxels need {need} bytes, "
                               f"{free} bytes are free on {dev}")
        self.tsdf = torch.zeros(self.dims, dtype=torch.float32, device=dev)
        self.weight = torch.zeros(self.dims, dtype=torch.float32, device=dev)
        self.color = torch.zeros(self.dims + (3,), dtype=torch.float32, device=dev) if color else None

    def _flush(self, depths, colors, c2ws, K):
        dev = self.device
        fx, fy, cx, cy = (float(k) for k in K)
        d = _c(torch.stack([torch.as_tensor(x).detach().to(dev, torch.float32) for x in depths]))
        if d.dim() != 3:
            raise RuntimeError(f"TSDFVolume.integrate: depth images must be [H,W], got {tuple(d.shape[1:])}")
        n, H, W = (int(v) for v in d.shape)
        col = None
        if self.color is not None:
            col = _c(torch.stack([torch.as_tensor(x).detach().to(dev, torch.float32) for x in colors]))
            if tuple(col.shape) != (n, H, W, 3):
                raise RuntimeError(f"TSDFVolume.integrate: colour images must be [H,W,3] like the depth, got {tuple(col.shape[1:])}")
        w2c = _w2c_rows(torch.stack([torch.as_tensor(c).detach().to("cpu", torch.float64).reshape(4, 4) for c in c2ws]), dev,
                        flip_yz=True)
        depth_max = _c(d.reshape(n, -1).amax(dim=1))
        o3 = (ctypes.c_float * 3)(*self.origin)
        with _hip.on_device(dev):
            _hip.check(_hip.lib().eslam_tsdf_integrate(_hip.ptr(self.tsdf), _hip.ptr(self.weight), _hip.ptr(self.color),
                                                       *self.dims, o3, self.voxel, self.trunc, _hip.ptr(d), _hip.ptr(col),
                                                       _hip.ptr(w2c), _hip.ptr(depth_max), n, H, W, fx, fy, cx, cy,
                                                       _hip.stream_handle(dev)), "eslam_tsdf_integrate")

    def integrate(self, frames, K, chunk=32):
        """Fuse `frames`, an iterable of (idx, colour [H,W,3], depth [H,W], c2w [4,4]) as the dataset readers and
        synthscene.make_sequence yield them (any device; colour is not read when the volume has none), K = (fx, fy, cx, cy).
        Poses are the reference's (camera looks along -z, y up): columns 1 and 2 are negated here, as Mesher.py:94-96 does.
        Frames are streamed `chunk` at a time, one launch each, applied in the order given; each chunk's poses are inverted
        on the host in float64, its depth maxima are taken on the device (no per-frame sync).  The result does not depend
        on `chunk`."""
        chunk = max(1, int(chunk))
        depths, colors, c2ws = [], [], []
        for _, colour, depth, c2w in frames:
            depths.append(depth)
            colors.append(colour)
            c2ws.append(c2w)
            if len(c2ws) == chunk:
                self._flush(depths, colors, c2ws, K)
                depths, colors, c2ws = [], [], []
        if c2ws:
            self._flush(depths, colors, c2ws, K)
        return self

    def extract_mesh(self, level=0.0):
        """(verts float32 [V,3], faces int32 [F,3], colours float32 [V,3] or None) on the device: marching cubes over the
        observed voxels (marching_cubes_masked), vertices at origin + (i + 0.5 + t) voxel, colours sampled trilinearly from
        the colour volume (on an edge vertex: the blend of the edge's two voxels)."""
        origin = tuple(o + 0.5 * self.voxel for o in self.origin)
        verts, faces = marching_cubes_masked(self.tsdf, self.weight, level, origin, (self.voxel,) * 3)
        if self.color is None:
            return verts, faces, None
        return verts, faces, self.sample_color(verts)

    def sample_color(self, pts):
        """float32 [N,3]: the colour volume sampled trilinearly at the world points pts [N,3] (eslam_tsdf_sample_color)."""
        if self.color is None:
            raise RuntimeError("TSDFVolume.sample_color: the volume has no colour")
        p = _gpu_points("pts", pts, self.device)
        out = torch.empty(p.shape[0], 3, dtype=torch.float32, device=self.device)
        o3 = (ctypes.c_float * 3)(*self.origin)
        with _hip.on_device(self.device):
            _hip.check(_hip.lib().eslam_tsdf_sample_color(_hip.ptr(self.color), *self.dims, o3, self.voxel, _hip.ptr(p),
                                                          p.shape[0], _hip.ptr(out), _hip.stream_handle(self.device)),
                       "eslam_tsdf_sample_color")
        return out


# ----------------------------------------------------------------------------------------------
# frame preparation (src/utils/datasets.py: BaseDataset.__getitem__ on the device)
# ----------------------------------------------------------------------------------------------
def frame_out_shape(color_hw, depth_hw, crop_size, crop_edge):
    """(H', W') of prepare_frame's outputs (eslam_frame_out_shape; host arithmetic, needs no GPU)."""
    ch, cw = (0, 0) if crop_size is None else (int(crop_size[0]), int(crop_size[1]))
    H, W = ctypes.c_int(0), ctypes.c_int(0)
    _hip.check(_hip.lib().eslam_frame_out_shape(int(color_hw[0]), int(color_hw[1]), int(depth_hw[0]), int(depth_hw[1]), ch, cw,
                                                int(crop_edge), ctypes.byref(H), ctypes.byref(W)), "eslam_frame_out_shape")
    return H.value, W.value


def prepare_frame(rgb_u8, depth_u16, spec):
    """(colour [H',W',3] float32, depth [H',W'] float32) on the device from the decoded images of one frame: rgb_u8
    [Hc,Wc,3] uint8 and depth_u16 [Hd,Wd] uint16 (or the same bits as int16), both on the GPU and contiguous.  `spec` is
    the dataset's datasets.FrameSpec.  What BaseDataset.__getitem__ returns, computed by eslam_frame_undistort (only with
    a distortion map) and eslam_frame_prepare on the caller's current stream; no synchronisation."""
    dev = rgb_u8.device
    if not rgb_u8.is_cuda or depth_u16.device != dev:
        raise RuntimeError(f"prepare_frame: expected both images on one GPU (got {rgb_u8.device}, {depth_u16.device}); "
                           "frame preparation has no CPU fallback")
    if rgb_u8.dtype != torch.uint8 or rgb_u8.dim() != 3 or rgb_u8.shape[2] != 3 or not rgb_u8.is_contiguous():
        raise RuntimeError(f"prepare_frame: rgb must be a contiguous [H,W,3] uint8 tensor, got {rgb_u8.dtype} {tuple(rgb_u8.shape)}")
    if depth_u16.dtype not in (torch.uint16, torch.int16) or depth_u16.dim() != 2 or not depth_u16.is_contiguous():
        raise RuntimeError(f"prepare_frame: depth must be a contiguous [H,W] uint16 tensor, got {depth_u16.dtype} "
                           f"{tuple(depth_u16.shape)}")
    Hc, Wc = int(rgb_u8.shape[0]), int(rgb_u8.shape[1])
    Hd, Wd = int(depth_u16.shape[0]), int(depth_u16.shape[1])
    ch, cw = (0, 0) if spec.crop_size is None else spec.crop_size
    Ho, Wo = frame_out_shape((Hc, Wc), (Hd, Wd), spec.crop_size, spec.crop_edge)
    lib = _hip.lib()
    color = torch.empty(Ho, Wo, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(Ho, Wo, dtype=torch.float32, device=dev)
    with _hip.on_device(dev):
        st = _hip.stream_handle(dev)
        grid = spec.grid_on(dev)
        if grid is not None:
            if tuple(grid.shape) != (Hc, Wc, 2) or grid.dtype != torch.float32 or not grid.is_contiguous():
                raise RuntimeError(f"prepare_frame: the undistortion map is {tuple(grid.shape)} {grid.dtype}, the colour image "
                                   f"{Hc} x {Wc}")
            flat = torch.empty_like(rgb_u8)
            _hip.check(lib.eslam_frame_undistort(_hip.ptr(rgb_u8), _hip.ptr(grid), Hc, Wc, _hip.ptr(flat), st),
                       "eslam_frame_undistort")
            rgb_u8 = flat
        _hip.check(lib.eslam_frame_prepare(_hip.ptr(rgb_u8), Hc, Wc, _hip.ptr(depth_u16), Hd, Wd, ch, cw, spec.crop_edge,
                                           spec.png_depth_scale, spec.scale, _hip.ptr(color), _hip.ptr(depth), st),
                   "eslam_frame_prepare")
    return color, depth


# ----------------------------------------------------------------------------------------------
# reconstruction evaluation (reference src/tools/cull_mesh.py, src/tools/eval_recon.py): culling, nearest neighbours,
# ICP moments, surface sampling
# ----------------------------------------------------------------------------------------------
def _gpu_points(name, p, dev=None):
    p = torch.as_tensor(p)
    if dev is None:
        dev = p.device if p.is_cuda else torch.device("cuda", torch.cuda.current_device())
    p = _c(p.detach().to(dev, torch.float32).reshape(-1, 3))
    _hip.require_gpu_f32(name, p)
    return p


def cull_vertices(verts, frames, K, H, W, truncation, depth_test, chunk=32):
    """bool [V] on verts' device: seen in at least one frame by the test of cull_mesh.py:61-104 (eslam_cull_vertices).
    verts [V,3]; frames: an iterable of (depth [Hi,Wi], c2w [4,4]) (any device); K = (fx, fy, cx, cy); H, W the config's
    image size; depth_test = cfg['meshing']['eval_rec'].  Frames are streamed `chunk` at a time: each c2w is inverted on
    the host in float64 (one sync per chunk), the chunk's depths are stacked on the device, one launch per chunk."""
    v = _gpu_points("verts", verts)
    dev = v.device
    fx, fy, cx, cy = (float(k) for k in K)
    seen = torch.zeros(v.shape[0], dtype=torch.uint8, device=dev)
    lib = _hip.lib()

    def flush(depths, c2ws):
        w2c = torch.linalg.inv(torch.stack([c.detach().to("cpu", torch.float64).reshape(4, 4) for c in c2ws]))
        w2c = _c(w2c[:, :3, :].to(torch.float32).reshape(-1, 12).to(dev))
        d = torch.stack([x.detach().to(dev, torch.float32) for x in depths]) if depth_test else None
        hi, wi = (int(d.shape[1]), int(d.shape[2])) if d is not None else (0, 0)
        with _hip.on_device(dev):
            _hip.check(lib.eslam_cull_vertices(_hip.ptr(v), v.shape[0], _hip.ptr(d), len(c2ws), hi, wi, _hip.ptr(w2c),
                                               fx, fy, cx, cy, int(H), int(W), float(truncation), 1 if depth_test else 0,
                                               _hip.ptr(seen), _hip.stream_handle(dev)), "eslam_cull_vertices")

    depths, c2ws = [], []
    for depth, c2w in frames:
        depths.append(depth)
        c2ws.append(c2w)
        if len(c2ws) == chunk:
            flush(depths, c2ws)
            depths, c2ws = [], []
    if c2ws:
        flush(depths, c2ws)
    return seen.bool()


class NNGrid:
    """Exact nearest neighbours among the reference points `ref` [N,3] (float32 on the GPU): a uniform grid built once
    (eslam_nn_grid_plan / eslam_nn_build; one host sync for the bounding box), queried any number of times.  Replaces
    scipy's cKDTree(ref).query (eval_recon.py:21-39) and open3d's correspondence search."""

    def __init__(self, ref):
        self.ref = _gpu_points("ref", ref)
        self.device = self.ref.device
        n = self.ref.shape[0]
        if n < 1:
            raise RuntimeError("NNGrid: no reference points")
        lo, hi = self.ref.aminmax(dim=0)
        bbox = torch.stack([lo, hi], 1).reshape(-1).cpu()
        self.grid = _hip.NnGrid()
        lib = _hip.lib()
        _hip.check(lib.eslam_nn_grid_plan(n, (ctypes.c_float * 6)(*bbox.tolist()), ctypes.byref(self.grid)),
                   "eslam_nn_grid_plan")
        self.ws = torch.empty(int(lib.eslam_nn_workspace_bytes(ctypes.byref(self.grid), n)), dtype=torch.uint8,
                              device=self.device)
        with _hip.on_device(self.device):
            _hip.check(lib.eslam_nn_build(_hip.ptr(self.ref), n, ctypes.byref(self.grid), _hip.ptr(self.ws),
                                          _hip.stream_handle(self.device)), "eslam_nn_build")

    @property
    def dims(self):
        return tuple(self.grid.dims)

    def query(self, q, max_dist=None, sort=True):
        """(dist float32 [Q], idx int32 [Q]) on the grid's device: the distance to the nearest reference point and its
        index (the smaller index among equal distances).  max_dist: only points with dist < max_dist count; a query with
        none gets (inf, -1).  sort=False processes the queries in input order instead of cell order (same results)."""
        q = _gpu_points("q", q, self.device)
        nq = q.shape[0]
        dist = torch.empty(nq, device=self.device)
        idx = torch.empty(nq, dtype=torch.int32, device=self.device)
        if nq == 0:
            return dist, idx
        lib = _hip.lib()
        qws = None
        if sort:
            qws = torch.empty(int(lib.eslam_nn_query_workspace_bytes(ctypes.byref(self.grid), nq)), dtype=torch.uint8,
                              device=self.device)
        md = float("inf") if max_dist is None else float(max_dist)
        with _hip.on_device(self.device):
            _hip.check(lib.eslam_nn_query(ctypes.byref(self.grid), _hip.ptr(self.ws), self.ref.shape[0], _hip.ptr(q), nq, md,
                                          0 if sort else _hip.NN_INPUT_ORDER, _hip.ptr(qws), _hip.ptr(dist), _hip.ptr(idx),
                                          _hip.stream_handle(self.device)), "eslam_nn_query")
        return dist, idx


def icp_moments(src, tgt, dist, idx, threshold):
    """float64 [17] on the device: count, sum d^2, sum s (3), sum t (3), sum s t^T (9) over the correspondences
    (src[i], tgt[idx[i]]) with idx[i] >= 0 and dist[i] < threshold (eslam_icp_moments: a fixed-order reduction)."""
    s = _gpu_points("src", src)
    dev = s.device
    t = _gpu_points("tgt", tgt, dev)
    dist = _c(dist.to(dev, torch.float32))
    idx = _c(idx.to(dev, torch.int32))
    lib = _hip.lib()
    ws = torch.empty(int(lib.eslam_icp_moments_workspace_bytes()), dtype=torch.uint8, device=dev)
    out = torch.empty(_hip.ICP_MOMENTS, dtype=torch.float64, device=dev)
    with _hip.on_device(dev):
        _hip.check(lib.eslam_icp_moments(_hip.ptr(s), _hip.ptr(t), _hip.ptr(dist), _hip.ptr(idx), s.shape[0], float(threshold),
                                         _hip.ptr(ws), _hip.ptr(out), _hip.stream_handle(dev)), "eslam_icp_moments")
    return out


# mesh clean-up (src/tools/clean_mesh.py): vertex merge, connected components, their face counts
def _mesh_gpu(name, t, dtype, cols):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the GPU (got {getattr(t, 'device', type(t).__name__)}); the mesh "
                           "clean-up has no CPU fallback")
    t = t.detach()
    if cols:
        t = t.reshape(-1, cols)
    else:
        t = t.reshape(-1)
    n = t.shape[0]
    if n > _hip.MESH_MAX_COUNT:
        raise RuntimeError(f"{name}: {n} entries, at most 2^30")
    return _c(t.to(dtype))


def _mesh_faces(faces, n_verts):
    """int32 [F,3] on the GPU, every index checked once against [0, n_verts) (one sync): the kernels do not check."""
    if not torch.is_tensor(faces) or not faces.is_cuda:
        raise RuntimeError(f"faces: expected a tensor on the GPU (got {getattr(faces, 'device', type(faces).__name__)})")
    f = faces.detach().reshape(-1, 3)
    if f.shape[0] > _hip.MESH_MAX_COUNT:
        raise RuntimeError(f"faces: {f.shape[0]} faces, at most 2^30")
    if f.shape[0]:
        lo, hi = f.aminmax()
        lo, hi = int(lo), int(hi)
        if lo < 0 or hi >= n_verts:
            raise ValueError(f"faces: indices span [{lo}, {hi}], the mesh has {n_verts} vertices")
    return _c(f.to(torch.int32))


def weld_vertices(verts):
    """int32 [V] on verts' device: rep[v] = the smallest index whose position equals v's, coordinate by coordinate with
    -0 == +0 (exact: one ulp apart is different); -1 for a vertex with a NaN or infinite coordinate (eslam_mesh_weld).
    verts float32 [V,3] on the GPU."""
    v = _mesh_gpu("verts", verts, torch.float32, 3)
    dev = v.device
    n = v.shape[0]
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return rep
    lib = _hip.lib()
    ws = torch.empty(int(lib.eslam_mesh_weld_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    with _hip.on_device(dev):
        _hip.check(lib.eslam_mesh_weld(_hip.ptr(v), n, _hip.ptr(ws), _hip.ptr(rep), _hip.stream_handle(dev)), "eslam_mesh_weld")
    return rep


def mesh_components(faces, n_verts):
    """int32 [n_verts] on faces' device: the smallest vertex index of every vertex's connected component, faces joined
    through shared VERTICES (eslam_mesh_components); a vertex in no face labels itself.  faces [F,3] integer on the GPU;
    an index outside [0, n_verts) raises ValueError."""
    n_verts = int(n_verts)
    if n_verts < 0 or n_verts > _hip.MESH_MAX_COUNT:
        raise RuntimeError(f"mesh_components: {n_verts} vertices (0 .. 2^30)")
    f = _mesh_faces(faces, n_verts)
    dev = f.device
    label = torch.empty(n_verts, dtype=torch.int32, device=dev)
    if n_verts == 0:
        return label
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_mesh_components(_hip.ptr(f), f.shape[0], n_verts, _hip.ptr(label),
                                                    _hip.stream_handle(dev)), "eslam_mesh_components")
    return label


def component_face_counts(faces, labels):
    """int32 [V] on faces' device: at every component's label the number of its faces (a face counts where its first
    corner's label points), 0 elsewhere (eslam_mesh_component_sizes; exact).  labels int32 [V] from mesh_components."""
    lab = _mesh_gpu("labels", labels, torch.int32, 0)
    n_verts = lab.shape[0]
    f = _mesh_faces(faces, n_verts)
    dev = f.device
    if lab.device != dev:
        raise RuntimeError(f"component_face_counts: faces on {dev}, labels on {lab.device}")
    count = torch.empty(n_verts, dtype=torch.int32, device=dev)
    if n_verts == 0:
        return count
    if f.shape[0]:
        lo, hi = lab.aminmax()
        if int(lo) < 0 or int(hi) >= n_verts:
            raise ValueError(f"labels: values span [{int(lo)}, {int(hi)}], the mesh has {n_verts} vertices")
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_mesh_component_sizes(_hip.ptr(f), f.shape[0], _hip.ptr(lab), n_verts, _hip.ptr(count),
                                                         _hip.stream_handle(dev)), "eslam_mesh_component_sizes")
    return count


class MeshDistance:
    """Exact distance from points to the triangle mesh (verts float32 [V,3], faces integer [F,3], both on the GPU): a
    uniform grid built once (eslam_tri_grid_plan / eslam_tri_count / eslam_tri_build), queried any number of times.  One
    host sync for the bounding box of the finite vertices and the mean face extent the plan takes, one for the entry
    count; a face index outside [0, V) raises ValueError.  A face with a non-finite coordinate is never returned.  No CPU
    fallback."""

    def __init__(self, verts, faces):
        self.verts = _mesh_gpu("verts", verts, torch.float32, 3)
        self.device = self.verts.device
        n_verts = self.verts.shape[0]
        self.faces = _mesh_faces(faces, n_verts)
        if self.faces.device != self.device:
            raise RuntimeError(f"MeshDistance: verts on {self.device}, faces on {self.faces.device}")
        n_faces = self.faces.shape[0]
        self.grid = _hip.TriGrid()
        self.faces_entered = 0
        self.ws = None
        lib = _hip.lib()
        stats = None
        if n_faces:
            tri = self.verts[self.faces.long()]                                  # [F,3,3]
            ok = torch.isfinite(tri).all(dim=2).all(dim=1)
            fin = torch.isfinite(self.verts).all(dim=1)
            if bool(fin.any()):                                                  # (part of the one sync below)
                v = self.verts[fin]
                lo, hi = v.aminmax(dim=0)
                ext = (tri.amax(dim=1) - tri.amin(dim=1)).amax(dim=1)            # largest axis extent of every face's box
                mean = torch.where(ok, ext, torch.zeros_like(ext)).double().sum() / ok.sum().clamp(min=1)
                stats = torch.cat([torch.stack([lo, hi], 1).reshape(-1).double(), mean.reshape(1)]).cpu().tolist()
        if stats is None:
            _hip.check(lib.eslam_tri_grid_plan(0, None, 0.0, ctypes.byref(self.grid)), "eslam_tri_grid_plan")
            return
        _hip.check(lib.eslam_tri_grid_plan(n_faces, (ctypes.c_float * 6)(*stats[:6]), float(stats[6]), ctypes.byref(self.grid)),
                   "eslam_tri_grid_plan")
        total = torch.empty(2, dtype=torch.int64, device=self.device)
        with _hip.on_device(self.device):
            _hip.check(lib.eslam_tri_count(_hip.ptr(self.verts), n_verts, _hip.ptr(self.faces), n_faces, ctypes.byref(self.grid),
                                           _hip.ptr(total), _hip.stream_handle(self.device)), "eslam_tri_count")
        self.grid.entries, self.faces_entered = (int(x) for x in total.cpu().tolist())
        if self.grid.entries == 0:
            return
        nbytes = int(lib.eslam_tri_workspace_bytes(ctypes.byref(self.grid)))
        if nbytes < 0:
            _hip.check(1, "eslam_tri_workspace_bytes")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with _hip.on_device(self.device):
            _hip.check(lib.eslam_tri_build(_hip.ptr(self.verts), n_verts, _hip.ptr(self.faces), n_faces, ctypes.byref(self.grid),
                                           _hip.ptr(self.ws), _hip.stream_handle(self.device)), "eslam_tri_build")

    @property
    def dims(self):
        return tuple(self.grid.dims)

    @property
    def entries(self):
        """The number of (face, cell) entries of the grid (a face is entered in every cell its box overlaps)."""
        return int(self.grid.entries)

    def query(self, q, max_dist=None, closest=False, sort=True):
        """(dist float32 [Q], face int32 [Q]) or, with closest=True, (dist, face, closest float32 [Q,3]) on the mesh's
        device: the distance to the nearest point of the mesh, the face it lies on (the smaller index among equal
        distances) and that point.  max_dist: only faces with dist < max_dist count.  A query with none, or with a
        non-finite coordinate, gets (inf, -1, NaN).  sort=False processes the queries in input order instead of cell
        order (same results)."""
        q = _gpu_points("q", q, self.device)
        nq = q.shape[0]
        dist = torch.full((nq,), float("inf"), device=self.device)
        face = torch.full((nq,), -1, dtype=torch.int32, device=self.device)
        near = torch.full((nq, 3), float("nan"), device=self.device) if closest else None
        md = float("inf") if max_dist is None else float(max_dist)
        if md != md:
            raise ValueError("MeshDistance.query: max_dist is NaN")
        if nq and self.grid.entries:
            lib = _hip.lib()
            qws = None
            if sort:
                qws = torch.empty(int(lib.eslam_tri_query_workspace_bytes(ctypes.byref(self.grid), nq)), dtype=torch.uint8,
                                  device=self.device)
            with _hip.on_device(self.device):
                _hip.check(lib.eslam_tri_query(ctypes.byref(self.grid), _hip.ptr(self.ws), _hip.ptr(q), nq, md,
                                               0 if sort else _hip.TRI_INPUT_ORDER, _hip.ptr(qws), _hip.ptr(dist),
                                               _hip.ptr(face), _hip.ptr(near), _hip.stream_handle(self.device)),
                           "eslam_tri_query")
        return (dist, face, near) if closest else (dist, face)


def sample_surface(verts, faces, n, seed=0):
    """(samples float64 [n,3], face_index int64 [n]) on verts' device, as trimesh.sample.sample_surface: faces picked
    with probability proportional to their area (float64 areas, cumulative sum, searchsorted of u * total, left side),
    then two uniforms per sample, reflected to (1 - r1, 1 - r2) when r1 + r2 > 1, sample = v0 + r1 (v1 - v0) + r2 (v2 - v0).
    Deviation: the draws come from a torch generator seeded with `seed`, not from numpy's global generator."""
    v = torch.as_tensor(verts).detach().to(torch.float64).reshape(-1, 3)
    f = torch.as_tensor(faces).detach().to(v.device, torch.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        raise RuntimeError("sample_surface: the mesh has no faces")
    dev = v.device
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    area = 0.5 * torch.linalg.cross(e1, e2).norm(dim=1)
    cum = torch.cumsum(area, 0)
    g = torch.Generator(device=dev).manual_seed(int(seed))
    pick = torch.rand(int(n), dtype=torch.float64, device=dev, generator=g) * area.sum()
    fi = torch.searchsorted(cum, pick).clamp_(max=f.shape[0] - 1)
    r = torch.rand(int(n), 2, dtype=torch.float64, device=dev, generator=g)
    flip = r.sum(dim=1) > 1.0
    r = torch.where(flip[:, None], 1.0 - r, r)
    return v0[fi] + r[:, :1] * e1[fi] + r[:, 1:] * e2[fi], fi


# ----------------------------------------------------------------------------------------------
# the 2D reconstruction metric (reference src/tools/eval_recon.py:59-85, 127-207): depth rasteriser, depth L1, check_proj
# ----------------------------------------------------------------------------------------------
def _w2c_rows(c2ws, dev, flip_yz=False):
    """float32 [n,12] on dev: the 3x4 rows of inverse(c2w) taken on the host in float64 (one sync); flip_yz negates
    columns 1 and 2 of each c2w first (check_proj, eval_recon.py:64-68)."""
    c = torch.as_tensor(c2ws).detach().to("cpu", torch.float64).reshape(-1, 4, 4).clone()
    if flip_yz:
        c[:, :3, 1] *= -1.0
        c[:, :3, 2] *= -1.0
    return _c(torch.linalg.inv(c)[:, :3, :].to(torch.float32).reshape(-1, 12).to(dev))


def render_mesh_depth(verts, faces, c2ws, K, H, W, z_near=_hip.RASTER_Z_NEAR, z_far=_hip.RASTER_Z_FAR, chunk=32,
                      large_area=0):
    """float32 [n,H,W] on the GPU: the depth images of the mesh (verts [V,3] float32, faces [F,3]) from the cameras
    c2ws [n,4,4] (camera looks along +z, x right, y down: the reference's param.extrinsic = inv(c2w)), K = (fx, fy, cx, cy):
    camera-space z of the nearest surface at each pixel centre within [z_near, z_far], 0 where nothing is hit
    (eslam_raster_depth; what open3d's capture_depth_float_buffer(True) returns in eval_recon.py:191,199).  Views are
    rendered `chunk` at a time, one call each; the poses are inverted on the host in float64.  large_area: the size
    threshold between the two triangle paths in pixels (0 = the library's default; the images do not depend on it)."""
    v = torch.as_tensor(verts)
    _hip.require_gpu_f32("verts", v)
    dev = v.device
    v = _c(v.detach().reshape(-1, 3))
    f = torch.as_tensor(faces)
    if not f.is_cuda:
        raise RuntimeError(f"faces: expected a tensor on the GPU (got device {f.device}); the rasteriser has no CPU fallback")
    f = _c(f.detach().to(dev, torch.int32).reshape(-1, 3))
    fx, fy, cx, cy = (float(k) for k in K)
    H, W, chunk = int(H), int(W), max(1, int(chunk))
    w2c = _w2c_rows(c2ws, dev)
    n = w2c.shape[0]
    out = torch.empty(n, H, W, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    lib = _hip.lib()
    nb = int(lib.eslam_raster_workspace_bytes(f.shape[0], min(chunk, n), H, W))
    if nb < 0:
        raise RuntimeError(f"render_mesh_depth: bad sizes ({f.shape[0]} faces, image {W} x {H})")
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    with _hip.on_device(dev):
        for lo in range(0, n, chunk):
            k = min(chunk, n - lo)
            _hip.check(lib.eslam_raster_depth(_hip.ptr(v), v.shape[0], _hip.ptr(f), f.shape[0], _hip.ptr(w2c[lo:]), k, fx, fy,
                                              cx, cy, H, W, float(z_near), float(z_far), int(large_area), _hip.ptr(ws),
                                              _hip.ptr(out[lo:]), _hip.stream_handle(dev)), "eslam_raster_depth")
    return out


def _u8_rows(name, t, dev, n=None):
    """uint8 [n,4] on dev (alpha 255) from a [n,3] / [n,4] colour tensor, or [1,4] from a [3] / [4] one."""
    c = torch.as_tensor(t)
    if c.dtype != torch.uint8:
        raise RuntimeError(f"{name}: expected uint8 colours, got {c.dtype}")
    c = c.detach().to(dev)
    if c.dim() == 1:
        c = c[None]
    if c.dim() != 2 or c.shape[1] not in (3, 4) or (n is not None and c.shape[0] not in (1, n)):
        raise RuntimeError(f"{name}: expected [3|4] or [{n},3|4] colours, got {tuple(c.shape)}")
    out = torch.full((c.shape[0], 4), 255, dtype=torch.uint8, device=dev)
    out[:, :3] = c[:, :3]
    return out


def shade_vertices(verts, normals, colors, cam_center, ambient=0.3):
    """uint8 [V,4] on the GPU: vertex colours under a headlight at cam_center (3 floats, host), for one view
    (eslam_shade_vertices): c k per channel, k = ambient + (1 - ambient) max(0, n^ . l^), l = cam_center - v, k = 1 where n or l
    has zero length; alpha 255.  verts, normals float32 [V,3] on the GPU; colors uint8 [V,3|4] on the GPU or None = 200 grey."""
    v = torch.as_tensor(verts)
    n = torch.as_tensor(normals)
    _hip.require_gpu_f32("verts", v)
    _hip.require_gpu_f32("normals", n)
    dev = v.device
    v = _c(v.detach().reshape(-1, 3))
    n = _c(n.detach().to(dev).reshape(-1, 3))
    if n.shape[0] != v.shape[0]:
        raise RuntimeError(f"normals: expected one normal per vertex ({v.shape[0]}), got {n.shape[0]}")
    c = None
    if colors is not None:
        if not torch.as_tensor(colors).is_cuda:
            raise RuntimeError("colors: expected a tensor on the GPU; the renderer has no CPU fallback")
        c = _u8_rows("colors", colors, dev, v.shape[0])
        if c.shape[0] != v.shape[0]:
            raise RuntimeError(f"colors: expected one colour per vertex ({v.shape[0]}), got {c.shape[0]}")
    return _shade_prepared(v, n, c, cam_center, ambient, torch.empty(v.shape[0], 4, dtype=torch.uint8, device=dev))


def _shade_prepared(v, n, c, cam_center, ambient, out):
    """shade_vertices on arguments already checked and laid out (v, n float32 [V,3], c uint8 [V,4] or None, out uint8 [V,4],
    all contiguous on one GPU): the launch alone.  Returns out."""
    dev = v.device
    centre = (ctypes.c_float * 3)(*[float(x) for x in cam_center])
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_shade_vertices(_hip.ptr(v), _hip.ptr(n), _hip.ptr(c), v.shape[0], centre, float(ambient),
                                                   _hip.ptr(out), _hip.stream_handle(dev)), "eslam_shade_vertices")
    return out


def render_view(meshes, points, c2ws, K, H, W, background=(255, 255, 255), z_near=_hip.RASTER_Z_NEAR, z_far=_hip.RASTER_Z_FAR,
                cull_backfaces=True, chunk=8, large_area=0, return_depth=False, shade=False, ambient=0.3):
    """uint8 [n,H,W,3] on the GPU: the colour images of meshes and point clouds from the cameras c2ws [n,4,4] (the
    convention of render_mesh_depth: the camera looks along +z, y down), K = (fx, fy, cx, cy); what the reference's open3d
    window shows (visualizer_util.py:178-200): meshes unlit with their vertex colours, back faces hidden when
    cull_backfaces, points drawn size x size pixels, the nearest fragment at each pixel (eslam_viewer_*).
    meshes: a list of (verts float32 [V,3], faces [F,3], colors uint8 [V,3|4] or None = grey); points: a list of
    (xyz float32 [N,3], rgb uint8 [3|4] for all or [N,3|4], size in pixels).  All tensors on one GPU.  Views are rendered `chunk` at a
    time; the poses are inverted on the host in float64.  With return_depth also float32 [n,H,W]: the camera-space z of the
    winning fragment, 0 where the background shows.  The images depend neither on the order of the lists nor on large_area.
    A mesh may carry a fourth element, normals float32 [V,3] on the GPU.  With shade=True the meshes that have normals are lit
    by a headlight at each view's camera centre (shade_vertices with `ambient`, then rasterised with those colours), one view
    at a time; meshes without normals, and every call with shade=False, are drawn unlit as before."""
    ms, ps, dev = [], [], None
    for k, (verts, faces, colors, *rest) in enumerate(meshes):
        v = torch.as_tensor(verts)
        _hip.require_gpu_f32(f"meshes[{k}] verts", v)
        dev = v.device if dev is None else dev
        v = _c(v.detach().reshape(-1, 3))
        f = torch.as_tensor(faces)
        if not f.is_cuda:
            raise RuntimeError(f"meshes[{k}] faces: expected a tensor on the GPU (got device {f.device}); the renderer has no CPU fallback")
        f = _c(f.detach().to(dev, torch.int32).reshape(-1, 3))
        c = None
        if colors is not None:
            if not torch.as_tensor(colors).is_cuda:
                raise RuntimeError(f"meshes[{k}] colors: expected a tensor on the GPU; the renderer has no CPU fallback")
            c = _u8_rows(f"meshes[{k}] colors", colors, dev, v.shape[0])
            if c.shape[0] != v.shape[0]:
                raise RuntimeError(f"meshes[{k}] colors: expected one colour per vertex ({v.shape[0]}), got {c.shape[0]}")
        nrm = None
        if shade and rest and rest[0] is not None:
            nrm = torch.as_tensor(rest[0])
            _hip.require_gpu_f32(f"meshes[{k}] normals", nrm)
            nrm = _c(nrm.detach().reshape(-1, 3))
            if nrm.shape[0] != v.shape[0]:
                raise RuntimeError(f"meshes[{k}] normals: expected one normal per vertex ({v.shape[0]}), got {nrm.shape[0]}")
        # (a lit mesh's colours are prepared once; its shaded colours live in one buffer that every view overwrites in turn,
        # in stream order behind the previous view's rasterisation)
        ms.append((v, f, c, nrm, torch.empty(v.shape[0], 4, dtype=torch.uint8, device=dev) if nrm is not None else None))
    for k, (xyz, rgb, size) in enumerate(points):
        p = torch.as_tensor(xyz)
        _hip.require_gpu_f32(f"points[{k}] xyz", p)
        dev = p.device if dev is None else dev
        p = _c(p.detach().reshape(-1, 3))
        ps.append((p, _u8_rows(f"points[{k}] rgb", rgb, dev, p.shape[0]), int(size)))
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    fx, fy, cx, cy = (float(k) for k in K)
    H, W, chunk = int(H), int(W), max(1, int(chunk))
    lit = any(m[3] is not None for m in ms)
    if lit:             # the light moves with the camera: colours per view
        chunk = 1
        centres = torch.as_tensor(c2ws).detach().to("cpu", torch.float32).reshape(-1, 4, 4)[:, :3, 3].tolist()
    bg = [int(b) for b in background]
    w2c = _w2c_rows(c2ws, dev)
    n = w2c.shape[0]
    out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
    depth = torch.empty(n, H, W, dtype=torch.float32, device=dev) if return_depth else None
    lib = _hip.lib()
    n_faces = max([m[1].shape[0] for m in ms], default=0)
    nb = int(lib.eslam_viewer_workspace_bytes(n_faces, max(1, min(chunk, n)), H, W))
    if nb < 0:
        raise RuntimeError(f"render_view: bad sizes ({n_faces} faces, image {W} x {H})")
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    st = _hip.stream_handle(dev)
    with _hip.on_device(dev):
        for lo in range(0, n, chunk):
            k = min(chunk, n - lo)
            cam = (_hip.ptr(w2c[lo:]), k, fx, fy, cx, cy, H, W, float(z_near), float(z_far))
            _hip.check(lib.eslam_viewer_begin(k, H, W, _hip.ptr(ws), st), "eslam_viewer_begin")
            for v, f, c, nrm, lit_c in ms:
                if nrm is not None:
                    c = _shade_prepared(v, nrm, c, centres[lo], ambient, lit_c)
                _hip.check(lib.eslam_viewer_mesh(_hip.ptr(v), v.shape[0], _hip.ptr(f), f.shape[0], _hip.ptr(c) if c is not None else None,
                                                 *cam, int(bool(cull_backfaces)), int(large_area), _hip.ptr(ws), st), "eslam_viewer_mesh")
            for p, c, size in ps:
                _hip.check(lib.eslam_viewer_points(_hip.ptr(p), p.shape[0], _hip.ptr(c), int(c.shape[0] != 1), size,
                                                   *cam, _hip.ptr(ws), st), "eslam_viewer_points")
            _hip.check(lib.eslam_viewer_resolve(k, H, W, bg[0], bg[1], bg[2], _hip.ptr(ws), _hip.ptr(out[lo:]),
                                                _hip.ptr(depth[lo:]) if return_depth else None, st), "eslam_viewer_resolve")
    return (out, depth) if return_depth else out


def depth_l1(a, b):
    """float64 [n] on the device: per view the sum over the pixels of |a - b|, a and b float32 [n,H,W] (eslam_depth_l1:
    a fixed-order float64 reduction)."""
    _hip.require_gpu_f32("a", a)
    _hip.require_gpu_f32("b", b)
    if a.shape != b.shape or a.dim() != 3 or a.device != b.device:
        raise RuntimeError(f"depth_l1: expected two [n,H,W] stacks of one shape on one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    a, b = _c(a.detach()), _c(b.detach())
    dev = a.device
    n, npix = a.shape[0], a.shape[1] * a.shape[2]
    out = torch.empty(n, dtype=torch.float64, device=dev)
    lib = _hip.lib()
    with _hip.on_device(dev):
        for lo in range(0, n, 65535):
            k = min(65535, n - lo)
            ws = torch.empty(int(lib.eslam_depth_l1_workspace_bytes(k)), dtype=torch.uint8, device=dev)
            _hip.check(lib.eslam_depth_l1(_hip.ptr(a[lo:]), _hip.ptr(b[lo:]), k, npix, _hip.ptr(ws), _hip.ptr(out[lo:]),
                                          _hip.stream_handle(dev)), "eslam_depth_l1")
    return out


def views_see_points(points, c2ws, K, H, W):
    """bool [n] on the points' device: view k sees at least one of points [N,3] (float32 on the GPU) by the test of the
    reference's check_proj (eval_recon.py:59-85; eslam_views_see_points), c2ws [n,4,4] in the reference's convention there."""
    p = torch.as_tensor(points)
    _hip.require_gpu_f32("points", p)
    p = _c(p.detach().reshape(-1, 3))
    dev = p.device
    fx, fy, cx, cy = (float(k) for k in K)
    w2c = _w2c_rows(c2ws, dev, flip_yz=True)
    n = w2c.shape[0]
    seen = torch.zeros(n, dtype=torch.uint8, device=dev)
    if n and p.shape[0]:
        with _hip.on_device(dev):
            _hip.check(_hip.lib().eslam_views_see_points(_hip.ptr(p), p.shape[0], _hip.ptr(w2c), n, fx, fy, cx, cy, int(H),
                                                         int(W), _hip.ptr(seen), _hip.stream_handle(dev)),
                       "eslam_views_see_points")
    return seen.bool()


# ----------------------------------------------------------------------------------------------
# render metrics and the frame visualiser's panel (reference src/utils/Frame_Visualizer.py; csrc/eslam_vis.hip)
# ----------------------------------------------------------------------------------------------
PLASMA_LUT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "plasma_lut.txt")


def load_plasma_lut():
    """The committed plasma table (data/plasma_lut.txt: 256 rows of R G B, CC0) as a numpy uint8 [256,3] array."""
    import numpy as np
    rows = np.loadtxt(PLASMA_LUT_PATH, dtype=np.int64, comments="#", ndmin=2)
    if rows.shape != (256, 3) or rows.min() < 0 or rows.max() > 255:
        raise RuntimeError(f"{PLASMA_LUT_PATH}: expected 256 rows of three values in [0, 255], got shape {rows.shape}")
    return rows.astype(np.uint8)


def plasma_lut(device):
    """The committed plasma table on `device` as uint8 [256,3], uploaded once per device."""
    def make():
        return torch.from_numpy(load_plasma_lut()).to(device).contiguous()
    return _cached(("plasma_lut", str(device)), make)


def _frame_args(who, depth, color, gt_depth, gt_color):
    """The four images of a rendered frame and its ground truth as contiguous float32 tensors on one GPU; `depth` may be the
    float64 that render_img returns (cast with .float(), as Slam.render_quality does)."""
    for name, t in (("depth", depth), ("color", color), ("gt_depth", gt_depth), ("gt_color", gt_color)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"{who}: {name}: expected a tensor on the GPU (got "
                               f"{t.device if torch.is_tensor(t) else type(t).__name__}); the metrics and the panel have "
                               "no CPU fallback")
    if depth.dtype == torch.float64:
        depth = depth.float()
    for name, t in (("depth", depth), ("color", color), ("gt_depth", gt_depth), ("gt_color", gt_color)):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{who}: {name}: expected float32, got {t.dtype}")
    dev = depth.device
    if (depth.dim() != 2 or depth.shape[0] < 1 or depth.shape[1] < 1 or gt_depth.shape != depth.shape
            or tuple(color.shape) != tuple(depth.shape) + (3,) or gt_color.shape != color.shape
            or any(t.device != dev for t in (color, gt_depth, gt_color))):
        raise RuntimeError(f"{who}: expected depth and gt_depth [H,W], color and gt_color [H,W,3] on one device, got "
                           f"{tuple(depth.shape)}, {tuple(gt_depth.shape)}, {tuple(color.shape)}, {tuple(gt_color.shape)}")
    return _c(depth.detach()), _c(color.detach()), _c(gt_depth.detach()), _c(gt_color.detach())


def _frame_stats(depth, color, gt_depth, gt_color):
    dev = depth.device
    H, W = int(depth.shape[0]), int(depth.shape[1])
    lib = _hip.lib()
    nbytes = int(lib.eslam_frame_stats_workspace_bytes(H, W))
    if nbytes < 0:
        raise RuntimeError(f"frame_stats: image size {H} x {W} is out of range")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    with _hip.on_device(dev):
        _hip.check(lib.eslam_frame_stats(_hip.ptr(depth), _hip.ptr(gt_depth), _hip.ptr(color), _hip.ptr(gt_color), H, W,
                                         _hip.ptr(ws), _hip.ptr(out), _hip.stream_handle(dev)), "eslam_frame_stats")
    return out


def frame_stats(depth, color, gt_depth, gt_color):
    """float64 [4] on the device: n_valid (pixels with gt_depth > 0), the sum over them of |depth - gt_depth|, the sum over all
    colour values of (color - gt_color)^2, max gt_depth (eslam_frame_stats: a fixed-order float64 reduction).  On the caller's
    current stream; no synchronisation."""
    return _frame_stats(*_frame_args("frame_stats", depth, color, gt_depth, gt_color))


def ssim(a, b, return_map=False):
    """Mean SSIM of two float32 [H,W,C] (C = 1 or 3) or [H,W] images on the GPU, as a float64 scalar tensor on the device
    (eslam_ssim: 11 x 11 Gaussian window, sigma 1.5, valid region, inputs clipped to [0, 1], C1 = 1e-4, C2 = 9e-4).  With
    return_map also the float32 map [H-10,W-10,C] (or [H-10,W-10]).  On the caller's current stream; no synchronisation."""
    _hip.require_gpu_f32("a", a)
    _hip.require_gpu_f32("b", b)
    if a.shape != b.shape or a.dim() not in (2, 3) or a.device != b.device:
        raise RuntimeError(f"ssim: expected two [H,W,C] images of one shape on one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    H, W = int(a.shape[0]), int(a.shape[1])
    C = int(a.shape[2]) if a.dim() == 3 else 1
    if H < 11 or W < 11 or C not in (1, 3):
        raise RuntimeError(f"ssim: images of {H} x {W} x {C}: the 11 x 11 window needs H, W >= 11, and 1 or 3 channels")
    a, b = _c(a.detach()), _c(b.detach())
    dev = a.device
    lib = _hip.lib()
    nbytes = int(lib.eslam_ssim_workspace_bytes(H, W, C))
    if nbytes < 0:
        _hip.check(1, "eslam_ssim_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    mean = torch.empty(1, dtype=torch.float64, device=dev)
    smap = torch.empty((H - 10, W - 10) + ((C,) if a.dim() == 3 else ()), dtype=torch.float32, device=dev) if return_map else None
    with _hip.on_device(dev):
        _hip.check(lib.eslam_ssim(_hip.ptr(a), _hip.ptr(b), H, W, C, _hip.ptr(ws), _hip.ptr(smap), _hip.ptr(mean),
                                  _hip.stream_handle(dev)), "eslam_ssim")
    return (mean[0], smap) if return_map else mean[0]


def _vis_panel(depth, color, gt_depth, gt_color, stats):
    dev = depth.device
    H, W = int(depth.shape[0]), int(depth.shape[1])
    lut = plasma_lut(dev)
    out = torch.empty(2 * H, 3 * W, 3, dtype=torch.uint8, device=dev)
    with _hip.on_device(dev):
        _hip.check(_hip.lib().eslam_vis_panel(_hip.ptr(depth), _hip.ptr(gt_depth), _hip.ptr(color), _hip.ptr(gt_color), H, W,
                                              _hip.ptr(stats), _hip.ptr(lut), _hip.ptr(out), _hip.stream_handle(dev)),
                   "eslam_vis_panel")
    return out


def vis_panel(depth, color, gt_depth, gt_color, stats=None):
    """uint8 [2H,3W,3] on the device: the frame visualiser's panel (eslam_vis_panel).  Row 0: input depth, rendered depth,
    depth residual through the plasma map with vmax = max gt_depth; row 1: input colour, rendered colour, colour residual;
    residuals are 0 where gt_depth == 0.  `stats` is frame_stats' result for the same frame, computed here when not given.
    On the caller's current stream; no synchronisation."""
    depth, color, gt_depth, gt_color = _frame_args("vis_panel", depth, color, gt_depth, gt_color)
    if stats is None:
        stats = _frame_stats(depth, color, gt_depth, gt_color)
    elif (not torch.is_tensor(stats) or stats.device != depth.device or stats.dtype != torch.float64 or tuple(stats.shape) != (4,)
          or not stats.is_contiguous()):
        raise RuntimeError("vis_panel: stats must be frame_stats' float64 [4] tensor on the images' device")
    return _vis_panel(depth, color, gt_depth, gt_color, stats)


def _metrics_from(stats_ssim, n_color_values):
    """dict(psnr, ssim, depth_l1, n_valid) from the five numbers [n_valid, sum |d|, sum c^2, max, ssim] on the host."""
    n_valid, s_abs, s_sq, _, ss = (float(v) for v in stats_ssim)
    mse = s_sq / n_color_values
    psnr = -10.0 * math.log10(mse) if mse > 0.0 else float("inf")
    return dict(psnr=psnr, ssim=ss, depth_l1=s_abs / n_valid if n_valid > 0 else float("nan"), n_valid=n_valid)


def frame_metrics(depth, color, gt_depth, gt_color, stats=None):
    """dict(psnr, ssim, depth_l1, n_valid) of Python floats for a rendered frame against its ground truth:
    psnr = -10 log10(sum_sq_color / (3 H W)), ssim = ssim(color, gt_color), depth_l1 = sum_abs_depth / n_valid (nan when no
    pixel has depth).  The one call here that synchronises (one download of five numbers).  `stats`: frame_stats' result
    for the same frame when the caller already has it."""
    depth, color, gt_depth, gt_color = _frame_args("frame_metrics", depth, color, gt_depth, gt_color)
    if stats is None:
        stats = _frame_stats(depth, color, gt_depth, gt_color)
    s = ssim(color, gt_color)
    return _metrics_from(torch.cat([stats, s[None]]).cpu().tolist(), 3 * depth.shape[0] * depth.shape[1])
