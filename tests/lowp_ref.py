"""Host model of the mixed-precision kernels (fp16 plane copies, bf16-MFMA decoders): the float64 oracle with the kernels'
rounding points, read from csrc/eslam_decode_tile.h (f2bf, stage_decoder_weights_lowp, mlp_hidden_lp, mlp_out_accum_lp,
gather8_half, store_features_lp), csrc/eslam_render_bwd.hip (the LOWP branches of mlp_bwd_kernel) and
csrc/eslam_render_lowp.hip (planes_to_half_kernel).  Everything that is not rounded - normalisation, bilinear index
arithmetic and weights, composite, losses - is oracle/eslam_oracle.py.  Test-only.

    planes   each float32 master rounded ONCE to IEEE half; bilinear gather and the three-orientation sum on those values
             with unrounded weights
    forward  f = bf16(features); a1 = bf16(W1) f + b1; h1 = bf16(relu a1); a2 = bf16(W2) h1 + b2; h2 = bf16(relu a2);
             out = bf16(W3) h2 + b3.  Biases, accumulation, tanh / sigmoid, composite and loss unrounded.
    backward g_o = gradient at the decoder's pre-activation output (unrounded composite / tanh / sigmoid backward);
             g_h2 = bf16(W3)^T bf16(g_o); g_z2 = g_h2 [a2 > 0]; g_h1 = bf16(W2)^T bf16(g_z2); g_z1 = g_h1 [a1 > 0];
             g_feat = bf16(W1)^T bf16(g_z1); g_b = sum of the UNROUNDED g_z / g_o;
             g_W3 = sum bf16(g_o) x h2, g_W2 = sum bf16(g_z2) x h1, g_W1 = sum bf16(g_z1) x f with the bf16 h2, h1, f of the
             forward.  Plane gradients: g_feat scattered with the unrounded bilinear weights straight onto the float32
             masters (the roundings of planes and features pass gradients through unchanged).  g_beta unrounded.
    not built: ray / pose gradients (ops.RenderFn.forward raises).

`Model(dtype=torch.float64)` accumulates in float64; `Model(dtype=torch.float32)` is the same model in the kernels' own
accumulation format (torch's summation order).  One known deviation of the float64 model: a float64 value that is rounded
float64 -> float32 -> bf16 is rounded twice, which can land on the other side of a bf16 tie than the kernel's single rounding
of its float32 value - it counts as a rounding flip (see `Criteria`).

`Model.identity()` replaces every rounder by the identity and is then the plain oracle (tests/test_lowp_ref.py).
The keyword arguments of Model other than dtype exist for the mutation tests: each switches ONE rounding point to a plausible
wrong reading of the kernel.
"""
from dataclasses import dataclass

import numpy as np
import torch

from oracle import eslam_oracle as orc


# ----------------------------------------------------------------------------------------------------------------------
# rounders (value in, value out, same dtype as the input; the rounding itself is that of a float32 input, as on the device)
# ----------------------------------------------------------------------------------------------------------------------
def _f32_bits(x):
    return x.detach().to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _from_bits(u, like):
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32)
    return u.view(torch.float32).to(like.dtype)


def bf16_rne(x):
    """f2bf of eslam_decode_tile.h bit for bit: u += 0x7FFF + ((u >> 16) & 1); u >>= 16 on the float32 bits (mod 2^32)."""
    u = _f32_bits(x)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF
    return _from_bits((u >> 16) << 16, x)


def bf16_trunc(x):
    """The wrong f2bf: drops the low 16 bits (mutation tests only)."""
    return _from_bits((_f32_bits(x) >> 16) << 16, x)


def fp16_rne(x):
    """float32 -> IEEE half (round to nearest even, subnormals below 2^-14, overflow to inf from 65520 on), as the
    (_Float16) conversion of planes_to_half_kernel; written in exact float64 arithmetic, not with torch's half type."""
    v = x.detach().to(torch.float32).to(torch.float64)
    _, e = torch.frexp(v)                               # |v| = m 2^e, m in [0.5, 1)  ->  floor(log2 |v|) = e - 1
    q = torch.ldexp(torch.ones_like(v), (e - 1).clamp(min=-14) - 10)          # spacing of half values around v
    r = torch.round(v / q) * q                          # both exact (powers of two); torch.round rounds halves to even
    r = torch.where(r.abs() >= 65520.0, torch.copysign(torch.full_like(r, float("inf")), v), r)
    r = torch.where(torch.isfinite(v), r, v)
    return r.to(x.dtype)


def identity(x):
    return x


class _Through(torch.autograd.Function):
    """y = fn(x) with the gradient passed through unchanged."""

    @staticmethod
    def forward(ctx, x, fn):
        return fn(x)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _Replace(torch.autograd.Function):
    """y = given values, with the gradient passed to x unchanged (teacher forcing)."""

    @staticmethod
    def forward(ctx, x, given):
        return given.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


class _Relu(torch.autograd.Function):
    """relu with the kernels' mask: the gradient passes where the PRE-activation is > 0."""

    @staticmethod
    def forward(ctx, a):
        ctx.save_for_backward(a)
        return a.clamp(min=0)

    @staticmethod
    def backward(ctx, g):
        (a,) = ctx.saved_tensors
        return torch.where(a > 0, g, torch.zeros_like(g))


class _Linear(torch.autograd.Function):
    """out = x rw(W)^T + rb(b) for an x that holds the values the kernel multiplies (already rounded).
    Backward, with g the unrounded gradient at `out`: g_x = rg(g) rw(W), g_W = rg(g)^T x, g_b = sum g."""

    @staticmethod
    def forward(ctx, x, W, b, rw, rb, rg, perm):
        Wq = rw(W)
        if perm is not None:
            Wq = Wq[:, perm]
        ctx.save_for_backward(x, Wq)
        ctx.rg, ctx.perm = rg, perm
        return x @ Wq.t() + rb(b)

    @staticmethod
    def backward(ctx, g):
        x, Wq = ctx.saved_tensors
        gq = ctx.rg(g)
        gW = gq.t() @ x
        if ctx.perm is not None:
            gW = gW[:, torch.argsort(ctx.perm)]
        return gq @ Wq, gW, g.sum(0), None, None, None, None


class Model:
    def __init__(self, dtype=torch.float64, bf=bf16_rne, plane=fp16_rne, bias=identity, round_h2=True, round_bwd=True,
                 swap_w1=None):
        self.dtype, self.bf, self.plane, self.bias = dtype, bf, plane, bias
        self.h2 = bf if round_h2 else identity
        self.rg = bf if round_bwd else identity
        self.swap_w1 = swap_w1                      # (k, k'): the sdf decoder reads W1[:, k] where it should read W1[:, k']

    @classmethod
    def identity(cls, dtype=torch.float64):
        return cls(dtype, bf=identity, plane=identity, round_h2=False, round_bwd=False)

    def mlp(self, feat, params, c, given=None):
        """One decoder (c = "" sdf, "c_" colour) on unrounded features [N,64]: (pre-activation output [N,nout], f).
        given: bf16 values [N,64] to use as f in place of bf16(feat)."""
        perm = None
        if self.swap_w1 is not None and c == "":
            perm = torch.arange(64)
            perm[list(self.swap_w1)] = perm[list(self.swap_w1)[::-1]]
        lin = lambda x, name, p=None: _Linear.apply(x, params[f"{c}{name}.weight"], params[f"{c}{name}.bias"], self.bf,
                                                    self.bias, self.rg, p)
        f = _Through.apply(feat, self.bf) if given is None else _Replace.apply(feat, given)
        h1 = _Through.apply(_Relu.apply(lin(f, "linears.0", perm)), self.bf)
        h2 = _Through.apply(_Relu.apply(lin(h1, "linears.1")), self.h2)
        return lin(h2, "output_linear"), f

    def render(self, all_planes, params, beta, bound, rays_o, rays_d, z_vals, feat=None):
        """The render kernel on given z_vals [R,S]: dict(depth [R], color [R,3], sdf [R,S], raw_rgb [R,S,3],
        feat [R*S,128] = the bf16 features of both decoders in natural channel order, as the forward saves them,
        feat_unrounded = the same before the rounding).
        feat [R*S,128]: TEACHER FORCING - the decoders' first layers consume these bf16 features (the ones a kernel run
        saved) instead of the model's own; gradients still flow to the planes through the model's bilinear weights.  Nearly
        all rounding flips between two evaluations start at a feature (its bilinear weights come from float32
        coordinates); with the features forced, what is left is the decoders and the composite on identical inputs."""
        dt = self.dtype
        bound = bound.to(dt)
        pts = rays_o[:, None, :] + rays_d[:, None, :] * z_vals[..., None]
        p_nor = orc.normalize_points(pts, bound)
        q = [[_Through.apply(p, self.plane) for p in grp] for grp in all_planes]
        u_s = orc.plane_features(p_nor, q[0], q[1], q[2])
        u_c = orc.plane_features(p_nor, q[3], q[4], q[5])
        given = (None, None) if feat is None else (feat[:, :64].to(dt), feat[:, 64:].to(dt))
        o_s, f_s = self.mlp(u_s, params, "", given[0])
        o_c, f_c = self.mlp(u_c, params, "c_", given[1])
        raw = torch.cat([torch.sigmoid(o_c), torch.tanh(o_s)], -1).reshape(*z_vals.shape, 4)
        depth, color = orc.composite(raw, z_vals, beta)
        return dict(depth=depth, color=color, sdf=raw[..., 3], raw_rgb=raw[..., :3], feat=torch.cat([f_s, f_c], -1).detach(),
                    feat_unrounded=torch.cat([u_s, u_c], -1).detach())


def run_model(model, fx, z_vals, backward=True, feat=None):
    """A fixture through `model` on the given z_vals (any float dtype; converted exactly): forward, the fixture's loss and
    - backward=True - autograd.  Returns numpy arrays: depth, color, sdf, raw_rgb, feat, loss, planes (12 gradients in
    all_planes order, [1,C,h,w]), dec {name: gradient}, beta (gradient or None).  feat: see Model.render."""
    from tests import helpers as hp
    dt = model.dtype
    sc, planes = hp.scene_and_planes(fx, dtype=torch.float32, channels_last=False)
    planes = tuple([p.to(dt).requires_grad_(backward) for p in grp] for grp in planes)
    params = hp.params_from(fx, dtype=dt, requires_grad=backward)
    beta = float(fx["beta"])
    if bool(fx["beta_is_param"]):
        beta = torch.tensor([beta], dtype=dt, requires_grad=backward)
    cv = lambda k: torch.from_numpy(fx[k]).to(dt)
    z = torch.as_tensor(z_vals).to(dt)
    with torch.set_grad_enabled(backward):
        r = model.render(planes, params, beta, sc.bound, cv("rays_o"), cv("rays_d"), z,
                         None if feat is None else torch.as_tensor(np.asarray(feat, dtype=np.float32)))
        loss_fn = orc.mapping_loss if str(fx["loss_kind"]) == "mapping" else orc.tracking_loss
        loss = loss_fn(r["depth"], r["color"], r["sdf"], z, cv("gt_depth"), cv("gt_color"), float(fx["truncation"]))
        if backward:
            loss.backward()
    out = {k: v.detach().numpy() for k, v in r.items()}
    out["loss"] = float(loss.detach())
    if backward:
        out["planes"] = [p.grad.numpy() for p in hp.flat_planes(planes)]
        out["dec"] = {k: p.grad.numpy() for k, p in params.items()}
        out["beta"] = beta.grad.numpy() if torch.is_tensor(beta) else None
    return out


def float32_z(fx):
    """z_vals [R,S] float32 of a fixture as the float32 oracle samples them on the unrounded float32 planes (what the
    mixed-precision path does too: its sampler is the float32 path on the masters)."""
    from tests import helpers as hp
    sc, planes = hp.scene_and_planes(fx, channels_last=False)
    t_rand, t_uni, u = hp.rand_inputs(fx)
    cv = lambda k: torch.from_numpy(fx[k])
    with torch.no_grad():
        return orc.sample_z(cv("rays_o"), cv("rays_d"), cv("gt_depth"), planes, hp.params_from(fx), float(fx["beta"]),
                            sc.bound, float(fx["truncation"]), int(fx["n_stratified"]), int(fx["n_importance"]),
                            t_rand, t_uni, u).numpy()


# ----------------------------------------------------------------------------------------------------------------------
# acceptance criteria, shared by the GPU test (kernel vs model) and the CPU tests (model vs model, mutant vs model)
# ----------------------------------------------------------------------------------------------------------------------
def bf16_ordinal(x):
    """int64 position of every (bf16-representable) value on the bf16 number line: neighbours differ by 1, -0 == +0."""
    u = (_f32_bits(torch.as_tensor(np.ascontiguousarray(x))) >> 16)
    return torch.where(u >= 0x8000, 0x8000 - u, u).numpy()


def bf16_ulp(x):
    """Spacing of bf16 values at |x| (8 significant bits), float64 array."""
    _, e = np.frexp(np.abs(np.float64(x)))
    return np.ldexp(1.0, np.maximum(e - 1, -126) - 7)


@dataclass(frozen=True)
class Criteria:
    """What `measure` must stay under for `got` to count as an evaluation of the model `ref`.  A rounding flip - float32
    accumulation or float32 coordinates landing a value on the other side of a bf16 tie than the model's - moves one sample
    by as much as the quantisation itself, so the per-sample criteria bound the SHARE of samples that move, not the largest
    move; the largest move stays under the bounds of the tolerance study."""
    tol: dict                    # T per quantity (sdf, raw_rgb: per sample; color, depth: per ray; depth relative to
                                 # max(|depth|, 1e-3)): the float32-level tolerance.  At most `outliers` of the samples on rays
                                 # with depth may be further from the model.
    feat_unequal: float          # largest share of saved bf16 features that may differ from the model's
    feat_abs: float              # a differing feature is within one bf16 ulp + feat_abs of the model's (see measure)
    plane_grad: float            # max-normalised error, the worst of the 12 planes
    dec_grad: float              # max-normalised error, the worst decoder tensor (and beta)
    closer: float                # every weight / plane gradient is this many times closer to the model than to the plain oracle
    max_sdf: float = np.inf      # the study bounds of the fixture: no sample / ray beyond them
    max_rgb: float = np.inf
    max_depth: float = np.inf
    outliers: float = 0.10
    loss: float = np.inf         # relative error of the loss (a handful of float32 means over all samples / rays)


def measure(got, ref, has_depth, plain=None, free=None):
    """The figures the criteria are about, as a dict.  got / ref / plain / free: dicts as run_model returns (got may lack
    the gradients).  ref = the model, teacher-forced with got's features or not; free = the model on its own features, for
    the feature criteria (default: ref); plain = the unquantised oracle's gradients for the `closer` ratios.
    has_depth: bool [R]."""
    from tests import helpers as hp
    hd = np.asarray(has_depth, dtype=bool)
    m = {}
    m["sdf"] = np.abs(np.float64(got["sdf"]) - ref["sdf"])[hd]
    if "raw_rgb" in got:
        m["raw_rgb"] = np.abs(np.float64(got["raw_rgb"]) - ref["raw_rgb"])[hd]
    m["color"] = np.abs(np.float64(got["color"]) - ref["color"])[hd].max(-1)
    m["depth"] = (np.abs(np.float64(got["depth"]) - ref["depth"]) / np.maximum(np.abs(ref["depth"]), 1e-3))[hd]
    free = ref if free is None else free
    if "feat" in got:
        a, b = np.float64(got["feat"]), np.float64(free["feat"])
        m["feat_unequal"] = float((bf16_ordinal(got["feat"]) != bf16_ordinal(free["feat"])).mean())
        # how far a feature is BEYOND one bf16 ulp of the model's.  A feature is a sum of 12 texel products whose bilinear
        # weights come from float32 coordinates: where the products cancel, the sum's own float32 error exceeds the ulp of
        # the small result, and two correct evaluations are then several of those small ulps apart (Criteria.feat_abs)
        m["feat_excess"] = float((np.abs(a - b) - bf16_ulp(np.maximum(np.abs(a), np.abs(b)))).max())
        if "feat_unrounded" in got:
            m["feat_unrounded"] = float(np.abs(np.float64(got["feat_unrounded"]) - free["feat_unrounded"]).max())
    if "planes" in got:
        m["loss"] = abs(got["loss"] - ref["loss"]) / abs(ref["loss"])
        m["plane_grad"] = [hp.rel_err(a, b) for a, b in zip(got["planes"], ref["planes"])]
        m["dec_grad"] = {k: hp.rel_err(got["dec"][k], ref["dec"][k]) for k in ref["dec"]}
        if ref.get("beta") is not None:
            m["dec_grad"]["beta"] = hp.rel_err(got["beta"], ref["beta"])
        if plain is not None:
            m["plane_plain"] = [hp.rel_err(a, b) for a, b in zip(got["planes"], plain["planes"])]
            m["dec_plain"] = {k: hp.rel_err(got["dec"][k], plain["dec"][k]) for k in ref["dec"]}
    return m


def summary(m, tol):
    """One printable line of the measured figures."""
    s = [f"{k}: max {m[k].max():.2e} q90 {np.quantile(m[k], 0.9):.2e} beyond T {(m[k] > tol[k]).mean():.4f}"
         for k in ("sdf", "raw_rgb", "color", "depth") if k in m]
    if "feat_unequal" in m:
        s.append(f"features: unequal {m['feat_unequal']:.2e}, beyond one ulp by {m['feat_excess']:.2e}"
                 + (f", unrounded {m['feat_unrounded']:.2e}" if "feat_unrounded" in m else ""))
    if "loss" in m:
        s.append(f"loss {m['loss']:.2e}  plane gradients {max(m['plane_grad']):.2e}  decoder gradients "
                 f"{max(m['dec_grad'].values()):.2e} ({max(m['dec_grad'], key=m['dec_grad'].get)})")
    if "plane_plain" in m:
        s.append(f"closer to the model than to the plain oracle by >= {closer_ratio(m):.1f}")
    return "; ".join(s)


def closer_ratio(m):
    """The smallest (error against the plain oracle) / (error against the model) over the plane gradients and the decoders'
    weight gradients.  Bias and beta gradients are left out: they are sums of unrounded values."""
    r = [p / max(e, 1e-300) for p, e in zip(m["plane_plain"], m["plane_grad"])]
    r += [m["dec_plain"][k] / max(m["dec_grad"][k], 1e-300) for k in m["dec_plain"] if k.endswith("weight")]
    return min(r)


def failures(m, c):
    """The criteria that the figures `m` miss, as a list of strings (empty = accepted)."""
    bad = []
    for k, cap in (("sdf", c.max_sdf), ("raw_rgb", c.max_rgb), ("color", c.max_rgb), ("depth", c.max_depth)):
        if k not in m:
            continue
        share = float((m[k] > c.tol[k]).mean())
        if share > c.outliers:
            bad.append(f"{k}: {share:.3f} of the samples beyond {c.tol[k]:.1e}")
        if m[k].max() >= cap:
            bad.append(f"{k}: max {m[k].max():.2e} >= {cap:.1e}")
    if "feat_unequal" in m:
        if m["feat_excess"] > c.feat_abs:
            bad.append(f"features: one bf16 ulp + {m['feat_excess']:.2e} off (> {c.feat_abs:.1e})")
        if m["feat_unequal"] > c.feat_unequal:
            bad.append(f"features: share unequal {m['feat_unequal']:.2e} > {c.feat_unequal:.2e}")
    if "loss" in m:
        if m["loss"] > c.loss:
            bad.append(f"loss {m['loss']:.2e} > {c.loss:.1e}")
        if max(m["plane_grad"]) > c.plane_grad:
            bad.append(f"plane gradients {max(m['plane_grad']):.2e} > {c.plane_grad:.1e}")
        worst = max(m["dec_grad"], key=m["dec_grad"].get)
        if m["dec_grad"][worst] > c.dec_grad:
            bad.append(f"decoder gradient {worst} {m['dec_grad'][worst]:.2e} > {c.dec_grad:.1e}")
    if "plane_plain" in m and closer_ratio(m) < c.closer:
        bad.append(f"gradients only {closer_ratio(m):.1f}x closer to the model than to the plain oracle (< {c.closer})")
    return bad


def assert_agrees(got, ref, has_depth, crit, plain=None, free=None, label=""):
    """THE assertion of the mixed-precision parity tests: prints the figures, then fails on any missed criterion."""
    m = measure(got, ref, has_depth, plain, free)
    print(f"{label}: {summary(m, crit.tol)}")
    bad = failures(m, crit)
    assert not bad, (label, bad)
    return m


# ----------------------------------------------------------------------------------------------------------------------
# The numbers behind the criteria.  Every one is measured on the REFERENCE alone - the model in float32 (torch's CPU summation
# order) against the float64 model teacher-forced with the float32 model's features, tests/test_lowp_ref.py re-measures and
# asserts them - and widened by MARGIN for a second float32 evaluation whose summation order is neither (MFMA blocks,
# 16-point partial sums, slabs, atomic scatter).  KERNEL_MEASURED is the place of the kernels' own figures (MI355X), for the
# reader only - they enter nothing; every GPU test prints its line of them (pytest -s).  It holds no figure: the GPU tests of
# this file's criteria have not been run on an MI355X, so whether the kernels fit under 4x the CPU figures is not known.
#   q97          the level 97 % of the reference's samples (rays) stay under: the reference meets the 10 % cap with room
#   feat_*       saved bf16 features against the free-running float64 model: share that differs, and how far beyond one
#                bf16 ulp the worst one is (a cancelled sum of 12 texel products whose weights come from float32 coordinates)
#   loss         relative error of the loss
#   plane / dec  max-normalised gradient errors (worst plane, worst decoder tensor); closer: see closer_ratio
# ----------------------------------------------------------------------------------------------------------------------
MARGIN = 4.0
EPS32 = 2.0 ** -23
MIXED_FIXTURES = ("freiburg1_desk_5000x56_zero10", "room0_4096x64_trained_zero10")
TRACKING_FIXTURE = "room0_200x40_tracking"        # forward only (frozen decoders, pose gradients are not built), S = 40
CPU_SELF_AGREEMENT = {
    "freiburg1_desk_5000x56_zero10": dict(                                  # the reference's initial state
        q97=dict(sdf=3.72e-9, raw_rgb=4.48e-8, color=7.88e-8, depth=7.57e-7),
        feat_unequal=3.91e-3, feat_excess=7.75e-7, loss=4.78e-8, plane=4.59e-6, dec=2.33e-5, closer=7.54),
    "room0_4096x64_trained_zero10": dict(                                   # trained-like: O(1) features
        q97=dict(sdf=3.94e-8, raw_rgb=4.56e-8, color=8.40e-8, depth=1.94e-7),
        feat_unequal=4.80e-3, feat_excess=6.10e-5, loss=8.11e-8, plane=3.43e-6, dec=1.97e-6, closer=637.0),
    "room0_200x40_tracking": dict(
        q97=dict(sdf=3.72e-9, raw_rgb=4.48e-8, color=8.97e-8, depth=6.92e-7),
        feat_unequal=4.89e-3, feat_excess=4.77e-7, loss=None, plane=None, dec=None, closer=None),
}
KERNEL_MEASURED = {}


def criteria(case, ref):
    """The Criteria of a fixture.  ref: the model's outputs (for the scale of one float32 ulp).
    T = MARGIN x max(the reference's q97, one float32 ulp of the quantity's largest magnitude): tanhf, expf and the division
    of the sigmoid are not correctly rounded on the device (nor need they be), so a float32 output cannot be held to less
    than ulps of its own scale, however well torch's float32 agrees with float64 on small values.  The loss bound has the
    same form: MARGIN x max(the reference's relative loss error, one float32 ulp) - torch's pairwise float32 sums land below
    one ulp of the result, which no other summation order can be asked to repeat.
    The largest move of any sample stays under the tolerance study's bounds (tests/test_gpu_parity.py MIXED_CASES, unchanged;
    the tracking fixture is the initial state and takes the initial-state fixture's)."""
    from tests.test_gpu_parity import MIXED_CASES
    c = CPU_SELF_AGREEMENT[case]
    scale = dict(sdf=np.abs(ref["sdf"]).max(), raw_rgb=np.abs(ref["raw_rgb"]).max(), color=np.abs(ref["color"]).max(), depth=1.0)
    tol = {k: MARGIN * max(c["q97"][k], EPS32 * float(scale[k])) for k in scale}
    b_sdf, b_rgb, b_dep = MIXED_CASES[case if case in MIXED_CASES else MIXED_FIXTURES[0]][0]
    inf = float("inf")
    return Criteria(tol=tol, feat_unequal=MARGIN * c["feat_unequal"], feat_abs=MARGIN * c["feat_excess"],
                    plane_grad=MARGIN * c["plane"] if c["plane"] else inf, dec_grad=MARGIN * c["dec"] if c["dec"] else inf,
                    closer=c["closer"] / MARGIN if c["closer"] else 0.0, max_sdf=b_sdf, max_rgb=b_rgb, max_depth=b_dep,
                    loss=MARGIN * max(c["loss"], EPS32) if c["loss"] else inf)


# ----------------------------------------------------------------------------------------------------------------------
# exact-arithmetic inputs: nothing the model rounds has anything to round
# ----------------------------------------------------------------------------------------------------------------------
EXACT_SHAPES = ((1, 40), (37, 24), (130, 56), (257, 64))      # R x S: a lone ray, partial 16-point blocks, partial waves


def _checked(fn, what):
    def g(x):
        y = fn(x)
        assert torch.equal(y, x), f"exact case: {what} has {int((y != x).sum())} values that are not representable"
        return y
    return g


def exact_case(R, S, seed=0):
    """Synthetic inputs on which the mixed-precision kernels compute what the float32 kernels compute: every value the model
    rounds is representable in the format it is rounded to, every float32 sum in front of a rounding is exact, so no
    rounding flip can occur and the PLAIN float64 oracle is the reference, at the float32 parity tolerance.

      bound [-1,1]^3; plane axes of 33 or 65 texels; ray origins on multiples of 1/32, direction components in
      {0, +-1/2, +-1}, z_vals on multiples of 1/32 (1/16 on rays with a +-1/2): normalised coordinates are multiples of
      1/32, bilinear t in {0, 1/2}; a good part of the samples leaves the box and is clamped to its border (t = 0);
      texels in {-1/2, -1/4, 0, 1/4, 1/2} (half-exact): features are multiples of 1/16 below 1.5 (bf16-exact);
      W1 in {-1,0,1}, every column in two rows; W2 in {-1,0,1}, three per row; b1, b2 multiples of 1/4: pre-activations are
      multiples of 1/16 and - asserted here, sample by sample - below 16, i.e. bf16-exact; W3 multiples of 1/256 up to
      1/16 (bf16-exact; outputs stay out of tanh's saturation); b3 is NOT bf16-representable: biases are not rounded.
    Rows of every weight matrix, feature channels and outputs are all different from one another, so that a lane, fragment
    or k-order mix-up changes the result.

    Returns dict(planes: 6 groups of [coarse, fine] float32 [1,32,h,w] (NCHW-contiguous), params {name: float32}, bound
    [3,2], beta, rays_o, rays_d [R,3], z_vals [R,S] float32, oracle: Model.identity().render(...) in float64)."""
    g = torch.Generator().manual_seed(1000 * R + S + seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    axes = {"": ((33, 65, 33), (65, 33, 65)), "c_": ((65, 33, 33), (33, 33, 65))}      # (nx, ny, nz) of coarse, fine
    planes = []
    for c in ("", "c_"):
        grp = [[], [], []]
        for nx, ny, nz in axes[c]:
            for k, (h, w) in enumerate(((ny, nx), (nz, nx), (nz, ny))):               # xy, xz, yz (scene.plane_shapes)
                grp[k].append(ri(-2, 2, (1, 32, h, w)).float() / 4)
        planes += grp
    params = {}
    for c in ("", "c_"):
        W1 = torch.zeros(16, 64)
        for col in range(64):
            r0 = col % 16
            r1 = (r0 + 1 + int(ri(0, 14, (1,)))) % 16
            W1[r0, col], W1[r1, col] = (float(v) for v in (ri(0, 1, (2,)) * 2 - 1))
        W2 = torch.zeros(16, 16)
        for row in range(16):
            while not W2[row].any() or any(torch.equal(W2[row], W2[k]) for k in range(row)):
                W2[row] = 0
                W2[row, torch.randperm(16, generator=g)[:3]] = (ri(0, 1, (3,)) * 2 - 1).float()
        nout = 1 if c == "" else 3
        W3 = ri(1, 16, (nout, 16)).float() / 256 * (ri(0, 1, (nout, 16)) * 2 - 1)
        params[f"{c}linears.0.weight"], params[f"{c}linears.1.weight"], params[f"{c}output_linear.weight"] = W1, W2, W3
        params[f"{c}linears.0.bias"] = ri(-4, 4, (16,)).float() / 4
        params[f"{c}linears.1.bias"] = ri(-4, 4, (16,)).float() / 4
        params[f"{c}output_linear.bias"] = ri(-4, 4, (nout,)).float() / 8 + 2.0 ** -12
        for name in ("linears.0.weight", "linears.1.weight", "output_linear.weight"):
            W = params[c + name]
            assert len({tuple(r.tolist()) for r in W}) == W.shape[0], "weight rows must differ"
        assert not torch.equal(bf16_rne(params[f"{c}output_linear.bias"]), params[f"{c}output_linear.bias"])
    rays_o = ri(-24, 24, (R, 3)).float() / 32
    rays_d = ri(-2, 2, (R, 3)).float() / 2
    rays_d[0] = torch.tensor([0.0, 0.0, 1.0])                                        # one axis-aligned ray, leaving the box
    rays_o[0, 2] = 0.25
    dead = (rays_d == 0).all(1)
    rays_d[dead, 0] = 1.0
    half = (rays_d.abs() == 0.5).any(1, keepdim=True)                                # those rays need z on multiples of 1/16
    z_vals = (ri(0, 8, (R, 1)).float() + torch.arange(S).float()[None, :]) / torch.where(half, 16.0, 32.0)
    bound = torch.tensor([[-1.0, 1.0]] * 3)
    out = dict(planes=tuple(planes), params=params, bound=bound, beta=10.0, rays_o=rays_o, rays_d=rays_d, z_vals=z_vals)
    to64 = lambda t: t.double()
    args = (tuple([to64(p) for p in grp] for grp in planes), {k: to64(v) for k, v in params.items()}, 10.0, bound,
            to64(rays_o), to64(rays_d), to64(z_vals))
    with torch.no_grad():
        chk = Model(bf=_checked(bf16_rne, "a bf16 operand"), plane=_checked(fp16_rne, "a texel"), round_bwd=False)
        rounded = chk.render(*args)
        out["oracle"] = Model.identity().render(*args)
    for k in ("sdf", "raw_rgb", "depth", "color", "feat"):
        assert torch.equal(rounded[k], out["oracle"][k]), k
    inside = ((to64(rays_o)[:, None] + to64(rays_d)[:, None] * to64(z_vals)[..., None]).abs() < 1).all(-1)
    assert 0.2 < float(inside.double().mean()) < 0.9, "the exact case needs samples inside and outside the box"
    assert float(out["oracle"]["sdf"].abs().max()) < 0.995, "outputs must stay out of tanh's saturation"
    return out
