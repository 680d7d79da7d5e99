"""Free points through the host model of the mixed-precision kernels: tests/lowp_ref.Model's decoders behind the oracle's
normalisation and tri-plane gather on the fp16-rounded planes - what eslam_decode_fwd / eslam_sdf_grid / eslam_decode_bwd
compute on planes that carry half copies (csrc/eslam_render_fwd.hip decode_fwd_kernel<..., true>, csrc/eslam_render_bwd.hip
mlp_bwd_kernel<0, ., true> and the point mode of coord_bwd_lowp_kernel).  Test-only.

    decode(model, planes, params, bound, pts, feat)   raw [N,4] = (sigmoid(colour), tanh(sdf)) and the bf16 features [N,128]
    gradients(model, state, n, feat)                  the same with autograd of L = sum(raw * G) for the state's fixed G:
                                                      points, all 12 planes and all decoder tensors are the leaves

The roundings of planes and features pass gradients through (lowp_ref), so the position derivative acts on the fp16-ROUNDED
texels, with the border clamp's gate and the (w - 1) / 2, 2 / (hi - lo) factors of the float32 path (lowp_pose_ref).

States (no golden file of their own: both come from committed fixtures):
    trained   planes and decoders of room0_200x40_trained_zero15, points = its 8000 samples rays_o + rays_d z_vals in float32
    initial   planes and decoders of room0_200x32, points = its 6400 samples
and in both a seeded tenth of the points is replaced by points uniform in the bound stretched by 10 % on each side, so that
some lie outside (border clamp, zero gradient for that coordinate).  `pts_plain` keeps the samples without that padding.
Prefixes of N points are run, N in SIZES; a state with fewer points than the largest N runs all it has.

Acceptance criteria (every figure from two evaluations of the model on the host, none from a kernel):
    ref = Model() in float64, f32 = Model(torch.float32), both TEACHER-FORCED with the features the run under test saved
    (free-running the two differ by 1e-1 in the gradients: a bf16 tie that flips at a feature moves the point's whole
    contribution).
  forward, per quantity (colour: max over the 3 channels; sdf): T = MARGIN x max(q97 of |f32 - ref|, 2^-23 max |ref|), the
    construction of lowp_ref.criteria; at most 10 % of the points beyond T; no point further from ref than CAP, the largest
    distance of the free-running model from the plain oracle over the state's FULL point set (a flipped hidden bf16 tie moves
    a point by the quantisation's own size, not more).
  saved features, against the free-running float64 model: the number that differ is at most ceil(MARGIN x rate x 128 n),
    rate = the float32 model's share on the full set (a share of 128 n features moves in steps of 1 / (128 n): the ceiling
    is that step, nothing else); a differing feature is within one bf16 ulp + MARGIN x the float32 model's excess
    (lowp_ref.measure's feat_unequal / feat_excess).
  gradients: g_pts, the worst of the 12 plane gradients, the worst decoder tensor: max-normalised error against ref
    <= MARGIN x max(error of f32 against ref, OUT_RTOL); and g_pts point by point (lowp_pose_ref.per_ray_excess):
    |got - ref| of a point <= MARGIN x max(|f32 - ref| of that point, OUT_RTOL max |ref|).
"""
import functools
import math

import numpy as np
import torch

from oracle import eslam_oracle as orc
from tests import helpers as hp
from tests import lowp_pose_ref as pr
from tests import lowp_ref as lr

MARGIN = lr.MARGIN
STATES = {"trained": "room0_200x40_trained_zero15", "initial": "room0_200x32"}
SIZES = (1, 15, 16, 17, 63, 64, 65, 255, 257, 8000)
QUANTITIES = ("color", "sdf")


def decode(model, planes, params, bound, pts, feat=None):
    """(raw [N,4], bf16 features [N,128] in natural channel order, as the forward saves them).  feat: teacher forcing,
    exactly as in lowp_ref.Model.render."""
    dt = model.dtype
    p_nor = orc.normalize_points(pts, bound.to(dt))
    q = [[lr._Through.apply(p, model.plane) for p in grp] for grp in planes]
    u_s = orc.plane_features(p_nor, q[0], q[1], q[2])
    u_c = orc.plane_features(p_nor, q[3], q[4], q[5])
    given = (None, None) if feat is None else (feat[:, :64].to(dt), feat[:, 64:].to(dt))
    o_s, f_s = model.mlp(u_s, params, "", given[0])
    o_c, f_c = model.mlp(u_c, params, "c_", given[1])
    return torch.cat([torch.sigmoid(o_c), torch.tanh(o_s)], -1), torch.cat([f_s, f_c], -1).detach()


def shortcut_decode(model, planes, params, bound, pts, feat=None):
    """The mutant an unchanged float32 coord_bwd_kernel behind the mixed-precision backward would be (lowp_pose_ref.
    ShortcutModel for free points): values from the half copies, their position derivative from the float32 masters."""
    dt = model.dtype
    p_nor = orc.normalize_points(pts, bound.to(dt))
    q = [[lr._Through.apply(p, model.plane) for p in grp] for grp in planes]
    m = [[p.detach() for p in grp] for grp in planes]

    def feats(k):
        value = orc.plane_features(p_nor.detach(), q[k], q[k + 1], q[k + 2])
        through = orc.plane_features(p_nor, m[k], m[k + 1], m[k + 2])
        return value + (through - through.detach())

    given = (None, None) if feat is None else (feat[:, :64].to(dt), feat[:, 64:].to(dt))
    o_s, f_s = model.mlp(feats(0), params, "", given[0])
    o_c, f_c = model.mlp(feats(3), params, "c_", given[1])
    return torch.cat([torch.sigmoid(o_c), torch.tanh(o_s)], -1), torch.cat([f_s, f_c], -1).detach()


@functools.lru_cache(maxsize=None)
def state(name):
    """dict(fx, bound [3,2], planes (float32, NCHW, CPU), params, pts [N,3] float32 (padded), pts_plain [N,3], G [N,4])."""
    fx = hp.load(STATES[name])
    sc, planes = hp.scene_and_planes(fx, channels_last=False)
    cv = lambda k: torch.from_numpy(fx[k]).double()
    plain = (cv("rays_o")[:, None, :] + cv("rays_d")[:, None, :] * cv("z_vals")[..., None]).reshape(-1, 3).float()
    n = plain.shape[0]
    g = torch.Generator().manual_seed(20 + len(name))
    lo, hi = sc.bound[:, 0].float(), sc.bound[:, 1].float()
    ext = hi - lo
    idx = torch.randperm(n, generator=g)[: n // 10]
    pts = plain.clone()
    pts[idx] = (lo - 0.1 * ext) + torch.rand(idx.shape[0], 3, generator=g) * (1.2 * ext)
    G = torch.randn(n, 4, generator=g)
    return dict(name=name, fx=fx, bound=sc.bound.float(), planes=planes, params=hp.params_from(fx), pts=pts, pts_plain=plain, G=G)


def sizes(name):
    """The prefix lengths of a state: SIZES, the largest cut to the points the state has."""
    n = state(name)["pts"].shape[0]
    return tuple(sorted({min(s, n) for s in SIZES}))


def gradients(model, st, n=None, feat=None, pts="pts", fn=decode, backward=True):
    """The first n points of a state through `model`: numpy dict raw [n,4], feat [n,128] (float32 values of the bf16 features),
    and - backward - g_pts [n,3], planes (12, [1,C,h,w]), dec {name} of L = sum(raw * G[:n])."""
    dt = model.dtype
    n = st[pts].shape[0] if n is None else n
    leaf = lambda t: t.detach().clone().to(dt).requires_grad_(backward)       # (a copy: the state's tensors are shared)
    planes = tuple([leaf(p) for p in grp] for grp in st["planes"])
    params = {k: leaf(v) for k, v in st["params"].items()}
    p = leaf(st[pts][:n])
    f = None if feat is None else torch.as_tensor(np.asarray(feat, dtype=np.float32))
    with torch.set_grad_enabled(backward):
        raw, bf = fn(model, planes, params, st["bound"], p, f)
        if backward:
            (raw * st["G"][:n].to(dt)).sum().backward()
    out = dict(raw=raw.detach().double().numpy(), feat=bf.float().numpy())
    if backward:
        out["g_pts"] = p.grad.double().numpy()
        out["planes"] = [q.grad.double().numpy() for q in hp.flat_planes(planes)]
        out["dec"] = {k: v.grad.double().numpy() for k, v in params.items()}
    return out


def _as_measure(r):
    """A run's outputs as the per-point quantities of the forward criteria (colour: [n,3], compared by its worst channel)."""
    return dict(sdf=np.asarray(r["raw"], dtype=np.float64)[:, 3], color=np.asarray(r["raw"], dtype=np.float64)[:, :3])


def _measure(got, ref, free=None):
    """|got - ref| per point and quantity; with `free` (a run with features) also lowp_ref.measure's feat_unequal and
    feat_excess of got's saved features against free's."""
    a, b = _as_measure(got), _as_measure(ref)
    m = dict(sdf=np.abs(a["sdf"] - b["sdf"]), color=np.abs(a["color"] - b["color"]).max(-1))
    if free is not None:
        z = np.zeros(2)        # (measure's ray quantities: not used here)
        blank = dict(sdf=z, color=np.zeros((2, 3)), depth=z)
        f = lr.measure(dict(blank, feat=got["feat"]), blank, np.ones(2, dtype=bool), free=dict(blank, feat=free["feat"]))
        m["feat_unequal"], m["feat_excess"] = f["feat_unequal"], f["feat_excess"]
    return m


@functools.lru_cache(maxsize=None)
def full_set_figures(name):
    """What is computed once on a state's full point set and applied to every prefix: the free-running float64 model (its
    features are the reference of the feature criteria), CAP per quantity, and the float32 model's feature share / excess."""
    return figures(state(name))


def figures(st):
    """full_set_figures of any state dict (planes, params, bound, pts, G)."""
    free = gradients(lr.Model(), st, backward=False)
    f32 = gradients(lr.Model(torch.float32), st, backward=False)
    plain = gradients(lr.Model.identity(), st, backward=False)
    gap = _measure(free, plain)
    m = _measure(f32, free, free)
    return dict(free=free, cap={k: float(gap[k].max()) for k in QUANTITIES}, feat_rate=m["feat_unequal"],
                feat_excess=max(m["feat_excess"], 0.0))


def model_pair(name, n, feat, backward=True, pts="pts"):
    """(ref, f32): the float64 and the float32 model on the first n points, both forced with `feat`.  name: a state's name
    or a state dict."""
    st = state(name) if isinstance(name, str) else name
    return (gradients(lr.Model(), st, n, feat, pts, backward=backward),
            gradients(lr.Model(torch.float32), st, n, feat, pts, backward=backward))


def forward_failures(got, ref, f32, cap, report=None):
    """The forward criteria that `got` misses (list of strings).  report: a list that receives one line of figures."""
    bad = []
    mg, mf = _measure(got, ref), _measure(f32, ref)
    for k in QUANTITIES:
        scale = float(np.abs(_as_measure(ref)[k]).max())
        T = MARGIN * max(float(np.quantile(mf[k], 0.97)), lr.EPS32 * scale)
        share = float((mg[k] > T).mean())
        if report is not None:
            report.append(f"{k}: max {mg[k].max():.2e} (cap {cap[k]:.2e}) beyond T={T:.2e}: {share:.4f}")
        if share > 0.10:
            bad.append(f"{k}: {share:.4f} of the points beyond T = {T:.2e}")
        if mg[k].max() > cap[k]:
            bad.append(f"{k}: a point {mg[k].max():.2e} from the model, further than the model is from the plain oracle ({cap[k]:.2e})")
    return bad


def feature_failures(got, name, report=None):
    """The saved-feature criteria against the free-running float64 model (rows of the full set's).  name: a state's name,
    or the figures() of a state dict."""
    fig = full_set_figures(name) if isinstance(name, str) else name
    n = got["feat"].shape[0]
    free = dict(raw=fig["free"]["raw"][:n], feat=fig["free"]["feat"][:n])
    m = _measure(got, free, free)
    count = int(round(m["feat_unequal"] * 128 * n))
    allowed = math.ceil(MARGIN * fig["feat_rate"] * 128 * n)
    bar = MARGIN * fig["feat_excess"]
    if report is not None:
        report.append(f"features: {count} of {128 * n} differ (allowed {allowed}), beyond one ulp by {m['feat_excess']:.2e} (bar {bar:.2e})")
    bad = []
    if count > allowed:
        bad.append(f"features: {count} differ, more than {allowed}")
    if m["feat_excess"] > bar:
        bad.append(f"features: one bf16 ulp + {m['feat_excess']:.2e} off (> {bar:.2e})")
    return bad


def gradient_failures(got, ref, f32, report=None, which=("g_pts", "planes", "dec")):
    """The gradient criteria that `got` misses.  got may lack some of g_pts / planes / dec (then name them in `which`)."""
    from tests.test_oracle_golden import OUT_RTOL
    bad = []

    def hold(label, e, fig):
        bar = MARGIN * max(fig, OUT_RTOL)
        if report is not None:
            report.append(f"{label}: {e:.2e} (float32 model {fig:.2e}, bar {bar:.2e})")
        if not e <= bar:
            bad.append(f"{label}: {e:.2e} > {bar:.2e}")

    if "g_pts" in which:
        hold("g_pts", hp.rel_err(got["g_pts"], ref["g_pts"]), hp.rel_err(f32["g_pts"], ref["g_pts"]))
        x = point_excess(got, ref, f32)
        if report is not None:
            report.append(f"worst point at {x:.2f} of its own bar")
        if not x <= 1.0:
            bad.append(f"g_pts: a point at {x:.2f} of its own bar")
    if "planes" in which:
        e = [hp.rel_err(a, b) for a, b in zip(got["planes"], ref["planes"])]
        f = [hp.rel_err(a, b) for a, b in zip(f32["planes"], ref["planes"])]
        hold("plane gradients", max(e), max(f))
    if "dec" in which:
        e = {k: hp.rel_err(got["dec"][k], ref["dec"][k]) for k in ref["dec"]}
        f = {k: hp.rel_err(f32["dec"][k], ref["dec"][k]) for k in ref["dec"]}
        hold(f"decoder gradients ({max(e, key=e.get)})", max(e.values()), max(f.values()))
    return bad


def point_excess(got, ref, f32):
    """The largest |got - ref| / bar over the points, each point with its own bar (lowp_pose_ref.per_ray_excess)."""
    return pr.per_ray_excess((got["g_pts"],), (ref["g_pts"],), (f32["g_pts"],))[0]
