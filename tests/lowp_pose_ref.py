"""Ray (pose) gradients of the mixed-precision path on the host: tests/lowp_ref.Model.render with rays_o / rays_d as autograd
leaves and the fixture's loss from oracle/eslam_oracle.py.  Test-only.

What the model defines as the gradient (and csrc/eslam_render_bwd.hip coord_bwd_lowp_kernel computes): the roundings of planes
and features pass gradients through, so g_feat is that of the bf16 backward pass (lowp_ref's docstring) and the derivative of
the bilinear form with respect to the sample position acts on the fp16-ROUNDED texels - the values the forward interpolated -
with the border clamp's gate, (w - 1) / 2 and 2 / (hi - lo) as in the float32 path.  g_rays_o = sum_s g_p, g_rays_d = sum_s g_p z.

Acceptance bar of a ray-gradient tensor, the construction of lowp_ref's criteria:
    error  = max |got - model64| / max |model64|
    bar    = MARGIN x max(figure, OUT_RTOL)
    figure = the float32 model against the float64 model on the same z_vals and the same forced features, computed by the
             test on the host - never taken from a kernel;  OUT_RTOL = 2e-5 (tests/test_oracle_golden.py).
Teacher forcing (Model.render's `feat`) is required: free-running, the float32 and the float64 model differ by 4.5e-4 - 3.8e-3
on about 1 % of the rays (a bf16 tie that flips at a feature moves that sample's whole contribution).
"""
import numpy as np
import torch

from oracle import eslam_oracle as orc
from tests import helpers as hp
from tests import lowp_ref as lr

POSE_FIXTURES = ("room0_200x40_tracking", "room0_200x32", "room0_200x40_zero15", "room0_200x40_trained_zero15")
PINNED_TO_REFERENCE = POSE_FIXTURES[:3]       # the trained fixture's depth-less rays' z differ from the reference's by more than
                                              # this gradient tolerates (4e-2): it is left out of the pin on the fixtures' own values


class ShortcutModel(lr.Model):
    """The mutant an unchanged float32 coord_bwd_kernel behind the mixed-precision backward would be: features (forward)
    from the half copies, their derivative with respect to the sample position from the float32 MASTERS."""

    def render(self, all_planes, params, beta, bound, rays_o, rays_d, z_vals, feat=None):
        dt = self.dtype
        bound = bound.to(dt)
        pts = rays_o[:, None, :] + rays_d[:, None, :] * z_vals[..., None]
        p_nor = orc.normalize_points(pts, bound)
        q = [[self.plane(p.detach()) for p in grp] for grp in all_planes]
        m = [[p.detach() for p in grp] for grp in all_planes]

        def feats(k):
            value = orc.plane_features(p_nor.detach(), q[k], q[k + 1], q[k + 2])
            through = orc.plane_features(p_nor, m[k], m[k + 1], m[k + 2])
            return value + (through - through.detach())          # the value of the copies, the position gradient of the masters

        u_s, u_c = feats(0), feats(3)
        given = (None, None) if feat is None else (feat[:, :64].to(dt), feat[:, 64:].to(dt))
        o_s, f_s = self.mlp(u_s, params, "", given[0])
        o_c, f_c = self.mlp(u_c, params, "c_", given[1])
        raw = torch.cat([torch.sigmoid(o_c), torch.tanh(o_s)], -1).reshape(*z_vals.shape, 4)
        depth, color = orc.composite(raw, z_vals, beta)
        return dict(depth=depth, color=color, sdf=raw[..., 3], raw_rgb=raw[..., :3], feat=torch.cat([f_s, f_c], -1).detach())


def ray_grads(model, fx, z_vals, feat=None, rows=None, loss_kind=None):
    """g_rays_o, g_rays_d [R,3] (float64 numpy) and the model's bf16 features [R*S,128] of a fixture through `model` on the given
    z_vals, with the fixture's loss - teacher-forced with `feat` exactly as lowp_ref.run_model does.  Planes, decoders and beta
    are constants here.  rows: a slice of the fixture's rays (z_vals and feat are those of the slice already): the loss is
    the loss of that batch.  loss_kind: "mapping" / "tracking" instead of the fixture's own."""
    dt = model.dtype
    rows = slice(None) if rows is None else rows
    sc, planes = hp.scene_and_planes(fx, dtype=torch.float32, channels_last=False)
    planes = tuple([p.to(dt) for p in grp] for grp in planes)
    params = hp.params_from(fx, dtype=dt)
    beta = float(fx["beta"])
    cv = lambda k: torch.from_numpy(fx[k][rows]).to(dt)
    ro, rd = cv("rays_o").requires_grad_(True), cv("rays_d").requires_grad_(True)
    z = torch.as_tensor(np.asarray(z_vals)).to(dt)
    r = model.render(planes, params, beta, sc.bound, ro, rd, z,
                     None if feat is None else torch.as_tensor(np.asarray(feat, dtype=np.float32)))
    loss_fn = orc.mapping_loss if (loss_kind or str(fx["loss_kind"])) == "mapping" else orc.tracking_loss
    loss = loss_fn(r["depth"], r["color"], r["sdf"], z, cv("gt_depth"), cv("gt_color"), float(fx["truncation"]))
    loss.backward()
    return ro.grad.double().numpy(), rd.grad.double().numpy(), r["feat"].float().numpy()


MARGIN = lr.MARGIN


def errors(got, ref):
    """(error of g_rays_o, error of g_rays_d): max |got - ref| / max |ref| per tensor.  got, ref: (g_o, g_d[, ...])."""
    return hp.rel_err(got[0], ref[0]), hp.rel_err(got[1], ref[1])


def bars(figure):
    from tests.test_oracle_golden import OUT_RTOL
    return tuple(MARGIN * max(f, OUT_RTOL) for f in figure)


def model_pair(fx, z_vals, feat, rows=None, loss_kind=None):
    """The float64 model's gradients, forced with `feat`, and the bars built from the float32 model on the same inputs:
    (ref64 = (g_o, g_d), f32 = (g_o, g_d), figure, bars)."""
    ref = ray_grads(lr.Model(), fx, z_vals, feat, rows, loss_kind)[:2]
    f32 = ray_grads(lr.Model(torch.float32), fx, z_vals, feat, rows, loss_kind)[:2]
    figure = errors(f32, ref)
    return ref, f32, figure, bars(figure)


def per_ray_excess(got, ref, f32):
    """The tensor-wide figure is the float32 model's WORST ray.  One sample with a hidden pre-activation within float32
    summation error of zero (helpers.ambiguous_samples) lands on the other side of its ReLU in one of two evaluations and moves
    its ray's gradient by 1e-4 - 1e-3 of the tensor's max - the float32 model against the float64 one does that at some batch
    sizes (torch's matmul changes its summation order with the row count) - and the tensor-wide bar then admits that much on
    EVERY ray.  So each ray is also held to its own bar, built the same way from the same two models:
        |got - model64| of the ray  <=  MARGIN x max(|float32 model - model64| of the ray, OUT_RTOL max |model64|).
    Never wider than the tensor-wide bar; on the rays without such a sample it is the OUT_RTOL floor.
    Returns per tensor (g_o, g_d) the largest error / bar over the rays (accepted: <= 1)."""
    from tests.test_oracle_golden import OUT_RTOL
    out = []
    for g, r, f in zip(got, ref, f32):
        g, r, f = (np.asarray(t, dtype=np.float64) for t in (g, r, f))
        scale = np.abs(r).max() + 1e-30
        bar = MARGIN * np.maximum(np.abs(f - r).max(-1), OUT_RTOL * scale)
        out.append(float((np.abs(g - r).max(-1) / bar).max()))
    return tuple(out)


def rejected(err, bar):
    """At least one of the two tensors is beyond its bar."""
    return err[0] > bar[0] or err[1] > bar[1]
