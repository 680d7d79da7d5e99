"""Model and acceptance criteria for the fused SDF gradient (eslam_sdf_grad, ops.sdf_gradient) and for the viewer's vertex
shading (eslam_shade_vertices).  Test-only, CPU code.

Model: autograd of oracle.decode(p, planes, params, bound)[:, 3].sum() with respect to p - what
tests/test_gpu_parity.py::test_decoders_forward_and_backward trusts for point gradients - in float64 (the reference value) and
in float32 (the reference's own arithmetic: how far a correct float32 evaluation sits from the float64 one).

Criteria (the GPU test applies them to the kernel, tests/test_sdf_normals_ref.py to the float32 model and to three mutants):
  gradient   helpers.rel_err(grad, grad64) <= GRAD_RTOL; exactly 0.0 at every component whose coordinate lies on or outside
             the bound (clamped_components); rows that are zero in the model are zero.
  normals    length within UNIT_TOL of 1 where non-zero; per row within MARGIN x max(that row's float32-model-vs-float64
             difference, NORMAL_FLOOR) of the float64 unit normal (the construction of lowp_pose_ref.per_ray_excess).
"""
import contextlib

import numpy as np
import torch

from tests import helpers as hp

GRAD_RTOL = 1e-4          # the project's bar (helpers.rel_err)
UNIT_TOL = 1e-6
MARGIN = 4.0
NORMAL_FLOOR = 2e-5
MUTANTS = ("no_border_gate", "no_tanh_factor", "no_relu2_mask")


def fixture_model(scene=None, channels_last=False):
    """(points float32 [2000,3], planes(dtype, device, channels_last) -> all_planes, params(dtype), scene) of the committed
    fixture decoders_room0_points: 2000 points with a 10 % margin outside the bound on every side, the two exact corners, the
    reference's decoder weights; planes from scene.synth_planes (of `scene`, default room0)."""
    from myslam_amd import scene as scn
    fx = hp.load("decoders_room0_points")
    sc = scn.make_scene("room0") if scene is None else scene
    pts = torch.from_numpy(fx["points"]).float().reshape(-1, 3)

    def planes(dtype=torch.float32, device="cpu", channels_last=channels_last):
        return scn.synth_planes(sc, device=device, dtype=dtype, channels_last=channels_last)

    def params(dtype=torch.float32):
        return hp.params_from(fx, dtype=dtype)

    return pts, planes, params, sc


@contextlib.contextmanager
def _mutated(name):
    from oracle import eslam_oracle as orc
    saved = (orc._unnormalize_clip, orc._mlp)
    try:
        if name == "no_border_gate":          # the clamp passes gradient everywhere
            def clip(coord, size):
                x = ((coord + 1) / 2) * (size - 1)
                return x + (x.detach().clamp(0, size - 1) - x.detach())
            orc._unnormalize_clip = clip
        elif name == "no_relu2_mask":         # the second hidden layer's ReLU passes gradient everywhere
            def mlp(feat, params, prefix):
                c = "c_" if prefix == "rgb" else ""
                h = torch.relu(feat @ params[f"{c}linears.0.weight"].t() + params[f"{c}linears.0.bias"])
                a = h @ params[f"{c}linears.1.weight"].t() + params[f"{c}linears.1.bias"]
                h = a + (torch.relu(a) - a).detach()
                return h @ params[f"{c}output_linear.weight"].t() + params[f"{c}output_linear.bias"]
            orc._mlp = mlp
        yield
    finally:
        orc._unnormalize_clip, orc._mlp = saved


def model(points, planes, params, bound, dtype=torch.float64, mutant=None):
    """(sdf [N], grad [N,3]) numpy arrays of `dtype`: oracle.decode's sdf and its autograd gradient w.r.t. the points."""
    from oracle import eslam_oracle as orc
    assert mutant is None or mutant in MUTANTS
    p = points.detach().cpu().to(dtype).reshape(-1, 3).clone().requires_grad_(True)
    with _mutated(mutant):
        sdf = orc.decode(p, planes, params, bound.to(dtype))[:, 3]
        sdf.sum().backward()
    s, g = sdf.detach().numpy(), p.grad.numpy()
    if mutant == "no_tanh_factor":
        g = g / (1.0 - s * s)[:, None]
    return s, g


def clamped_components(points, bound):
    """bool [N,3]: coordinate components on or outside the bound (the border clamp is active: zero gradient)."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    b = np.asarray(bound, dtype=np.float32)
    return (p <= b[None, :, 0]) | (p >= b[None, :, 1])


def unit_rows(g):
    """float64 [N,3]: rows divided by their length, zero rows kept zero."""
    g = np.asarray(g, dtype=np.float64)
    n = np.sqrt((g * g).sum(-1, keepdims=True))
    return np.where(n > 0, g / np.where(n > 0, n, 1.0), 0.0)


def gradient_figures(grad, grad64, clamped):
    """dict: rel_err against the float64 model, the number of clamped components that are not exactly 0.0, the number of the
    model's zero rows that are not zero."""
    g = np.asarray(grad)
    zero_rows = ~np.asarray(grad64).any(-1)
    return {"rel_err": hp.rel_err(g, grad64), "clamped_nonzero": int((g[clamped] != 0.0).sum()),
            "zero_rows_nonzero": int(g[zero_rows].any(-1).sum())}


def gradient_ok(fig):
    return fig["rel_err"] <= GRAD_RTOL and fig["clamped_nonzero"] == 0 and fig["zero_rows_nonzero"] == 0


def normal_figures(unit, grad64, grad32):
    """dict: the largest | |n| - 1 | over the non-zero rows; the largest error / bar over the rows, the bar rebuilt per row
    from the two CPU models; rows that are zero in the model but not here."""
    u = np.asarray(unit, dtype=np.float64)
    r, f = unit_rows(grad64), unit_rows(grad32)
    nz = u.any(-1)
    length = np.abs(np.sqrt((u[nz] ** 2).sum(-1)) - 1.0).max() if nz.any() else 0.0
    bar = MARGIN * np.maximum(np.abs(f - r).max(-1), NORMAL_FLOOR)
    return {"length": float(length), "excess": float((np.abs(u - r).max(-1) / bar).max()),
            "zero_rows_nonzero": int(u[~r.any(-1)].any(-1).sum()), "nan": int(np.isnan(u).sum())}


def normals_ok(fig):
    return fig["length"] <= UNIT_TOL and fig["excess"] <= 1.0 and fig["zero_rows_nonzero"] == 0 and fig["nan"] == 0


# ----------------------------------------------------------------------------------------------
# vertex shading (include/eslam_hip.h, eslam_shade_vertices), float64
# ----------------------------------------------------------------------------------------------
def shade(verts, normals, colors, cam_center, ambient):
    """float64 [V,3]: c k before rounding, k = ambient + (1 - ambient) max(0, n^ . l^), l = c - v, k = 1 when n or l has zero
    length; colors uint8 [V,3|4] or None = 200 grey."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    n = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    l = np.asarray(cam_center, dtype=np.float64)[None] - v
    nn, ll = np.sqrt((n * n).sum(-1)), np.sqrt((l * l).sum(-1))
    ok = (nn > 0) & (ll > 0)
    cos = (n * l).sum(-1) / np.where(ok, nn * ll, 1.0)
    k = np.where(ok, ambient + (1.0 - ambient) * np.maximum(0.0, cos), 1.0)
    c = np.full((v.shape[0], 3), 200.0) if colors is None else np.asarray(colors)[:, :3].astype(np.float64)
    return c * k[:, None]


def shade_u8(verts, normals, colors, cam_center, ambient):
    """uint8 [V,4]: (uint8)floor(min(255, c k) + 0.5), alpha 255."""
    c = np.floor(np.minimum(255.0, shade(verts, normals, colors, cam_center, ambient)) + 0.5).astype(np.uint8)
    return np.concatenate([c, np.full((c.shape[0], 1), 255, np.uint8)], 1)


# ----------------------------------------------------------------------------------------------
# PLY
# ----------------------------------------------------------------------------------------------
def parent_write_ply(path, vertices, faces, colors=None):
    """Mesher.write_ply as it was before normals (its signature and bytes)."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}",
            "property float x", "property float y", "property float z"]
    vfields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colors is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
        vfields += [("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")]
    head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    vrec = np.empty(v.shape[0], dtype=vfields)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        c = np.clip(np.round(255.0 * np.asarray(colors, dtype=np.float64)), 0, 255).astype(np.uint8).reshape(-1, 3)
        vrec["red"], vrec["green"], vrec["blue"] = c[:, 0], c[:, 1], c[:, 2]
        vrec["alpha"] = 255
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"] = 3
    frec["v"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())
