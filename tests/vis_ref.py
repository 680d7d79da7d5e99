"""numpy models of the render metrics and the visualiser's panel (csrc/eslam_vis.hip; include/eslam_hip.h eslam_frame_stats,
eslam_ssim, eslam_vis_panel), written from the header's definitions:

  ssim64        the float64 SSIM map and mean: the definition itself.  Its keyword arguments are the MUTATIONS the acceptance
                criterion has to reject (another sigma, no clipping, sample covariance, C2 = C1); shift_window is one more
  ssim32        float32 in the kernel's documented operation order, tile by tile with the per-tile constants
  panel32       the float32 panel model (bit for bit); unmasked_residual / round_index are its two mutations
  stats64       the four sums of eslam_frame_stats, through math.fsum

and the input set, the shapes and the acceptance criterion the GPU tests use (ssim_inputs, ssim_shapes, ssim_tolerance,
ssim_accepts).  The tolerance is not a chosen number: it is 4 x the worst deviation of the float32 model from the float64
model over exactly the cases the GPU test runs (the kernel follows the float32 model's operation order; tile order and
the reduction differ by rounding only).  profiles/vis_margins.txt records it next to the mutations' deviations
(tools/vis_margins.py writes that file from margins())."""
import functools
import math

import numpy as np

WIN = 11
C1, C2 = 1e-4, 9e-4
INPUT_KINDS = ("uniform_noise", "smooth_2pc_noise", "flat_0.7_1e-3_noise", "outside_0_1", "itself")
CHANNELS = (1, 3)
TOL_FACTOR = 4.0


def window(sigma=1.5):
    """The 11 weights: normalised in float64, rounded to float32."""
    k = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def _as3(a):
    a = np.asarray(a)
    return a[:, :, None] if a.ndim == 2 else a


def _filter2(v, w):
    """Separable valid filter of [H,W,C] with the 1D window w: rows (along W) first, then columns."""
    Ho, Wo = v.shape[0] - WIN + 1, v.shape[1] - WIN + 1
    h = w[0] * v[:, 0:Wo]
    for k in range(1, WIN):
        h = h + w[k] * v[:, k:k + Wo]
    m = w[0] * h[0:Ho]
    for k in range(1, WIN):
        m = m + w[k] * h[k:k + Ho]
    return m


def ssim64(a, b, sigma=1.5, clip=True, sample_covariance=False, c2=C2, shift_window=0):
    """(map [H-10,W-10,C] float64, mean) of the definition.  The defaults are the definition; anything else is a mutation.
    shift_window: the windows moved by that many pixels along W (the images rolled, so the shape stays)."""
    a, b = _as3(a).astype(np.float64), _as3(b).astype(np.float64)
    if shift_window:
        a, b = np.roll(a, -shift_window, axis=1), np.roll(b, -shift_window, axis=1)
    if clip:
        a, b = np.clip(a, 0.0, 1.0), np.clip(b, 0.0, 1.0)
    w = window(sigma).astype(np.float64)
    ux, uy = _filter2(a, w), _filter2(b, w)
    vx = _filter2(a * a, w) - ux * ux
    vy = _filter2(b * b, w) - uy * uy
    vxy = _filter2(a * b, w) - ux * uy
    if sample_covariance:
        n = WIN * WIN
        vx, vy, vxy = vx * (n / (n - 1.0)), vy * (n / (n - 1.0)), vxy * (n / (n - 1.0))
    s = ((2.0 * ux * uy + C1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + C1) * (vx + vy + c2))
    return s, float(s.mean())


def ssim32(a, b, tile_h, tile_w):
    """(map float32, mean float64) in the kernel's operation order (header, eslam_ssim): per tile and channel the clipped
    values are shifted by the tile's first pixel, every window sum runs k = 0 .. 10 as acc = w[0] v[0], acc = acc + w[k] v[k]
    in float32 with no fused operation; the mean is the float64 mean of the float32 map."""
    f = np.float32
    a, b = _as3(a).astype(f), _as3(b).astype(f)
    H, W, C = a.shape
    Ho, Wo = H - WIN + 1, W - WIN + 1
    w = window()
    a, b = np.clip(a, f(0), f(1)), np.clip(b, f(0), f(1))
    out = np.empty((Ho, Wo, C), dtype=f)
    c1, c2, two = f(C1), f(C2), f(2)
    for y0 in range(0, Ho, tile_h):
        th = min(tile_h, Ho - y0)
        for x0 in range(0, Wo, tile_w):
            tw = min(tile_w, Wo - x0)
            pa, pb = a[y0:y0 + th + WIN - 1, x0:x0 + tw + WIN - 1], b[y0:y0 + th + WIN - 1, x0:x0 + tw + WIN - 1]
            kx, ky = pa[0:1, 0:1], pb[0:1, 0:1]                          # [1,1,C]: per channel
            x, y = pa - kx, pb - ky
            m_x, m_y = _filter2(x, w), _filter2(y, w)
            m_xx, m_yy, m_xy = _filter2(x * x, w), _filter2(y * y, w), _filter2(x * y, w)
            vx, vy, vxy = m_xx - m_x * m_x, m_yy - m_y * m_y, m_xy - m_x * m_y
            ux, uy = kx + m_x, ky + m_y
            num = (two * (ux * uy) + c1) * (two * vxy + c2)
            den = (ux * ux + uy * uy + c1) * (vx + vy + c2)
            s = num / den
            assert s.dtype == f
            out[y0:y0 + th, x0:x0 + tw] = s
    return out, float(out.astype(np.float64).mean())


# ---- the panel ---------------------------------------------------------------------------------------------------------
def plasma_index(v, vmax, round_index=False):
    """LUT index of float32 values v: t = v / vmax (float32); 0 for t <= 0 or NaN, else min(255, int(t 256))."""
    f = np.float32
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = np.asarray(v, dtype=f) / f(vmax)
        idx = np.zeros(t.shape, dtype=np.int64)
        pos = t > 0                                                       # (False for NaN)
        s = np.minimum(t[pos], f(1)) * f(256)
        idx[pos] = np.minimum(255, np.rint(s).astype(np.int64) if round_index else s.astype(np.int64))
    return idx


def panel32(depth, color, gt_depth, gt_color, lut, unmasked_residual=False, round_index=False):
    """uint8 [2H,3W,3]: eslam_vis_panel operation by operation in float32."""
    f = np.float32
    depth, gt_depth = np.asarray(depth, dtype=f), np.asarray(gt_depth, dtype=f)
    color, gt_color = np.asarray(color, dtype=f), np.asarray(gt_color, dtype=f)
    H, W = gt_depth.shape
    vmax = f(gt_depth.max())
    if vmax == 0:
        vmax = f(1)
    hole = gt_depth == 0
    with np.errstate(invalid="ignore"):
        d_res = np.abs(gt_depth - depth)
        c_res = np.abs(gt_color - color)
    if not unmasked_residual:
        d_res[hole] = 0
        c_res[hole] = 0
    out = np.empty((2 * H, 3 * W, 3), dtype=np.uint8)
    for k, v in enumerate((gt_depth, depth, d_res)):
        out[:H, k * W:(k + 1) * W] = lut[plasma_index(v, vmax, round_index)]
    for k, v in enumerate((gt_color, color, c_res)):
        c = np.clip(v, f(0), f(1))
        out[H:, k * W:(k + 1) * W] = (c * f(255) + f(0.5)).astype(np.uint8)
    return out


# ---- the stats -----------------------------------------------------------------------------------------------------------
def stats64(depth, color, gt_depth, gt_color):
    """[n_valid, sum |depth - gt_depth| over gt_depth > 0, sum (color - gt_color)^2, max gt_depth]: the differences in float32,
    widened to double, summed exactly (math.fsum)."""
    f = np.float32
    depth, gt_depth = np.asarray(depth, dtype=f), np.asarray(gt_depth, dtype=f)
    color, gt_color = np.asarray(color, dtype=f), np.asarray(gt_color, dtype=f)
    valid = gt_depth > 0
    d = np.abs(depth[valid] - gt_depth[valid]).astype(np.float64)
    c = (color - gt_color).astype(np.float64).reshape(-1)
    return [float(valid.sum()), math.fsum(d), math.fsum(c * c), float(gt_depth.max())]


# ---- the GPU test's cases and its acceptance criterion -------------------------------------------------------------------
def ssim_shapes(tile_h, tile_w):
    """(H, W): one output pixel; one row of one tile; a row and a column more; exactly one tile; one row more than a tile and
    one column short of two tiles and a half; an odd size of several tiles."""
    return [(11, 11), (11, tile_w + 10), (12, tile_w + 11), (tile_h + 10, tile_w + 10), (tile_h + 11, 2 * tile_w + 9), (37, 45)]


def ssim_inputs(H, W, C, seed=0):
    """[(kind, a, b)] float32 [H,W,C], the five kinds of INPUT_KINDS.  "2 % noise" and "1e-3 noise" are Gaussian with that
    standard deviation, drawn independently for a and b: with variances of 4e-4 against C2 = 9e-4 and no correlation, the
    SSIM is where a wrong variance estimate (sample covariance, another C2) moves it most."""
    rng = np.random.default_rng(1000 * seed + 100 * C + 7 * H + W)
    f = np.float32
    yy, xx, cc = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    smooth = 0.5 + 0.3 * np.sin(xx / 9.0 + cc) * np.cos(yy / 7.0)
    noise = lambda s: rng.normal(0.0, s, (H, W, C))
    u = rng.uniform(0.0, 1.0, (H, W, C))
    wide = rng.uniform(-0.5, 1.5, (H, W, C))
    own = rng.uniform(0.0, 1.0, (H, W, C)).astype(f)
    return [("uniform_noise", u.astype(f), rng.uniform(0.0, 1.0, (H, W, C)).astype(f)),
            ("smooth_2pc_noise", (smooth + noise(0.02)).astype(f), (smooth + noise(0.02)).astype(f)),
            ("flat_0.7_1e-3_noise", (0.7 + noise(1e-3)).astype(f), (0.7 + noise(1e-3)).astype(f)),
            ("outside_0_1", wide.astype(f), (wide + noise(0.1)).astype(f)),
            ("itself", own, own.copy())]


def ssim_cases(tile_h, tile_w):
    """Every case of the GPU test: (H, W, C, kind, a, b)."""
    for H, W in ssim_shapes(tile_h, tile_w):
        for C in CHANNELS:
            for kind, a, b in ssim_inputs(H, W, C):
                yield H, W, C, kind, a, b


def deviation(got_map, got_mean, want_map, want_mean):
    """The larger of the worst map deviation and the mean's deviation."""
    return max(float(np.abs(np.asarray(got_map, dtype=np.float64).reshape(want_map.shape) - want_map).max()),
               abs(float(got_mean) - want_mean))


@functools.lru_cache(maxsize=None)
def model_error(tile_h, tile_w):
    """The float32 model's worst deviation from the float64 model over ssim_cases."""
    worst = 0.0
    for H, W, C, kind, a, b in ssim_cases(tile_h, tile_w):
        worst = max(worst, deviation(*ssim32(a, b, tile_h, tile_w), *ssim64(a, b)))
    return worst


def ssim_tolerance(tile_h, tile_w):
    return TOL_FACTOR * model_error(tile_h, tile_w)


def ssim_accepts(candidate, tile_h, tile_w):
    """The acceptance criterion: candidate(a, b) -> (map, mean) is within ssim_tolerance of the float64 model, map and mean, on
    every case.  Returns (accepted, worst deviation)."""
    tol = ssim_tolerance(tile_h, tile_w)
    worst = 0.0
    for H, W, C, kind, a, b in ssim_cases(tile_h, tile_w):
        worst = max(worst, deviation(*candidate(a, b), *ssim64(a, b)))
    return worst <= tol, worst


SSIM_MUTATIONS = {
    "window shifted by one pixel": dict(shift_window=1),
    "sigma = 1.4": dict(sigma=1.4),
    "no clipping": dict(clip=False),
    "sample covariance": dict(sample_covariance=True),
    "C2 = C1": dict(c2=C1),
}


def panel_cases(seed=0):
    """[(name, depth, color, gt_depth, gt_color)] float32 at 5 x 7 and 37 x 45: zeros in gt_depth (with a rendered depth and
    colours that differ there), a NaN in the rendered depth, colours outside [0, 1], depths beyond vmax; and vmax == 0."""
    f = np.float32
    out = []
    for H, W in ((5, 7), (37, 45)):
        rng = np.random.default_rng(seed + H)
        gd = rng.uniform(0.5, 4.0, (H, W)).astype(f)
        gd[rng.uniform(size=(H, W)) < 0.2] = 0
        gd[0, 0] = 0
        d = (gd + rng.normal(0, 0.3, (H, W))).astype(f)
        d[gd == 0] = rng.uniform(0.5, 5.0, int((gd == 0).sum())).astype(f)   # rendered depth where there is no ground truth
        d[H // 2, W // 2] = np.nan
        d[H - 1, W - 1] = -0.25
        d[H - 1, 0] = 1e30
        gc = rng.uniform(0, 1, (H, W, 3)).astype(f)
        c = (gc + rng.normal(0, 0.4, (H, W, 3))).astype(f)                   # many values outside [0, 1]
        gc[1, 1] = (-0.5, 1.5, 0.5)
        out.append((f"{H}x{W}", d, c, gd, gc))
        out.append((f"{H}x{W}_vmax0", d, c, np.zeros((H, W), dtype=f), gc))
    return out


def margins(tile_h, tile_w, lut):
    """The numbers of profiles/vis_margins.txt."""
    err = model_error(tile_h, tile_w)
    rows = {}
    for name, kw in SSIM_MUTATIONS.items():
        rows[name] = ssim_accepts(lambda a, b: ssim64(a, b, **kw), tile_h, tile_w)[1]
    panel = {}
    for name, kw in (("a residual that is not masked", dict(unmasked_residual=True)),
                     ("a LUT index rounded instead of floored", dict(round_index=True))):
        panel[name] = sum(int((panel32(*case[1:], lut, **kw) != panel32(*case[1:], lut)).sum()) for case in panel_cases())
    return dict(model_error=err, tolerance=TOL_FACTOR * err, ssim_mutations=rows, panel_mutations=panel)
