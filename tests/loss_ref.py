"""The fused mapping / tracking loss (reference src/Mapper.py:110-144,337-346; src/Tracker.py:114-148,197-204) in numpy: the
operation the six places that share myslam_amd/csrc/eslam_loss_final.h compute, written without torch and without library code.
Test infrastructure; tests/test_loss_ref.py pins it against the oracle under float64 autograd and against float32 torch.

loss_ref() classifies every sample in float32 with the thresholds the reference forms (torch casts the Python floats
`truncation` and `0.4 * truncation` to float32 and subtracts / adds them to the float32 depth), then does everything else in
`dtype` with pairwise sums.  border_batch() builds inputs that put samples one float32 step below, on and above each of the four
thresholds of the region rule, and the variants in which a set the loss takes a mean over is empty.
"""
import numpy as np

from myslam_amd import synth

# accumulator slots: the A_* enum of eslam_loss_final.h
A_N_FRONT, A_N_CENTER, A_N_TAIL, A_S_FRONT, A_S_CENTER, A_S_TAIL, A_N_DEPTH, A_S_DEPTH, A_S_COLOR, A_N_COLOR = range(10)
A_COUNT = 10
ACC = 16                                   # ESLAM_LOSS_ACC
COUNTS = (A_N_FRONT, A_N_CENTER, A_N_TAIL, A_N_DEPTH, A_N_COLOR)
SUMS = (A_S_FRONT, A_S_CENTER, A_S_TAIL, A_S_DEPTH, A_S_COLOR)
SLOT_NAMES = ("n_front", "n_center", "n_tail", "s_front", "s_center", "s_tail", "n_depth", "s_depth", "s_color", "n_color")
MAPPING_W5 = (5.0, 200.0, 10.0, 0.1, 5.0)          # {fs, center, tail, depth, color}, configs/ESLAM.yaml:53-57
TRACKING_W5 = (10.0, 200.0, 50.0, 1.0, 5.0)        # configs/ESLAM.yaml:29-33
FRONT, CENTER, TAIL, BACK = 0, 1, 2, 3


def thresholds(gt_depth, truncation):
    """float32 (d - t, d - 0.4 t, d + 0.4 t, d + t) per ray, formed as the reference forms them."""
    d = np.asarray(gt_depth, dtype=np.float32)
    t, t04 = np.float32(truncation), np.float32(0.4 * float(truncation))
    return d - t, d - t04, d + t04, d + t


def regions(z, gt_depth, truncation):
    """int8 [R,S]: 0 front, 1 centre, 2 tail, 3 back (no loss) of every sample, compared in float32 (all four strict)."""
    z = np.asarray(z, dtype=np.float32)
    lo, clo, chi, hi = (a[:, None] for a in thresholds(gt_depth, truncation))
    front, back = z < lo, z > hi
    center = (z > clo) & (z < chi)
    return np.where(front, FRONT, np.where(back, BACK, np.where(center, CENTER, TAIL))).astype(np.int8)


def pairwise_sum(x, dtype):
    """Sum of a 1-D array by halving, every partial sum held in `dtype`; 0 for an empty array."""
    x = np.asarray(x, dtype=dtype).reshape(-1)
    if x.size == 0:
        return dtype(0.0)
    while x.size > 1:
        if x.size & 1:
            x = np.concatenate([x, np.zeros(1, dtype)])
        x = x[0::2] + x[1::2]
    return dtype(x[0])


def members(gt_depth, ray_mask=None):
    """(mc, m): rays of the colour term (mask byte non-zero), and of the SDF and depth terms (those with gt_depth > 0 as well -
    zero, minus zero, negative and NaN depths are out)."""
    gd = np.asarray(gt_depth, dtype=np.float32)
    mc = np.ones(gd.shape, bool) if ray_mask is None else (np.asarray(ray_mask).astype(np.uint8) != 0)
    with np.errstate(invalid="ignore"):
        m = mc & (gd > 0)
    return mc, m


def value_from_acc(acc, weights5, dtype=np.float64):
    """The loss from the ten accumulators; 0/0 stays NaN, as torch.mean over an empty set."""
    a = np.asarray(acc, dtype=dtype)
    w = [dtype(v) for v in weights5]
    with np.errstate(invalid="ignore", divide="ignore"):
        return dtype(w[0] * (a[A_S_FRONT] / a[A_N_FRONT]) + w[1] * (a[A_S_CENTER] / a[A_N_CENTER]) + w[2] * (a[A_S_TAIL] / a[A_N_TAIL])
                     + w[4] * (a[A_S_COLOR] / a[A_N_COLOR]) + w[3] * (a[A_S_DEPTH] / a[A_N_DEPTH]))


def loss_ref(depth, rgb, sdf, z, gt_depth, gt_color, truncation, weights5, ray_mask=None, upstream=1.0, dtype=np.float64):
    """-> acc16 (A_* layout, `dtype`), loss, g_depth [R], g_rgb [R,3], g_sdf [R,S], region [R,S] (int8; -1 for the samples of
    rays outside the SDF terms).  Gradients are d (upstream * loss) / d (depth, rgb, sdf); a term whose set is empty makes the
    value NaN and leaves the gradients of the other terms finite, and rays outside a term get exactly 0."""
    dt = np.dtype(dtype).type
    reg = regions(z, gt_depth, truncation)
    mc, m = members(gt_depth, ray_mask)
    reg = np.where(m[:, None], reg, np.int8(-1)).astype(np.int8)
    depth, rgb, sdf, z, gd, gc = (np.asarray(a).astype(dt) for a in (depth, rgb, sdf, z, gt_depth, gt_color))
    t = dt(truncation)
    w_fs, w_center, w_tail, w_depth, w_color = (dt(v) for v in weights5)
    up = dt(upstream)
    with np.errstate(invalid="ignore"):
        e_front = sdf - dt(1.0)
        e_pred = (z + sdf * t) - gd[:, None]
        e_depth = gd - depth
    e_color = gc - rgb
    acc = np.zeros(ACC, dt)
    for slot_n, slot_s, e, sel in ((A_N_FRONT, A_S_FRONT, e_front, reg == FRONT), (A_N_CENTER, A_S_CENTER, e_pred, reg == CENTER),
                                   (A_N_TAIL, A_S_TAIL, e_pred, reg == TAIL), (A_N_DEPTH, A_S_DEPTH, e_depth, m),
                                   (A_N_COLOR, A_S_COLOR, e_color, np.repeat(mc[:, None], 3, 1))):
        acc[slot_n] = dt(int(sel.sum()))
        acc[slot_s] = pairwise_sum(e[sel] * e[sel], dt)
    loss = value_from_acc(acc, weights5, dt)
    two = dt(2.0)
    g_sdf = np.zeros(sdf.shape, dt)
    for code, n_slot, k, e in ((FRONT, A_N_FRONT, two * (w_fs * up), e_front), (CENTER, A_N_CENTER, two * (w_center * up) * t, e_pred),
                               (TAIL, A_N_TAIL, two * (w_tail * up) * t, e_pred)):
        sel = reg == code
        if sel.any():
            g_sdf[sel] = (k / acc[n_slot]) * e[sel]
    g_depth = np.zeros(depth.shape, dt)
    if m.any():
        g_depth[m] = -two * (w_depth * up) * e_depth[m] / acc[A_N_DEPTH]
    g_rgb = np.zeros(rgb.shape, dt)
    if mc.any():
        g_rgb[mc] = -two * (w_color * up) * e_color[mc] / acc[A_N_COLOR]
    return acc, loss, g_depth, g_rgb, g_sdf, reg


# ---- the border batch ------------------------------------------------------------------------------------------------------
# 0.15 in front of the five round depths: the one at which forming 0.4 t in float32 (0.4f * 0.1f, one ulp of 0.04 away from the
# cast double product) moves d - 0.4 t and d + 0.4 t; at the others the difference is rounded away (tests/test_loss_ref.py)
DEPTHS = (0.15, 0.3, 1.0, 2.0, 3.7, 9.9)
TRUNCATIONS = (0.06, 0.1)                   # the scenes', and a second one
VARIANTS = ("plain", "depthless_masked", "no_depth", "all_masked", "no_tail")
DEPTHLESS = (0.0, -0.0, -1.0, float("nan"))
N_BORDER = 12                               # three float32 values at each of the four thresholds


def border_values(d, truncation):
    """float32 [12]: nextafter(theta, -inf), theta, nextafter(theta, +inf) for theta = d - t, d - 0.4 t, d + 0.4 t, d + t."""
    out = []
    for th in thresholds(np.float32(d), truncation):
        th = np.float32(th)
        out += [np.nextafter(th, np.float32(-np.inf)), th, np.nextafter(th, np.float32(np.inf))]
    return np.asarray(out, dtype=np.float32)


def _fillers(d, truncation, u, first=0):
    """Samples well inside front / centre / lower tail / upper tail / back in turn, one per entry of u (uniform [0,1))."""
    d, t = np.float64(np.float32(d)), float(truncation)
    k = (np.arange(u.size) + first) % 5
    v = np.select([k == 0, k == 1, k == 2, k == 3],
                  [(d - t) * (0.1 + 0.8 * u), d + 0.3 * t * (2.0 * u - 1.0), d - t * (0.55 + 0.3 * u), d + t * (0.55 + 0.3 * u)],
                  d + t * (1.5 + 3.0 * u))
    return v.astype(np.float32)


def border_batch(R, S, truncation, variant="plain", stream=0):
    """dict of float32 arrays depth [R], rgb [R,3], sdf [R,S], z [R,S], gt_depth [R], gt_color [R,3] and ray_mask (uint8 [R] or
    None).  Ray i has depth DEPTHS[i % 6]; its row holds the twelve border values of that depth (a rotation of them, cut to S,
    when S < 12) and fillers well inside each region, sorted ascending, all positive.  stream: selects the hash streams of the
    fillers, sdf, depth and colours (another stream, another batch)."""
    assert variant in VARIANTS, variant
    base = 700_000 + 1_000 * int(stream)
    d_all = np.asarray([DEPTHS[i % len(DEPTHS)] for i in range(R)], dtype=np.float32)
    n_fill = max(S - N_BORDER, 0)
    u_fill = synth.hash_uniform((R, max(n_fill, 1)), base + 1).astype(np.float64)
    z = np.empty((R, S), np.float32)
    for i in range(R):
        row = np.roll(border_values(d_all[i], truncation), -((7 * i) % N_BORDER))
        row = np.concatenate([row, _fillers(d_all[i], truncation, u_fill[i, :n_fill], first=i)])[:S]
        if variant == "no_tail":             # the tail region left empty: its samples become centre samples
            tail = regions(row[None], d_all[i:i + 1], truncation)[0] == TAIL
            u = synth.hash_uniform((S,), base + 10 + i).astype(np.float64)
            row = np.where(tail, (np.float64(d_all[i]) + 0.3 * float(truncation) * (2.0 * u - 1.0)).astype(np.float32), row)
        z[i] = np.sort(row)
    assert (z > 0).all() and (np.diff(z, axis=1) >= 0).all()
    # sdf: the sign of z - d and a magnitude in [0.25, 0.95): |sdf - 1| >= 0.05 and |z + sdf t - d| >= 0.25 t >= 1e-2
    mag = np.float32(0.25) + np.float32(0.7) * synth.hash_uniform((R, S), base + 2)
    sdf = np.where(z < d_all[:, None], -mag, mag).astype(np.float32)
    off = np.float32(0.05) + np.float32(0.5) * synth.hash_uniform((R,), base + 3)
    depth = (d_all + np.where((np.arange(R) % 2 == 0) | (d_all < 0.5), off, -off * np.float32(0.5))).astype(np.float32)
    rgb, gt_color = synth.hash_uniform((R, 3), base + 4), synth.hash_uniform((R, 3), base + 5)
    gt_depth, mask = d_all.copy(), None
    if variant == "depthless_masked":
        mask = np.ones(R, np.uint8)
        for i in range(R):
            if i % 9 in (1, 3, 5, 7):
                gt_depth[i] = DEPTHLESS[(i % 9) // 2]
            if i % 9 in (2, 5):
                mask[i] = 0
        if R > 4:
            mask[R - 1] = 200                # any non-zero byte counts
    elif variant == "no_depth":
        gt_depth = np.asarray([DEPTHLESS[i % 4] for i in range(R)], dtype=np.float32)
    elif variant == "all_masked":
        mask = np.zeros(R, np.uint8)
    if variant == "no_tail":
        assert not (regions(z, gt_depth, truncation) == TAIL).any()
    return dict(depth=depth, rgb=rgb, sdf=sdf, z=z, gt_depth=gt_depth, gt_color=gt_color, ray_mask=mask)


def loss_ref_of(batch, truncation, weights5, upstream=1.0, dtype=np.float64, **override):
    """loss_ref on a border_batch dict; override: e.g. depth / rgb / sdf as a kernel produced them."""
    b = dict(batch, **override)
    return loss_ref(b["depth"], b["rgb"], b["sdf"], b["z"], b["gt_depth"], b["gt_color"], truncation, weights5, b["ray_mask"], upstream, dtype)


# ---- acceptance bars -----------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24
RTOL = 1e-4                                 # the project's parity tolerance: holds whatever the bars below allow


def rel(a, b):
    """|a - b| / |b|; 0 when both are 0."""
    a, b = float(a), float(b)
    return 0.0 if a == b else abs(a - b) / abs(b)


def max_rel(a, b):
    """Max-normalised difference of two arrays (tests/helpers.rel_err); 0 when both are all zero."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.abs(b).max(initial=0.0)
    e = np.abs(a - b).max(initial=0.0)
    return 0.0 if e == 0.0 else float(e / (s + 1e-30))


def sum_bar(gap32, workgroups):
    """Relative bar of a sum of non-negative terms formed by `workgroups` partial sums added in sequence: four times what the
    float32 evaluation of the reference differs from the float64 one by, plus one rounding per sequential add and sixteen for
    the tree inside a workgroup - never more than RTOL."""
    return min(RTOL, 4.0 * gap32 + (workgroups + 16) * EPS32)


def grad_bar(gap32):
    return min(RTOL, 4.0 * gap32 + 8.0 * EPS32)
