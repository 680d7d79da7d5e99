"""Float64 numpy restatement of ONE plane's gradient scatter, done the two ways the render backward can do it.

A decoder's first layer is Linear(64 -> 16) and the features feed nothing else, so the gradient of a sample's 32 features of one
plane level is  g_feat = g_z1 @ W  with g_z1 the 16-wide gradient at the first hidden layer's pre-activation and W the
level's [16, 32] slice of W1.  The bilinear scatter is linear, so a texel's sum over samples can be formed in the 16-wide space
and expanded once:

    expand_then_scatter     per sample: 32 values, bilinear scatter-add                       (the full-width path)
    accumulate_then_expand  per cell: four 16-wide sums (corner x, corner y), expanded once   (the rank-16 path)

`walk_wave` is the second way with the kernel's own lane bookkeeping (scatter_sort_kernel with GZ): 64 lanes, one accumulator
each, records sorted by cell along the minor axis, the carried column of a minor-axis neighbour, the lower-half-only flush.
"""
import numpy as np

HID = 16       # hidden width = rank of the feature gradient
CH = 32        # channels of a plane


def axis_coord(u, n):
    """grid_sample(align_corners=True, padding_mode='border') for one axis: (i0, i1, t)."""
    x = np.clip((np.asarray(u, np.float64) + 1.0) * 0.5 * (n - 1), 0.0, float(n - 1))
    i0 = np.floor(x).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, x - i0


def corner_weights(tx, ty):
    """[n, 2 (corner x), 2 (corner y)]: the record's four weights, indexed 2 * hx + row in the kernel."""
    wx = np.stack([1.0 - tx, tx], 1)
    wy = np.stack([1.0 - ty, ty], 1)
    return wx[:, :, None] * wy[:, None, :]


def expand_then_scatter(gz, W, u, v, h, w):
    """grad [h, w, 32]: every sample's 16 -> 32 expansion first, then its four bilinear contributions."""
    x0, x1, tx = axis_coord(u, w)
    y0, y1, ty = axis_coord(v, h)
    gf = np.asarray(gz, np.float64) @ np.asarray(W, np.float64)
    wt = corner_weights(tx, ty)
    grad = np.zeros((h, w, CH))
    for hx, xs in enumerate((x0, x1)):
        for row, ys in enumerate((y0, y1)):
            np.add.at(grad, (ys, xs), wt[:, hx, row, None] * gf)
    return grad


def accumulate_then_expand(gz, W, u, v, h, w):
    """grad [h, w, 32]: per bilinear cell (x0, y0) four 16-wide sums, one expansion per cell."""
    x0, x1, tx = axis_coord(u, w)
    y0, y1, ty = axis_coord(v, h)
    wt = corner_weights(tx, ty)
    gz = np.asarray(gz, np.float64)
    W = np.asarray(W, np.float64)
    cell = y0 * w + x0
    grad = np.zeros((h, w, CH))
    for cid in np.unique(cell):
        m = cell == cid
        A = np.einsum("nxr,nj->xrj", wt[m], gz[m])           # [hx, row, j]
        out = A @ W                                          # [hx, row, c]
        cy, cx = divmod(int(cid), w)
        for hx in range(2):
            for row in range(2):
                grad[min(cy + row, h - 1), min(cx + hx, w - 1)] += out[hx, row]
    return grad


# ---- lane bookkeeping of the rank-16 walk ----------------------------------------------------------------------------------
def walk_lane(lane):
    """Accumulating role: lane -> (hx, row, j)."""
    return lane >> 5, (lane >> 4) & 1, lane & 15


def flush_lane(lane):
    """Flushing role: lane -> (hx, c); the lane issues the atomics of rows 0 and 1."""
    return lane >> 5, lane & 31


def source_lane(hx, row, j):
    return (hx << 5) | (row << 4) | j


def expand_wave(acc, W):
    """acc [64] in the accumulating role -> out [64, 2]: lane (hx, c) gets sum_j W[j, c] * A[hx][row][j] for row 0 and 1."""
    out = np.zeros((64, 2))
    for lane in range(64):
        hx, c = flush_lane(lane)
        for row in range(2):
            out[lane, row] = sum(W[j, c] * acc[source_lane(hx, row, j)] for j in range(HID))
    return out


def carry_column(acc):
    """A minor-axis neighbour follows: its first texel column is the finished cell's second one - the upper half-wave's sums
    move to the lower half, the upper half starts from zero."""
    return np.concatenate([acc[32:], np.zeros(32)])


def walk_wave(gz, W, u, v, h, w):
    """The kernel's walk of one plane with x as the minor axis: records sorted by cell, one accumulator per lane."""
    x0, x1, tx = axis_coord(u, w)
    y0, y1, ty = axis_coord(v, h)
    wt = corner_weights(tx, ty).reshape(-1, 4)               # [n, 2 hx + row]
    gz = np.asarray(gz, np.float64)
    W = np.asarray(W, np.float64)
    order = np.argsort(y0 * (w + 1) + x0, kind="stable")
    grad = np.zeros((h, w, CH))
    lanes = np.arange(64)
    l_hx, l_row, l_j = walk_lane(lanes)

    def flush(cur, acc, lower_half_only):
        if cur is None:
            return
        cx, cy, step_m, step_M = cur
        out = expand_wave(acc, W)
        for lane in range(32 if lower_half_only else 64):
            hx, c = flush_lane(lane)
            xx = cx + (step_m & hx)
            grad[cy, xx, c] += out[lane, 0]
            grad[cy + step_M, xx, c] += out[lane, 1]

    cur, acc = None, np.zeros(64)
    for e in order:
        rec = (int(x0[e]), int(y0[e]), int(x1[e] > x0[e]), int(y1[e] > y0[e]))
        if cur is None or rec[:2] != cur[:2]:
            adjacent = cur is not None and cur[2] == 1 and rec[1] == cur[1] and rec[0] == cur[0] + 1
            if adjacent:
                flush(cur, acc, True)
                acc = carry_column(acc)
            else:
                flush(cur, acc, False)
                acc = np.zeros(64)
            cur = rec
        acc = acc + wt[e, 2 * l_hx + l_row] * gz[e, l_j]
    flush(cur, acc, False)
    return grad
