"""Float64 numpy restatement of the rank-16 scatter's walk that takes FOUR sorted entries per step (scatter_sort_kernel with GZ).

tests/rank16_ref.py states what the rank-16 path computes (accumulate_then_expand) and the one-entry-per-step bookkeeping.  Here the
64 lanes of a wave are (slot s = lane >> 4, j = lane & 15): step t of a wave's list handles entries 4 t .. 4 t + 3, slot s takes
entry 4 t + s and adds  g_z1[entry][j] * w[entry][k]  to its four sums k = 2 hx + row.  A cell's sum is therefore held as four
partial sums, one per slot, and the flush adds them (a transposing exchange over lane bits 4 and 5 that leaves lane (s, j) with
the total of k = s: the layout the expansion by W1 reads).  A step none of whose four entries starts a new cell does nothing else.
A step with a fresh entry takes its entries one after the other: a fresh entry closes the cell in front of it - flush, then zero,
or, when the new cell is the next one along the minor axis, every lane keeps ITS OWN partial sums of the shared texel column
(k = 2, 3 -> k = 0, 1) - and entry kk is then added in slot kk's lanes only.

`walk_quad` is that walk for one plane with x as the minor axis; `cases` reports, for a sorted list of cells alone, which of the
(position of the fresh entry in its step 0..3) x (adjacent / not) cases occur and whether a cell spans a 64-entry block or a wave
boundary: what a test's inputs must reach.  `kernel_cells` forms the sorted cell list of one bundle and plane the way the kernel
does (float32 coordinates, bounding box, minor axis = the longer side of the box).
"""
import numpy as np

from tests import rank16_ref as r16

SLOTS = 4
BLOCK = 64         # entries per record block (one per lane)


def slot_lane(s, j):
    return (s << 4) | j


def slot_sum(acc):
    """acc [4 slots, 4 k, 16 j] -> [64]: lane (s, j) ends with the sum over the slots of k = s, by the kernel's two exchanges."""
    out = np.zeros(64)
    r = np.zeros((SLOTS, 2, r16.HID))                              # after the exchange over lane bit 4: k = (s & 1), 2 + (s & 1)
    for s in range(SLOTS):
        b = s & 1
        r[s, 0] = acc[s, b] + acc[s ^ 1, b]
        r[s, 1] = acc[s, 2 + b] + acc[s ^ 1, 2 + b]
    for s in range(SLOTS):
        hi = s >> 1
        out[slot_lane(s, 0):slot_lane(s, 0) + r16.HID] = r[s, hi] + r[s ^ 2, hi]      # k = 2 (s >> 1) + (s & 1) = s
    return out


def carry_column(acc):
    """Minor-axis neighbour follows: per slot, the sums of corner x = 1 become those of corner x = 0; no exchange between slots."""
    nxt = np.zeros_like(acc)
    nxt[:, 0:2] = acc[:, 2:4]
    return nxt


def walk_quad(gz, W, u, v, h, w, chunk=256):
    """One plane, x the minor axis: the sorted list is cut into waves of `chunk` entries (each walks its own, as in the kernel:
    a cell that spans two waves is flushed by both), padded to a multiple of four with zero-weight entries of no cell."""
    x0, x1, tx = r16.axis_coord(u, w)
    y0, y1, ty = r16.axis_coord(v, h)
    wt = r16.corner_weights(tx, ty).reshape(-1, 4)                 # [n, k = 2 hx + row]
    gz = np.asarray(gz, np.float64)
    W = np.asarray(W, np.float64)
    order = np.argsort(y0 * (w + 1) + x0, kind="stable")
    grad = np.zeros((h, w, r16.CH))

    def flush(cur, acc, lower_half_only):
        if cur is None:
            return
        cx, cy, step_m, step_M = cur
        out = r16.expand_wave(slot_sum(acc), W)                    # lane (hx, c): rows 0 and 1
        for lane in range(32 if lower_half_only else 64):
            hx, c = r16.flush_lane(lane)
            xx = cx + (step_m & hx)
            grad[cy, xx, c] += out[lane, 0]
            grad[cy + step_M, xx, c] += out[lane, 1]

    for w0 in range(0, len(order), chunk):
        ent = list(order[w0:w0 + chunk])
        ent += [None] * (-len(ent) % SLOTS)
        cur, acc = None, np.zeros((SLOTS, 4, r16.HID))
        for t0 in range(0, len(ent), SLOTS):
            step = ent[t0:t0 + SLOTS]
            recs = [None if e is None else (int(x0[e]), int(y0[e]), int(x1[e] > x0[e]), int(y1[e] > y0[e])) for e in step]
            prev, fresh = cur, []
            for rec in recs:
                fresh.append((rec is None) != (prev is None) or (rec is not None and rec[:2] != prev[:2]))
                prev = rec
            if not any(fresh):                                     # the fast step: every slot adds its entry, nothing else
                for s, e in enumerate(step):
                    if e is not None:
                        acc[s] += wt[e][:, None] * gz[e][None, :]
                continue
            for kk, (e, rec) in enumerate(zip(step, recs)):
                if fresh[kk]:
                    adjacent = (cur is not None and rec is not None and cur[2] == 1 and rec[1] == cur[1] and rec[0] == cur[0] + 1)
                    flush(cur, acc, adjacent)
                    acc = carry_column(acc) if adjacent else np.zeros_like(acc)
                    cur = rec
                if e is not None:
                    acc[kk] += wt[e][:, None] * gz[e][None, :]
        flush(cur, acc, False)
    return grad


# ---- which cases a sorted list exercises ---------------------------------------------------------------------------------------
ALL_CASES = frozenset((pos, adj) for pos in range(SLOTS) for adj in (False, True))


def cases(minor, major, step_m, chunk):
    """minor / major / step_m: the SORTED list's cell coordinates and minor-axis step flags (valid entries only; the kernel's
    padding follows them).  Returns (set of (position of a fresh entry in its step, adjacent) over the fresh entries that close a
    cell, whether a cell continues across a 64-entry block boundary inside a wave, whether one continues across a wave boundary)."""
    minor, major, step_m = (np.asarray(a, np.int64) for a in (minor, major, step_m))
    n = len(minor)
    seen, block_span, wave_span = set(), False, False
    if n == 0:
        return seen, block_span, wave_span
    same = np.zeros(n, bool)
    same[1:] = (minor[1:] == minor[:-1]) & (major[1:] == major[:-1])
    adj = np.zeros(n, bool)
    adj[1:] = ~same[1:] & (step_m[:-1] == 1) & (major[1:] == major[:-1]) & (minor[1:] == minor[:-1] + 1)
    idx = np.arange(n)
    in_wave = idx % chunk
    for i in np.nonzero(~same & (in_wave > 0))[0]:                 # a wave's first entry closes nothing
        seen.add((int(in_wave[i] % SLOTS), bool(adj[i])))
    if n % chunk:                                                  # the first padding entry closes the last cell (never adjacent)
        seen.add((int((n % chunk) % SLOTS), False))
    block_span = bool((same & (in_wave % BLOCK == 0) & (in_wave > 0)).any())
    wave_span = bool((same & (in_wave == 0) & (idx > 0)).any())
    return seen, block_span, wave_span


def _axis_cell_f32(u, n):
    """axis_coord of the kernel in float32: (i0, step flag)."""
    nm1 = np.float32(n - 1)
    x = ((np.asarray(u, np.float32) + np.float32(1.0)) * np.float32(0.5)) * nm1
    x = np.minimum(np.maximum(x, np.float32(0.0)), nm1)
    i0 = np.floor(x).astype(np.int64)
    return i0, (np.minimum(i0 + 1, n - 1) > i0).astype(np.int64)


def kernel_cells(pts, lo, hi, orientation, pw, ph):
    """The sorted cell list of one workgroup: pts [n, 3] float32 (a bundle's samples), the bound, the plane's orientation
    (0: xy, 1: xz, 2: yz) and size.  Returns (minor, major, step_m) in the kernel's order: key = major * extent + minor with
    the minor axis along the longer side of the samples' bounding box (ties inside a cell in any order)."""
    pts, lo, hi = (np.asarray(a, np.float32) for a in (pts, lo, hi))
    nrm = ((pts - lo) / (hi - lo)) * np.float32(2.0) - np.float32(1.0)
    ax = nrm[:, 1] if orientation == 2 else nrm[:, 0]
    ay = nrm[:, 1] if orientation == 0 else nrm[:, 2]
    cx, sx = _axis_cell_f32(ax, pw)
    cy, sy = _axis_cell_f32(ay, ph)
    swap = (cy.max() - cy.min()) > (cx.max() - cx.min())
    minor, major, step_m = (cy, cx, sy) if swap else (cx, cy, sx)
    order = np.argsort(major * (int(minor.max()) + 2) + minor, kind="stable")
    return minor[order], major[order], step_m[order]
