"""The four-entries-per-step walk of the rank-16 scatter (tests/quad_walk_ref.py) in float64 on the CPU: slots, the step that closes
a cell, the slot sum and the carried column give what tests/rank16_ref.accumulate_then_expand gives, and `cases` sees every
(position of the fresh entry in its step) x (adjacent / not) case in lists made to contain them."""
import numpy as np
import pytest

from tests import quad_walk_ref as qw
from tests import rank16_ref as r16
from tests.test_rank16_ref import _inputs, _maxnorm

TOL = 1e-12      # max-normalised, float64: sums of <= a few hundred terms reordered


@pytest.mark.parametrize("chunk", [256, 128, 8])
@pytest.mark.parametrize("seed,n,h,w", [(0, 400, 7, 9), (1, 1000, 5, 4), (2, 64, 2, 2), (3, 300, 1, 6), (4, 300, 6, 1), (5, 1021, 9, 33),
                                        (6, 3, 4, 4)])
def test_quad_walk_matches_accumulate_then_expand(seed, n, h, w, chunk):
    """Random sorted lists with samples on texel boundaries, on the last texel and beyond the border; list lengths that are no
    multiple of four; waves of 256 and 128 entries (the two bundle sizes) and of 8 (every cell spans waves)."""
    gz, W, u, v = _inputs(seed, n, h, w)
    ref = r16.accumulate_then_expand(gz, W, u, v, h, w)
    assert np.abs(ref).max() > 0
    assert _maxnorm(qw.walk_quad(gz, W, u, v, h, w, chunk=chunk), ref) <= TOL


def test_quad_walk_matches_the_one_entry_walk():
    gz, W, u, v = _inputs(7, 500, 6, 11)
    assert _maxnorm(qw.walk_quad(gz, W, u, v, 6, 11), r16.walk_wave(gz, W, u, v, 6, 11)) <= TOL


def test_slot_sum_is_the_sum_over_slots_in_the_expansion_layout():
    rng = np.random.default_rng(8)
    acc = rng.normal(size=(qw.SLOTS, 4, r16.HID))
    out = qw.slot_sum(acc)
    tot = acc.sum(0)                                               # [k, j]
    for lane in range(64):
        hx, row, j = r16.walk_lane(lane)                           # the layout rank16_ref.expand_wave reads: lane = k * 16 + j
        assert abs(out[lane] - tot[2 * hx + row, j]) <= 1e-13
        assert lane == qw.slot_lane(2 * hx + row, j)


def test_carried_column_stays_in_its_slot():
    acc = np.arange(qw.SLOTS * 4 * r16.HID, dtype=np.float64).reshape(qw.SLOTS, 4, r16.HID) + 1.0
    nxt = qw.carry_column(acc)
    assert np.array_equal(nxt[:, 0:2], acc[:, 2:4]) and not nxt[:, 2:4].any()
    # the sum over slots of the carried sums is the carried sum over slots: nothing has to be exchanged at the carry
    assert np.allclose(qw.slot_sum(nxt).reshape(4, r16.HID)[0:2], acc.sum(0)[2:4])


def _run(minor, major, step_m, chunk=256):
    return qw.cases(np.array(minor), np.array(major), np.array(step_m), chunk)


def test_cases_positions_and_adjacency():
    # cells of 5 entries along one row, each the minor-axis neighbour of the one before: fresh entries at 5, 10, 15, 20 ->
    # positions 1, 2, 3, 0, all adjacent
    minor = np.repeat(np.arange(5), 5)
    seen, blk, wav = _run(minor, np.zeros(25, int), np.ones(25, int))
    assert {(1, True), (2, True), (3, True), (0, True)} <= seen and not blk and not wav
    assert (25 % 4, False) in seen                                 # the first padding entry closes the last cell
    # the same cells with the step flag off (last texel column) or a gap between them: never adjacent
    seen, _, _ = _run(minor, np.zeros(25, int), np.zeros(25, int))
    assert {(1, False), (2, False), (3, False), (0, False)} <= seen and not any(a for _, a in seen)
    seen, _, _ = _run(minor * 2, np.zeros(25, int), np.ones(25, int))
    assert not any(a for _, a in seen)
    # a new row is never adjacent, whatever the minor coordinate
    seen, _, _ = _run([0, 0, 1, 1], [0, 0, 1, 1], [1, 1, 1, 1])
    assert (2, False) in seen and (2, True) not in seen


def test_cases_spans():
    n = 300
    _, blk, wav = _run(np.zeros(n, int), np.zeros(n, int), np.ones(n, int))          # one cell: spans blocks and the wave boundary
    assert blk and wav
    minor = np.arange(n) // 64                                                        # cells end exactly at the block boundaries
    _, blk, wav = _run(minor, np.zeros(n, int), np.ones(n, int))
    assert not blk and not wav
    minor = np.arange(n) // 100                                                       # 100-entry cells: spans at 64, 128 and 256
    _, blk, wav = _run(minor, np.zeros(n, int), np.ones(n, int))
    assert blk and wav
    _, blk, wav = _run(minor, np.zeros(n, int), np.ones(n, int), chunk=128)           # 128-entry waves: 128 is a wave boundary
    assert wav


def test_kernel_cells_sorts_along_the_longer_side():
    lo, hi = np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0])
    t = np.linspace(-0.9, 0.9, 40)
    pts = np.stack([0.1 * t, t, 0.0 * t], 1)                       # travels along y: in the xy plane y is the minor axis
    minor, major, step_m = qw.kernel_cells(pts, lo, hi, 0, 16, 16)
    assert major.max() - major.min() <= 2 and minor.max() - minor.min() >= 12
    assert np.all(np.diff(major * 100 + minor) >= 0) and set(step_m) <= {0, 1}
    seen, _, _ = qw.cases(minor, major, step_m, 256)
    assert any(a for _, a in seen)
