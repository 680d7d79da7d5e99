"""The rank-16 scatter (tests/rank16_ref.py) in float64 on the CPU: accumulating a cell's sums 16 wide and expanding them once
gives what expanding every sample and scattering it gives, and the kernel's lane bookkeeping reproduces both."""
import numpy as np
import pytest

from tests import rank16_ref as r16

TOL = 1e-12      # max-normalised, float64: sums of <= a few hundred terms reordered


def _inputs(seed, n, h, w):
    rng = np.random.default_rng(seed)
    gz = rng.normal(size=(n, r16.HID))
    W = rng.normal(size=(r16.HID, r16.CH))
    u = rng.uniform(-1.0, 1.0, size=n)
    v = rng.uniform(-1.0, 1.0, size=n)
    k = n // 8
    # samples exactly on texel boundaries (t == 0) ...
    u[:k] = 2.0 * rng.integers(0, w, size=k) / max(w - 1, 1) - 1.0
    v[k:2 * k] = 2.0 * rng.integers(0, h, size=k) / max(h - 1, 1) - 1.0
    # ... on the last texel (i1 == i0: both corners are one texel) and beyond the border (clamped)
    u[2 * k:3 * k] = 1.0
    v[3 * k:4 * k] = rng.choice([-1.0, 1.0, -1.7, 2.5], size=k)
    u[4 * k:5 * k] = rng.choice([-1.0, -3.0, 1.25], size=k)
    return gz, W, u, v


def _maxnorm(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("seed,n,h,w", [(0, 400, 7, 9), (1, 1000, 5, 4), (2, 64, 2, 2), (3, 300, 1, 6), (4, 300, 6, 1)])
def test_accumulate_then_expand_matches_expand_then_scatter(seed, n, h, w):
    gz, W, u, v = _inputs(seed, n, h, w)
    ref = r16.expand_then_scatter(gz, W, u, v, h, w)
    assert np.abs(ref).max() > 0
    assert _maxnorm(r16.accumulate_then_expand(gz, W, u, v, h, w), ref) <= TOL


@pytest.mark.parametrize("seed,n,h,w", [(0, 400, 7, 9), (1, 1000, 5, 4), (2, 64, 2, 2), (3, 300, 1, 6), (4, 300, 6, 1)])
def test_wave_walk_matches_expand_then_scatter(seed, n, h, w):
    """Carried columns, lower-half-only flushes and the clamped border (a step flag of 0 folds both corners onto one texel)."""
    gz, W, u, v = _inputs(seed, n, h, w)
    ref = r16.expand_then_scatter(gz, W, u, v, h, w)
    assert _maxnorm(r16.walk_wave(gz, W, u, v, h, w), ref) <= TOL


def test_lane_roles():
    """(hx, row, j) accumulates, (hx, c) flushes rows 0 and 1; both roles are bijections onto the wave."""
    seen = set()
    for lane in range(64):
        hx, row, j = r16.walk_lane(lane)
        assert 0 <= hx < 2 and 0 <= row < 2 and 0 <= j < r16.HID
        assert r16.source_lane(hx, row, j) == lane
        seen.add((hx, row, j))
        fx, c = r16.flush_lane(lane)
        assert fx == hx and c == (row << 4 | j)              # the half-wave is the x corner in both roles
    assert len(seen) == 64
    # expansion: lane (hx, c) reads the 16 + 16 accumulators of ITS half-wave only
    rng = np.random.default_rng(5)
    acc, W = rng.normal(size=64), rng.normal(size=(r16.HID, r16.CH))
    out = r16.expand_wave(acc, W)
    A = acc.reshape(2, 2, r16.HID)
    np.testing.assert_allclose(out.reshape(2, r16.CH, 2), np.einsum("xrj,jc->xcr", A, W), rtol=0, atol=1e-13)


def test_carried_column():
    """The sums of corner x = 1 become the next cell's corner x = 0; the new corner x = 1 starts empty."""
    acc = np.arange(64, dtype=np.float64) + 1.0
    nxt = r16.carry_column(acc)
    for lane in range(64):
        hx, row, j = r16.walk_lane(lane)
        assert nxt[lane] == (acc[r16.source_lane(1, row, j)] if hx == 0 else 0.0)
