"""tests/rng_ref.py, the host replica of the samplers' in-kernel uniform numbers, against a second statement of the same
contract (csrc/eslam_sample.hip, "Counter-based uniform numbers"; ops.py, "Reproducibility contract").  No GPU."""
import numpy as np

from tests import rng_ref

# (key, step, stream, element index, top 24 bits of the hash): evaluated once by hand from the contract in Python int
# arithmetic with an explicit `& 0xFFFFFFFF` behind every multiply and add - not with the replica
TABLE = [
    (0x0, 0x0, 0, 0x0, 0),
    (0x0, 0x0, 0, 0x1, 13938800),
    (0x0, 0x7, 2, 0x3039, 8458000),
    (0x4d, 0x0, 0, 0x5, 3678781),
    (0x4d, 0x1, 1, 0x5, 3731917),
    (0x4d00000000, 0x3, 2, 0x3e8, 9270510),
    (0xdeadbeef12345678, 0x2, 0, 0x3ffff, 13420325),                 # ray 4095, element 63 of 64
    (0x123456789abcdef, 0xffffffff, 1, 0xffffffff, 13178462),       # the last index, the last step: every product wraps
    (0x63, 0x5, 2, 0xfffffffc, 2941069),
    (0x63, 0x5, 2, 0xfffffffb, 572427),                              # the last index the ABI admits at 4 columns
]


def _at(key, step, stream, idx, cols):
    """The replica's number for element index idx, reached as (ray, element) of a [*, cols] call."""
    ray, col = divmod(idx, cols)
    lo = max(0, ray - 2)
    return rng_ref.uniform(key, step, stream, ray - lo + 1, cols, ray_offset=lo)[ray - lo, col]


def test_replica_reproduces_the_hand_evaluated_table():
    for key, step, stream, idx, top24 in TABLE:
        for cols in (1, 3, 4, 5, 64):
            got = _at(key, step, stream, idx, cols)
            assert got.dtype == np.float32 and float(got) == top24 / 2.0 ** 24, (hex(key), step, stream, hex(idx), cols)


def test_values_lie_on_the_24_bit_grid_in_the_unit_interval():
    u = rng_ref.uniform(0x1234567800000009, 3, 0, 257, 64)
    assert u.shape == (257, 64) and u.dtype == np.float32
    assert (u >= 0).all() and (u < 1).all()
    k = u.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(k, np.round(k)) and k.max() < 2 ** 24
    assert len(np.unique(u)) > 0.99 * u.size                         # (16448 draws from 2^24 values)
    assert abs(float(u.mean()) - 0.5) < 0.01 and abs(float(u.var()) - 1 / 12) < 0.005


def test_stream_step_and_both_key_halves_matter():
    base = rng_ref.uniform(77, 4, 0, 16, 32)
    assert np.array_equal(base, rng_ref.uniform(77, 4, 0, 16, 32))
    others = {"stream 1": rng_ref.uniform(77, 4, 1, 16, 32), "stream 2": rng_ref.uniform(77, 4, 2, 16, 32),
              "step": rng_ref.uniform(77, 5, 0, 16, 32), "key_lo": rng_ref.uniform(78, 4, 0, 16, 32),
              "key_hi": rng_ref.uniform(77 | (1 << 32), 4, 0, 16, 32), "key_hi top bit": rng_ref.uniform(77 | (1 << 63), 4, 0, 16, 32)}
    for name, t in others.items():
        assert (t != base).mean() > 0.99, name
    vals = list(others.values())
    for i in range(len(vals)):
        for j in range(i):
            assert (vals[i] != vals[j]).mean() > 0.99
    # the stride of a row is the stream's own column count: the same rays at another width draw other numbers past row 0
    a, b = rng_ref.uniform(77, 4, 0, 8, 32), rng_ref.uniform(77, 4, 0, 8, 24)
    assert np.array_equal(a[0, :24], b[0]) and (a[1:, :24] != b[1:]).mean() > 0.99
    t_rand, t_uni, u = rng_ref.sampler_numbers(77, 4, 16, 24, 8)
    assert t_rand.shape == (16, 32) and t_uni.shape == (16, 24) and u.shape == (16, 8)
    assert np.array_equal(t_rand, base) and np.array_equal(t_uni, rng_ref.uniform(77, 4, 1, 16, 24))
    assert np.array_equal(u, rng_ref.uniform(77, 4, 2, 16, 8))


def test_ray_offset_selects_rows_of_the_whole_batch():
    whole = rng_ref.uniform(0xABCDEF0123, 9, 2, 1000, 8)
    for a, b in ((0, 1000), (1, 1), (137, 400), (999, 1)):
        assert np.array_equal(rng_ref.uniform(0xABCDEF0123, 9, 2, b, 8, ray_offset=a), whole[a:a + b])
    assert rng_ref.uniform(5, 0, 0, 0, 8).shape == (0, 8) and rng_ref.uniform(5, 0, 2, 4, 0).shape == (4, 0)


def test_indices_wrap_as_uint32():
    # the last rows the ABI admits: (ray_offset + rows) * cols just under 2^32 - each index times the odd constant wraps
    cols, rows = 4, 7
    lo = (1 << 30) - 1 - rows
    got = rng_ref.uniform(0x63, 5, 2, rows, cols, ray_offset=lo)
    assert (lo + rows) * cols == (1 << 32) - 4
    assert float(got[rows - 1, cols - 1]) == 572427 / 2.0 ** 24      # index 0xfffffffb: TABLE's last entry (by hand)
    # the index itself is formed in uint32: 2^30 rays of 4 elements further on, the numbers repeat
    assert np.array_equal(rng_ref.uniform(0x63, 5, 2, 3, cols, ray_offset=1 << 30), rng_ref.uniform(0x63, 5, 2, 3, cols))
    # ... and so is the step: k0 and k1 see it modulo 2^32
    assert np.array_equal(rng_ref.uniform(0x63, 1 << 32, 0, 3, cols), rng_ref.uniform(0x63, 0, 0, 3, cols))


def test_key_for_with_an_explicit_seed_is_taken_modulo_2_64():
    assert rng_ref.key_for("cpu", explicit=77) == 77
    assert rng_ref.key_for("cpu", explicit=(1 << 64) + 5) == 5
    assert rng_ref.key_for("cpu", explicit=-1) == (1 << 64) - 1
