"""Host replica of the samplers' in-kernel uniform numbers (eslam_sample_z_all_rng), written from the contract in the comments
of csrc/eslam_sample.hip ("Counter-based uniform numbers ...") and ops.py ("Reproducibility contract ..."), in numpy uint32
arithmetic: every multiply and add wraps modulo 2^32, as on the device.

    U(key, step, stream, ray, element) = top 24 bits of mix(mix(idx * 0x9E3779B1 + k0 + stream * 0x85EBCA77) + k1) * 2^-24
    k0 = key_lo ^ (step * 0x9E3779B9)        k1 = key_hi + step * 0x7F4A7C15        idx = (ray_offset + ray) * cols + element

stream 0: jitter of the depth-guided samples (cols = S = n_strat + n_imp); stream 1: jitter of the uniform samples of
depth-less rays (cols = n_strat); stream 2: the importance draw u (cols = n_imp).  Test-only.
"""
import numpy as np

STREAM_JITTER, STREAM_JITTER_UNI, STREAM_IMPORTANCE = 0, 1, 2


def _mix(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x7FEB352D)
    h = h ^ (h >> np.uint32(15))
    h = h * np.uint32(0x846CA68B)
    return h ^ (h >> np.uint32(16))


def uniform(key, step, stream, rows, cols, ray_offset=0):
    """float32 [rows, cols]: the numbers the sampler draws for rays ray_offset .. ray_offset + rows - 1 of a batch."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over="ignore"):
        step = np.uint32(int(step) & 0xFFFFFFFF)
        k0 = np.uint32(key & 0xFFFFFFFF) ^ (step * np.uint32(0x9E3779B9))
        k1 = np.uint32(key >> 32) + step * np.uint32(0x7F4A7C15)
        ray = np.uint32(int(ray_offset) & 0xFFFFFFFF) + np.arange(rows, dtype=np.uint32)[:, None]
        idx = ray * np.uint32(cols) + np.arange(cols, dtype=np.uint32)[None, :]
        h = _mix(idx * np.uint32(0x9E3779B1) + k0 + np.uint32(stream) * np.uint32(0x85EBCA77))
        h = _mix(h + k1)
    assert h.dtype == np.uint32
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def sampler_numbers(key, step, rows, n_strat, n_imp, ray_offset=0):
    """(t_rand [rows, S], t_rand_uni [rows, n_strat], u [rows, n_imp]) of one sampler call, as `_rand=` takes them."""
    return (uniform(key, step, STREAM_JITTER, rows, n_strat + n_imp, ray_offset),
            uniform(key, step, STREAM_JITTER_UNI, rows, n_strat, ray_offset),
            uniform(key, step, STREAM_IMPORTANCE, rows, n_imp, ray_offset))


def key_for(device, explicit=None):
    """The 64-bit key of the contract: the value given to ops.seed if any, else the CPU generator's seed times the 64-bit
    golden-ratio constant plus the device generator's seed, modulo 2^64."""
    import torch
    if explicit is not None:
        return int(explicit) % (1 << 64)
    cpu_seed = torch.default_generator.initial_seed()
    dev_seed = torch.cuda.default_generators[torch.device(device).index or 0].initial_seed()
    return (cpu_seed * 0x9E3779B97F4A7C15 + dev_seed) % (1 << 64)
