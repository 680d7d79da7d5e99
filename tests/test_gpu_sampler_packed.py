"""The one-launch sampler (eslam_sample_z_all, eslam_sample_z_all_rng) packs its work: four rays with depth per workgroup, and
a fixed number of workgroups that find the depth-less rays of their segment of 1024 rays on their own and take them in turn.
The two single-purpose entries keep one wave (eslam_sample_z) / one workgroup (eslam_importance_z) per ray and are the oracle of
the work assignment: on the same inputs the packed launch must write the same bits, every row exactly once and nothing else.

Everything here is exact equality; the arithmetic itself is held to the reference by tests/test_gpu_parity.py and
tests/test_gpu_kernel_rng_parity.py.
"""
import ctypes
import os
import re

import pytest
import torch

from tests import rng_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGMENT = 1024                       # rays per segment of the depth-less role (IMP_SEG in csrc/eslam_sample.hip)
SENTINEL = -7.25


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _max_samples():
    with open(os.path.join(ROOT, "include", "eslam_hip.h")) as f:
        return int(re.search(r"#define\s+ESLAM_MAX_SAMPLES\s+(\d+)", f.read()).group(1))


def _depthless_workgroups(R):
    """Workgroups of the depth-less role per segment, as sample_z_all_impl sizes them: four per CU (what the chip holds at once)
    shared among the segments, at most one per ray of a segment."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nseg = (R + SEGMENT - 1) // SEGMENT
    return min(max(1, 4 * cus // nseg), min(R, SEGMENT))


@pytest.fixture(scope="module")
def scene():
    """Planes, decoders and 8200+ rays of one camera (trained-like state: the SDF varies along a ray, so the importance samples
    of a depth-less ray depend on its decode)."""
    from myslam_amd import harness
    wl = harness.make_workload("room0", 12600, 16, 4, device=_dev(), state="trained")
    assert wl.R >= 8200, wl.R
    return wl


class _Call:
    """The argument plumbing of the three injected entries and the in-kernel one on rays [lo, lo + R) of the scene."""

    def __init__(self, wl, gd, ns, ni, lo=0):
        from myslam_amd import _hip, ops
        self.hip, self.dev = _hip, wl.device
        self.R, self.ns, self.ni, self.S = int(gd.shape[0]), ns, ni, ns + ni
        self.ro = wl.rays_o.detach()[lo:lo + self.R].contiguous()
        self.rd = wl.rays_d.detach()[lo:lo + self.R].contiguous()
        self.gd = gd.contiguous()
        self.arr, self._keep_planes = _hip.make_planes(wl.planes)
        self.dec, self._keep_dec = _hip.make_decoders(ops.decoder_params(wl.decoders), ops.beta_tensor(wl.decoders.beta, wl.device))
        self.bound = _hip.make_bound(wl.renderer._bound6)
        self.trunc = float(wl.truncation)
        self.t_free, self.t_surf = ops.linspace01(ns, wl.device), ops.linspace01(ni, wl.device)

    def _z(self, guard_rows=0):
        return torch.full((self.R + 2 * guard_rows, self.S), SENTINEL, device=self.dev)

    def pair(self, rand):
        """eslam_sample_z, then eslam_importance_z: one wave / one workgroup per ray."""
        h, p = self.hip, self.hip.ptr
        t_rand, t_uni, u = rand
        z = self._z()
        with h.on_device(self.dev):
            st = h.stream_handle(self.dev)
            h.check(h.lib().eslam_sample_z(p(self.gd), self.R, self.ns, self.ni, self.trunc, p(self.t_free), p(self.t_surf), p(t_rand),
                                           p(z), st), "eslam_sample_z")
            h.check(h.lib().eslam_importance_z(self.arr, ctypes.byref(self.dec), self.bound, p(self.ro), p(self.rd), p(self.gd), self.R,
                                               self.ns, self.ni, p(self.t_free), p(t_uni), p(u), p(z), st), "eslam_importance_z")
        return z

    def packed(self, rand, guard_rows=0):
        h, p = self.hip, self.hip.ptr
        t_rand, t_uni, u = rand
        buf = self._z(guard_rows)
        z = buf[guard_rows:guard_rows + self.R]
        with h.on_device(self.dev):
            h.check(h.lib().eslam_sample_z_all(self.arr, ctypes.byref(self.dec), self.bound, p(self.ro), p(self.rd), p(self.gd), self.R,
                                               self.ns, self.ni, self.trunc, p(self.t_free), p(self.t_surf), p(t_rand), p(t_uni), p(u),
                                               p(z), h.stream_handle(self.dev)), "eslam_sample_z_all")
        return buf

    def in_kernel(self, key, step, ray_offset=0):
        h, p = self.hip, self.hip.ptr
        state = torch.tensor([step], dtype=torch.int32, device=self.dev)
        z = self._z()
        with h.on_device(self.dev):
            h.check(h.lib().eslam_sample_z_all_rng(self.arr, ctypes.byref(self.dec), self.bound, p(self.ro), p(self.rd), p(self.gd), self.R,
                                                   self.ns, self.ni, self.trunc, p(self.t_free), p(self.t_surf), 1, key, p(state),
                                                   ray_offset, p(z), h.stream_handle(self.dev)), "eslam_sample_z_all_rng")
        assert int(state[0]) == step, "the sampler reads the step counter and leaves it alone"
        return z

    def numbers(self, key=0xC0FFEE, step=3, ray_offset=0):
        return tuple(torch.from_numpy(a).to(self.dev) for a in rng_ref.sampler_numbers(key, step, self.R, self.ns, self.ni, ray_offset))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _depths(wl, R, depthless, values=None):
    """gt_depth of the first R rays of the scene with the rays `depthless` (indices) made depth-less: 0, or values[k]."""
    gd = wl.gt_depth[:R].clone()
    assert bool((gd > 0).all())
    idx = torch.as_tensor(list(depthless), dtype=torch.long, device=gd.device)
    if idx.numel():
        gd[idx] = 0.0 if values is None else torch.tensor(values, dtype=torch.float32, device=gd.device)
    return gd


def _case(name):
    """-> (R, n_strat, n_imp, depth-less ray indices, their depth values or None)."""
    nan = float("nan")
    half = _max_samples() // 2
    return {
        "one_ray_with_depth": (1, 16, 4, [], None),
        "one_ray_depthless": (1, 16, 4, [0], None),
        # seven rays: the last workgroup of the row role holds rays 4..6, two of them depth-less
        "seven_mixed": (7, 16, 4, [2, 5, 6], None),
        # 130 depth-less rays: three ballot words, the last with two rays
        "all_depthless_130": (130, 16, 4, range(130), None),
        # more depth-less rays than workgroups that take them (premise asserted in the test)
        "more_rays_than_workgroups": (1300, 16, 4, [i for i in range(1300) if i % 16 != 0], None),
        # segment borders (multiples of SEGMENT; 8192 is one whatever power of two below it SEGMENT is): the last ray of one
        # segment and the first of the next
        "segment_border": (8200, 16, 4, [0, 63, 64, 1023, 1024, 4095, 8191, 8192, 8199], None),
        "mixed_56_8": (70, 56, 8, [1, 2, 33, 64, 69], None),
        "mixed_88_8": (70, 88, 8, [0, 31, 32, 68], None),
        # S above half of ESLAM_MAX_SAMPLES: depth_guided_row cannot stage both sequences in the wave's row
        "unstaged_rows": (9, half - 8, 16, [3, 8], None),
        # what counts as depth-less is `not (depth > 0)`: zero, minus zero, negative, NaN
        "zero_negative_nan": (12, 16, 4, [1, 2, 3, 7, 10], [0.0, -1.0, nan, -0.0, nan]),
    }[name]


CASES = ["one_ray_with_depth", "one_ray_depthless", "seven_mixed", "all_depthless_130", "more_rays_than_workgroups", "segment_border",
         "mixed_56_8", "mixed_88_8", "unstaged_rows", "zero_negative_nan"]


@pytest.mark.parametrize("name", CASES)
def test_packed_launch_equals_one_workgroup_per_ray(scene, name):
    """eslam_sample_z_all against eslam_sample_z followed by eslam_importance_z, injected numbers, bit for bit - and the rows in
    front of and behind the buffer it was given stay as they were."""
    R, ns, ni, less, values = _case(name)
    gd = _depths(scene, R, less, values)
    n_less = int((~(gd > 0)).sum())
    assert n_less == len(list(less))
    if name == "more_rays_than_workgroups":
        n0 = int((~(gd[:SEGMENT] > 0)).sum())                   # rays are dealt out inside a segment
        assert n0 > _depthless_workgroups(R), (n0, _depthless_workgroups(R))             # some workgroup takes two rays
    if name == "unstaged_rows":
        assert 2 * (ns + ni) > _max_samples() >= ns + ni
    c = _Call(scene, gd, ns, ni)
    rand = c.numbers()
    want = c.pair(rand)
    buf = c.packed(rand, guard_rows=2)
    torch.cuda.synchronize()
    assert not bool((want == SENTINEL).any()), "the oracle pair writes every row"
    got = buf[2:2 + R]
    bad = (got.view(torch.int32) != want.view(torch.int32)).any(1).nonzero().flatten().tolist()
    assert not bad, (name, "rows that differ", bad[:10], len(bad))
    assert bool((buf[:2] == SENTINEL).all()) and bool((buf[2 + R:] == SENTINEL).all()), "wrote outside its rows"
    has = gd > 0
    if has.any():
        assert bool((got[has][:, 1:] >= got[has][:, :-1]).all())


def test_in_kernel_numbers_rows_reproducibility_and_ray_offset(scene):
    """eslam_sample_z_all_rng: every row equals the injected entry fed the host replica's numbers of the same (key, step) -
    rays with depth (stream 0) and without (streams 1, 2); a second call gives the same bits; a call on rays [k, R) with
    ray_offset = k gives rows [k, R) of the whole call, k not a multiple of the four rays a workgroup takes."""
    R, ns, ni = 150, 16, 4
    less = [0, 5, 6, 7, 64, 65, 127, 128, 149]
    gd = _depths(scene, R, less)
    key, step = 0x1234ABCD5678, 9
    c = _Call(scene, gd, ns, ni)
    mine = c.in_kernel(key, step)
    want = c.pair(c.numbers(key, step))
    has = gd > 0
    assert _same_bits(mine[has], want[has]), "rays with depth"
    assert _same_bits(mine[~has], want[~has]), "depth-less rays"
    assert _same_bits(mine, c.in_kernel(key, step)), "same (key, step), same samples"
    assert not _same_bits(mine, c.in_kernel(key, step + 1))
    k = 5
    tail = _Call(scene, gd[k:], ns, ni, lo=k)
    assert _same_bits(tail.in_kernel(key, step, ray_offset=k), mine[k:])
    assert not _same_bits(tail.in_kernel(key, step, ray_offset=0), mine[k:])
