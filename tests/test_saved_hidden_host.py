"""The saved first hidden layer, host side (no GPU needed): the library exports the entry points that take the buffer, the
header declares them, the binding has their prototypes, the size query is 2 * R * ceil(S / 16) * 256 floats, and a backward that
was told to read the buffer refuses a missing or short one before anything is launched.
"""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eslam_saved_hidden_floats", "eslam_render_fwd_h", "eslam_render_fwd_loss_h", "eslam_render_bwd_h", "eslam_render_bwd_loss_h",
       "eslam_last_backward_saved_hidden")
# the entry each new one extends by ONE pointer in front of the stream
EXTENDS = {"eslam_render_fwd_h": "eslam_render_fwd", "eslam_render_fwd_loss_h": "eslam_render_fwd_loss",
           "eslam_render_bwd_h": "eslam_render_bwd", "eslam_render_bwd_loss_h": "eslam_render_bwd_loss"}


def _header():
    src = open(os.path.join(ROOT, "include", "eslam_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_library_header_and_binding_carry_the_new_symbols():
    from myslam_amd import _hip
    lib = _hip.load_library()
    hdr = _header()
    for n in NEW:
        assert hasattr(lib, n), f"{n} is not exported"
        assert re.search(r"\b%s\s*\(" % n, hdr), f"{n} is not declared in include/eslam_hip.h"
        assert n in _hip.SIGNATURES, f"{n} has no ctypes prototype"
    assert lib.eslam_abi_version() == _hip.ABI_VERSION == 5
    assert int(re.search(r"#define ESLAM_ABI_VERSION (\d+)", hdr).group(1)) == 5


def test_new_entries_take_the_old_arguments_plus_one_pointer_in_front_of_the_stream():
    from myslam_amd import _hip
    hdr = _header()

    def params(name):
        m = re.search(r"\bint %s\s*\((.*?)\);" % name, hdr, flags=re.S)
        assert m, name
        return [" ".join(p.split()) for p in m.group(1).split(",")]

    for new, old in EXTENDS.items():
        res_n, args_n = _hip.SIGNATURES[new]
        res_o, args_o = _hip.SIGNATURES[old]
        assert res_n is res_o and list(args_n) == list(args_o[:-1]) + [ctypes.c_void_p, args_o[-1]], new
        pn, po = params(new), params(old)
        assert pn[:-2] == po[:-1] and pn[-1] == po[-1] == "eslam_stream_t stream", new
        assert re.fullmatch(r"(const )?float\* hidden", pn[-2]), (new, pn[-2])


@pytest.mark.parametrize("S", [40, 56, 64, 96])
def test_size_query(S):
    from myslam_amd import _hip, ops
    lib = _hip.load_library()
    for R in (1, 37, 1100, 4096):
        want = 2 * R * -(-S // 16) * 256
        assert lib.eslam_saved_hidden_floats(R, S) == want
        assert ops.saved_hidden_floats(R, S) == want
    assert lib.eslam_saved_hidden_floats(0, S) == 0
    assert lib.eslam_saved_hidden_floats(-1, S) == -1


def test_missing_or_short_buffer_is_refused_before_any_launch():
    """What RenderFn.backward checks first when its forward saved the layer (no GPU here: nothing could be launched at all)."""
    from myslam_amd import ops
    R, S = 37, 40
    n = ops.saved_hidden_floats(R, S)
    with pytest.raises(RuntimeError, match="saved hidden layer: the forward pass left no buffer"):
        ops.require_saved_hidden(None, R, S)
    with pytest.raises(RuntimeError, match=f"saved hidden layer: {n - 1} .* {n} contiguous float32 needed"):
        ops.require_saved_hidden(torch.empty(n - 1), R, S)
    with pytest.raises(RuntimeError, match="saved hidden layer"):
        ops.require_saved_hidden(torch.empty(n, dtype=torch.float64), R, S)
    with pytest.raises(RuntimeError, match="saved hidden layer"):
        ops.require_saved_hidden(torch.empty(2 * n)[::2], R, S)
    h = torch.empty(n)
    assert ops.require_saved_hidden(h, R, S) is h


def test_compiled_glue_makes_the_same_refusal():
    """RenderNode::backward's check (eslam_torch_ext.cpp require_saved_hidden), the function itself, on host tensors."""
    from myslam_amd import ops
    ext = ops.torch_ext()
    assert ext is not None, "eslam_torch_ext is not built"
    R, S = 37, 40
    n = ops.saved_hidden_floats(R, S)
    with pytest.raises(RuntimeError, match=f"saved hidden layer: 0 elements, {n} contiguous float32 needed"):
        ext.require_saved_hidden(None, R, S)
    with pytest.raises(RuntimeError, match=f"saved hidden layer: {n - 1} elements, {n} contiguous float32 needed"):
        ext.require_saved_hidden(torch.empty(n - 1), R, S)
    with pytest.raises(RuntimeError, match="saved hidden layer"):
        ext.require_saved_hidden(torch.empty(n, dtype=torch.float64), R, S)
    with pytest.raises(RuntimeError, match="saved hidden layer"):
        ext.require_saved_hidden(torch.empty(2 * n)[::2], R, S)
    ext.require_saved_hidden(torch.empty(n), R, S)


def test_python_backward_checks_the_buffer_before_it_touches_the_library(monkeypatch):
    """RenderFn.backward on a context whose forward saved the layer but whose buffer is short: the refusal comes before the
    library is even looked up, so nothing can have been launched."""
    from types import SimpleNamespace
    from myslam_amd import _hip, ops
    R, S = 5, 40
    z = torch.zeros(R, S)
    t = torch.zeros(1)
    called = []
    monkeypatch.setattr(_hip, "lib", lambda: called.append(1) or (_ for _ in ()).throw(AssertionError("library reached")))
    n = 2 * R * 3 * 256
    monkeypatch.setattr(ops, "saved_hidden_floats", lambda r, s: 2 * r * -(-s // 16) * 256)
    for hid, msg in ((torch.empty(n - 1), f"saved hidden layer: {n - 1} "), (None, "the forward pass left no buffer")):
        saved = (t, t, z) + (t,) * 31 + (() if hid is None else (hid,))
        ctx = SimpleNamespace(saved_tensors=saved, saved_hidden=True)
        with pytest.raises(RuntimeError, match=msg):
            ops.RenderFn.backward(ctx, None, None, None)
    assert not called


def test_forward_entries_refuse_a_hidden_buffer_without_features_or_beyond_32_bit_offsets():
    """Decided on the host before the launch: the hidden layer is saved beside the features, and its blocks are addressed with
    32-bit byte offsets (R * ceil(S / 16) * 2048 < 2^32 - 256)."""
    from myslam_amd import _hip
    lib = _hip.load_library()
    planes = (_hip.PlaneDesc * 12)()
    dec = _hip.DecodersDesc()
    bound = (ctypes.c_float * 6)(-1, 1, -1, 1, -1, 1)
    one = ctypes.c_void_p(256)          # never dereferenced: the calls below return before validating the planes
    rc = lib.eslam_render_fwd_h(planes, ctypes.byref(dec), bound, one, one, one, 8, 16, one, one, one, None, None, None, None, one, None)
    assert rc != 0 and "feat is NULL" in lib.eslam_last_error().decode()
    R = (1 << 32) // 2048 + 1           # S = 16: one block per ray and decoder
    rc = lib.eslam_render_fwd_h(planes, ctypes.byref(dec), bound, one, one, one, R, 16, one, one, one, one, one, None, None, one, None)
    assert rc != 0 and "saved hidden layer" in lib.eslam_last_error().decode()


def test_keyword_and_context_manager():
    from myslam_amd import ops
    assert ops.saved_hidden_on() == ops.SAVED_HIDDEN_DEFAULT
    with ops.saved_hidden(False):
        assert ops.saved_hidden_on() is False
        with ops.saved_hidden(True):
            assert ops.saved_hidden_on() is True
        with ops.saved_hidden(None):
            assert ops.saved_hidden_on() == ops.SAVED_HIDDEN_DEFAULT
        assert ops.saved_hidden_on() is False
    assert ops.saved_hidden_on() == ops.SAVED_HIDDEN_DEFAULT
