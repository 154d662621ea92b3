"""CPU: the bounds of the wide batched step in the two public headers, and the argument checks
that refuse more than 128 streams, reached without a GPU."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

pytestmark = pytest.mark.cpu

PKG = os.path.join(ROOT, "voxtral.c_amd")


def _define(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    m = re.search(rf"^#define\s+{name}\s+(\d+)\s*$", text, re.M)
    assert m, (header, name)
    return int(m.group(1)), text


def test_headers_carry_the_bounds():
    slots, lib_h = _define("voxtral_hip.h", "VOX_HIP_BATCH_MAX_SLOTS")
    sched, host_h = _define("vox_hip_host.h", "VH_SCHED_MAX")
    assert slots == sched == 128
    internal = open(os.path.join(PKG, "csrc", "vox_hip_internal.h")).read()
    assert re.search(r"constexpr int VOX_MAX_BATCH = 32;", internal)
    assert re.search(r"constexpr int VOX_MAX_SLOTS = 128;", internal)
    # what the changed bounds mean for memory, and what stays unevaluated, is said where they are
    for text in (lib_h, host_h):
        assert "225 GB" in text and "113 GB" in text and "56 GB" in text and "unevaluated" in text
    import vox_hip
    assert vox_hip.BATCH_MAX_SLOTS == slots and vox_hip.SCHED_MAX == sched


def test_scheduler_refuses_129_streams():
    """vh_sched_create on a wrapped context (no device work: the batch object is made by the
    first batched step): 128 accepted, 0 and 129 refused with the range in the message"""
    import vox_hip
    L = ctypes.CDLL(os.path.join(PKG, "libvox_hip_host.so"))
    L.vh_ctx_wrap.restype = ctypes.c_void_p
    L.vh_ctx_wrap.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.vh_sched_create.restype = ctypes.c_void_p
    L.vh_sched_create.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.vh_sched_free.argtypes = [ctypes.c_void_p]
    L.vh_free.argtypes = [ctypes.c_void_p]
    L.vh_last_error.restype = ctypes.c_char_p
    from vox_weights import TINY
    cfg = TINY.ctypes_struct(vox_hip.ConfigC)
    model = ctypes.create_string_buffer(64)   # never dereferenced: the context only keeps the pointer
    ctx = L.vh_ctx_wrap(ctypes.cast(model, ctypes.c_void_p), ctypes.byref(cfg), 6)
    assert ctx
    for n in (0, 129, 1 << 20):
        assert not L.vh_sched_create(ctx, n), n
        assert b"1..128" in L.vh_last_error(), L.vh_last_error()
    for n in (1, 33, 128):
        q = L.vh_sched_create(ctx, n)
        assert q, n
        L.vh_sched_free(q)
    L.vh_free(ctx)


def test_batch_create_refuses_129_streams():
    """vox_hip_batch_create checks its range before anything touches the device"""
    import vox_hip
    L = vox_hip.lib()
    for n in (0, 129):
        assert not L.vox_hip_batch_create(None, n)
        assert b"1..128" in L.vox_hip_last_error(), L.vox_hip_last_error()
    with pytest.raises(ValueError, match="1..128"):
        vox_hip.Batch(None, 129)
