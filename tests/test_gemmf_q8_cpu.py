"""CPU: the host-visible side of k_gemmf over int8 fragments -- the exported
entry points, the int8 fragment order the kernel streams, and the exactness of int8 -> bf16."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.cpu

NEW = ["vox_hip_set_gemmf_q8", "vox_hip_gemmf_q8", "vox_hip_model_gemmf_q8_stats", "vox_hip_gemmf_q8_rows"]


def frag_pack_q8(W):
    """k_frag_pack<1> restated: W int8 [N, K] -> [N / 16, K / 64, 64 lanes, 16 B]; lane l of the
    1-KiB block of 16-row group g and 64-k block b holds W[16 g + (l & 15)][64 b + 16 (l >> 4) .. + 15]"""
    N, K = W.shape
    assert N % 16 == 0 and K % 64 == 0
    out = np.empty((N // 16, K // 64, 64, 16), np.int8)
    for lane in range(64):
        r, q = lane & 15, lane >> 4
        # rows 16 g + r of every group, columns 64 b + 16 q .. + 15 of every block
        out[:, :, lane, :] = W.reshape(N // 16, 16, K // 64, 64)[:, r, :, 16 * q:16 * q + 16]
    return out


def frag_pack_bf16(W):
    """k_frag_pack<0> restated: W [N, K] -> [N / 16, K / 64, 2 halves, 64 lanes, 8]; lane l of half
    t holds W[16 g + (l & 15)][64 b + 16 (l >> 4) + 8 t .. + 7]"""
    N, K = W.shape
    out = np.empty((N // 16, K // 64, 2, 64, 8), W.dtype)
    for lane in range(64):
        r, q = lane & 15, lane >> 4
        for t in range(2):
            out[:, :, t, lane, :] = W.reshape(N // 16, 16, K // 64, 64)[:, r, :, 16 * q + 8 * t:16 * q + 8 * t + 8]
    return out


def test_new_symbols_are_declared_exported_and_bound():
    import vox_hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voxtral_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in vox_hip.EXPORTS, n
    for n in ("set_gemmf_q8", "gemmf_q8", "gemmf_q8_rows"):
        assert callable(getattr(vox_hip, n)), n
    assert callable(vox_hip.Model.gemmf_q8_stats)


def test_int8_fragment_order_is_the_bf16_copys_two_halves():
    """The int8 block's 16 B of a lane are that lane's 8 elements of half 0 followed by its 8 of
    half 1 in the bf16 copy: the kernel's `first 8 B feed half 0, the last 8 half 1`.  The
    element-by-element formula is checked on a matrix whose entries encode their own (row, col)."""
    N, K = 48, 192
    rows, cols = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    code = (rows * K + cols).astype(np.int32)
    W8 = (code % 251 - 125).astype(np.int8)
    f8 = frag_pack_q8(W8)
    assert f8.size == N * K and f8.reshape(-1).shape[0] == (N // 16) * (K // 64) * 1024
    for g, b, lane, e in [(0, 0, 0, 0), (2, 1, 37, 9), (1, 2, 63, 15), (0, 2, 16, 7), (2, 0, 15, 8)]:
        assert f8[g, b, lane, e] == W8[16 * g + (lane & 15), 64 * b + 16 * (lane >> 4) + e]
    fb = frag_pack_bf16(W8)
    assert np.array_equal(f8[..., :8], fb[:, :, 0]) and np.array_equal(f8[..., 8:], fb[:, :, 1])
    # every element lands exactly once
    ids = np.empty((N // 16, K // 64, 64, 16), np.int32)
    for lane in range(64):
        ids[:, :, lane, :] = code.reshape(N // 16, 16, K // 64, 64)[:, lane & 15, :, 16 * (lane >> 4):16 * (lane >> 4) + 16]
    assert np.array_equal(np.sort(ids.reshape(-1)), np.arange(N * K))


def test_every_int8_is_a_bf16():
    """float32(int8) has no bit below the bf16 mantissa: its high half is the value (i8x8_bf16)"""
    v = np.arange(-128, 128, dtype=np.int8)
    bits = np.float32(v).view(np.uint32)
    assert not np.any(bits & 0xFFFF)
    back = ((bits >> 16).astype(np.uint32) << 16).view(np.float32)
    assert np.array_equal(back, v.astype(np.float32))


def test_switch_follows_the_setter_and_the_environment_gives_the_initial_value():
    """no GPU call: the process-wide switch alone"""
    import vox_hip
    first = vox_hip.gemmf_q8()
    assert first == (1 if os.environ.get("VOX_HIP_GEMMF_Q8") == "1" else 0)
    try:
        vox_hip.set_gemmf_q8(True)
        assert vox_hip.gemmf_q8() == 1
        vox_hip.set_gemmf_q8(False)
        assert vox_hip.gemmf_q8() == 0
    finally:
        vox_hip.set_gemmf_q8(bool(first))
