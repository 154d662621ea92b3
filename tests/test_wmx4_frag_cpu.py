"""CPU: the wmx4 fragment plane (csrc/vox_wmx4.h, through libvox_synth.so) -- the layout against a
numpy restatement built from frag_off's arithmetic (csrc/vox_hip_dev.h), its size, its stored bits
per weight and the round trip back to the bf16 matrix -- and the margin precondition of every id
comparison tests/test_gpu_wmx4_batch.py makes.

The rule restated: in the bf16 fragment-major copy, element (row j of a 16-row group, column k)
sits at frag_off(j, k) = ((b * 2 + t) * 64 + q * 16 + j) * 8 + (k & 7) with b = k >> 6,
t = (k >> 3) & 1, q = (k & 63) >> 4: lane l = 16 q + j of the wave holds, for 64-k block b, the 8
elements of half t at bytes 16 l of the half's 1024.  The mx4 record of (group g, block b) gives
the same lane the same 16 weights as nibbles: dword 2 l + t of the record holds half t (weight k
in bits 4 (k & 7)..), and byte l of the 64 scale bytes that follow the 128 nibble dwords is the
e8m0 byte of the row's 32-k block 2 b + (q >> 1).

Margin rule (tests/test_wmx4_cpu.py's): on the oracle alone, on the run's weights, every compared
step keeps (top1 - top2) / max|logit| of at least 4x the logit bar.  The worst gap of each run is
printed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_wmx4_batch as g  # noqa: E402  (the cases, the matrices and the oracle sessions; nothing runs on a GPU)

from vox_weights import synth_lib  # noqa: E402

pytestmark = pytest.mark.cpu
NAMES = ["vox_hip_set_wmx4_batch", "vox_hip_wmx4_batch", "vox_hip_model_wmx4_batch_stats", "vox_hip_batch_set_wmx4",
         "vox_hip_skinny_wmx4"]
SHAPES = [(16, 64), (48, 256), (6144, 768), (768, 1280)]
REC = 144   # dwords per (16-row group, 64-k block)


def test_header_library_and_binding_have_the_names():
    import vox_hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voxtral_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in vox_hip.EXPORTS, n
    for f in (vox_hip.set_wmx4_batch, vox_hip.wmx4_batch, vox_hip.skinny_wmx4, vox_hip.Model.wmx4_batch_stats,
              vox_hip.Batch.set_wmx4):
        assert callable(f)


def _pack(w):
    rows, K = w.shape
    nib, scl = np.zeros((rows, K // 8), np.uint32), np.zeros((rows, K // 32), np.uint8)
    synth_lib().vox_wmx4_pack(w.ctypes.data, rows, K, nib.ctypes.data, scl.ctypes.data)
    return nib, scl


def _frag_off(j, k):
    b, r = k >> 6, k & 63
    return ((b * 2 + ((r >> 3) & 1)) * 64 + (r >> 4) * 16 + j) * 8 + (r & 7)


def _where(N, K):
    """for every weight (row, k): its record, its lane, its half and its nibble, from frag_off"""
    row, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    off = _frag_off(row & 15, k)              # element offset inside the group's bf16 fragment copy
    blk, half, lane, nibble = off >> 10, (off >> 9) & 1, (off >> 3) & 63, off & 7
    rec = (row >> 4) * (K // 64) + blk
    return row, k, rec, lane, half, nibble


def _ref_layout(nib, scl, N, K):
    """the plane from the compact form by the rule"""
    row, k, rec, lane, half, nibble = _where(N, K)
    code = (nib[row, k >> 3] >> (4 * (k & 7)).astype(np.uint32)) & 15
    words = np.zeros((N // 16 * (K // 64), REC), np.uint32)
    halves = np.zeros((words.shape[0], 64, 2, 8), np.uint32)
    halves[rec, lane, half, nibble] = code
    words[:, :128] = (halves << (4 * np.arange(8, dtype=np.uint32))).sum(axis=3, dtype=np.uint32).reshape(-1, 128)
    # scale bytes: lane l = 16 q + j of record (g, b) takes row 16 g + j, block 2 b + (q >> 1)
    gi, bi, li = np.meshgrid(np.arange(N // 16), np.arange(K // 64), np.arange(64), indexing="ij")
    sb = scl[gi * 16 + (li & 15), 2 * bi + (li >> 5)].astype(np.uint32).reshape(-1, 16, 4)
    words[:, 128:] = (sb << (8 * np.arange(4, dtype=np.uint32))).sum(axis=2, dtype=np.uint32)
    return words.reshape(-1)


def _decode(code, e):
    """vox_wmx4_decode in numpy: bf16 bits of e2m1 code (sign in bit 3) times 2^e"""
    de = np.array([0, -1, 0, 0, 1, 1, 2, 2])
    c, s = code & 7, (code >> 3) & 1
    mant = np.where((c & 1) & (c > 1), 0x40, 0)
    v = (s << 15) | np.where(c == 0, 0, ((e + de[c] + 127) << 7) | mant)
    return v.astype(np.uint16)


def _ref_unlayout(words, N, K):
    """the bf16 matrix back from the plane, by the rule"""
    row, k, rec, lane, half, nibble = _where(N, K)
    words = words.reshape(-1, REC)
    code = (words[rec, 2 * lane + half] >> (4 * nibble).astype(np.uint32)) & 15
    byte = (words[rec, 128 + (lane >> 2)] >> (8 * (lane & 3)).astype(np.uint32)) & 255
    return _decode(code.astype(np.int64), byte.astype(np.int64) - 127)


def _layout(nib, scl, N, K):
    words = synth_lib().vox_wmx4_frag_words_of(N, K)
    out = np.full(words + 8, 0xdeadbeef, np.uint32)
    synth_lib().vox_wmx4_frag_layout(nib.ctypes.data, scl.ctypes.data, N, K, out.ctypes.data)
    assert (out[words:] == 0xdeadbeef).all()
    return out[:words]


@pytest.mark.parametrize("N,K", SHAPES)
def test_frag_layout_words_bits_and_round_trip(N, K):
    w = g.mx4_matrix(N, K, seed=N + K)
    # what the matrices are said to hold
    blocks = w.reshape(N, K // 32, 32)
    nz = ((blocks & 0x7fff) != 0).sum(axis=2)
    assert synth_lib().vox_wmx4_scan(w.ctypes.data, N, K) == 1
    assert (w == 0x8000).any() and (nz == 0).any() and (nz == 1).any()
    nib, scl = _pack(w)
    assert {int(scl.min()), int(scl.max())} == {127 - 64, 127 + 64}
    # size and stored bits
    words = synth_lib().vox_wmx4_frag_words_of(N, K)
    assert words == N // 16 * (K // 64) * REC
    assert words * 32 / (N * K) == 4.5 <= 5
    # layout, word for word, and the round trip
    got = _layout(nib, scl, N, K)
    assert np.array_equal(got, _ref_layout(nib, scl, N, K))
    assert np.array_equal(_ref_unlayout(got, N, K), w)


def test_frag_words_refuses_other_shapes():
    f = synth_lib().vox_wmx4_frag_words_of
    assert f(16, 64) == REC and f(32, 128) == 4 * REC
    for N, K in [(8, 64), (16, 32), (24, 64), (16, 96), (0, 64), (16, 0)]:
        assert f(N, K) == 0, (N, K)


def test_frag_layout_follows_the_w13_interleave():
    """W1|W3 needs no special case: the plane is laid out from the device row order (16 rows of
    W1, then the 16 matching rows of W3), exactly as any other matrix"""
    H, K = 64, 128
    w1, w3 = g.mx4_matrix(H, K, seed=1), g.mx4_matrix(H, K, seed=3)
    dev = np.stack([w1.reshape(H // 16, 16, K), w3.reshape(H // 16, 16, K)], axis=1).reshape(2 * H, K)
    got = _layout(*_pack(dev), 2 * H, K)
    back = _ref_unlayout(got, 2 * H, K).reshape(H // 16, 2, 16, K)
    assert np.array_equal(back[:, 0].reshape(H, K), w1) and np.array_equal(back[:, 1].reshape(H, K), w3)


# ---- the margin precondition of the GPU file's id comparisons ----------------------------------
@pytest.mark.parametrize("run", sorted(g.ORACLE_RUNS))
def test_oracle_margin(run):
    _, _, n, kv16, seed = g.ORACLE_RUNS[run]
    margin = g.MARGIN_KV16 if kv16 else g.MARGIN_F32
    ref = g._oracle(run)
    assert len(ref) == n
    worst, steps = np.inf, 0
    for i, (ids, lg) in enumerate(ref):
        assert len(ids) == lg.shape[0] == g.STEPS, (run, i, len(ids))
        top = np.partition(lg, -2, axis=1)[:, -2:]
        gap = (top[:, 1] - top[:, 0]) / np.max(np.abs(lg), axis=1)
        assert np.array_equal(np.argmax(lg, axis=1), np.asarray(ids)), (run, i)
        k = int(np.argmin(gap))
        assert gap[k] >= margin, (run, i, k, float(gap[k]), margin)
        worst = min(worst, float(gap[k]))
        steps += len(ids)
    print(f"{run}: mel seed {seed}, oracle top-2 gap >= {worst:.2e} of the largest logit over {steps} steps "
          f"(rule: {margin:.0e})")
