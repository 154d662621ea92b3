"""CPU: the wpack13 fragment plane (csrc/vox_wpack.h) of the batched MFMA step: vox_wpack13_frag_layout
against a numpy restatement built from frag_off's lane arithmetic (vox_hip_dev.h), and the kernel's
decode rule on the plane giving the bf16 matrix back bit for bit."""
import ctypes

import numpy as np
import pytest

from vox_weights import synth_lib

REC = 416  # dwords per (16-row group, 64-k block)


def _matrix(N, K, lo, seed):
    """bf16 bits [N, K]: exponents lo .. lo + 29 (both ends of the window), one weight in 8 a zero of either sign"""
    rng = np.random.default_rng(seed)
    e = rng.integers(lo, lo + 30, size=(N, K))
    e[0, :2] = (lo, lo + 29)
    w = (rng.integers(0, 2, size=(N, K)) << 15) | (e << 7) | rng.integers(0, 128, size=(N, K))
    w[rng.integers(0, 8, size=(N, K)) == 0] &= 0x8000
    w[0, :2] |= e[0, :2] << 7
    return w.astype(np.uint16)


def _lanes(a, N, K):
    """[N, K] -> [group, block, lane, 16]: (row n, col k) is weight r & 15 of lane (r >> 4) * 16 + (n & 15) of block
    k >> 6, r = k & 63 (half (r >> 3) & 1, element r & 7 of frag_off)"""
    return a.reshape(N // 16, 16, K // 64, 4, 16).transpose(0, 2, 3, 1, 4).reshape(N // 16, K // 64, 64, 16)


def _plane(w, D):
    N, K = w.shape
    c = w.astype(np.int64)
    e, s = (c >> 7) & 0xff, _lanes((c >> 15).astype(np.uint32), N, K)
    low = _lanes(np.where(e == 0, 0, ((e - 112 - D) << 7) | (c & 0x7f)).astype(np.uint32), N, K)
    d = []
    for p in range(6):
        t, sh = 12 + 2 * (p // 3), 4 * (p % 3)
        d.append(low[..., 2 * p] | ((low[..., t] >> sh) & 15) << 12 | low[..., 2 * p + 1] << 16 | ((low[..., t + 1] >> sh) & 15) << 28)
    sg = sum(s[..., 2 * p] << p | s[..., 2 * p + 1] << (8 + p) for p in range(8))
    rec = np.zeros(low.shape[:2] + (REC,), np.uint32)
    rec[..., :256] = np.stack(d[:4], -1).reshape(low.shape[:2] + (256,))
    rec[..., 256:384] = np.stack(d[4:], -1).reshape(low.shape[:2] + (128,))
    rec[..., 384:] = sg[..., 0::2] | sg[..., 1::2] << 16
    return rec.reshape(-1)


def _decode(plane, N, K, D):
    """the kernel's rule: bits = s << 15 | (low + ((112 + D) << 7)), or s << 15 when low is 0"""
    rec = plane.reshape(N // 16, K // 64, REC)
    d = np.concatenate([rec[..., :256].reshape(rec.shape[:2] + (64, 4)), rec[..., 256:384].reshape(rec.shape[:2] + (64, 2))], -1)
    sg = np.stack([rec[..., 384:] & 0xffff, rec[..., 384:] >> 16], -1).reshape(rec.shape[:2] + (64,))
    low = np.zeros(rec.shape[:2] + (64, 16), np.uint32)
    low[..., 0:12:2], low[..., 1:12:2] = d & 0xfff, (d >> 16) & 0xfff
    for h in range(2):
        nib = (d >> (12 + 16 * h)) & 15
        low[..., 12 + h] = nib[..., 0] | nib[..., 1] << 4 | nib[..., 2] << 8
        low[..., 14 + h] = nib[..., 3] | nib[..., 4] << 4 | nib[..., 5] << 8
    i = np.arange(16)
    s = (sg[..., None] >> (i // 2 + 8 * (i % 2))) & 1
    bits = s << 15 | np.where(low != 0, low + ((112 + D) << 7), 0)
    return bits.reshape(N // 16, K // 64, 4, 16, 16).transpose(0, 3, 1, 2, 4).reshape(N, K).astype(np.uint16)


@pytest.mark.parametrize("lo", [90, 120])
@pytest.mark.parametrize("N,K", [(16, 64), (48, 256), (768, 1280)])
def test_frag_layout(N, K, lo):
    L = synth_lib()
    L.vox_wpack13_frag_words_of.restype = ctypes.c_longlong
    w = _matrix(N, K, lo, seed=N + K + lo)
    emin, emax, D = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.vox_wpack13_scan(ctypes.c_void_p(w.ctypes.data), ctypes.c_size_t(w.size), *map(ctypes.byref, (emin, emax, D))) == 1
    assert (emin.value, emax.value) == (lo, lo + 29) and (D.value < 0) == (lo == 90) and D.value != 0
    words = L.vox_wpack13_frag_words_of(ctypes.c_longlong(N), ctypes.c_longlong(K))
    assert words * 32 == N * K * 13 and L.vox_wpack13_frag_words_of(ctypes.c_longlong(N + 8), ctypes.c_longlong(K)) == 0
    out = np.zeros(words, np.uint32)
    L.vox_wpack13_frag_layout(ctypes.c_void_p(w.ctypes.data), ctypes.c_longlong(N), ctypes.c_longlong(K), D,
                              ctypes.c_void_p(out.ctypes.data))
    assert np.array_equal(out, _plane(w, D.value))
    assert np.array_equal(_decode(out, N, K, D.value), w) and (w == 0x8000).any() and (w == 0).any()
