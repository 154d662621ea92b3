"""CPU: wpack13 (csrc/vox_wpack.h) -- the lossless 13-bit storage of a bf16 weight tensor that
the single-stream decode GEMV streams: window scan, choice of D, pack, unpack and the side
plane's layout, through the exports of libvox_synth.so.

A packable tensor's nonzero bf16 exponent fields span at most 29 (30 binades) with no Inf /
NaN and no nonzero subnormal; every weight is then h * 2^D with h an IEEE-half normal (or
+-0), D the value of [Emax - 142, Emin - 113] nearest 0, and |D| <= 40.
"""
import ctypes

import numpy as np
import pytest

from vox_weights import synth_lib

pytestmark = pytest.mark.cpu

KS = (64, 72)   # chunks per row 8 and 9: a row is never a multiple of the kernel's 256 chunks


def _lib():
    L = synth_lib()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    ip = ctypes.POINTER(ctypes.c_int)
    L.vox_wpack13_scan.restype = I
    L.vox_wpack13_scan.argtypes = [P, ctypes.c_size_t, ip, ip, ip]
    L.vox_wpack13_pack.restype = None
    L.vox_wpack13_pack.argtypes = [P, LL, LL, I, P, P]
    L.vox_wpack13_unpack.restype = None
    L.vox_wpack13_unpack.argtypes = [P, P, LL, LL, I, P]
    L.vox_wpack13_side_words_of.restype = I
    L.vox_wpack13_side_words_of.argtypes = [LL, I]
    L.vox_wpack13_side_layout.restype = None
    L.vox_wpack13_side_layout.argtypes = [P, LL, LL, I, I, P]
    return L


def scan(w):
    w = np.ascontiguousarray(w, np.uint16)
    lo, hi, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ok = _lib().vox_wpack13_scan(w.ctypes.data, w.size, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(d))
    return bool(ok), lo.value, hi.value, d.value


def pack(w, d):
    w = np.ascontiguousarray(w, np.uint16)
    rows, K = w.shape
    main = np.zeros((rows, K // 8, 3), np.uint32)
    side = np.zeros((rows, K // 8), np.uint8)
    _lib().vox_wpack13_pack(w.ctypes.data, rows, K, d, main.ctypes.data, side.ctypes.data)
    return main, side


def unpack(main, side, d):
    rows, kc, _ = main.shape
    out = np.zeros((rows, kc * 8), np.uint16)
    _lib().vox_wpack13_unpack(main.ctypes.data, side.ctypes.data, rows, kc * 8, d, out.ctypes.data)
    return out


def bf16(e, m=0, s=0):
    """bf16 bits from exponent field, mantissa, sign"""
    return np.uint16(s << 15 | e << 7 | m)


def synth(rows, K, seed=3):
    out = np.zeros((rows, K), np.uint16)
    synth_lib().vox_synth_bf16(ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(out.size), ctypes.c_uint64(seed),
                               ctypes.c_float(1.0 / np.sqrt(3072.0)), ctypes.c_float(0.0))
    return out


def span_tensor(rows, K, emin, emax, seed=5):
    """random signs / mantissas, exponent fields uniform in [emin, emax] with both ends present"""
    rng = np.random.default_rng(seed)
    e = rng.integers(emin, emax + 1, size=(rows, K))
    e.flat[0], e.flat[-1] = emin, emax
    m = rng.integers(0, 128, size=(rows, K))
    s = rng.integers(0, 2, size=(rows, K))
    return (s << 15 | e << 7 | m).astype(np.uint16)


def roundtrip(w):
    ok, lo, hi, d = scan(w)
    assert ok, (lo, hi, d)
    main, side = pack(w, d)
    assert np.array_equal(unpack(main, side, d), w)
    return main, side, d


@pytest.mark.parametrize("K", KS)
def test_roundtrip_synth(K):
    w = synth(48, K)
    _, _, d = roundtrip(w)
    assert -40 <= d <= 0


@pytest.mark.parametrize("K", KS)
def test_roundtrip_signed_zeros(K):
    w = synth(16, K, seed=9)
    rng = np.random.default_rng(1)
    z = rng.random(w.shape) < 0.2
    w[z] = np.where(rng.random(int(z.sum())) < 0.5, 0x0000, 0x8000).astype(np.uint16)
    assert (w == 0x8000).any() and (w == 0).any()
    roundtrip(w)
    roundtrip(np.zeros((2, K), np.uint16))  # all zero: packable, D = 0
    assert scan(np.zeros((2, K), np.uint16)) == (True, 0, 0, 0)


@pytest.mark.parametrize("K", KS)
def test_roundtrip_span_29(K):
    w = span_tensor(8, K, 100, 129)
    ok, lo, hi, d = scan(w)
    assert (ok, lo, hi) == (True, 100, 129)
    assert d == -13   # the interval [129 - 142, 100 - 113] is the single value -13
    main, side, _ = roundtrip(w)
    # every stored half is a normal (exponent 1..30) with zero low mantissa bits once masked
    h = np.concatenate([(main & 0xfff8).ravel(), (main >> 16 & 0xfff8).ravel()])
    e5 = h >> 10 & 0x1f
    assert e5.min() >= 1 and e5.max() <= 30


@pytest.mark.parametrize("K", KS)
def test_roundtrip_single_row(K):
    roundtrip(synth(1, K, seed=11))
    roundtrip(span_tensor(1, K, 90, 119))


def test_window_rule():
    base = span_tensor(4, 64, 100, 129)
    w = base.copy()
    w[1, 3] = bf16(130)                 # 30 binades' span
    assert scan(w)[0] is False
    w = base.copy()
    w[2, 5] = bf16(0, 1)                # nonzero subnormal
    assert scan(w)[0] is False
    w = base.copy()
    w[0, 7] = bf16(255, 0, 1)           # -Inf
    assert scan(w)[0] is False
    w = base.copy()
    w[0, 7] = bf16(255, 5)              # NaN
    assert scan(w)[0] is False


@pytest.mark.parametrize("emin,emax,want", [
    (100, 120, -13),     # [-22, -13]: 0 is above the interval
    (120, 140, 0),       # [-2, 7] holds 0
    (150, 160, 18),      # [18, 37]: 0 is below
    (60, 80, -53),       # [-62, -53]: |D| > 40
    (190, 200, 58),      # [58, 77]: |D| > 40
    (73, 73, -40),       # the last packable D on the small side
    (72, 72, -41),
    (182, 182, 40),
    (183, 183, 41),
])
def test_choice_of_d(emin, emax, want):
    ok, lo, hi, d = scan(span_tensor(2, 64, emin, emax))
    assert (lo, hi, d) == (emin, emax, want)
    assert ok == (abs(want) <= 40)
    assert emax - 142 <= d <= emin - 113


def np_pack(w, d):
    """the format restated in numpy (csrc/vox_wpack.h, top comment)"""
    w = w.astype(np.uint32)
    s, e, m = w >> 15, w >> 7 & 0xff, w & 0x7f
    code = np.where(e == 0, s << 12, s << 12 | ((e.astype(np.int64) - 112 - d) << 7).astype(np.uint32) | m)
    c = code.reshape(w.shape[0], -1, 8)
    main = np.zeros(c.shape[:2] + (3,), np.uint32)
    for p in range(3):
        main[..., p] = (c[..., 2 * p] << 3 | c[..., 2 * p + 1] << 19 | (c[..., 6] >> (3 * p) & 7)
                        | (c[..., 7] >> (3 * p) & 7) << 16)
    side = (c[..., 6] >> 9 | (c[..., 7] >> 9) << 4).astype(np.uint8)
    return main, side


def np_side_layout(side, K, rb, swiglu):
    rows, kc = side.shape
    kq = (kc + 255) // 256
    sw = (kq * rb + 3) // 4
    out = np.zeros((rows // rb, 256, sw), np.uint32)
    for g in range(rows // rb):
        for i in range(rb):
            if swiglu:
                u = g * (rb // 2) + (i >> 1)
                row = ((u >> 4) << 5) + (u & 15) + ((i & 1) << 4)
            else:
                row = g * rb + i
            for j in range(kq):
                t = np.arange(256)
                c = (j * 4 + t // 64) * 64 + t % 64
                b = side[row, np.where(c < kc, c, 0)].astype(np.uint32)
                slot = j * rb + i
                q = slot & 3
                out[g, :, slot >> 2] |= (b & 15) << (12 - 4 * q) | (b >> 4) << (28 - 4 * q)
    return out


def test_numpy_restatement_matches_c_packer():
    w = synth(64, 72, seed=21)
    w[3, 8:16] = [0, 0x8000, bf16(122, 127), bf16(122, 127, 1), bf16(99), bf16(99, 1, 1), 0x8000, 0]
    ok, _, _, d = scan(w)
    assert ok
    main, side = pack(w, d)
    nmain, nside = np_pack(w, d)
    assert main.tobytes() == nmain.tobytes()
    assert side.tobytes() == nside.tobytes()
    # the side plane as the kernel reads it: plain 2-row groups, 4-row SwiGLU pairs, and a row
    # of 4 * 256 + 128 chunks (ragged last round of five, like W2)
    for rows, K, rb, swiglu in ((64, 72, 2, 0), (64, 72, 4, 1), (4, 8 * (4 * 256 + 128), 2, 0)):
        ww = synth(rows, K, seed=23)
        _, sd = pack(ww, scan(ww)[3])
        sw = _lib().vox_wpack13_side_words_of(K, rb)
        out = np.zeros((rows // rb, 256, sw), np.uint32)
        _lib().vox_wpack13_side_layout(sd.ctypes.data, rows, K, rb, swiglu, out.ctypes.data)
        assert out.tobytes() == np_side_layout(sd, K, rb, swiglu).tobytes()
