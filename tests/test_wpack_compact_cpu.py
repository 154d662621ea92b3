"""CPU: the compact wpack13 side plane (csrc/vox_wpack.h) -- the layout the single-stream decode
GEMV reads for a tensor whose rows span more than one K round of 256 chunks and end inside the
last one: no slot for a (round, lane) without a chunk.  A numpy restatement of the layout is
compared byte for byte with the C function (libvox_synth.so); shapes with one round or whole
rounds must come out of it exactly as they come out of the padded layout's function.

The minimum a group's record can take with one dword-granular load per lane and section:
every lane holds the (KQ - 1) * rb slots of the whole rounds, ceil of that / 4 dwords, and each
of the NR = K / 8 - (KQ - 1) * 256 lanes with a chunk in the last round ceil(rb / 4) dwords
more.  Where rb is a multiple of 4 that is rows * K / 8 bytes per group's rb rows, one byte per
chunk: 13 bits per weight, 0.8125 of bf16.  With 2-row groups (W2) a last-round lane's dword is
half used: at most one spare dword per such lane above the byte minimum.
"""
import ctypes

import numpy as np
import pytest

from vox_weights import synth_lib

pytestmark = pytest.mark.cpu

# (K, rb, swiglu): QKV / W1|W3 (SwiGLU row pairs) / the LM head's 8-row groups at K = 3072
# (1.5 rounds), W2 (4.5 rounds, 2-row groups), and a last round of one wave
CASES = [(3072, 4, 0), (3072, 4, 1), (3072, 8, 0), (9216, 2, 0), (2560, 4, 0)]
ROWS = 64


def _lib():
    L = synth_lib()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.vox_wpack13_side_words_of.restype = I
    L.vox_wpack13_side_words_of.argtypes = [LL, I]
    L.vox_wpack13_side_layout.restype = None
    L.vox_wpack13_side_layout.argtypes = [P, LL, LL, I, I, P]
    L.vox_wpack13_side_compact_of.restype = I
    L.vox_wpack13_side_compact_of.argtypes = [LL, I]
    L.vox_wpack13_side_compact_group_words_of.restype = LL
    L.vox_wpack13_side_compact_group_words_of.argtypes = [LL, I]
    L.vox_wpack13_side_compact_layout.restype = None
    L.vox_wpack13_side_compact_layout.argtypes = [P, LL, LL, I, I, P]
    return L


def side_bytes(rows, K, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(rows, K // 8), dtype=np.uint8)


def np_row(g, i, rb, swiglu):
    if not swiglu:
        return g * rb + i
    u = g * (rb // 2) + (i >> 1)
    return ((u >> 4) << 5) + (u & 15) + ((i & 1) << 4)


def np_group_words(K, rb):
    kc = K // 8
    kq = (kc + 255) // 256
    nr = kc - (kq - 1) * 256
    return 256 * (((kq - 1) * rb + 3) // 4) + nr * ((rb + 3) // 4)


def np_compact_layout(side, K, rb, swiglu):
    """[groups][group words]: section A (256 lanes x the whole rounds' slots), then section B (the
    last round's lanes x rb slots); a dword holds slot s % 4 = q as the padded layout does"""
    rows, kc = side.shape
    kq = (kc + 255) // 256
    nr = kc - (kq - 1) * 256
    assert kq > 1 and nr < 256 and (kq - 1) * rb % 4 == 0
    swa, swb = (kq - 1) * rb // 4, (rb + 3) // 4
    out = np.zeros((rows // rb, 256 * swa + nr * swb), np.uint32)

    def put(dst, slot, b):
        q = slot & 3
        dst[slot >> 2] |= (int(b) & 15) << (12 - 4 * q) | (int(b) >> 4) << (28 - 4 * q)

    for g in range(rows // rb):
        for i in range(rb):
            row = np_row(g, i, rb, swiglu)
            for c in range(kc):
                j, t = divmod(c, 256)
                if j < kq - 1:
                    put(out[g, t * swa:(t + 1) * swa], j * rb + i, side[row, c])
                else:
                    put(out[g, 256 * swa + t * swb:256 * swa + (t + 1) * swb], i, side[row, c])
    return out


def c_compact_layout(side, K, rb, swiglu):
    rows = side.shape[0]
    gw = _lib().vox_wpack13_side_compact_group_words_of(K, rb)
    out = np.full((rows // rb, gw), 0xdeadbeef, np.uint32)
    _lib().vox_wpack13_side_compact_layout(side.ctypes.data, rows, K, rb, swiglu, out.ctypes.data)
    return out


def c_padded_layout(side, K, rb, swiglu):
    rows = side.shape[0]
    sw = _lib().vox_wpack13_side_words_of(K, rb)
    out = np.zeros((rows // rb, 256 * sw), np.uint32)
    _lib().vox_wpack13_side_layout(side.ctypes.data, rows, K, rb, swiglu, out.ctypes.data)
    return out


@pytest.mark.parametrize("K,rb,swiglu", CASES)
def test_compact_layout_matches_numpy_restatement(K, rb, swiglu):
    assert _lib().vox_wpack13_side_compact_of(K, rb) == 1
    side = side_bytes(ROWS, K, seed=K + rb + swiglu)
    got = c_compact_layout(side, K, rb, swiglu)
    assert got.tobytes() == np_compact_layout(side, K, rb, swiglu).tobytes()


@pytest.mark.parametrize("K,rb,swiglu", CASES)
def test_side_bytes_per_group_are_the_minimum(K, rb, swiglu):
    kc = K // 8
    kq = (kc + 255) // 256
    nr = kc - (kq - 1) * 256
    gw = _lib().vox_wpack13_side_compact_group_words_of(K, rb)
    assert gw == np_group_words(K, rb)
    floor = rb * kc            # one side byte per (row, chunk)
    if rb % 4 == 0:
        assert gw * 4 == floor
        # with the 12-byte main chunks: 13 bits per weight
        assert (gw * 4 + rb * kc * 12) * 16 == 13 * rb * K * 2
    else:
        assert floor < gw * 4 <= floor + 4 * nr
    assert gw < 256 * _lib().vox_wpack13_side_words_of(K, rb)


@pytest.mark.parametrize("K", [2048, 4096, 256, 8 * 100])
@pytest.mark.parametrize("rb,swiglu", [(2, 0), (4, 0), (4, 1), (8, 0)])
def test_one_round_and_whole_rounds_keep_the_padded_plane(K, rb, swiglu):
    assert _lib().vox_wpack13_side_compact_of(K, rb) == 0
    assert _lib().vox_wpack13_side_compact_group_words_of(K, rb) == 256 * _lib().vox_wpack13_side_words_of(K, rb)
    side = side_bytes(ROWS, K, seed=K + rb)
    assert c_compact_layout(side, K, rb, swiglu).tobytes() == c_padded_layout(side, K, rb, swiglu).tobytes()


def test_a_last_round_that_shares_a_dword_keeps_the_padded_plane():
    # 2-row groups at 1.5 rounds: the last round's two slots share the whole round's dword, and
    # a section of their own would take more bytes than the padding it removes
    K, rb = 3072, 2
    assert _lib().vox_wpack13_side_compact_of(K, rb) == 0
    side = side_bytes(ROWS, K, seed=5)
    assert c_compact_layout(side, K, rb, 0).tobytes() == c_padded_layout(side, K, rb, 0).tobytes()


@pytest.mark.parametrize("K,rb,swiglu", CASES)
def test_compact_plane_holds_the_padded_plane_s_slots(K, rb, swiglu):
    """what a thread's registers hold: section A then section B is the padded record, for every
    lane with a chunk in the last round; the others' section A is its leading dwords"""
    side = side_bytes(ROWS, K, seed=9)
    kc = K // 8
    kq = (kc + 255) // 256
    nr = kc - (kq - 1) * 256
    swa, swb = (kq - 1) * rb // 4, (rb + 3) // 4
    sw = _lib().vox_wpack13_side_words_of(K, rb)
    assert sw == swa + swb
    pad = c_padded_layout(side, K, rb, swiglu).reshape(ROWS // rb, 256, sw)
    cmp_ = c_compact_layout(side, K, rb, swiglu)
    a = cmp_[:, :256 * swa].reshape(ROWS // rb, 256, swa)
    b = cmp_[:, 256 * swa:].reshape(ROWS // rb, nr, swb)
    assert np.array_equal(a, pad[:, :, :swa])
    assert np.array_equal(b, pad[:, :nr, swa:])
