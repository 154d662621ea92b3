"""CPU: the wmx4 format (csrc/vox_wmx4.h, through libvox_synth.so) -- the MXFP4 rounding against
an independent numpy restatement of the rule, the scan, pack / unpack, the device plane layout
against a direct restatement of its index formula -- and the margin precondition of every id
comparison tests/test_gpu_wmx4.py makes.

Margin rule (tests/test_batch_gemv_cpu.py's): an id comparison against the oracle only means
something where the oracle's own top-2 gap exceeds what the logit tolerance allows, so on the
oracle alone, on the rounded weights, every compared step keeps (top1 - top2) / max|logit| of
at least 4x the logit bar (2e-4 for f32 rings, 4e-4 for fp16 rings).  The worst gap of each
case is printed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_wmx4 as g  # noqa: E402  (the cases, the configs and the oracle sessions; nothing runs on a GPU)

from vox_weights import f32_to_bf16, mxfp4_round, synth_lib  # noqa: E402

pytestmark = pytest.mark.cpu
NAMES = ["vox_hip_set_wmx4", "vox_hip_wmx4", "vox_hip_model_wmx4_stats"]


def test_header_library_and_binding_have_the_names():
    import vox_hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voxtral_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in vox_hip.EXPORTS, n
    assert callable(vox_hip.set_wmx4) and callable(vox_hip.wmx4) and callable(vox_hip.Model.wmx4_stats)


# ---- the rule, restated in numpy on float64 values -------------------------------------------
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _val(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _ref_round(bits):
    """the rule of the issue on a [rows, K] tensor of finite, normal-or-zero bf16 (K % 32 == 0):
    e = floor(log2(amax)) - 2 per block of 32; v / 2^e to the nearest of E2M1, ties to the even
    code, saturating at 6; signs kept (of zeros too); back to bf16 bits (exact)"""
    bits = np.asarray(bits, np.uint16)
    rows, K = bits.shape
    v = _val(bits).reshape(rows, K // 32, 32)
    sign = (bits >> 15).reshape(v.shape).astype(np.uint16)
    amax = np.abs(v).max(axis=2, keepdims=True)
    e = np.where(amax > 0, np.floor(np.log2(np.where(amax > 0, amax, 1.0))) - 2, 0.0)
    q = np.abs(v) / np.exp2(e)
    # nearest code: distances to the 8 values (exact in float64); a tie has two neighbouring
    # candidates lo and lo + 1, of which the even one is taken
    d = np.abs(q[..., None] - E2M1)
    cand = d == d.min(axis=-1, keepdims=True)
    lo = np.argmax(cand, axis=-1)
    code = np.where((cand.sum(axis=-1) > 1) & (lo % 2 == 1), lo + 1, lo)
    code = np.where(q > 6.0, 7, code)
    out = E2M1[code] * np.exp2(e)
    ob = f32_to_bf16(out.astype(np.float32))
    assert np.array_equal(_val(ob), out.reshape(ob.shape))     # every MXFP4 value is a bf16
    return (ob | (sign << 15)).reshape(rows, K)


def _rand_bf16(rows, K, seed, std=0.05):
    out = np.zeros((rows, K), np.uint16)
    synth_lib().vox_synth_bf16(ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(out.size), ctypes.c_uint64(seed),
                               ctypes.c_float(std), ctypes.c_float(0.0))
    return out


def _scan(w):
    w = np.ascontiguousarray(w, np.uint16)
    return synth_lib().vox_wmx4_scan(w.ctypes.data, w.shape[0], w.shape[1])


def _bf(x):
    return f32_to_bf16(np.asarray(x, np.float32))


def _special():
    """[rows, 64]: blocks with amax in (6, 8) 2^e, exact ties, all-zero blocks, negative zeros"""
    rng = np.random.default_rng(7)
    rows = []
    for e in (-9, -3, 0, 5):
        s = 2.0 ** e
        # saturation: amax 7 and 7.5 (in (6, 8)); ties at every midpoint, both signs
        ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
        a = np.concatenate([[7.0], ties, -ties, [0.0, -0.0, 6.5, -7.75, 0.125, 0.26, 0.24, 4.0, 6.0, 3.0],
                            rng.uniform(-7.9, 7.9, 7)])
        b = np.concatenate([[7.5, -6.25], ties * 0.5, rng.uniform(-1, 1, 23)])     # amax 7.5, then small values
        rows.append(np.concatenate([a, b]) * s)
    rows.append(np.zeros(64))                                    # all-zero blocks
    z = np.zeros(64)
    z[::3] = -0.0
    rows.append(z)                                               # zeros of both signs
    m = np.concatenate([np.copysign(0.0, -1.0) * np.ones(32), rng.uniform(-1, 1, 32)])
    rows.append(m)
    w = _bf(np.stack(rows))
    assert ((w == 0x8000).sum() > 30) and (w == 0).sum() > 60
    return w


def test_round_matches_the_rule_bits():
    for seed, (rows, K) in enumerate([(64, 128), (33, 736), (8, 9216)]):
        w = _rand_bf16(rows, K, seed + 11, std=(0.02, 1.0, 30.0)[seed])
        w[1, ::7] = 0x8000
        w[2, :40] = 0
        assert np.array_equal(mxfp4_round(w), _ref_round(w)), (rows, K)
    w = _special()
    got, ref = mxfp4_round(w), _ref_round(w)
    assert np.array_equal(got, ref)
    # the special cases do what their names say: 7 and 7.5 saturate to 6, ties go to the even code
    v, r = _val(w), _val(got)
    assert r[2, 0] == 6.0 and r[2, 32] == 6.0 and r[2, 33] == -6.0
    assert list(r[2, 1:8]) == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0] and list(r[2, 8:15]) == [-0.0, -1.0, -1.0, -2.0, -2.0, -4.0, -4.0]
    assert (got[4] == 0).all() and np.array_equal(got[5], w[5]) and (got[6, :32] == 0x8000).all()
    assert np.array_equal(np.signbit(r), np.signbit(v))          # no sign is lost, of zeros either


def test_round_is_idempotent_and_scans():
    for seed, (rows, K) in enumerate([(64, 128), (16, 3072)]):
        r1 = mxfp4_round(_rand_bf16(rows, K, seed + 3))
        assert np.array_equal(mxfp4_round(r1), r1)
        assert _scan(r1) == 1
    s = mxfp4_round(_special())
    assert np.array_equal(mxfp4_round(s), s) and _scan(s) == 1


def test_scan_refuses():
    assert _scan(_rand_bf16(64, 128, 5)) == 0                    # an ordinary bf16 tensor
    ok = mxfp4_round(_rand_bf16(4, 96, 6))
    assert _scan(ok) == 1
    assert _scan(mxfp4_round(_rand_bf16(4, 72, 6))) == 0         # K % 32 != 0
    w = ok.copy()
    w[1, 32:64] = 0
    w[1, 40], w[1, 41] = _bf([6.0])[0], _bf([0.25])[0]          # 6 and 0.25: e = 0, 0.25 is below 0.5
    assert _scan(w) == 0
    w[1, 41] = _bf([0.5])[0]
    assert _scan(w) == 1
    for bad in (0x7f80, 0xff80, 0x7fc0, 0x0001, 0x807f):         # Inf, -Inf, NaN, subnormals
        w = ok.copy()
        w[3, 95] = bad
        assert _scan(w) == 0, hex(bad)
    # the exponent window: |e| <= 64
    for e, want in ((64, 1), (65, 0), (-64, 1), (-65, 0)):
        w = ok.copy()
        w[2, 0:32] = _bf(np.array([4.0, 6.0, -0.5, 0.0] * 8) * 2.0 ** e)
        assert _scan(w) == want, e


def _pack(w):
    rows, K = w.shape
    nib, scl = np.zeros((rows, K // 8), np.uint32), np.zeros((rows, K // 32), np.uint8)
    synth_lib().vox_wmx4_pack(w.ctypes.data, rows, K, nib.ctypes.data, scl.ctypes.data)
    return nib, scl


@pytest.mark.parametrize("K", [64, 72 * 8])
def test_pack_unpack_roundtrip(K):
    w = mxfp4_round(_rand_bf16(24, K, K))
    w[1, ::7] = 0x8000
    w[2, :32] = 0
    w = mxfp4_round(w)
    nib, scl = _pack(w)
    # the compact form as documented: weight k of a chunk in bits 4 (k % 8).., scale byte e + 127
    v = _val(w).reshape(24, K // 32, 32)
    amax = np.abs(v).max(axis=2)
    e = np.where(amax > 0, np.floor(np.log2(np.where(amax > 0, amax, 1.0))) - 2, 0)
    assert np.array_equal(scl, (e + 127).astype(np.uint8))
    codes = (nib[:, :, None] >> (4 * np.arange(8, dtype=np.uint32))) & 15
    dec = E2M1[codes & 7] * np.where(codes & 8, -1.0, 1.0) * np.exp2(np.repeat(e, 4, axis=1))[:, :, None]
    assert np.array_equal(dec.reshape(24, K), _val(w))
    back = np.zeros_like(w)
    synth_lib().vox_wmx4_unpack(nib.ctypes.data, scl.ctypes.data, 24, K, back.ctypes.data)
    assert np.array_equal(back, w)


@pytest.mark.parametrize("rb,swiglu,K", [(2, 0, 64), (4, 0, 576), (8, 0, 64), (4, 1, 96), (2, 1, 64)])
def test_plane_layout(rb, swiglu, K):
    """record (g, c) at dword (g * K / 8 + c) * RW, RW = rb + ceil(rb / 4): dwords 0 .. rb - 1
    the nibble dwords of chunk c of the group's rows, then their blocks' scale bytes"""
    rows = 64
    w = mxfp4_round(_rand_bf16(rows, K, 100 + rb + K))
    nib, scl = _pack(w)
    rw = rb + (rb + 3) // 4
    words = synth_lib().vox_wmx4_plane_words_of(rows, K, rb)
    assert words == rows // rb * (K // 8) * rw
    out = np.full(words + 8, 0xdeadbeef, np.uint32)
    synth_lib().vox_wmx4_plane_layout(nib.ctypes.data, scl.ctypes.data, rows, K, rb, swiglu, out.ctypes.data)
    assert (out[words:] == 0xdeadbeef).all()
    want = np.zeros(words, np.uint32)
    for gq in range(rows // rb):
        for c in range(K // 8):
            base = (gq * (K // 8) + c) * rw
            for i in range(rb):
                if swiglu:
                    u = gq * (rb // 2) + (i >> 1)
                    r = ((u >> 4) << 5) + (u & 15) + ((i & 1) << 4)
                else:
                    r = gq * rb + i
                want[base + i] = nib[r, c]
                want[base + rb + i // 4] |= np.uint32(int(scl[r, c // 4]) << (8 * (i % 4)))
    assert np.array_equal(out[:words], want)


def test_quantize_mxfp4_rounds_the_decode_matrices_only(tiny_weights):
    from vox_weights import mxfp4_tensor_names, quantize_mxfp4
    q = quantize_mxfp4(tiny_weights)
    names = set(mxfp4_tensor_names(tiny_weights.cfg))
    assert len(names) == 7 * tiny_weights.cfg.dec_layers + 1
    for n, a in tiny_weights.t.items():
        if n in names:
            assert _scan(q.t[n]) == 1 and _scan(a) == 0, n
            assert np.array_equal(q.t[n], _ref_round(a)), n
        else:
            assert q.t[n] is a, n


# ---- the margin precondition of the GPU file's id comparisons ----------------------------------
@pytest.mark.parametrize("case", sorted(g.ORACLE_RUNS))
def test_oracle_margin(case):
    cname, kv16 = g.ORACLE_RUNS[case]
    margin = g.MARGIN_KV16 if kv16 else g.MARGIN_F32
    ref = g._oracle(case)
    worst, steps = np.inf, 0
    for i, (ids, lg) in enumerate(ref):
        assert len(ids) == lg.shape[0] == g.STEPS, (case, i, len(ids))
        top = np.partition(lg, -2, axis=1)[:, -2:]
        gap = (top[:, 1] - top[:, 0]) / np.max(np.abs(lg), axis=1)
        assert np.array_equal(np.argmax(lg, axis=1), np.asarray(ids)), (case, i)
        k = int(np.argmin(gap))
        assert gap[k] >= margin, (case, i, k, float(gap[k]), margin)
        worst = min(worst, float(gap[k]))
        steps += len(ids)
    print(f"{case}: oracle top-2 gap on the rounded weights >= {worst:.2e} of the largest logit over {steps} "
          f"steps (rule: {margin:.0e})")
