"""The encoder's attention over IEEE-half K/V rings on the f16 matrix pipe (k_attn_rows_mf16).

Both kernels against numpy float64 at ACT_TOL = 5e-5 of max |out| per (query, head) row (measured on
an MI355X: worst 0.132 of the bar, default kernel 0.160); the instruction's treatment of subnormal
f16 inputs; the engine's paths and the batched pass under tests/test_gpu_enc_kv16.py's
ring-conditioned replay; the switch.  Fails without the feature: vox_hip.enc_attn_kv16 does not exist."""
import ctypes

import numpy as np
import pytest

import test_gpu_enc_kv16 as E
from test_gpu_enc_attn_mf8 import CASES
from test_gpu_enc_kv16 import ACT_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def pristine(tiny_cfg, tiny_weights):
    """Before the first test, the switch never set: off, a half stream's passes count nothing; the smoke
    run is kept for the last test.  The borrowed helpers mark their module's setter flag: put back."""
    import vox_hip
    flag = E._SETTER_CALLED
    hm = vox_hip.Model(tiny_cfg, tiny_weights)
    assert vox_hip.enc_attn_mf16() == 0 and vox_hip.enc_attn_mf16_stats() == 0
    out = E._smoke_run(hm, tiny_cfg)
    s = E._stream(hm, True)
    s.encode_mel(E._mel(tiny_cfg, 8000, 100))
    s.close()
    hm.close()
    assert vox_hip.enc_attn_mf16_stats() == 0
    yield out
    vox_hip.set_enc_attn_mf16(False)
    E._SETTER_CALLED = flag


@pytest.fixture(scope="module")
def models(tiny_cfg, tiny_weights):
    import vox_hip
    from vox_weights import TINY_LONG
    ms = {"TINY": (vox_hip.Model(tiny_cfg, tiny_weights), tiny_cfg),
          "TINY_LONG": (vox_hip.Model(TINY_LONG, tiny_weights), TINY_LONG)}
    yield ms
    for hm, _ in ms.values():
        hm.close()


@pytest.fixture
def switch_on():
    import vox_hip
    vox_hip.set_enc_attn_mf16(True)
    yield
    vox_hip.set_enc_attn_mf16(False)


@pytest.mark.parametrize("heads", [(2, 2), (4, 2)])
@pytest.mark.parametrize("case", CASES)
def test_kernel_against_float64(case, heads):
    """Query rows over 16 binades, one of them zero; rings with zeros, subnormals and V outliers.  Every
    ring slot outside the call's key range holds the half NaN: reading one turns a row NaN."""
    import vox_hip
    (M, q_pos0, window, cap, use_splits), (H, KVH) = case, heads
    rng = np.random.default_rng(100 * M + H)
    lo, hi = max(0, q_pos0 - window + 1), q_pos0 + M - 1
    n = hi - lo + 1
    Q = (rng.standard_normal((M, H * 64)) * 2.0 ** rng.integers(-12, 4, (M, 1))).astype(np.float32)
    if M == 25 and not use_splits:
        Q[7] = 0
    kv = (1.5 * rng.standard_normal((2, n, KVH * 64))).astype(np.float16)
    kv[1][rng.random(kv[1].shape) < 0.01] *= np.float16(1024)
    bits = kv.view(np.uint16)
    bits[rng.random(bits.shape) < 0.02] = 0
    sub = rng.random(bits.shape) < 0.02
    bits[sub] = rng.integers(1, 1024, int(sub.sum())) | rng.choice([0, 0x8000], int(sub.sum()))
    rings = np.full((2, cap, KVH * 64), 0x7e00, np.uint16)
    rings[:, np.arange(lo, hi + 1) % cap] = bits
    K, V = bits.view(np.float16).astype(np.float64).reshape(2, n, KVH, 64)
    qp, kp = q_pos0 + np.arange(M)[:, None], lo + np.arange(n)[None, :]
    seen = (kp <= qp) & (kp >= qp - window + 1)
    ref = np.empty((M, H, 64))
    for h in range(H):
        s = np.where(seen, Q[:, h * 64:(h + 1) * 64].astype(np.float64) @ K[:, h // (H // KVH)].T * 0.125, -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        ref[:, h] = (p / p.sum(axis=1, keepdims=True)) @ V[:, h // (H // KVH)]
    bar = ACT_TOL * np.max(np.abs(ref), axis=2, keepdims=True)
    d = []
    for mf16 in (False, True):
        got = vox_hip.enc_attn_kv16(Q, rings[0], rings[1], H, KVH, 0.125, window, q_pos0, use_splits, mf16).reshape(M, H, 64)
        assert np.all(np.isfinite(got)), f"mf16 {mf16}: a slot outside the key range was read"
        d.append(float(np.max(np.abs(got - ref) / bar)))
    print(f"case {case} H {H} KVH {KVH}: distance / bar: default kernel {d[0]:.4f}, mf16 {d[1]:.4f}")
    assert d[0] < 1.0 and d[1] < 1.0, d


def test_mfma_keeps_subnormal_f16_inputs():
    """All 2046 subnormal half codes against 1.0, 2^14 and the neighbouring code, in either operand, plus
    64 pairs of normals: every product equals the float64 product rounded to f32 (exact there)."""
    import vox_hip
    sub = np.concatenate([np.arange(1, 1024), 0x8000 | np.arange(1, 1024)]).astype(np.uint16)
    nrm = np.random.default_rng(8100).standard_normal((2, 64)).astype(np.float16).view(np.uint16)
    a = np.concatenate([sub, sub, sub, nrm[0]])
    b = np.concatenate([np.full(2046, 0x3c00, np.uint16), np.full(2046, 0x7000, np.uint16), np.roll(sub, 1), nrm[1]])
    for x, y in ((a, b), (b, a)):
        want = (x.view(np.float16).astype(np.float64) * y.view(np.float16).astype(np.float64)).astype(np.float32)
        got = vox_hip.enc_attn_mf16_probe(x, y)
        bad = got.view(np.uint32) != want.view(np.uint32)
        print(f"probe: {x.size} products, {int(bad.sum())} differ from the exact product")
        assert not bad.any(), (x[bad][:4], y[bad][:4], got[bad][:4], want[bad][:4])


def _replayed(hm, cfg, weights, seed, sizes):
    """E._ring_conditioned; every pass it took is one counted attention launch per layer"""
    import vox_hip
    n0 = vox_hip.enc_attn_mf16_stats()
    r, _, s = E._ring_conditioned(hm, cfg, weights, E._mel(cfg, seed, sum(sizes)), sizes)
    took = s.enc_paths()
    s.close()
    passes = sum(v for k, v in took.items() if k != "fused_split")
    assert vox_hip.enc_attn_mf16_stats() - n0 == cfg.enc_layers * passes > 0, (took, n0)
    print(f"ring-conditioned half + enc_attn_mf16 {sizes}: adapter rows rel {r:.2e}")
    assert r < ACT_TOL, r
    return took


@pytest.mark.parametrize("name", ["gemm_200_rows", "one_row_chunks", "split_grid_and_combine"])
def test_engine_paths_ring_conditioned(models, tiny_weights, switch_on, name):
    cfg_name, sizes, passes = E.PATHS[name]
    hm, cfg = models[cfg_name]
    assert _replayed(hm, cfg, tiny_weights, 8200 + len(sizes), sizes) == {**E.NO_PASSES, **passes}


def test_batched_pass_of_half_streams(models, switch_on):
    """4 half streams, ragged rounds, encode_mel_batch against the same chunks one stream at a time"""
    import enc_kv_ref
    import vox_hip
    hm, cfg = models["TINY"]
    mels = [E._mel(cfg, 8300 + i, sum(r[i] for r in E.ROUNDS)) for i in range(4)]
    bs, ss = [E._stream(hm, True) for _ in range(4)], [E._stream(hm, True) for _ in range(4)]
    offs, batched = [0] * 4, 0
    for r in E.ROUNDS:
        chunk = [mels[i][offs[i]:offs[i] + r[i]] for i in range(4)]
        n0 = vox_hip.enc_attn_mf16_stats()
        added = vox_hip.encode_mel_batch(bs, chunk)
        batched += vox_hip.enc_attn_mf16_stats() - n0
        assert added == [ss[i].encode_mel(chunk[i]) if r[i] else 0 for i in range(4)]
        offs = [o + n for o, n in zip(offs, r)]
    assert batched >= cfg.enc_layers * len(E.ROUNDS), batched
    for i in range(4):
        a, b = bs[i].read_adapter(), ss[i].read_adapter()
        assert a.shape == b.shape and a.shape[0] > 0 and enc_kv_ref.rel(a, b) < ACT_TOL, i
    for s in bs + ss:
        s.close()


@pytest.mark.parametrize("dtype", [0, 2])
def test_other_ring_types_are_bit_equal_under_the_switch(models, dtype):
    """f32 (0) and FP8 (2) encoder rings"""
    import vox_hip
    hm, cfg = models["TINY"]
    out = []
    for on in (False, True):
        vox_hip.set_enc_attn_mf16(on)
        n0 = vox_hip.enc_attn_mf16_stats()
        hm.set_enc_kv_dtype(dtype)
        s = vox_hip.Stream(hm)
        hm.set_enc_kv_dtype(0)
        assert s.enc_kv_dtype == dtype
        for p in (E._mel(cfg, 8400, 400), E._mel(cfg, 8401, 50), E._mel(cfg, 8402, 2)):
            s.encode_mel(p)
        out.append(s.read_adapter())
        s.close()
        assert vox_hip.enc_attn_mf16_stats() == n0
    vox_hip.set_enc_attn_mf16(False)
    assert np.array_equal(out[0], out[1])


def test_setter_is_refused_inside_a_begun_call(models):
    import vox_hip
    hm, cfg = models["TINY"]
    ss = [E._stream(hm, True) for _ in range(2)]
    for i, s in enumerate(ss):
        s.encode_mel(E._mel(cfg, 8500 + i, 400))
    b, L, IP = vox_hip.Batch(hm, 4), vox_hip.lib(), ctypes.POINTER(ctypes.c_int)
    arr = (ctypes.c_void_p * 2)(*[s.h for s in ss])
    rows = np.array([s.adapter_tokens for s in ss], np.int32)
    toks, cnt = np.zeros((2, 2), np.int32), np.zeros(2, np.int32)
    assert L.vox_hip_batch_begin_rows(b.h, arr, 2, rows.ctypes.data_as(IP), 2, 0, toks.ctypes.data_as(IP),
                                      cnt.ctypes.data_as(IP)) == 0, L.vox_hip_last_error()
    with pytest.raises(RuntimeError, match="begun"):
        vox_hip.set_enc_attn_mf16(True)
    assert L.vox_hip_batch_finish(b.h) >= 0 and vox_hip.enc_attn_mf16() == 0
    b.close()
    for s in ss:
        s.close()


def test_default_is_untouched_after_on_and_off(pristine, models, tiny_cfg):
    import vox_hip
    rows0, ids0 = pristine
    vox_hip.set_enc_attn_mf16(True)
    vox_hip.set_enc_attn_mf16(False)
    n0 = vox_hip.enc_attn_mf16_stats()
    rows, ids = E._smoke_run(models["TINY"][0], tiny_cfg)
    assert np.array_equal(rows, rows0) and np.array_equal(ids, ids0) and vox_hip.enc_attn_mf16_stats() == n0
