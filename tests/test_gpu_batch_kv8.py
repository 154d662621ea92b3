"""The batched decode step at the real model's head geometry (32 query / 8 kv heads) and with
more than one split-K slab, on configs small enough for the CPU oracle to follow in seconds.

TINY (4 / 2 heads, K = 256 and 512) never reaches several shipped branches of the step, and the
full-size batch test stops at 16 streams.  What selects a branch is the slot bucket, the kv head
count and the K / 64 factors of the decoder widths, not 4B-scale widths:

KV8 (dec_dim 768, DQ 4096, QKV width 6144, dec_hidden 1280), 17..32 slots (two 16-row blocks,
Z = 2), as read from skl_splits, skl_nw_for, launch_gemm_skl, launch_gemm_sklx, launch_gemm_skf2
and attn_batch_fused:
  * attention, <= 256 keys: nb * KVH = 32 * 8 = 256, so the default takes
    k_attn_decode<128, 4, 0, 1, ATT_WAVES, KT> (one 1024-thread block per (slot, kv head), the
    new key shared through LDS); VOX_HIP_ATT_BSPLIT=2 and any context past 256 keys take the
    128-key k_attn_decode<128, 4, 0, 1, ATT_LWAVES, KT> grid with the last-arriver merge;
  * QKV     K =  768 (12 64-k blocks): 3 slabs of ks = 4, 4 waves -> k_skl2<Q, 4, 4, 1> with
            the RMSNorm sum of squares over nsl = 3 slices; psum2 sums 3 slabs;
  * wo      K = 4096: 8 slabs of ks = 8, N = 768 -> 4 waves, k_skl2<Q, 4, 8, 0>;
            k_resid_xw_fplanes sums 8 slabs;
  * W1|W3   K =  768, N = 2560: bf16 k_sklx<4, 4, SCALE, SWIGLU> (3 slabs, 40 column slices x 2
            row blocks = 80 tickets); Q8 k_skl2<1, 4, 4, 1> + k_swiglu_fplanes over 3 slabs;
  * w2      K = 1280 (20 blocks): 5 slabs of ks = 4, k_skl2<Q, 4, 4, 0>; Sres = 5;
  * LM head K =  768, vocab 4096: k_skf<Q, 4, 4, 2, 2> (launch_gemm_skf2), 12 k blocks over 4
            waves = 3 per wave, so the 2-deep ring goes round with an odd tail;
            VOX_HIP_SKF2=0: k_skf<Q, 1, 4, 2> once per row block (256 column groups -> R = 1).
MID (dec_dim 1536, dec_hidden 3072; K / 64 = 24 and 48 divide by both 8 and 6):
  * QKV     K = 1536, N = 6144: ks = 8 would give 288 blocks (2 residency rounds x 8 x 4 = 64
            block-loads per CU), ks = 6 gives 384 (2 x 6 x 4 = 48) -> 4 slabs of ks = 6,
            k_skl2<0, 4, 6, 1>, nsl = 6 (the real 3072 x 6144 takes ks = 6 the same way);
  * wo      K = 4096, N = 1536: 8 slabs of ks = 8, 4 waves;
  * W1|W3   k_sklx uses skl_splits(K) without N: 3 slabs of ks = 8, k_sklx<4, 8, SCALE, SWIGLU>,
            96 slices x 2 row blocks = 192 tickets;
  * w2      K = 3072, N = 1536: 144 blocks at ks = 8 (32 per CU) against 192 at ks = 6 (24) ->
            8 slabs of ks = 6, k_skl2<0, 4, 6, 0>; Sres = 8;
  * LM head K = 1536: 6 k blocks per wave.
WIDE (dec_dim 2048, dec_hidden 6144; a config of this file's own, for the 8-wave variants that
the full-size widths select and that TINY, KV8 and MID never do):
  * QKV     K = 2048, N = 6144: 4 slabs of ks = 8, 4 waves, k_skl2<0, 4, 8, 1>, nsl = 8;
  * wo      K = 4096, N = 2048: 8 slabs, (N / 128) * 8 = 128 blocks -> 8 waves, k_skl2<0, 8, 8, 0>
            (the real wo 3072 x 4096 and w2 3072 x 9216 take this variant);
  * W1|W3   K = 2048, N = 12288: (N / 128) * 4 = 384 -> k_sklx<8, 8, SCALE, SWIGLU> (the real
            18432 x 3072 takes it), 96 slices x 2 row blocks;
  * w2      K = 6144, N = 2048: ks = 6 (512 blocks, 2 x 24 against 1 x 64) -> 16 slabs,
            k_skl2<0, 4, 6, 0>; Sres = 16;
  * LM head K = 2048: 8 k blocks per wave.

Every test compares every stream's greedy ids with its own CPU-oracle session, and the named
steps' logits at LOGIT_TOL of that step's largest logit.  An id comparison only means something
where the oracle's own top-2 gap exceeds what the tolerance allows, so every test first asserts,
on the oracle's logits alone and with no step left out, that (top1 - top2) / max|logit| is at
least 4x its logit bar (MARGIN_F32 / MARGIN_KV16)."""
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

from vox_weights import TINY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOGIT_TOL = 5e-5     # of the largest logit magnitude, as tests/test_gpu_batch.py
LOGIT_TOL16 = 1e-4   # fp16 KV rings, as tests/test_gpu_kv16.py
MARGIN_F32 = 4 * LOGIT_TOL
MARGIN_KV16 = 4 * LOGIT_TOL16

KV8 = replace(TINY, dec_heads=32, dec_kv_heads=8, dec_dim=768, dec_hidden=1280)
KV8_LONG = replace(KV8, enc_window=750, dec_window=8192)
KV8_W256 = replace(KV8, dec_window=256)
MID = replace(KV8, dec_dim=1536, dec_hidden=3072)
WIDE = replace(KV8, dec_dim=2048, dec_hidden=6144)

SIZES_32 = [420 + 13 * i for i in range(32)]
SIZES_17 = [400 + 24 * i for i in range(17)]
Q8_SEED = 3201   # the first mel seed from 3200 on at which the Q8 oracle passes the margin rule
                 # (3200: 8.0e-5, 3201: 2.5e-4; scanned on the CPU oracle)


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))


def _mels(cfg, sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-0.6, 1.4, size=(n, cfg.mel_bins)).astype(np.float32) for n in sizes]


# ---- weights and oracle sessions, computed once per module -----------------------------------
_W = {}
_ORACLE = {}


def _weights(cfg, q8=False):
    """synth_weights(cfg, seed=1); the windows do not enter the tensors, so KV8, KV8_LONG and
    KV8_W256 share one set"""
    from vox_weights import quantize_q8, synth_weights
    key = (cfg.dec_dim, cfg.dec_hidden, q8)
    if key not in _W:
        if q8:
            _W[key] = quantize_q8(_weights(cfg))
        else:
            _W[key] = synth_weights(replace(cfg, enc_window=TINY.enc_window, dec_window=TINY.dec_window), seed=1)
    return _W[key]


def _oracle(name, cfg, sizes, seed, kv16=False, q8=False):
    """[(ids, logits [steps, vocab])] per stream: each stream's own oracle session decoded to
    the end of its adapter rows.  Encoder and prefill + first token in turn (the oracle's
    M > 1 linears share one scratch buffer), then the single-threaded greedy decodes side by
    side in threads (ctypes releases the GIL; the M = 1 path touches no shared state)."""
    from concurrent.futures import ThreadPoolExecutor
    import vox_oracle
    key = (name, tuple(sizes), seed, kv16, q8)
    if key in _ORACLE:
        return _ORACLE[key]
    om = vox_oracle.OracleModel(cfg, _weights(cfg, q8))
    vox_oracle.set_kv_fp16(kv16)
    try:
        # 4 threads: these widths are too small for more (8 on 8 cores took 10x as long)
        vox_oracle.set_threads(min(4, os.cpu_count() or 1))
        sts, first = [], []
        for mel in _mels(cfg, sizes, seed):
            st = vox_oracle.OracleStream(om)
            st.encode_mel(mel)
            first.append(st.decode(max_steps=1, stop_at_eos=False, want_logits=True))
            sts.append(st)
        vox_oracle.set_threads(1)
        with ThreadPoolExecutor(min(16, len(sts))) as ex:
            rest = list(ex.map(lambda st: st.decode(stop_at_eos=False, want_logits=True), sts))
    finally:
        vox_oracle.set_kv_fp16(False)
        vox_oracle.set_threads(1)
    for st in sts:
        st.close()
    om.close()
    out = []
    for (t0, l0), (t1, l1) in zip(first, rest):
        ids = np.concatenate([t0, t1]).tolist()
        lg = np.concatenate([l0, l1])
        lg.setflags(write=False)
        out.append((ids, lg))
    _ORACLE[key] = out
    return out


def _assert_margin(ref, margin, what):
    """the margin rule, on the oracle's logits alone, every step of every stream"""
    worst, steps = np.inf, 0
    for i, (ids, lg) in enumerate(ref):
        assert len(ids) == lg.shape[0] > 0, i
        top = np.partition(lg, -2, axis=1)[:, -2:]
        gap = (top[:, 1] - top[:, 0]) / np.max(np.abs(lg), axis=1)
        assert np.array_equal(np.argmax(lg, axis=1), np.asarray(ids)), i
        k = int(np.argmin(gap))
        assert gap[k] >= margin, (what, i, k, float(gap[k]), margin)
        worst = min(worst, float(gap[k]))
        steps += len(ids)
    print(f"{what}: oracle top-2 gap >= {worst:.2e} of the largest logit over {steps} steps (rule: {margin:.0e})")


def _step_err(got, want):
    """one step's logit error, of that step's largest oracle logit"""
    return rel(got, want)


def _open(hm, mels, kv16=False):
    import vox_hip
    hm.set_kv_fp16(kv16)
    ss = [vox_hip.Stream(hm) for _ in mels]
    hm.set_kv_fp16(False)
    for s, mel in zip(ss, mels):
        assert s.kv_fp16 == kv16
        s.encode_mel(mel)
    return ss


def _decode_stepwise(hm, mels, slots, steps=6, kv16=False):
    """One Batch over all the streams: `steps` single-step calls reading the logits of `slots`
    after each, then the drain.  Returns (ids per stream, {slot: [steps, vocab]})."""
    import vox_hip
    ss = _open(hm, mels, kv16)
    b = vox_hip.Batch(hm, len(ss))
    got = [[] for _ in ss]
    lg = {i: [] for i in slots}
    for _ in range(steps):
        for i, t in enumerate(b.decode(ss, max_steps=1, stop_at_eos=False)):
            assert len(t) == 1, i
            got[i] += t.tolist()
        for i in lg:
            lg[i].append(b.read_logits(ss[i]))
    for i, t in enumerate(b.decode(ss, max_steps=1000, stop_at_eos=False)):
        got[i] += t.tolist()
    assert all(len(t) == 0 for t in b.decode(ss, max_steps=1000, stop_at_eos=False))
    for s in ss:
        s.close()
    b.close()
    return got, {i: np.stack(v) for i, v in lg.items()}


def _compare(got, lg, ref, tol, what):
    """ids of every stream, and the first steps' logits of the slots read, against the oracle"""
    for i, (ids, _) in enumerate(ref):
        first_diff = next((k for k in range(min(len(ids), len(got[i]))) if got[i][k] != ids[k]), None)
        assert first_diff is None and len(got[i]) == len(ids), (what, i, first_diff, len(got[i]), len(ids))
    worst = 0.0
    for i, l in lg.items():
        for k in range(l.shape[0]):
            r = _step_err(l[k], ref[i][1][k])
            worst = max(worst, r)
            assert r < tol, (what, i, k, r)
    print(f"{what}: {sum(len(g) for g in got)} ids equal, worst logit err {worst:.2e} (bar {tol:.0e})")
    return worst


@pytest.fixture(scope="module")
def kv8_model():
    import vox_hip
    hm = vox_hip.Model(KV8, _weights(KV8))
    yield hm
    hm.close()


def test_kv8_32_streams_sliding_window(kv8_model):
    """KV8 (48-key window), 32 streams of 14 to 64 tokens: the 1024-thread fused attention grid
    (32 x 8 = 256 blocks) with slots dropping out raggedly and the 48-key window sliding under
    the fused RoPE / KV append; every projection with 3, 5 or 8 slabs at Z = 2.  Logits of
    slots 0, 15, 16 and 31 (both row blocks' edges) on the first six single-step calls.
    (These lengths end at position 102 of the 112-slot ring, window + DEC_SLACK, so the ring
    itself does not wrap here: test_kv8_ring_wrap_window_48 and
    test_kv8_256_keys_on_wrapped_ring decode past it.)"""
    ref = _oracle("kv8", KV8, SIZES_32, 3200)
    _assert_margin(ref, MARGIN_F32, "kv8 32 streams")
    n = [len(ids) for ids, _ in ref]
    assert min(n) >= 6 and max(n) + 38 > 2 * KV8.dec_window and len(set(n)) > 8, n
    got, lg = _decode_stepwise(kv8_model, _mels(KV8, SIZES_32, 3200), (0, 15, 16, 31))
    _compare(got, lg, ref, LOGIT_TOL, "kv8 32 streams")


@pytest.mark.parametrize("kv16", [False, True], ids=["f32", "kv16"])
def test_kv8_17_streams(kv8_model, kv16):
    """17 streams: the smallest batch of the 32-slot bucket, so the smallest on the
    1024-thread attention grid, with 15 slots that were never live; f32 and fp16 KV rings (the
    oracle rounding every K/V append to half, at test_gpu_kv16's bar).  Logits of slots 0 and
    16 (the only live row of the second row block) on six steps."""
    ref = _oracle("kv8", KV8, SIZES_17, 1700, kv16=kv16)
    _assert_margin(ref, MARGIN_KV16 if kv16 else MARGIN_F32, f"kv8 17 streams kv16={kv16}")
    got, lg = _decode_stepwise(kv8_model, _mels(KV8, SIZES_17, 1700), (0, 16), kv16=kv16)
    worst = _compare(got, lg, ref, LOGIT_TOL16 if kv16 else LOGIT_TOL, f"kv8 17 streams kv16={kv16}")
    if kv16:
        # the rounding is applied: closer to the rounded-KV oracle than to the f32 one
        f32 = _oracle("kv8", KV8, SIZES_17, 1700)
        far = max(_step_err(lg[i][k], f32[i][1][k]) for i in lg for k in range(lg[i].shape[0]))
        print(f"kv8 17 streams kv16: worst logit err against the f32 oracle {far:.2e}")
        assert far > worst, (far, worst)


def test_kv8_growth_through_256_keys():
    """KV8_LONG (8192-key window), one long stream among 19 short ones (20 streams, 32 slots):
    stream 0 goes from 39 keys to about 300 in calls of at most 16 steps, so the 1024-thread
    block runs with every count of full waves up to 16, and the call that passes 256 keys
    captures the 2-split graph (the 128-key grid at 32 slots x 8 kv heads).  Stream 0's logits
    on every call whose last step is at a position from 253 to 258 (254 to 259 keys)."""
    import vox_hip
    sizes = [2400] + [420 + 8 * i for i in range(19)]
    ref = _oracle("kv8_long", KV8_LONG, sizes, 61)
    _assert_margin(ref, MARGIN_F32, "kv8 growth")
    assert len(ref[0][0]) + 38 > 290, len(ref[0][0])
    hm = vox_hip.Model(KV8_LONG, _weights(KV8_LONG))
    ss = _open(hm, _mels(KV8_LONG, sizes, 61))
    b = vox_hip.Batch(hm, len(ss))
    got = [[] for _ in ss]
    checked, worst = [], 0.0
    caps_below, caps_past = None, None
    while True:
        pos = ss[0].state()["kv_pos"] if got[0] else 38   # position of stream 0's next step
        # single steps from position 253 to 258, calls of up to 16 steps before and after
        steps = 1 if 253 <= pos <= 258 else min(16, 253 - pos) if pos < 253 else 16
        out = b.decode(ss, max_steps=steps, stop_at_eos=False)
        if not any(len(t) for t in out):
            break
        for i, t in enumerate(out):
            got[i] += t.tolist()
        caps = b.stats()["captures"]
        if pos + len(out[0]) <= 256:
            caps_below = caps
        elif caps_past is None:
            caps_past = caps
        last = pos + len(out[0]) - 1   # position of the call's last step
        if len(out[0]) == steps and 253 <= last <= 258:
            k = len(got[0]) - 1
            r = _step_err(b.read_logits(ss[0]), ref[0][1][k])
            checked.append(last)
            worst = max(worst, r)
            assert r < LOGIT_TOL, (last, r)
    assert checked == [253, 254, 255, 256, 257, 258], checked
    # the first call past 256 keys needed a graph the calls below had not captured
    assert caps_below is not None and caps_past is not None and caps_past > caps_below, (caps_below, caps_past)
    assert ss[0].state()["kv_pos"] == 38 + len(ref[0][0])
    for i, (ids, _) in enumerate(ref):
        assert got[i] == ids, (i, len(got[i]), len(ids))
    print(f"kv8 growth: {sum(len(g) for g in got)} ids equal, stream 0 to position {ss[0].state()['kv_pos']}, "
          f"captures {caps_below} -> {caps_past}, worst logit err {worst:.2e}")
    for s in ss:
        s.close()
    b.close()
    hm.close()


def _decode_tail(hm, mels, n0, tail=8):
    """One Batch: n0 - tail steps in one call, then `tail` single steps reading stream 0's
    logits (n0 = stream 0's token count, the longest).  Returns (ids, [tail, vocab], stats,
    stream 0's final position)."""
    import vox_hip
    ss = _open(hm, mels)
    b = vox_hip.Batch(hm, len(ss))
    got = [t.tolist() for t in b.decode(ss, max_steps=n0 - tail, stop_at_eos=False)]
    assert len(got[0]) == n0 - tail
    lg = []
    for _ in range(tail):
        for i, t in enumerate(b.decode(ss, max_steps=1, stop_at_eos=False)):
            got[i] += t.tolist()
        lg.append(b.read_logits(ss[0]))
    assert all(len(t) == 0 for t in b.decode(ss, max_steps=1000, stop_at_eos=False))
    st, pos = b.stats(), ss[0].state()["kv_pos"]
    for s in ss:
        s.close()
    b.close()
    return got, np.stack(lg), st, pos


def _compare_tail(got, lg, ref, what):
    n0 = len(ref[0][0])
    for i, (ids, _) in enumerate(ref):
        assert got[i] == ids, (what, i, len(got[i]), len(ids))
    worst = 0.0
    for k in range(lg.shape[0]):
        r = _step_err(lg[k], ref[0][1][n0 - lg.shape[0] + k])
        worst = max(worst, r)
        assert r < LOGIT_TOL, (what, k, r)
    return worst


W256_SIZES = [2700, 2500] + [400 + 24 * i for i in range(15)]


def _tail_logits_past_the_ring(cfg, name, sizes, seed):
    """Streams 0 and 1 long enough to decode past the ring's capacity (window + 64 slots) among
    15 short ones, one split count all the way: ids of every stream, and stream 0's logits on
    its last 8 steps (wrapped slots in the fused 1024-thread block), against the oracle."""
    import vox_hip
    ref = _oracle(name, cfg, sizes, seed)
    _assert_margin(ref, MARGIN_F32, name)
    n0 = len(ref[0][0])
    assert n0 + 38 > cfg.dec_window + 64 + 8 and n0 > len(ref[1][0]), (n0, len(ref[1][0]))
    hm = vox_hip.Model(cfg, _weights(cfg))
    got, lg, st, pos = _decode_tail(hm, _mels(cfg, sizes, seed), n0)
    hm.close()
    worst = _compare_tail(got, lg, ref, name)
    assert st["captures"] <= 1, st   # one bucket, one split count, all the way
    assert pos == 38 + n0
    print(f"{name}: {sum(len(g) for g in got)} ids equal, stream 0 to position {pos} "
          f"of a {cfg.dec_window + 64}-slot ring, worst logit err on its last 8 steps {worst:.2e}")


def test_kv8_256_keys_on_wrapped_ring():
    """KV8_W256 (window exactly 256, ring of 320 slots): two long streams of about 300 tokens
    among 15 short ones.  splits stays 1 for ever, so the fused 1024-thread block runs L = 256
    with all 16 waves full and, once the position passes 320, over wrapped slots -- the case
    launch_attn_decode's comment names as the dangerous one for the single-stream path.
    Stream 0's logits on its last 8 steps."""
    _tail_logits_past_the_ring(KV8_W256, "kv8 window 256", W256_SIZES, 41)


def test_kv8_ring_wrap_window_48():
    """KV8 (48-key window, ring of 112 slots), 17 streams, two of them of 87 and 82 tokens:
    positions pass 112, so the fused block's three waves of keys straddle the ring's end while
    it appends the new key behind them.  (The 32-stream test's lengths stop at position 102.)
    Shapes chosen here: the shortest streams that wrap by more than the 8 steps read; mel seed
    4800 is the first tried and passes the margin rule (9.5e-4)."""
    _tail_logits_past_the_ring(KV8, "kv8 window 48 wrap", [1000, 960] + [400 + 8 * i for i in range(15)], 4800)


def test_kv8_q8_32_streams():
    """Q8 weights at KV8, 32 streams: k_skf<1, 4, 4, 2, 2> for the LM head, the Q8 k_skl2
    pairs with wscale, and k_swiglu_fplanes over 3 slabs at two row blocks; the oracle on the
    same quantised weights.  Sizes as the 32-stream test; mel seed Q8_SEED (see there)."""
    import vox_hip
    ref = _oracle("kv8", KV8, SIZES_32, Q8_SEED, q8=True)
    _assert_margin(ref, MARGIN_F32, "kv8 q8 32 streams")
    hm = vox_hip.Model(KV8, _weights(KV8, q8=True))
    got, lg = _decode_stepwise(hm, _mels(KV8, SIZES_32, Q8_SEED), (0, 15, 16, 31))
    hm.close()
    _compare(got, lg, ref, LOGIT_TOL, "kv8 q8 32 streams")


def test_mid_17_streams():
    """MID (K = 1536 and 3072): the only small shapes at which skl_splits weighs 6-block
    against 8-block splits, as it does for the real 3072 and 9216 -- QKV and w2 take ks = 6 (4
    and 8 slabs) -- and k_sklx's last-arriver tickets run over 96 column slices per row block
    at Z = 2.  17 streams, logits of slots 0 and 16 on six steps."""
    import vox_hip
    ref = _oracle("mid", MID, SIZES_17, 1701)
    _assert_margin(ref, MARGIN_F32, "mid 17 streams")
    hm = vox_hip.Model(MID, _weights(MID))
    got, lg = _decode_stepwise(hm, _mels(MID, SIZES_17, 1701), (0, 16))
    hm.close()
    _compare(got, lg, ref, LOGIT_TOL, "mid 17 streams")


def test_wide_17_streams():
    """WIDE (K = 2048, 4096, 6144): the 8-wave k_skl2 pair (wo) and the 8-wave k_sklx (W1|W3)
    that the full-size widths select, which no other test runs at 17 to 32 rows, and 16 slabs
    for the residual sum.  17 streams of 12 to 28 tokens (shapes chosen here: the smallest
    batch of the 32 bucket, short streams to bound the oracle's work at these widths; mel seed
    1702, the first tried, passes the margin rule at 1.7e-3).  Logits of slots 0 and 16 on six
    steps."""
    import vox_hip
    sizes = [400 + 8 * i for i in range(17)]
    ref = _oracle("wide", WIDE, sizes, 1702)
    _assert_margin(ref, MARGIN_F32, "wide 17 streams")
    hm = vox_hip.Model(WIDE, _weights(WIDE))
    got, lg = _decode_stepwise(hm, _mels(WIDE, sizes, 1702), (0, 16))
    hm.close()
    _compare(got, lg, ref, LOGIT_TOL, "wide 17 streams")


# ---- the attention grids and the LM head paths, one child process per knob setting ----------
def _child_main(out_path, n0):
    """in a fresh process (VOX_HIP_ATT_BSPLIT / VOX_HIP_SKF2 are read once per process), on the
    GPU only: the 17-stream f32 case (ids, six steps' logits of slots 0 and 16) and the
    256-key-window case (ids, stream 0's last 8 steps' logits), to a file"""
    import vox_hip
    hm = vox_hip.Model(KV8, _weights(KV8))
    got, lg = _decode_stepwise(hm, _mels(KV8, SIZES_17, 1700), (0, 16))
    hm.close()
    hm = vox_hip.Model(KV8_W256, _weights(KV8_W256))
    wgot, wlg, _, _ = _decode_tail(hm, _mels(KV8_W256, W256_SIZES, 41), n0)
    hm.close()

    def flat(g):
        return np.array([len(x) for x in g]), np.concatenate([np.asarray(x, np.int32) for x in g])
    n, ids = flat(got)
    wn, wids = flat(wgot)
    np.savez(out_path, n=n, ids=ids, lg0=lg[0], lg16=lg[16], wn=wn, wids=wids, wlg=wlg)


def _bits_equal(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_kv8_attention_grids_and_lm_head_paths(tmp_path):
    """The 17-stream f32 case in four fresh processes: default, VOX_HIP_ATT_BSPLIT=0 (the
    1024-thread grid forced), VOX_HIP_ATT_BSPLIT=2 (the 128-key grid forced) and
    VOX_HIP_SKF2=0 (the LM head as one launch per row block).  Every run: the oracle's ids,
    logits within LOGIT_TOL.  The default's logits are bit-identical to BSPLIT=0's -- the
    observable proof that the default took the nb * KVH >= 256 branch -- and to SKF2=0's
    (launch_gemm_skf2's comment: "the same bits").  Whether BSPLIT=2 differs in bits is printed,
    not asserted.  On those six steps (39 to 44 keys) it does not: a 128-key block that holds
    the whole context merges the same three waves of keys, the other waves contribute exact
    zeros.  So every child also runs the 256-key-window case, where the two grids split the
    keys differently (one block of 16 waves against two of 8 and the last-arriver merge), under
    the same assertions on stream 0's last 8 steps; measured there, BSPLIT=2 differs in bits."""
    ref = _oracle("kv8", KV8, SIZES_17, 1700)
    _assert_margin(ref, MARGIN_F32, "kv8 17 streams (children)")
    wref = _oracle("kv8 window 256", KV8_W256, W256_SIZES, 41)
    _assert_margin(wref, MARGIN_F32, "kv8 window 256 (children)")
    code = ("import sys; sys.path[:0] = [{!r}, {!r}, {!r}]; import test_gpu_batch_kv8 as t; "
            "t._child_main(sys.argv[1], int(sys.argv[2]))"
            .format(os.path.join(ROOT, "voxtral.c_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")))
    runs = {}
    for name, knobs in (("default", {}), ("bsplit0", {"VOX_HIP_ATT_BSPLIT": "0"}),
                        ("bsplit2", {"VOX_HIP_ATT_BSPLIT": "2"}), ("skf2_0", {"VOX_HIP_SKF2": "0"})):
        env = {k: v for k, v in os.environ.items() if k not in ("VOX_HIP_ATT_BSPLIT", "VOX_HIP_SKF2")}
        env.update(knobs)
        out = str(tmp_path / f"{name}.npz")
        r = subprocess.run([sys.executable, "-c", code, out, str(len(wref[0][0]))], env=env, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:] + r.stderr[-4000:])   # stops the test
        z = np.load(out)

        def unflat(n, ids):
            ends = np.cumsum(n)
            return [ids[e - k:e].tolist() for e, k in zip(ends, n)]
        runs[name] = {0: z["lg0"], 16: z["lg16"], "w": z["wlg"]}
        _compare(unflat(z["n"], z["ids"]), {0: z["lg0"], 16: z["lg16"]}, ref, LOGIT_TOL, f"kv8 17 streams, {name}")
        worst = _compare_tail(unflat(z["wn"], z["wids"]), z["wlg"], wref, f"kv8 window 256, {name}")
        print(f"kv8 window 256, {name}: ids equal, worst logit err on stream 0's last 8 steps {worst:.2e}")
    for other in ("bsplit0", "skf2_0"):
        for k in (0, 16, "w"):
            assert _bits_equal(runs["default"][k], runs[other][k]), (other, k)
    print("VOX_HIP_ATT_BSPLIT=2 logits differ in bits from the default's: 17 streams (39..44 keys) "
          f"{any(not _bits_equal(runs['default'][k], runs['bsplit2'][k]) for k in (0, 16))}, "
          f"256-key window {not _bits_equal(runs['default']['w'], runs['bsplit2']['w'])}")
