"""Batched decode calls of 33..128 streams: the wide step (batch_step_wide).

A call with more than 32 streams runs the slot bucket 64 or 128: the stacked prefill's k_gemmf
layers over the bf16 fragment-major copies (the row-major launch_gemm layers on a model with Q8
step tensors), the slot-table decode attention k_attn_decode<128, 4, 0, 1, *, KT, AttnSlots>
(RoPE + K/V append at each live slot's own position, output as the wo input planes), the LM head
through k_gemmf and the 128-row argmax, captured into step graphs of their own.

The config is tests/test_gpu_batch_kv8.py's KV8 (32 query / 8 kv heads, dec_dim 768, dec_hidden
1280): the real head geometry, and it passes dec_gemmf_ok.  Its helpers and margin rule are
imported, not copied: every oracle comparison first asserts, on the oracle's logits alone and
with no step left out, (top1 - top2) / max|logit| >= 4 x the logit bar.  Mel sizes are
[400 + 2 i for i < n] from one _mels call, so a shorter list is a prefix with identical mels and
one 128-stream oracle run (seed 6408, gap 2.80e-4 over 3,520 steps) serves every f32 test.
Seeds were scanned on the CPU oracle: f32 6408 (128 streams 2.80e-4), half rings 6410 (64
streams 8.28e-4, rule 4e-4), Q8 6417 (64 streams 6.04e-4), KV8_LONG 6600 (6.06e-4, the first
tried), FP8 6503 (see FP8_SEED).  6400-6407, 6409 and 6411 fail at 128."""
import ctypes

import numpy as np
import pytest

import kv8_ref
import test_gpu_batch_kv8 as g
from test_gpu_batch_kv8 import KV8, KV8_LONG, LOGIT_TOL, LOGIT_TOL16, MARGIN_F32, MARGIN_KV16

pytestmark = pytest.mark.gpu

SEED = 6408
SIZES = [400 + 2 * i for i in range(128)]
TOKEN_EOS = 2
_MELS = {}


def _mels(n, seed=SEED):
    if seed not in _MELS:
        _MELS[seed] = g._mels(KV8, SIZES, seed)
    return _MELS[seed][:n]


def _ref(n):
    """the first n streams of the 128-stream f32 oracle run (a prefix has the same mels)"""
    ref = g._oracle("kv8", KV8, SIZES, SEED)
    return ref[:n]


@pytest.fixture(scope="module")
def kv8_model():
    import vox_hip
    hm = vox_hip.Model(KV8, g._weights(KV8))
    yield hm
    hm.close()


@pytest.mark.parametrize("n", [64, 128])
def test_wide_streams_match_oracle(kv8_model, n):
    """64 and 128 streams in one Batch: every stream's ids equal its oracle session; the first
    six steps' logits of the slots at the edges of the 16-row blocks and of the 32 / 64
    boundaries within 5e-5.  Fails without the feature: Batch(hm, 64) is refused."""
    ref = _ref(n)
    g._assert_margin(ref, MARGIN_F32, f"wide {n} streams")
    slots = (0, 15, 16, 31, 32, 63) + ((64, 127) if n == 128 else ())
    got, lg = g._decode_stepwise(kv8_model, _mels(n), slots)
    g._compare(got, lg, ref, LOGIT_TOL, f"wide {n} streams")


@pytest.mark.parametrize("n", [33, 65, 100])
def test_wide_dead_rows_inside_a_bucket(kv8_model, n):
    """33, 65 and 100 streams: the smallest call of the 64 bucket (31 rows never live), the
    smallest of the 128 bucket (63) and an uneven one; ids against the oracle."""
    ref = _ref(n)
    g._assert_margin(ref, MARGIN_F32, f"wide {n} streams")
    got, lg = g._decode_stepwise(kv8_model, _mels(n), ())
    g._compare(got, lg, ref, LOGIT_TOL, f"wide {n} streams")


def test_wide_half_rings_64_streams(kv8_model):
    """IEEE-half KV rings at 64 streams (the kvh_t attention instances): the oracle rounds every
    K/V append to half; bar 1e-4 as tests/test_gpu_kv16.py, margin rule 4e-4."""
    ref = g._oracle("kv8", KV8, SIZES[:64], 6410, kv16=True)
    g._assert_margin(ref, MARGIN_KV16, "wide 64 streams kv16")
    got, lg = g._decode_stepwise(kv8_model, _mels(64, 6410), (0, 31, 32, 63), kv16=True)
    g._compare(got, lg, ref, LOGIT_TOL16, "wide 64 streams kv16")


# FP8: 40 streams of 10..12 steps, as kv8_ref's batch17 run is built (a stream of n steps gets
# 39 + n + 5 adapter rows).  The seed is picked on the CPU by the rule of tests/test_kv8_cpu.py: the
# unforced FP8 reference (kv8_ref.kv8_hook) keeps a top-2 margin of 4 x 5e-5 on every step of every
# stream.  Scanned from 6500 on: 6500 2.47e-4, 6501 1.27e-4, 6502 1.43e-4, 6503 1.45e-3.  6500 passes
# that rule with so little to spare that the ring-conditioned replay, which adopts the GPU's stored
# codes, measured 1.89e-4 on one step of stream 22; 6503 is the first with room for the replay too.
FP8_SEED = 6503
FP8_STEPS = [10 + (i % 3) for i in range(40)]


def _fp8_mels():
    rng = np.random.default_rng(FP8_SEED)
    return [rng.uniform(-0.6, 1.4, size=(kv8_ref.FRAMES_PER_ROW * (39 + n + 5), KV8.mel_bins)).astype(np.float32)
            for n in FP8_STEPS]


def test_wide_fp8_40_streams():
    """FP8 (E4M3) rings at 40 streams (the kv8_t instances, bucket 64): the ring-conditioned
    check of test_gpu_kv8.test_kv8_batch_17_streams_kv8_config -- every stored K/V element is the
    reference's rounding or the adjacent code across a midpoint within ACT_TOL, the replay
    adopts the stored rows, and ids and the last two steps' logits are held to 5e-5.  Every
    stream is replayed."""
    import test_gpu_kv8 as k8
    import vox_hip
    hm, _, _ = k8._models("KV8")
    try:
        mels = _fp8_mels()
        ss = [k8._stream(hm, vox_hip.KV_FP8, mel) for mel in mels]
        rgs = [k8.Rings(s) for s in ss]
        ids = [[] for _ in ss]
        lgs = [[] for _ in ss]
        b = vox_hip.Batch(hm, 64)

        def live():
            return [k for k in range(len(ss)) if len(ids[k]) < FP8_STEPS[k]]
        while live():
            act = live()
            left = min(FP8_STEPS[k] - len(ids[k]) for k in act)
            n = 1 if left <= 2 else left - 2
            for k, t in zip(act, b.decode([ss[k] for k in act], max_steps=n, stop_at_eos=False)):
                assert len(t) == n
                ids[k] += t.tolist()
                lgs[k] += [None] * (n - 1) + [b.read_logits(ss[k])]
                rgs[k].pull()
        b.close()
        for k, s in enumerate(ss):
            s.close()
            rgs[k].done()
            assert len(ids[k]) == FP8_STEPS[k]
            k8._replay("KV8", mels[k], ids[k], lgs[k], rgs[k], f"wide fp8 stream {k}")
    finally:
        for m, om, _ in k8._M.values():
            m.close()
            om.close()
        k8._M.clear()


def test_wide_q8_64_streams():
    """A model with Q8 step tensors at 64 streams: dec_gemmf_ok is false, so the step takes the
    row-major launch_gemm layers and LM head, fed by the attention's f32 rows."""
    import vox_hip
    ref = g._oracle("kv8", KV8, SIZES[:64], 6417, q8=True)
    g._assert_margin(ref, MARGIN_F32, "wide q8 64 streams")
    hm = vox_hip.Model(KV8, g._weights(KV8, q8=True))
    got, lg = g._decode_stepwise(hm, _mels(64, 6417), (0, 31, 32, 63))
    hm.close()
    g._compare(got, lg, ref, LOGIT_TOL, "wide q8 64 streams")


def _until_eos(ids):
    return ids[:ids.index(TOKEN_EOS) + 1] if TOKEN_EOS in ids else ids


def test_wide_churn_in_one_batch(kv8_model):
    """One Batch(hm, 128): 40 streams for 3 steps (bucket 64, two stacked prefill passes), 20 of
    them for 2 (bucket 32, the skinny step), then those 20 with 50 new ones (bucket 128, two more
    passes) for 5 steps and to the end with stop_at_eos, then all 90.  Every call but the drains
    ends by max_steps exhaustion.  ids against the oracle (up to the first EOS, if any); no
    capture beyond one per bucket used."""
    import vox_hip
    ref = _ref(90)
    g._assert_margin(ref, MARGIN_F32, "wide churn")
    ss = g._open(kv8_model, _mels(90))
    b = vox_hip.Batch(kv8_model, 128)
    got = [[] for _ in ss]

    def run(idx, steps, eos):
        out = b.decode([ss[i] for i in idx], max_steps=steps, stop_at_eos=eos)
        for i, t in zip(idx, out):
            got[i] += t.tolist()
        return out
    a = list(range(40))
    assert all(len(t) == 3 for t in run(a, 3, False))
    st = b.stats()
    assert st["prefill_passes"] == 2 and st["prefilled"] == 40, st
    a20 = a[::2]
    assert all(len(t) == 2 for t in run(a20, 2, False))
    c = a20 + list(range(40, 90))
    out = run(c, 5, True)
    assert all(len(t) == 5 or t[-1] == TOKEN_EOS for t in out)
    st = b.stats()
    assert st["prefill_passes"] == 4 and st["prefilled"] == 90, st
    run(c, 1000, True)
    run(list(range(90)), 1000, True)
    assert all(len(t) == 0 for t in b.decode(ss, max_steps=1000, stop_at_eos=True))
    st = b.stats()
    assert st["captures"] <= 3, st   # buckets 64, 32 and 128, one attention splits bucket
    for i, (ids, _) in enumerate(ref):
        assert got[i] == _until_eos(ids), (i, len(got[i]), len(ids))
    print(f"wide churn: {sum(len(x) for x in got)} ids equal, stats {st}")
    for s in ss:
        s.close()
    b.close()


def test_wide_alternatives_on_a_high_slot(kv8_model):
    """--alt streams in slots 3 and 35 of a 40-stream call (the argmax rows past 32): their
    records agree with the reference rule (stream_fill_alts) on the oracle's logits, as
    tests/test_gpu_batch.py::test_batch_alternatives_match_stream_fill_alts holds the <= 32 step."""
    import vox_hip
    import vox_oracle
    ref = _ref(40)
    g._assert_margin(ref, MARGIN_F32, "wide alts")
    settings = {3: (3, 1.0), 35: (4, 0.5)}
    ss = [vox_hip.Stream(kv8_model) for _ in range(40)]
    for i, (s, mel) in enumerate(zip(ss, _mels(40))):
        if i in settings:
            s.set_alt(*settings[i])
        s.encode_mel(mel)
    b = vox_hip.Batch(kv8_model, 64)
    got = [t.tolist() for t in b.decode(ss, max_steps=1000, stop_at_eos=False)]
    n_with = 0
    for i, (ids, ol) in enumerate(ref):
        assert got[i] == ids, i
        if i not in settings:
            continue
        na, co = settings[i]
        aid, pr = ss[i].read_alts(0, len(ids))
        for k, tok in enumerate(ids):
            rid, rpr = vox_oracle.fill_alts(ol[k], tok, na, co)
            assert aid[k].tolist() == rid, (i, k, aid[k], rid)
            np.testing.assert_allclose(pr[k], rpr, rtol=2 * LOGIT_TOL * float(np.max(np.abs(ol[k]))), atol=1e-9)
            n_with += aid[k][1] >= 0
    assert n_with > 0
    for s in ss:
        s.close()
    b.close()


LONG_SIZES = [2400, 2300] + [400 + 2 * i for i in range(62)]
LONG_SEED = 6600


def test_wide_long_context_split_grid():
    """KV8_LONG (8192-key window), two streams that pass 256 keys among 62 short ones in a
    64-stream call: 200 steps on the one-block-per-(slot, kv head) grid, then the 2-split graph
    (128-key blocks, the last arriver merging) while the short slots have stopped.  Stream 0's
    logits after the calls that end at positions 238, 270 and its last one."""
    import vox_hip
    ref = g._oracle("kv8_long", KV8_LONG, LONG_SIZES, LONG_SEED)
    g._assert_margin(ref, MARGIN_F32, "wide long")
    n0 = len(ref[0][0])
    assert n0 + 38 > 290 and len(ref[1][0]) + 38 > 270, (n0, len(ref[1][0]))
    hm = vox_hip.Model(KV8_LONG, g._weights(KV8_LONG))
    ss = g._open(hm, g._mels(KV8_LONG, LONG_SIZES, LONG_SEED))
    b = vox_hip.Batch(hm, 64)
    got = [[] for _ in ss]
    worst, caps = 0.0, []
    for steps in (200, 32, 1000):
        for i, t in enumerate(b.decode(ss, max_steps=steps, stop_at_eos=False)):
            got[i] += t.tolist()
        caps.append(b.stats()["captures"])
        r = g._step_err(b.read_logits(ss[0]), ref[0][1][len(got[0]) - 1])
        worst = max(worst, r)
        assert r < LOGIT_TOL, (steps, len(got[0]), r)
    assert caps[0] <= 1 and caps[1] <= caps[0] + 1 and caps[2] == caps[1], caps
    assert ss[0].state()["kv_pos"] == 38 + n0
    for i, (ids, _) in enumerate(ref):
        assert got[i] == ids, (i, len(got[i]), len(ids))
    print(f"wide long: {sum(len(x) for x in got)} ids equal, stream 0 to position {38 + n0}, captures {caps}, "
          f"worst logit err {worst:.2e}")
    for s in ss:
        s.close()
    b.close()
    hm.close()


def test_wide_decode_rows_and_begin_finish(kv8_model):
    """64 streams through vox_hip_batch_begin_rows + vox_hip_batch_finish (4 steps in flight), a
    row-bounded vox_hip_batch_decode_rows (each stream's first 45 adapter rows: the steps that
    read rows 42, 43 and 44), then the rest: the ids vox_hip_batch_decode gives (the oracle's)."""
    import vox_hip
    ref = _ref(64)
    g._assert_margin(ref, MARGIN_F32, "wide rows")
    ss = g._open(kv8_model, _mels(64))
    b = vox_hip.Batch(kv8_model, 64)
    n = len(ss)
    got = [[] for _ in ss]
    arr = (ctypes.c_void_p * n)(*[s.h for s in ss])
    rows = (ctypes.c_int * n)(*[s.adapter_tokens for s in ss])
    toks = np.zeros((n, 4), np.int32)
    cnt = np.zeros(n, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    L = vox_hip.lib()
    assert L.vox_hip_batch_begin_rows(b.h, arr, n, rows, 4, 0, toks.ctypes.data_as(ip), cnt.ctypes.data_as(ip)) == 0
    assert L.vox_hip_batch_finish(b.h) == 4 * n
    for i in range(n):
        assert cnt[i] == 4
        got[i] += toks[i].tolist()
    for i, t in enumerate(b.decode(ss, max_steps=1000, stop_at_eos=False, rows=[45] * n)):
        assert len(t) == 3, (i, len(t))
        got[i] += t.tolist()
    for i, t in enumerate(b.decode(ss, max_steps=1000, stop_at_eos=False, rows=[s.adapter_tokens for s in ss])):
        got[i] += t.tolist()
    for i, (ids, _) in enumerate(ref):
        assert got[i] == ids, (i, len(got[i]), len(ids))
    for s in ss:
        s.close()
    b.close()
