"""Decoder K/V rings that grow on demand (vox_hip_model_set_kv_grow).

A stream created under the switch starts with rings of slots0 slots and doubles them (capped at
window + 64) before any call that would append past their end.  A ring below the full size has
not wrapped, so growth is a prefix copy into a longer buffer: the stored values, the kernels'
arithmetic and the tokens are those of a full ring.  These tests hold that to the bit wherever a
grown stream and a full-ring stream run the same kernels -- single stream at >= 256 slots
(TINY_LONG) and at TINY, every batched call -- and to the oracle (ids equal, logits within 5e-5)
where a ring below 256 slots takes the general decode attention instead of the short-context
kernel.  Batched calls that list a shorter ring run the ragged attention instances (per-slot ring
capacity) on step graphs of their own; the counters say which ran.

Capacities and byte counts are predicted by tests/kv_grow_ref.py (pinned on the CPU by
tests/test_kv_grow_cpu.py, with the margin rule of the oracle sessions whose ids are compared).
The allocation-failure path is read, not run: no test exhausts device memory."""
import ctypes

import numpy as np
import pytest

import kv_grow_ref as R
from kv_grow_ref import LOGIT_TOL, MARGIN, PROMPT, STEP_BATCH

pytestmark = pytest.mark.gpu

IP = ctypes.POINTER(ctypes.c_int)
CHUNK = 4096
MAX_CALL = 64        # steps per single-stream decode call between ring read-backs


@pytest.fixture(scope="module")
def hm():
    import vox_hip
    from vox_weights import TINY
    m = vox_hip.Model(TINY, R.weights())
    yield m
    m.close()


@pytest.fixture(scope="module")
def hm_long():
    import vox_hip
    from vox_weights import TINY_LONG
    m = vox_hip.Model(TINY_LONG, R.weights())
    yield m
    m.close()


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-6, float(np.max(np.abs(b)))))


def _esize(dtype):
    import vox_hip
    return {vox_hip.KV_F32: 4, vox_hip.KV_F16: 2, vox_hip.KV_FP8: 1}[dtype]


def _stream(m, mel, slots0=0, dtype=0):
    """a stream created under set_kv_grow(slots0) and set_kv_dtype(dtype), its mel encoded"""
    import vox_hip
    m.set_kv_grow(slots0)
    m.set_kv_dtype(dtype)
    try:
        s = vox_hip.Stream(m)
    finally:
        m.set_kv_grow(0)
        m.set_kv_dtype(vox_hip.KV_F32)
    want = R.clamp_slots0(slots0, m.cfg) or R.full_slots(m.cfg)
    assert s.kv_slots == want and s.kv_dtype == dtype
    assert s.kv_bytes == R.ring_bytes(m.cfg, want, _esize(dtype))
    assert s.kv_grow_stats() == dict(grows=0, copied=0, slots=want)
    for i in range(0, mel.shape[0], CHUNK):
        s.encode_mel(mel[i:i + CHUNK])
    return s


def _rings(s, keep=1 << 30):
    """raw K and V of the last min(position, keep) positions of every layer"""
    pos = s.state()["kv_pos"]
    first = max(0, pos - keep)
    return [s.read_kv(l, first, pos - first) for l in range(s.cfg.dec_layers)]


def _same_rings(a, b):
    assert len(a) == len(b)
    for (ka, va), (kb, vb) in zip(a, b):
        assert ka.shape == kb.shape and ka.shape[0] > 0
        assert np.array_equal(ka, kb) and np.array_equal(va, vb)


def _mel(cfg, seed, steps):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.6, 1.4, size=(R.FPR * (PROMPT + 1 + steps + 4), cfg.mel_bins)).astype(np.float32)


# ---- invariant 1 ------------------------------------------------------------------------------------
def test_default_is_untouched():
    """A model whose switch was never touched, then the same model after set_kv_grow(64) and
    set_kv_grow(0): streams of window + 64 slots, no growth, the same memory per stream, the same
    graph captures and replays for the same calls, no ragged step, and ids and logits equal to the
    bit (single stream, and a batched call of two chunks)."""
    import vox_hip
    from vox_weights import TINY
    m = vox_hip.Model(TINY, R.weights())
    L = vox_hip.lib()
    mels = [_mel(TINY, 9400 + i, 50) for i in range(3)]
    full = R.full_slots(TINY)

    def run():
        m0 = L.vox_hip_memory_used()
        ss = [vox_hip.Stream(m) for _ in mels]
        per_stream = (L.vox_hip_memory_used() - m0) // len(ss)
        for s, mel in zip(ss, mels):
            assert s.kv_slots == full and s.kv_bytes == R.ring_bytes(TINY, full, 4)
            s.encode_mel(mel)
        b = vox_hip.Batch(m, 4)
        t0, lg0 = ss[0].decode(max_steps=20, stop_at_eos=False, want_logits=True)
        call = b.decode(ss, max_steps=24, stop_at_eos=False)
        lgb = [b.read_logits(s) for s in ss]
        out = dict(per_stream=per_stream, single=t0.tolist(), single_logits=lg0, call=[t.tolist() for t in call],
                   logits=lgb, stats=b.stats(), grow=b.kv_grow_stats(), rings=[_rings(s) for s in ss],
                   sstats=[s.kv_grow_stats() for s in ss])
        b.close()
        for s in ss:
            s.close()
        return out

    before = run()
    m.set_kv_grow(64)
    m.set_kv_grow(0)
    after = run()
    m.close()
    for r in (before, after):
        assert r["grow"] == dict(ragged_calls=0, ragged_replays=0, ragged_captures=0)
        assert r["sstats"] == [dict(grows=0, copied=0, slots=full)] * 3
        assert [len(t) for t in r["call"]] == [24, 24, 24] and r["stats"]["captures"] == 1
    assert before["per_stream"] == after["per_stream"]
    assert before["stats"] == after["stats"]
    assert before["single"] == after["single"] and before["call"] == after["call"]
    assert np.array_equal(before["single_logits"], after["single_logits"])
    for a, c in zip(before["logits"], after["logits"]):
        assert np.array_equal(a, c)
    for a, c in zip(before["rings"], after["rings"]):
        _same_rings(a, c)


# ---- invariant 2: one stream -----------------------------------------------------------------------
_SINGLE = {}


def _single(m, name, slots0):
    """one session of kv_grow_ref.SESSIONS on the GPU in calls of MAX_CALL steps: ids, logits, and
    after every call the capacity, the rings' bytes and the ring rows (all of them, or the last 64
    once a ring may have wrapped)"""
    key = (name, slots0)
    if key not in _SINGLE:
        cfg, steps, _ = R.SESSIONS[name]
        s = _stream(m, R.session_mel(name), slots0)
        keep = 1 << 30 if name == "long" else 64
        ids, lgs, caps, nbytes, rings = [], [], [], [], []
        while len(ids) < steps:
            t, lg = s.decode(max_steps=min(MAX_CALL, steps - len(ids)), stop_at_eos=False, want_logits=True)
            assert len(t) > 0
            ids += t.tolist()
            lgs.append(lg)
            caps.append(s.kv_slots)
            nbytes.append(s.kv_bytes)
            rings.append(_rings(s, keep))
        _SINGLE[key] = dict(ids=ids, logits=np.concatenate(lgs), caps=caps, bytes=nbytes, rings=rings,
                            stats=s.kv_grow_stats())
        s.close()
    return _SINGLE[key]


def _needs(steps):
    return [PROMPT + min(steps, MAX_CALL * (k + 1)) for k in range((steps + MAX_CALL - 1) // MAX_CALL)]


def test_single_stream_256_slots_bit_equal(hm_long):
    """TINY_LONG, slots0 = 256, 424 steps: one growth, 256 -> 512, in the call that reaches position
    294.  Both capacities are >= 256, so the grown stream runs the full ring's kernels (k_attn_short
    up to 256 keys, k_attn_decode past them): ids, every step's logits and, after every call, every
    ring row so far equal the full-ring stream's to the bit.  Both equal the oracle's ids."""
    from vox_weights import TINY_LONG
    ref = R.session_oracle("long")
    assert R.worst_margin(ref["logits"]) >= MARGIN
    full = _single(hm_long, "long", 0)
    grown = _single(hm_long, "long", 256)
    caps, grows = R.schedule(256, TINY_LONG, _needs(424))
    assert grows == 1 and caps[-1] == 512
    assert grown["caps"] == caps and grown["stats"]["grows"] == 1 and grown["stats"]["slots"] == 512
    assert grown["bytes"] == [R.ring_bytes(TINY_LONG, c, 4) for c in caps]
    # the copy moved the rows of the calls before the growth: positions [0, 230)
    assert grown["stats"]["copied"] == R.ring_bytes(TINY_LONG, PROMPT + 3 * MAX_CALL, 4)
    assert full["caps"] == [8256] * len(caps) and full["stats"] == dict(grows=0, copied=0, slots=8256)
    assert full["ids"] == ref["ids"] and grown["ids"] == full["ids"]
    assert np.array_equal(grown["logits"], full["logits"])
    for a, c in zip(grown["rings"], full["rings"]):
        _same_rings(a, c)


def test_single_stream_64_slots_matches_oracle(hm_long):
    """TINY_LONG, slots0 = 64: three growths, 64 -> 128 -> 256 -> 512.  Below 256 slots the single
    stream's attention is k_attn_decode where a full ring runs k_attn_short (the one
    capacity-dependent choice, launch_attn_decode's cap >= 256): another summation order, so the
    bar is the project's usual one -- ids equal to the oracle's, logits within 5e-5 of the largest
    magnitude -- and the ring rows are held to the full-ring stream's at that bar too."""
    from vox_weights import TINY_LONG
    ref = R.session_oracle("long")
    assert R.worst_margin(ref["logits"]) >= MARGIN
    grown = _single(hm_long, "long", 64)
    full = _single(hm_long, "long", 0)
    caps, grows = R.schedule(64, TINY_LONG, _needs(424))
    assert grows == 3 and sorted(set(caps)) == [128, 256, 512]
    assert grown["caps"] == caps and grown["stats"]["grows"] == 3
    assert grown["bytes"] == [R.ring_bytes(TINY_LONG, c, 4) for c in caps]
    assert grown["ids"] == ref["ids"]
    err = max(_rel(g, o) for g, o in zip(grown["logits"], ref["logits"]))
    print(f"slots0 = 64: logits {err:.2e} of the oracle's largest")
    assert err < LOGIT_TOL
    for a, c in zip(grown["rings"], full["rings"]):
        for (ka, va), (kc, vc) in zip(a, c):
            assert ka.shape == kc.shape and _rel(ka, kc) < LOGIT_TOL and _rel(va, vc) < LOGIT_TOL


def test_single_stream_tiny_grows_to_112_then_wraps(hm):
    """TINY (window 48, full ring 112), slots0 = 64, 200 steps: the first call needs 102 slots and
    gets 112, not 128; from position 112 on the ring wraps as a full ring does.  Both capacities
    are below 256 (one attention kernel): ids, logits and the ring's last 64 rows after every
    call equal the full-ring stream's to the bit, and the ids the oracle's through the wrap."""
    from vox_weights import TINY
    ref = R.session_oracle("wrap")
    assert R.worst_margin(ref["logits"]) >= MARGIN
    full = _single(hm, "wrap", 0)
    grown = _single(hm, "wrap", 64)
    assert R.schedule(64, TINY, _needs(200)) == ([112] * 4, 1)
    assert grown["caps"] == [112] * 4 and grown["stats"] == dict(grows=1, copied=0, slots=112)
    assert grown["bytes"] == [R.ring_bytes(TINY, 112, 4)] * 4
    assert PROMPT + 200 > 112 + TINY.dec_window
    assert full["ids"] == ref["ids"] and grown["ids"] == full["ids"]
    assert np.array_equal(grown["logits"], full["logits"])
    for a, c in zip(grown["rings"], full["rings"]):
        _same_rings(a, c)


# ---- invariants 3 and 5: batched calls ---------------------------------------------------------------
def _begin_finish(b, ss, max_steps, check=None):
    """one batched call over all of each stream's rows through begin_rows / finish; check runs
    between the two.  Returns the ids per stream."""
    import vox_hip
    L = vox_hip.lib()
    n = len(ss)
    arr = (ctypes.c_void_p * n)(*[s.h for s in ss])
    rows = np.array([s.adapter_tokens for s in ss], np.int32)
    toks = np.zeros((n, max_steps), np.int32)
    cnt = np.zeros(n, np.int32)
    assert L.vox_hip_batch_begin_rows(b.h, arr, n, rows.ctypes.data_as(IP), max_steps, 0, toks.ctypes.data_as(IP),
                                      cnt.ctypes.data_as(IP)) == 0, L.vox_hip_last_error()
    if check:
        check()
    assert L.vox_hip_batch_finish(b.h) >= 0, L.vox_hip_last_error()
    return [toks[i, :cnt[i]].tolist() for i in range(n)]


LONG_PRE = (300, 100, 0)     # single-stream steps before the batched call
LONG_SLOTS0 = (0, 256, 64)
LONG_CALL = 40


def _batched_long(m, grown):
    import vox_hip
    mel = R.session_mel("long")
    ss = [_stream(m, mel, c if grown else 0) for c in LONG_SLOTS0]
    pre = [s.decode(max_steps=p, stop_at_eos=False).tolist() if p else [] for s, p in zip(ss, LONG_PRE)]
    b = vox_hip.Batch(m, 4)
    seen = {}

    def between():
        seen["slots"] = [s.kv_slots for s in ss]
        seen["stats"] = [s.kv_grow_stats() for s in ss]
        seen["pos"] = [s.state()["kv_pos"] for s in ss]

    call = _begin_finish(b, ss, LONG_CALL, between)
    out = dict(pre=pre, call=call, logits=[b.read_logits(s) for s in ss], rings=[_rings(s) for s in ss],
               slots=[s.kv_slots for s in ss], stats=[s.kv_grow_stats() for s in ss], seen=seen,
               bstats=b.stats(), grow=b.kv_grow_stats())
    b.close()
    for s in ss:
        s.close()
    return out


def test_batched_three_capacities_in_one_call(hm_long):
    """TINY_LONG, one session's mel on three streams at different positions and capacities: a
    full ring at position 338, a 256-slot ring at 138, a 64-slot ring that joins (its prompt is
    prefilled by the call).  One call of 40 steps (chunks of 16, 16, 8) through begin_rows /
    finish: the joining ring grows to 128 before the prefill, nothing moves between begin and
    finish, every step is a ragged replay, and each stream's ids are its own single-stream run's.
    The same three streams on full rings in another batch give the same ids, last-step logits and
    ring rows to the bit, on plain replays."""
    ref = R.session_oracle("long")
    assert R.worst_margin(ref["logits"]) >= MARGIN
    single = _single(hm_long, "long", 0)
    assert single["ids"] == ref["ids"]
    run = _batched_long(hm_long, True)
    twin = _batched_long(hm_long, False)
    # the call's own growth, done before begin returned, and nothing after it (invariant 5)
    assert run["seen"]["slots"] == [8256, 256, 128] == run["slots"]
    assert run["seen"]["stats"] == run["stats"]
    assert [s["grows"] for s in run["stats"]] == [0, 0, 1]
    assert LONG_CALL > 2 * STEP_BATCH
    for i, p in enumerate(LONG_PRE):
        assert run["seen"]["slots"][i] >= PROMPT + p + LONG_CALL
    assert twin["slots"] == [8256] * 3 and all(s["grows"] == 0 for s in twin["stats"])
    # which instances ran
    assert run["grow"] == dict(ragged_calls=1, ragged_replays=LONG_CALL, ragged_captures=1)
    assert run["bstats"]["replays"] == LONG_CALL
    assert twin["grow"] == dict(ragged_calls=0, ragged_replays=0, ragged_captures=0)
    assert twin["bstats"]["replays"] == LONG_CALL
    # each stream's own single-stream run
    for i, p in enumerate(LONG_PRE):
        assert run["pre"][i] == single["ids"][:p], i
        assert run["call"][i] == single["ids"][p:p + LONG_CALL], (i, run["call"][i])
    # invariant 3
    assert twin["pre"] == run["pre"] and twin["call"] == run["call"]
    for a, c in zip(run["logits"], twin["logits"]):
        assert np.array_equal(a, c)
    for a, c in zip(run["rings"], twin["rings"]):
        _same_rings(a, c)


TINY_PRE = 90        # single-stream steps of the full-ring members: position 128, past the ring's wrap
TINY_CALL = 20


def _batched_tiny(m, dtype, grown):
    import vox_hip
    ss = []
    for i in range(8):
        mel = _mel(m.cfg, 9300 + i, TINY_PRE + TINY_CALL)
        ss.append(_stream(m, mel, 64 if (grown and i % 2 == 0) else 0, dtype))
    for i in range(1, 8, 2):
        assert len(ss[i].decode(max_steps=TINY_PRE, stop_at_eos=False)) == TINY_PRE
    b = vox_hip.Batch(m, 8)
    call = [t.tolist() for t in b.decode(ss, max_steps=TINY_CALL, stop_at_eos=False)]
    out = dict(call=call, logits=[b.read_logits(s) for s in ss], rings=[_rings(s, 58) for s in ss],
               slots=[s.kv_slots for s in ss], grows=[s.kv_grow_stats()["grows"] for s in ss],
               grow=b.kv_grow_stats(), replays=b.stats()["replays"])
    b.close()
    for s in ss:
        s.close()
    return out


@pytest.mark.parametrize("dtype", [0, 1, 2], ids=["f32", "half", "fp8"])
def test_batched_mixed_64_and_112(hm, dtype):
    """TINY, 8 streams in one call of 20 steps (chunks of 16 and 4), f32 / half / FP8 rings: the
    even ones on 64-slot rings, joining (positions 38..57 stay inside 64 slots, so they stay
    short), the odd ones on full rings at position 128, past the wrap.  Against the same streams
    on full rings in another batch: ids, last-step logits and ring rows to the bit."""
    run = _batched_tiny(hm, dtype, True)
    twin = _batched_tiny(hm, dtype, False)
    assert run["slots"] == [64, 112] * 4 and run["grows"] == [0] * 8
    assert twin["slots"] == [112] * 8
    assert all(len(t) == TINY_CALL for t in run["call"]) and TINY_CALL > STEP_BATCH
    assert run["grow"] == dict(ragged_calls=1, ragged_replays=TINY_CALL, ragged_captures=1)
    assert run["replays"] == TINY_CALL == twin["replays"]
    assert twin["grow"] == dict(ragged_calls=0, ragged_replays=0, ragged_captures=0)
    assert run["call"] == twin["call"]
    for a, c in zip(run["logits"], twin["logits"]):
        assert np.array_equal(a, c)
    for a, c in zip(run["rings"], twin["rings"]):
        _same_rings(a, c)


WIDE_N = 33
WIDE_CALL = 10


def _batched_wide(m, grown):
    import vox_hip
    mels = [_mel(m.cfg, 9500 + i, 2 * WIDE_CALL) for i in range(WIDE_N)]
    late = WIDE_N - 1                 # an even member: a 64-slot ring in the grown run
    ss = []
    for i, mel in enumerate(mels):
        ss.append(_stream(m, mel if i != late else mel[:R.FPR * 20], 64 if (grown and i % 2 == 0) else 0))
    assert ss[late].adapter_tokens == 20 < PROMPT + 1
    b = vox_hip.Batch(m, 64)
    c1 = [t.tolist() for t in b.decode(ss, max_steps=WIDE_CALL, stop_at_eos=False)]
    assert [len(t) for t in c1] == [WIDE_CALL] * late + [0]
    ss[late].encode_mel(mels[late][R.FPR * 20:])
    rows = [s.adapter_tokens for s in ss]
    # bounded rows: the late member's prompt goes through the stacked prefill on the batch queue
    c2 = [t.tolist() for t in b.decode(ss, max_steps=WIDE_CALL, stop_at_eos=False, rows=rows)]
    assert [len(t) for t in c2] == [WIDE_CALL] * WIDE_N
    out = dict(c1=c1, c2=c2, logits=[b.read_logits(s) for s in ss], rings=[_rings(s) for s in ss],
               slots=[s.kv_slots for s in ss], grow=b.kv_grow_stats(), stats=b.stats())
    b.close()
    for s in ss:
        s.close()
    return out


def test_wide_step_alternating_capacities(hm):
    """TINY, 33 streams on a 64-slot batch (the wide step's AttnSlots attention), alternating
    64-slot and full rings, two calls of 10 steps; the last member has 20 rows at the first call
    and joins at the second through the stacked prefill while the others run on.  Against the same
    streams on full rings: ids of both calls, last-step logits and every ring row to the bit."""
    run = _batched_wide(hm, True)
    twin = _batched_wide(hm, False)
    assert run["slots"] == [64 if i % 2 == 0 else 112 for i in range(WIDE_N)]
    assert twin["slots"] == [112] * WIDE_N
    assert run["grow"]["ragged_calls"] == 2 and run["grow"]["ragged_replays"] == 2 * WIDE_CALL
    assert run["stats"]["replays"] == 2 * WIDE_CALL == twin["stats"]["replays"]
    assert twin["grow"] == dict(ragged_calls=0, ragged_replays=0, ragged_captures=0)
    assert run["c1"] == twin["c1"] and run["c2"] == twin["c2"]
    for a, c in zip(run["logits"], twin["logits"]):
        assert np.array_equal(a, c)
    for a, c in zip(run["rings"], twin["rings"]):
        _same_rings(a, c)


# ---- invariant 4 ------------------------------------------------------------------------------------
def test_plain_stays_plain_once_every_ring_is_full(hm):
    """TINY: four full-ring streams capture the plain graph of their bucket; four streams created
    at 64 slots and grown to 112 then run the same call on the same batch with no new capture and
    no ragged replay; four streams still at 64 slots take a ragged capture and ragged replays."""
    import vox_hip
    mels = [_mel(hm.cfg, 9600 + i, 8) for i in range(4)]
    b = vox_hip.Batch(hm, 4)
    full = [_stream(hm, mel) for mel in mels]
    want = [t.tolist() for t in b.decode(full, max_steps=8, stop_at_eos=False)]
    st0 = b.stats()
    assert st0["captures"] == 1 and b.kv_grow_stats()["ragged_replays"] == 0
    grown = [_stream(hm, mel, 64) for mel in mels]
    for s in grown:
        s.reserve_kv(112)
        assert s.kv_slots == 112 and s.kv_grow_stats()["grows"] == 1
    got = [t.tolist() for t in b.decode(grown, max_steps=8, stop_at_eos=False)]
    st1 = b.stats()
    assert got == want
    assert st1["captures"] == st0["captures"] and st1["replays"] == st0["replays"] + 8
    assert b.kv_grow_stats() == dict(ragged_calls=0, ragged_replays=0, ragged_captures=0)
    short = [_stream(hm, mel, 64) for mel in mels]
    got = [t.tolist() for t in b.decode(short, max_steps=8, stop_at_eos=False)]
    assert got == want and [s.kv_slots for s in short] == [64] * 4
    assert b.stats()["captures"] == st1["captures"] + 1
    assert b.kv_grow_stats() == dict(ragged_calls=1, ragged_replays=8, ragged_captures=1)
    b.close()
    for s in full + grown + short:
        s.close()


# ---- reserve, reset ---------------------------------------------------------------------------------
def test_reserve_kv_grows_ahead_and_is_refused_in_a_begun_call(hm_long):
    """reserve_kv(300) on a fresh 64-slot stream: 512 slots, nothing to copy; the 200 steps that
    follow grow nothing.  reserve_kv(600) at position 238 copies exactly those rows -- the ring
    read back is kv_grow_ref.repitch of the ring before -- and the session goes on with the
    reference ids.  Inside a begun call the reservation is refused with the begun-call message
    and changes nothing."""
    import vox_hip
    from vox_weights import TINY_LONG
    L = vox_hip.lib()
    single = _single(hm_long, "long", 0)
    s = _stream(hm_long, R.session_mel("long"), 64)
    s.reserve_kv(300)
    assert s.kv_grow_stats() == dict(grows=1, copied=0, slots=R.grow_cap(64, 8256, 300)) and s.kv_slots == 512
    ids = s.decode(max_steps=200, stop_at_eos=False).tolist()
    assert s.kv_grow_stats() == dict(grows=1, copied=0, slots=512)
    pos = s.state()["kv_pos"]
    assert pos == PROMPT + 200
    before = _rings(s)
    s.reserve_kv(600)
    assert s.kv_slots == 1024 and s.kv_bytes == R.ring_bytes(TINY_LONG, 1024, 4)
    assert s.kv_grow_stats() == dict(grows=2, copied=R.ring_bytes(TINY_LONG, pos, 4), slots=1024)
    after = _rings(s)
    C = TINY_LONG.dec_kv_heads * TINY_LONG.dec_head_dim
    for w in range(2):
        old = np.zeros((TINY_LONG.dec_layers, 512, C), np.float32)
        for l in range(TINY_LONG.dec_layers):
            old[l, :pos] = before[l][w]
        new = R.repitch(old, np.zeros((TINY_LONG.dec_layers, 1024, C), np.float32), pos)
        for l in range(TINY_LONG.dec_layers):
            assert np.array_equal(after[l][w], new[l, :pos])
    s.reserve_kv(100)                                  # already held: nothing happens
    assert s.kv_grow_stats()["grows"] == 2
    b = vox_hip.Batch(hm_long, 4)
    seen = {}

    def between():
        st = s.kv_grow_stats()
        rc = L.vox_hip_stream_reserve_kv(s.h, 5000)
        msg = L.vox_hip_last_error() or b""
        seen["refused"] = rc != 0 and b"begun call" in msg
        seen["same"] = s.kv_grow_stats() == st and s.kv_slots == 1024
        L.vox_hip_clear_error()

    call = _begin_finish(b, [s], 24, between)
    assert seen == dict(refused=True, same=True)
    ids += call[0]
    assert ids == single["ids"][:224]
    s.reserve_kv(5000)                                 # the call is over
    assert s.kv_slots == 8192
    s.reserve_kv(1 << 20)                              # never above the full ring
    assert s.kv_slots == 8256 and s.kv_grow_stats()["grows"] == 4
    b.close()
    s.close()


def test_reset_returns_to_slots0_and_reset_decoder_keeps(hm_long):
    """stream_reset (new audio, the scheduler's slot reuse) gives the rings' growth back --
    vox_hip_memory_used drops by exactly the difference -- and the stream then runs the reference
    session again from 64 slots; stream_reset_decoder (the continuous-mode restart) keeps the
    capacity."""
    import vox_hip
    from vox_weights import TINY_LONG
    L = vox_hip.lib()
    single = _single(hm_long, "long", 0)
    mel = R.session_mel("long")
    s = _stream(hm_long, mel, 64)
    # the first call makes what a stream allocates once (prefill planes, the rope table's rows)
    ids = s.decode(max_steps=10, stop_at_eos=False).tolist()
    assert s.kv_slots == 64
    m0 = L.vox_hip_memory_used()
    ids += s.decode(max_steps=240, stop_at_eos=False).tolist()
    assert ids == single["ids"][:250]
    assert s.kv_slots == 512 and s.kv_grow_stats()["grows"] == 1
    m1 = L.vox_hip_memory_used()
    assert m1 - m0 == R.ring_bytes(TINY_LONG, 512, 4) - R.ring_bytes(TINY_LONG, 64, 4)
    assert L.vox_hip_stream_reset_decoder(s.h) == 0
    assert s.kv_slots == 512 and L.vox_hip_memory_used() == m1
    s.reset()
    assert s.kv_slots == 64 and s.kv_bytes == R.ring_bytes(TINY_LONG, 64, 4)
    assert L.vox_hip_memory_used() == m0
    for i in range(0, mel.shape[0], CHUNK):
        s.encode_mel(mel[i:i + CHUNK])
    assert s.decode(max_steps=100, stop_at_eos=False).tolist() == single["ids"][:100]
    assert s.kv_slots == 256 and s.kv_grow_stats()["grows"] == 2
    s.close()


# ---- the scheduler ------------------------------------------------------------------------------------
def test_scheduler_serves_growing_streams_and_reuses_a_slot(hm_long, jfk_samples):
    """TINY_LONG, the switch at 64 slots, 6 staggered clips of 4..8 s through vh_sched_run under a
    step cap of 8: every stream's ids equal its own oracle session, every ring grew.  The first
    stream is then detached, reset -- back at 64 slots -- and serves a seventh clip on the same
    scheduler with that clip's oracle ids."""
    import vox_hip
    ref = R.sched_oracle(jfk_samples)
    audios, again = R.sched_audios(jfk_samples)
    ctx = vox_hip.HostCtx(hm_long)
    q = vox_hip.Scheduler(ctx, 8)
    q.set_step_cap(R.SCHED_STEP_CAP)
    ctx.set_kv_grow(64)
    try:
        ss = [vox_hip.HostStream(ctx, interval_s=R.SCHED_INTERVAL) for _ in audios]
    finally:
        ctx.set_kv_grow(0)
    assert [s.kv_slots() for s in ss] == [64] * 6

    def serve(streams, clips, starts):
        pos = [0] * len(clips)
        done = [False] * len(clips)
        ids = [[] for _ in clips]
        tick = 0
        while not all(done) or any(s.pending() for s in streams):
            for k, (a, s) in enumerate(zip(clips, streams)):
                if done[k] or tick < starts[k]:
                    continue
                if pos[k] < len(a):
                    s.feed(a[pos[k]:pos[k] + R.SCHED_PIECE])
                    pos[k] += R.SCHED_PIECE
                else:
                    s.finish()
                    done[k] = True
            q.run()
            for k, s in enumerate(streams):
                ids[k] += s.get()
            tick += 1
            assert tick < 400
        return ids

    for s in ss:
        q.attach(s)
    ids = serve(ss, audios, R.SCHED_STARTS)
    for k in range(6):
        assert len(ref[k]) > 50 and ids[k] == ref[k], (k, len(ids[k]), len(ref[k]))
    slots = [s.kv_slots() for s in ss]
    print("scheduler: ring slots after the clips", slots, q.stats())
    assert all(c in (128, 256) for c in slots), slots
    q.detach(ss[0])
    ss[0].reset()
    assert ss[0].kv_slots() == 64
    q.attach(ss[0])
    ids2 = serve([ss[0]], [again], [0])
    assert ids2[0] == ref[6], (len(ids2[0]), len(ref[6]))
    assert ss[0].kv_slots() >= 128
    for s in ss:
        q.detach(s)
        s.close()
    q.close()
    ctx.close()
