"""Per-stream transcription delay (vox_hip_stream_set_delay): streams of one model
at delays of their own, alone, in one batched call (the per-slot norm instances of the 32-slot and
the wide step, one stacked prefill pass per distinct delay) and on one scheduler.

The runs and their CPU-oracle references are tests/delay_ref.py's; tests/test_stream_delay_cpu.py
pins, on the oracle alone, the margin rule for every (delay, frames, seed) used here and that a
wrong ada table moves the logits by far more than the bars.  Each stream's reference is its own
oracle session on an OracleModel at its delay: ids equal, the named steps' logits within 5e-5 of
that step's largest oracle logit (1e-4 on half rings).  Stream i of a run has delay
(1, 3, 6, 12, 30)[i % 5]; the model is at 6, and every other stream of delay 6 follows the model
instead of carrying the delay itself, so a mixed call holds both kinds.

Without the feature vox_hip_stream_set_delay does not exist and every test here fails."""
import numpy as np
import pytest

import delay_ref as d
from delay_ref import KV8, LOGIT_TOL, LOGIT_TOL16, MARGIN_F32, MARGIN_KV16
from vox_weights import TINY

pytestmark = pytest.mark.gpu


def _delay_arg(i):
    """what stream i is given: its delay, or None (follow the model) for every other delay-6 stream"""
    dl = d.delay_of(i)
    return None if dl == d.MODEL_DELAY and (i // 5) % 2 == 0 else dl


def _open(hm, mels, delays, kv16=False):
    import vox_hip
    hm.set_kv_fp16(kv16)
    ss = [vox_hip.Stream(hm) for _ in mels]
    hm.set_kv_fp16(False)
    for s, mel, dl in zip(ss, mels, delays):
        assert s.kv_fp16 == kv16
        if dl is not None:
            s.set_delay(dl)
        assert s.delay_tokens == (d.MODEL_DELAY if dl is None else dl)
        s.encode_mel(mel)
    return ss


def _stepwise(hm, mels, delays, slots, steps=6, kv16=False):
    """One Batch over all the streams: `steps` single-step calls reading the logits of `slots`
    after each, then the drain.  Returns (ids per stream, {slot: [steps, vocab]}, stats)."""
    import vox_hip
    ss = _open(hm, mels, delays, kv16)
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
    st = b.stats()
    for s in ss:
        s.close()
    b.close()
    return got, {i: np.stack(v) for i, v in lg.items()}, st


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))


def _compare(got, lg, ref, tol, what):
    for i, (ids, _) in enumerate(ref):
        first_diff = next((k for k in range(min(len(ids), len(got[i]))) if got[i][k] != ids[k]), None)
        assert first_diff is None and len(got[i]) == len(ids), (what, i, first_diff, len(got[i]), len(ids))
    worst = 0.0
    for i, l in lg.items():
        for k in range(l.shape[0]):
            r = _rel(l[k], ref[i][1][k])
            worst = max(worst, r)
            print(f"{what}: slot {i} (delay {d.delay_of(i)}) step {k}: logit err {r:.2e}")
            assert r < tol, (what, i, k, r)
    print(f"{what}: {sum(len(g) for g in got)} ids equal, worst logit err {worst:.2e} (bar {tol:.0e})")


@pytest.fixture(scope="module")
def kv8_model():
    import vox_hip
    hm = vox_hip.Model(KV8, d.weights(KV8), d.MODEL_DELAY)
    yield hm
    hm.close()


@pytest.fixture(scope="module")
def tiny_model():
    import vox_hip
    hm = vox_hip.Model(TINY, d.weights(TINY), d.MODEL_DELAY)
    yield hm
    hm.close()


# ---- 1. tables --------------------------------------------------------------------------------
def test_stream_tables_equal_a_model_created_at_the_delay(tiny_model):
    import vox_hip
    st = vox_hip.Stream(tiny_model)
    assert st.delay_tokens == d.MODEL_DELAY
    assert np.array_equal(st.ada_scale(), tiny_model.ada_scale())
    for dl in (0, 1, 3, 12, 30):
        st.set_delay(dl)
        assert st.delay_tokens == dl
        hm = vox_hip.Model(TINY, d.weights(TINY), dl)
        want = hm.ada_scale()
        hm.close()
        assert np.array_equal(st.ada_scale(), want), dl
        assert dl == d.MODEL_DELAY or not np.array_equal(want, tiny_model.ada_scale())
    st.set_delay(None)
    assert st.delay_tokens == d.MODEL_DELAY and np.array_equal(st.ada_scale(), tiny_model.ada_scale())
    st.close()


# ---- 2. single stream --------------------------------------------------------------------------
def test_single_streams_at_12_and_1_on_a_model_at_6(tiny_model):
    """streams 3 (delay 12) and 0 (delay 1) of the single run: ids to the end and the logits of
    six steps against the oracle at that delay; the prompt boundary 1 + 32 + d"""
    import vox_hip
    ref = d.oracle("single", only=(0, 3))
    d.assert_margin(ref, MARGIN_F32, "single streams")
    mels = d.mels("single")
    for i in (3, 0):
        dl = d.delay_of(i)
        ids, olg = ref[i]
        st = vox_hip.Stream(tiny_model)
        st.set_delay(dl)
        st.encode_mel(mels[i])
        toks, lg = st.decode(max_steps=6, stop_at_eos=False, want_logits=True)
        rest = st.decode(stop_at_eos=False)
        got = toks.tolist() + rest.tolist()
        assert got == ids, (dl, len(got), len(ids))
        for k in range(6):
            r = _rel(lg[k], olg[k])
            print(f"single stream delay {dl} step {k}: logit err {r:.2e}")
            assert r < LOGIT_TOL, (dl, k, r)
        st.close()
        # 1 + 32 + d - 1 adapter rows: nothing; one more row: the first token
        st = vox_hip.Stream(tiny_model)
        st.set_delay(dl)
        st.encode_mel(mels[i][:8 * (32 + dl)])
        assert st.adapter_tokens == 32 + dl
        assert len(st.decode(stop_at_eos=False)) == 0 and st.state()["started"] == 0
        st.encode_mel(mels[i][8 * (32 + dl):8 * (33 + dl)])
        assert st.adapter_tokens == 33 + dl
        first = st.decode(stop_at_eos=False)
        assert first.tolist() == ids[:1]
        st.close()


# ---- 3. errors ---------------------------------------------------------------------------------
def test_set_delay_errors_and_reset(tiny_model):
    import vox_hip
    ref = d.oracle("single", only=(0, 3))
    mels = d.mels("single")
    st = vox_hip.Stream(tiny_model)
    for bad in (31, -2):
        with pytest.raises(RuntimeError, match="stream_set_delay"):
            st.set_delay(bad)
    assert st.delay_tokens == d.MODEL_DELAY
    st.set_delay(12)
    st.encode_mel(mels[3])
    assert st.decode(max_steps=1, stop_at_eos=False).tolist() == ref[3][0][:1]
    with pytest.raises(RuntimeError, match="decoder has started"):
        st.set_delay(1)
    assert st.delay_tokens == 12
    st.reset()
    assert st.delay_tokens == 12   # a reset keeps the delay, and allows a new one
    st.set_delay(1)
    st.encode_mel(mels[0])
    assert st.decode(stop_at_eos=False).tolist() == ref[0][0]
    st.close()


# ---- 4. 32 slots -------------------------------------------------------------------------------
def test_32_slots_mixed_delays(kv8_model):
    """KV8, 32 streams, delays cycling over the slots so both 16-row blocks are mixed
    (k_resid_xw_fplanes_slot); logits of slots 0, 15, 16, 31 on six steps; one stacked prefill
    pass per distinct delay"""
    ref = d.oracle("f32", 32)
    d.assert_margin(ref, MARGIN_F32, "32 mixed slots")
    got, lg, st = _stepwise(kv8_model, d.mels("f32", 32), [_delay_arg(i) for i in range(32)], (0, 15, 16, 31))
    _compare(got, lg, ref, LOGIT_TOL, "32 mixed slots")
    assert st["prefill_passes"] == len(d.DELAYS) and st["prefilled"] == 32, st


# ---- 5. wide step ------------------------------------------------------------------------------
def test_wide_64_mixed(kv8_model):
    ref = d.oracle("f32", 64)
    d.assert_margin(ref, MARGIN_F32, "wide 64 mixed")
    got, lg, st = _stepwise(kv8_model, d.mels("f32", 64), [_delay_arg(i) for i in range(64)], (0, 15, 16, 31, 32, 63))
    _compare(got, lg, ref, LOGIT_TOL, "wide 64 mixed")
    assert st["prefill_passes"] == len(d.DELAYS) and st["prefilled"] == 64, st


def test_wide_33_mixed_dead_rows(kv8_model):
    ref = d.oracle("f32", 33)
    d.assert_margin(ref, MARGIN_F32, "wide 33 mixed")
    got, lg, _ = _stepwise(kv8_model, d.mels("f32", 33), [_delay_arg(i) for i in range(33)], (0, 32))
    _compare(got, lg, ref, LOGIT_TOL, "wide 33 mixed")


def test_wide_q8_64_mixed_row_major_norm():
    """a Q8 model with the k_gemmf switch off: the row-major layers, k_rmsnorm_rows_slot"""
    import vox_hip
    assert vox_hip.gemmf_q8() == 0
    ref = d.oracle("q8", 64)
    d.assert_margin(ref, MARGIN_F32, "wide q8 64 mixed")
    hm = vox_hip.Model(KV8, d.weights(KV8, q8=True), d.MODEL_DELAY)
    got, lg, _ = _stepwise(hm, d.mels("q8", 64), [_delay_arg(i) for i in range(64)], (0, 15, 16, 31, 32, 63))
    hm.close()
    _compare(got, lg, ref, LOGIT_TOL, "wide q8 64 mixed")


def test_wide_half_rings_40_mixed(kv8_model):
    ref = d.oracle("kv16", 40)
    d.assert_margin(ref, MARGIN_KV16, "wide kv16 40 mixed")
    got, lg, _ = _stepwise(kv8_model, d.mels("kv16", 40), [_delay_arg(i) for i in range(40)], (0, 15, 16, 31, 32, 39),
                           kv16=True)
    _compare(got, lg, ref, LOGIT_TOL16, "wide kv16 40 mixed")


# ---- 6. same arithmetic ------------------------------------------------------------------------
def test_per_slot_path_is_bit_equal_to_the_shared_row_path(kv8_model):
    """16 streams each explicitly set to the model's delay (a mixed call: the per-slot instances)
    against 16 following the model (a plain call): ids and every slot's logits of six steps"""
    import vox_hip
    mels = d.mels("f32", 16)
    runs = []
    for delay in (d.MODEL_DELAY, None):
        ss = _open(kv8_model, mels, [delay] * 16)
        b = vox_hip.Batch(kv8_model, 16)
        ids, lgs = [[] for _ in ss], []
        for _ in range(6):
            for i, t in enumerate(b.decode(ss, max_steps=1, stop_at_eos=False)):
                assert len(t) == 1
                ids[i] += t.tolist()
            lgs.append(np.stack([b.read_logits(s) for s in ss]))
        for i, t in enumerate(b.decode(ss, max_steps=1000, stop_at_eos=False)):
            ids[i] += t.tolist()
        runs.append((ids, np.stack(lgs)))
        for s in ss:
            s.close()
        b.close()
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1].view(np.uint32), runs[1][1].view(np.uint32))


# ---- 7. plain calls untouched ------------------------------------------------------------------
def test_plain_call_between_mixed_calls(kv8_model):
    """one Batch: a mixed call (streams 0..7), a plain one (8..15, following the model), a mixed
    one again (16..23); ids equal fresh Batches'; the plain bucket's capture count is a plain-only
    Batch's, and the second mixed call captures nothing"""
    import vox_hip
    mels = d.mels("f32", 24)
    groups = [(range(0, 8), True), (range(8, 16), False), (range(16, 24), True)]

    def run(b, idx, mixed):
        ss = _open(kv8_model, [mels[i] for i in idx], [d.delay_of(i) if mixed else None for i in idx])
        out = [t.tolist() for t in b.decode(ss, max_steps=1000, stop_at_eos=False)]
        for s in ss:
            s.close()
        return out
    fresh, plain_caps = [], None
    for idx, mixed in groups:
        b = vox_hip.Batch(kv8_model, 8)
        fresh.append(run(b, idx, mixed))
        if not mixed:
            plain_caps = b.stats()["captures"]
        b.close()
    ref = d.oracle("f32", 24)
    for (idx, mixed), out in zip(groups, fresh):
        if mixed:
            assert out == [ref[i][0] for i in idx]
    b = vox_hip.Batch(kv8_model, 8)
    caps = []
    for (idx, mixed), want in zip(groups, fresh):
        assert run(b, idx, mixed) == want, (list(idx), mixed)
        caps.append(b.stats()["captures"])
    b.close()
    assert plain_caps is not None and plain_caps > 0
    assert caps[1] - caps[0] == plain_caps and caps[2] == caps[1], (caps, plain_caps)


# ---- 8. GEMV switch ----------------------------------------------------------------------------
def test_mixed_call_takes_the_mfma_step_under_set_gemv_rows(kv8_model):
    import vox_hip
    ref = d.oracle("f32", 4)
    mels = d.mels("f32", 8)
    b = vox_hip.Batch(kv8_model, 4)
    assert b.set_gemv_rows(8) == 0
    ss = _open(kv8_model, mels[:4], [d.delay_of(i) for i in range(4)])
    got = [t.tolist() for t in b.decode(ss, max_steps=1000, stop_at_eos=False)]
    assert got == [ref[i][0] for i in range(4)]
    st, gst = b.stats(), b.gemv_stats()
    assert gst[0] == 8 and gst[1] == 0 and gst[2] == 0 and st["replays"] > 0, (st, gst)
    for s in ss:
        s.close()
    # a plain call right after takes the GEMV path as before
    ss = _open(kv8_model, mels[4:8], [None] * 4)
    got = [t.tolist() for t in b.decode(ss, max_steps=1000, stop_at_eos=False)]
    st2, gst2 = b.stats(), b.gemv_stats()
    assert gst2[1] == st2["replays"] - st["replays"] > 0 and gst2[2] == sum(len(g) for g in got), (st2, gst2)
    for s in ss:
        s.close()
    b.close()
    b = vox_hip.Batch(kv8_model, 4)
    ss = _open(kv8_model, mels[4:8], [None] * 4)
    assert got == [t.tolist() for t in b.decode(ss, max_steps=1000, stop_at_eos=False)]
    for s in ss:
        s.close()
    b.close()


# ---- 9. scheduler ------------------------------------------------------------------------------
PIECE = 8000   # 0.5 s of 16 kHz samples per feed
SCHED_MS = (80, 240, 480, 960, 2400, 960, 240, 2400)


def _solo(ctx, audio, delay_ms):
    """the single-stream host path alone at that delay"""
    import vox_hip
    s = vox_hip.HostStream(ctx, interval_s=0.5)
    s.set_delay(delay_ms)
    assert s.delay_ms() == delay_ms
    ids = []
    for i in range(0, len(audio), PIECE):
        s.feed(audio[i:i + PIECE])
        ids += s.get()
    s.finish()
    ids += s.get()
    s.close()
    return ids


def test_scheduler_streams_at_delays_of_their_own(tiny_weights, jfk_samples):
    """8 TINY_LONG streams on one vh_sched, staggered feeds of 0.5 s, delays set per stream
    through vh_stream_set_delay; each stream's ids equal the single-stream host path alone at that
    delay (the per-stream right pad at finish included); then slot 0's stream is reset and reused
    for another client at another delay"""
    import vox_hip
    from vox_weights import TINY_LONG
    hm = vox_hip.Model(TINY_LONG, tiny_weights)
    ctx = vox_hip.HostCtx(hm)
    long = np.concatenate([jfk_samples] * 2)
    lens = [2.5, 6.0, 3.5, 7.5, 5.0, 4.0, 8.0, 3.0]
    audios = [np.ascontiguousarray(long[int(k * 24000) % 16000:][:int(s * 16000)]) for k, s in enumerate(lens)]
    want = [_solo(ctx, a, ms) for a, ms in zip(audios, SCHED_MS)]
    assert all(len(w) > 0 for w in want) and len({len(w) for w in want}) > 4
    q = vox_hip.Scheduler(ctx, 8)
    ss = [vox_hip.HostStream(ctx, interval_s=0.5) for _ in audios]
    for s, ms in zip(ss, SCHED_MS):
        s.set_delay(ms)
        q.attach(s)

    def serve(idx, auds, starts):
        pos = {k: 0 for k in idx}
        done = {k: False for k in idx}
        ids = {k: [] for k in idx}
        tick = 0
        while not all(done.values()) or any(ss[k].pending() for k in idx):
            for k in idx:
                if done[k] or tick < starts[k]:
                    continue
                if pos[k] < len(auds[k]):
                    ss[k].feed(auds[k][pos[k]:pos[k] + PIECE])
                    pos[k] += PIECE
                else:
                    ss[k].finish()
                    done[k] = True
            q.run()
            for k in idx:
                ids[k] += ss[k].get()
            tick += 1
            assert tick < 400
        return ids
    ids = serve(range(8), audios, [2 * k for k in range(8)])
    for k in range(8):
        assert ids[k] == want[k], (k, SCHED_MS[k], len(ids[k]), len(want[k]))
    st = q.stats()
    assert st["tokens"] > st["prefills"] > 0 and st["batch_calls"] > 0, st
    # slot 0's stream for the next client, at 2400 ms where it served 80
    q.detach(ss[0])
    ss[0].reset()
    assert ss[0].delay_ms() == SCHED_MS[0]
    ss[0].set_delay(2400)
    q.attach(ss[0])
    again = serve([0], {0: audios[3]}, {0: 0})
    assert again[0] == _solo(ctx, audios[3], 2400)
    for s in ss:
        s.close()
    q.close()
    ctx.close()
    hm.close()
