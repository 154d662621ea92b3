"""Adapter-buffer growth, alone and under a begun batched call.

A stream's adapter rows live in one device buffer that doubles when an encoder pass needs more
(stream_alloc_adapter, csrc/vox_hip.hip): new buffer, copy of the rows, the stream's step graphs
captured again on the new address.  At the default first capacity of 1024 rows (82 s of audio)
no test reached that path; vox_hip_set_adapter_rows0 brings it down to 16 or 64 rows.

Between vox_hip_batch_begin_rows and vox_hip_batch_finish the call's slot table holds each
member's adapter pointer, and the scheduler enqueues its encoder pass exactly there.  A growth
in that window used to free the buffer the later chunks of steps read.  These tests grow members
inside the window -- through vox_hip_stream_encode_mel, through _encode_mel_batch, on the wide
step, in a call of mixed delays, with --alt members, and through vh_sched_run -- and hold every
id to the CPU oracle and ids, logits and adapter rows bit for bit to a twin run that encodes the
same mel after finish (growth is a copy; the kernels and their order do not depend on it).

Every test that grows asserts from vox_hip_stream_adapter_stats that it grew, and every test of
the window that a member grew inside a begun call that ran more than one chunk of 16 steps.
Inputs and oracle runs: tests/adapter_growth_ref.py (margins and row schedules are pinned on the
CPU by tests/test_adapter_growth_cpu.py)."""
import ctypes

import numpy as np
import pytest

import adapter_growth_ref as R
from adapter_growth_ref import LOGIT_TOL, MARGIN, STEP_BATCH

pytestmark = pytest.mark.gpu

IP = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def hm():
    import vox_hip
    from vox_weights import TINY
    m = vox_hip.Model(TINY, R.weights())
    yield m
    m.close()


def _rel(a, b):
    """max |a - b| as a fraction of the largest |b|"""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-6, float(np.max(np.abs(b)))))


# ---- a. one stream --------------------------------------------------------------------------------
def _single_run(hm, rows0):
    import vox_hip
    vox_hip.set_adapter_rows0(rows0)
    try:
        s = vox_hip.Stream(hm)
    finally:
        vox_hip.set_adapter_rows0(0)
    assert s.adapter_stats() == dict(cap=rows0 or 1024, grows=0, grows_held=0)
    ids, lg, rows = R.single_schedule(s, R.single_mel())
    out = dict(ids=ids, logits=lg, rows=rows, adapter=s.read_adapter(), stats=s.adapter_stats())
    s.close()
    return out


def test_single_stream_grows_under_decode(hm):
    """Capacity 16, the ragged schedule of adapter_growth_ref (355, 50, 50, 1, 2, 7, 200, 3 and
    50s: 296 rows), a decode after every chunk: the step graph captured on the old buffer is
    replayed after each of the four growths (16 -> 64 before the prompt exists, -> 128, -> 256,
    -> 512).  Ids, adapter rows and every step's logits against the oracle (5e-5); all of them bit
    for bit against the same schedule at the default capacity, which never grows."""
    ref = R.single_oracle()
    assert R.worst_margin(ref["logits"]) >= MARGIN
    small = _single_run(hm, 16)
    big = _single_run(hm, 0)
    # the guards: it grew, the first time with no prompt row in the buffer; the default did not
    assert small["stats"]["grows"] >= 4 and small["stats"]["cap"] == 512, small["stats"]
    assert small["rows"][0] > 16 and ref["rows"][0] == small["rows"][0]
    assert big["stats"] == dict(cap=1024, grows=0, grows_held=0)
    assert small["stats"]["grows_held"] == 0
    assert small["rows"] == ref["rows"] == big["rows"] and small["rows"][-1] == 296
    # the oracle
    assert len(ref["ids"]) == 296 - 38 and small["ids"] == ref["ids"]
    err_ad = _rel(small["adapter"], ref["adapter"])
    err_lg = max(_rel(g, o) for g, o in zip(small["logits"], ref["logits"]))
    print(f"single stream: adapter rows {err_ad:.2e}, logits {err_lg:.2e} of the oracle's largest")
    assert err_ad < LOGIT_TOL and err_lg < LOGIT_TOL
    # growth is a copy
    assert big["ids"] == small["ids"]
    assert np.array_equal(big["adapter"], small["adapter"])
    assert np.array_equal(big["logits"], small["logits"])


def test_growth_before_the_prompt_exists(hm):
    """the first chunk of the schedule at capacity 16: 44 rows arrive in one pass, the buffer goes
    16 -> 64 with nothing to copy, and no decoder step has run"""
    import vox_hip
    vox_hip.set_adapter_rows0(16)
    try:
        s = vox_hip.Stream(hm)
    finally:
        vox_hip.set_adapter_rows0(0)
    mel = R.single_mel()[:R.SINGLE_CHUNKS[0]]
    assert s.encode_mel(mel) == 44
    assert s.adapter_stats() == dict(cap=64, grows=1, grows_held=0)
    assert s.state()["started"] == 0
    assert _rel(s.read_adapter(), R.single_oracle()["adapter"][:44]) < LOGIT_TOL
    s.close()


# ---- b. a begun call ------------------------------------------------------------------------------
class Begun:
    """One run of adapter_growth_ref's begun-call case on the GPU: streams at capacity 64 with
    60..63 rows, one batched step to start them, vox_hip_batch_begin_rows bounded to those rows,
    the growing members' next 10 rows encoded before (inside=True) or after vox_hip_batch_finish,
    then the drain of those rows.  between: called after begin with the run, for the refusals."""

    def __init__(self, hm, name, inside, between=None):
        import vox_hip
        L = vox_hip.lib()
        n, cap, grow, delays, alts, _ = R.BEGUN[name]
        mels = R.begun_mels(name)
        vox_hip.set_adapter_rows0(64)   # before any stream exists
        try:
            self.ss = ss = [vox_hip.Stream(hm) for _ in range(n)]
        finally:
            vox_hip.set_adapter_rows0(0)
        self.b = b = vox_hip.Batch(hm, cap)
        for i, s in enumerate(ss):
            assert s.adapter_stats()["cap"] == 64
            if delays is not None:
                s.set_delay(R.begun_delay(name, i))
            if i in alts:
                s.set_alt(3, 0.5)
            assert s.encode_mel(mels[i][0]) == R.begun_rows(i)
        self.start = [t.tolist() for t in b.decode(ss, max_steps=1, stop_at_eos=False)]
        assert all(len(t) == 1 for t in self.start)
        self.rows = rows = np.array([s.adapter_tokens for s in ss], np.int32)
        self.allowed = [int(rows[i]) - s.state()["gen_pos"] for i, s in enumerate(ss)]
        arr = (ctypes.c_void_p * n)(*[s.h for s in ss])
        toks = np.zeros((n, R.BEGUN_STEPS), np.int32)
        self.cnt = cnt = np.zeros(n, np.int32)
        assert L.vox_hip_batch_begin_rows(b.h, arr, n, rows.ctypes.data_as(IP), R.BEGUN_STEPS, 0,
                                          toks.ctypes.data_as(IP), cnt.ctypes.data_as(IP)) == 0, L.vox_hip_last_error()

        def encode():
            gs = [i for i in range(n) if mels[i][1] is not None]
            assert tuple(gs) == tuple(sorted(grow))
            if name == "enc_batch":
                # as the scheduler's pass: every member listed, those without a chunk with 0 frames
                empty = np.zeros((0, hm.cfg.mel_bins), np.float32)
                added = vox_hip.encode_mel_batch(ss, [empty if m[1] is None else m[1] for m in mels])
                assert added == [0 if m[1] is None else R.GROW_ROWS for m in mels]
            else:
                for i in gs:
                    assert ss[i].encode_mel(mels[i][1]) == R.GROW_ROWS

        if inside:
            encode()
        if between:
            between(self)
        self.total = L.vox_hip_batch_finish(b.h)
        assert self.total >= 0, L.vox_hip_last_error()
        if not inside:
            encode()
        self.call = [toks[i, :cnt[i]].tolist() for i in range(n)]
        # logits of the call's last step, for the members that ran to it
        last = int(cnt.max())
        self.logits = {i: b.read_logits(ss[i]) for i in range(n) if cnt[i] == last}
        self.stats = [s.adapter_stats() for s in ss]
        self.drain = [t.tolist() for t in b.decode(ss, max_steps=64, stop_at_eos=False)]
        self.adapter = [s.read_adapter() for s in ss]
        self.alts = {i: ss[i].read_alts(0, ss[i].state()["generated"]) for i in alts}

    def close(self):
        for s in self.ss:
            s.close()
        self.b.close()


def _check_begun(name, run, twin):
    """run grew inside the window, twin after it: the guards, the oracle, the bits"""
    n, _, grow, _, alts, _ = R.BEGUN[name]
    ref = R.begun_oracle(name)
    assert min(R.worst_margin(x["logits"]) for x in ref) >= MARGIN
    # the guards: the growing members grew inside the begun call, the others not at all, and
    # the call ran more than one chunk
    for i in range(n):
        want = dict(cap=128, grows=1, grows_held=1) if i in grow else dict(cap=64, grows=0, grows_held=0)
        assert run.stats[i] == want, (i, run.stats[i])
        assert twin.stats[i] == dict(want, grows_held=0), (i, twin.stats[i])
    assert R.BEGUN_STEPS > STEP_BATCH and all(int(run.cnt[i]) > STEP_BATCH for i in grow), run.cnt
    # counts are what the bound allows: every row the stream had at begin, none of the new ones
    assert run.cnt.tolist() == run.allowed == [len(x["call"]) for x in ref]
    assert run.total == int(run.cnt.sum())
    # the oracle's ids, before, in and after the call
    for i in range(n):
        assert run.start[i] == ref[i]["start"], i
        assert run.call[i] == ref[i]["call"], (i, run.call[i], ref[i]["call"])
        assert run.drain[i] == ref[i]["drain"], i
        assert _rel(run.adapter[i], ref[i]["adapter"]) < LOGIT_TOL, i
    # the twin's bits
    assert twin.cnt.tolist() == run.cnt.tolist()
    assert twin.call == run.call and twin.drain == run.drain and twin.start == run.start
    assert sorted(run.logits) == sorted(twin.logits) and len(run.logits) >= 1
    for i in run.logits:
        assert np.array_equal(run.logits[i], twin.logits[i]), i
    for i in range(n):
        assert np.array_equal(run.adapter[i], twin.adapter[i]), i
    for i in alts:
        assert np.array_equal(run.alts[i][0], twin.alts[i][0]) and np.array_equal(run.alts[i][1], twin.alts[i][1]), i
        assert run.alts[i][0][:, 0].tolist() == run.start[i] + run.call[i] + run.drain[i]
    if alts:
        assert any((run.alts[i][0][:, 1] >= 0).any() for i in alts), "no alternative was ever accepted"


@pytest.mark.parametrize("name", list(R.BEGUN))
def test_growth_inside_a_begun_call(hm, name):
    """Members of a begun call outgrow their adapter buffers (64 -> 128 rows) between begin_rows
    and finish, and finish then runs the call's second chunk of steps through the slot table
    uploaded at begin.  plain: vox_hip_stream_encode_mel on two members of four; enc_batch: one
    vox_hip_stream_encode_mel_batch over all four, as the scheduler's pass; wide33: 33 streams on
    a 64-slot batch (the wide step's slot-table attention and k_gemmf projections); mixed_delay:
    delays 6, 3, 10 and 1 in one call (19..29 steps); alt: two --alt members, one of them growing
    (the slot's alternatives and token rings).  Ids = the oracle's; counts = what the bound allows;
    ids, the last step's logits, adapter rows and alternatives = the twin's bits."""
    run = Begun(hm, name, inside=True)
    twin = Begun(hm, name, inside=False)
    try:
        _check_begun(name, run, twin)
    finally:
        run.close()
        twin.close()


# ---- c. refusals ----------------------------------------------------------------------------------
def test_begun_call_refuses_what_would_move_its_buffers(hm):
    """Between begin_rows and finish every entry point that would free, move or rewrite what the
    slot table names, or move a member's decoder, returns an error that names the begun call and
    changes nothing: stream_free, _reset, _reset_decoder, _decode, the decoder twins, _set_alt,
    _set_delay, a second call that lists a member, and model_set_delay.  Encoding stays allowed
    (the plain case's two members grow meanwhile).  finish then delivers the oracle's ids, and
    every call works again afterwards."""
    import vox_hip
    L = vox_hip.lib()
    seen = []

    def refused(what, rc):
        msg = L.vox_hip_last_error() or b""
        assert rc != 0 and b"begun call" in msg, (what, rc, msg)
        seen.append(what)
        L.vox_hip_clear_error()

    def between(run):
        s = run.ss[1]
        cfg = s.cfg
        before = s.state()
        L.vox_hip_clear_error()
        L.vox_hip_stream_free(s.h)   # void: the error alone
        refused("stream_free", -1 if L.vox_hip_last_error() else 0)
        refused("stream_reset", L.vox_hip_stream_reset(s.h))
        refused("stream_reset_decoder", L.vox_hip_stream_reset_decoder(s.h))
        tok = np.zeros(4, np.int32)
        refused("stream_decode", L.vox_hip_stream_decode(s.h, 4, 0, tok.ctypes.data_as(IP), None))
        x = np.zeros((1, cfg.dec_dim), np.float32)
        rope = np.zeros(cfg.dec_head_dim, np.float32)
        refused("decoder_prefill_step", L.vox_hip_decoder_prefill_step(s.h, vox_hip.fptr(x), 1, vox_hip.fptr(rope), 0))
        refused("decoder_full_step", L.vox_hip_decoder_full_step(s.h, vox_hip.fptr(rope), 0, None))
        refused("stream_set_alt", L.vox_hip_stream_set_alt(s.h, 3, 0.5))
        refused("stream_set_delay", L.vox_hip_stream_set_delay(s.h, 3))
        refused("model_set_delay", L.vox_hip_model_set_delay(run.ss[0].model.h, 3))
        other = vox_hip.Batch(hm, 4)
        arr = (ctypes.c_void_p * 1)(s.h)
        one = np.zeros(1, np.int32)
        refused("second batch", L.vox_hip_batch_decode(other.h, arr, 1, 1, 0, one.ctypes.data_as(IP),
                                                       one.ctypes.data_as(IP)))
        other.close()
        assert s.state() == before and s.adapter_tokens == R.begun_rows(1) + R.GROW_ROWS

    run = Begun(hm, "plain", inside=True, between=between)
    twin = Begun(hm, "plain", inside=False)
    try:
        assert len(seen) == 10, seen
        _check_begun("plain", run, twin)
        # the window is over: the same calls work, on a member that went through it
        s = run.ss[1]
        assert L.vox_hip_stream_set_alt(s.h, 1, 0.0) == 0
        assert L.vox_hip_model_set_delay(hm.h, hm.delay_tokens) == 0
        assert L.vox_hip_stream_reset(s.h) == 0 and s.adapter_tokens == 0
    finally:
        run.close()
        twin.close()


# ---- d / e. the scheduler -------------------------------------------------------------------------
def _serve(hm_long, audios, fail_at=None):
    """tests/test_gpu_sched.py's serving loop in 4 s pieces under a step cap of 24, lifted to 0 (a
    run drains everything) once every stream has finished.  fail_at: the tick whose run is told
    to fail its encoder pass; returns (ids, stats per stream, scheduler stats, failed runs)."""
    import vox_hip
    ctx = vox_hip.HostCtx(hm_long)
    q = vox_hip.Scheduler(ctx, 4)
    q.set_step_cap(R.SCHED_STEP_CAP)
    vox_hip.set_adapter_rows0(R.SCHED_CAP0)   # before any stream exists
    try:
        ss = [vox_hip.HostStream(ctx, interval_s=R.SCHED_INTERVAL) for _ in audios]
    finally:
        vox_hip.set_adapter_rows0(0)
    for s in ss:
        q.attach(s)
    pos = [0] * len(audios)
    done = [False] * len(audios)
    ids = [[] for _ in audios]
    failed = []
    tick = 0
    while not all(done) or any(s.pending() for s in ss):
        for k, (a, s) in enumerate(zip(audios, ss)):
            if done[k] or tick < R.SCHED_STARTS[k]:
                continue
            if pos[k] < len(a):
                s.feed(a[pos[k]:pos[k] + R.SCHED_PIECE])
                pos[k] += R.SCHED_PIECE
            else:
                s.finish()
                done[k] = True
        if all(done):
            q.set_step_cap(0)
        if tick == fail_at:
            q.fail_next_encode()
            with pytest.raises(RuntimeError, match="vh_sched_debug_fail_next_encode"):
                q.run()
            failed.append(tick)
        else:
            q.run()
        for k, s in enumerate(ss):
            ids[k] += s.get()
        tick += 1
        assert tick < 200
    stats = [s.adapter_stats() for s in ss]
    st = q.stats()
    for s in ss:
        s.close()
    q.close()
    ctx.close()
    return ids, stats, st, failed


@pytest.fixture(scope="module")
def hm_long():
    import vox_hip
    from vox_weights import TINY_LONG
    m = vox_hip.Model(TINY_LONG, R.weights())
    yield m
    m.close()


@pytest.mark.parametrize("overlap", ["1", "0"])
def test_scheduler_grows_inside_its_begun_calls(hm_long, jfk_samples, monkeypatch, overlap):
    """4 staggered streams of 12..25 s at capacity 64, 4 s pieces (about 50 rows per tick), a step
    cap of 24 and 0 for the drain after the last finish.  With the overlap every run after a
    stream's first begins 24 steps for it (two chunks) and enqueues the pass that takes its
    buffer past 128 and 256 rows before it finishes them (the schedule: adapter_growth_ref.
    sched_row_schedule); without it the same growths happen outside any call.  Every stream's
    ids = its oracle session's."""
    monkeypatch.setenv("VOX_HIP_SCHED_OVERLAP", overlap)
    ref = R.sched_oracle(jfk_samples)
    ids, stats, st, _ = _serve(hm_long, R.sched_audios(jfk_samples))
    print("scheduler", overlap, stats, st)
    for k, (want, rows) in enumerate(ref):
        assert len(want) > 100
        assert ids[k] == want, (k, len(ids[k]), len(want))
        assert stats[k]["grows"] >= 2 and stats[k]["cap"] >= rows[-1], (k, stats[k])
    held = [s["grows_held"] for s in stats]
    if overlap == "1":
        assert R.SCHED_STEP_CAP > STEP_BATCH and all(h >= 1 for h in held), held
    else:
        assert held == [0] * len(stats), held


def test_scheduler_survives_a_failed_encoder_pass(hm_long, jfk_samples, monkeypatch):
    """vh_sched_debug_fail_next_encode at tick 2, when three streams have steps begun: that run
    finishes its begun call, queues its ids and returns the error; every later run works (before
    the fix the batch refused them all: "a begun call was not finished"), the chunks the failed
    pass left deferred are encoded by the next feed or run, and every stream's ids = its oracle
    session's: none lost, none repeated."""
    monkeypatch.setenv("VOX_HIP_SCHED_OVERLAP", "1")
    ref = R.sched_oracle(jfk_samples)
    ids, stats, st, failed = _serve(hm_long, R.sched_audios(jfk_samples), fail_at=2)
    assert failed == [2]
    for k, (want, _) in enumerate(ref):
        assert ids[k] == want, (k, len(ids[k]), len(want))
    assert any(s["grows_held"] >= 1 for s in stats), stats
