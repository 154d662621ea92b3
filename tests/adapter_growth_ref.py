"""The inputs of tests/test_gpu_adapter_growth.py and their CPU-oracle references, shared with
tests/test_adapter_growth_cpu.py, which pins on the oracle alone what makes the GPU comparisons
mean something: the top-2 margin rule of tests/test_gpu_batch_kv8.py on every step whose logits
are compared, and the row schedules that make an adapter buffer grow where the tests say it does.

8 mel frames make one adapter row (conv stride 2, 4x downsample).  A stream's adapter buffer
starts at vox_hip_set_adapter_rows0 rows and doubles, so at 16 rows a 300-row stream grows at
rows 17, 65, 129 and 257, and at 64 rows a stream of 60..63 rows grows with its next 10.
"""
import os

import numpy as np

from vox_weights import TINY, TINY_LONG

FPR = 8              # mel frames per adapter row
LOGIT_TOL = 5e-5     # of the largest logit magnitude, the project's bar (tests/test_gpu_batch.py)
MARGIN = 4 * LOGIT_TOL
STEP_BATCH = 16      # steps per chunk of a batched call (csrc/vox_hip.hip)

_W = {}
_REF = {}


def weights():
    """synth_weights(TINY, seed=1), as conftest's tiny_weights; the windows do not enter the tensors"""
    if "w" not in _W:
        from vox_weights import synth_weights
        _W["w"] = synth_weights(TINY, seed=1)
    return _W["w"]


def _oracle_model(cfg, delay=6):
    import vox_oracle
    # two threads: on matrices of 256 x 512 a wider team costs more in hand-offs than it computes
    # (the 296-row schedule below: 0.3 s on 1 or 2 threads, 13 s on 8)
    vox_oracle.set_threads(min(2, os.cpu_count() or 1))
    return vox_oracle.OracleModel(cfg, weights(), delay)


def worst_margin(logits):
    """the smallest (top1 - top2) / max|logit| over the rows of logits [n, vocab]"""
    lg = np.asarray(logits, np.float32).reshape(-1, np.asarray(logits).shape[-1])
    top = np.partition(lg, -2, axis=1)[:, -2:]
    return float(np.min((top[:, 1] - top[:, 0]) / np.max(np.abs(lg), axis=1)))


# ---- a. one stream, ragged chunks, a decode after every chunk --------------------------------------
# The issue's schedule: 355, 50, 50, 1, 2, 7, 200, 3, 50 and then 50s: 2368 frames, 296 rows.  The
# first chunk alone makes 44 rows, so at capacity 16 the first growth (16 -> 64) comes before the
# prompt's 39 rows exist; 64 -> 128, -> 256 and -> 512 follow.
SINGLE_CHUNKS = [355, 50, 50, 1, 2, 7, 200, 3, 50] + [50] * 33
# seeds scanned on the CPU oracle from 8100 on, worst top-2 gap of the 257 steps beside each; the
# first that passes the margin rule is taken (see tests/test_adapter_growth_cpu.py)
SINGLE_SEED = 8100


def single_mel(seed=None):
    rng = np.random.default_rng(SINGLE_SEED if seed is None else seed)
    return rng.uniform(-0.6, 1.4, size=(sum(SINGLE_CHUNKS), TINY.mel_bins)).astype(np.float32)


def single_schedule(stream, mel):
    """the schedule on a GPU Stream or an OracleStream: encode a chunk, decode what it allows.
    Returns (ids, logits [steps, vocab], rows after each chunk)."""
    ids, lgs, rows, pos = [], [], [], 0
    for n in SINGLE_CHUNKS:
        stream.encode_mel(mel[pos:pos + n])
        pos += n
        rows.append(stream.adapter_tokens)
        t, lg = stream.decode(stop_at_eos=False, want_logits=True)
        ids += t.tolist()
        lgs.append(lg)
    return ids, np.concatenate(lgs), rows


def single_oracle(seed=None):
    key = ("single", seed)
    if key not in _REF:
        import vox_oracle
        om = _oracle_model(TINY)
        s = vox_oracle.OracleStream(om)
        ids, lg, rows = single_schedule(s, single_mel(seed))
        _REF[key] = dict(ids=ids, logits=lg, rows=rows, adapter=s.read_adapter())
        s.close()
        om.close()
    return _REF[key]


# ---- b / c. a begun call whose members' adapter buffers grow before finish -------------------------
# Stream i: 60 + i % 4 rows encoded (capacity 64), its decoder started by one batched step, then a
# bounded begin of up to BEGUN_STEPS steps (every row it has: 33 + delay + 1 rows are behind it, so
# 20..23 steps at the model's delay of 6: two chunks), then GROW_ROWS more rows for the members in
# `grow` (64 -> 128), then the drain of those rows.
BEGUN_STEPS = 40
GROW_ROWS = 10
# name -> (streams, batch capacity, members that grow, per-stream delays or None, --alt members, mel seed)
# seeds scanned on the CPU oracle from each base on, the worst top-2 gap over every step of the
# run beside each; the first that passes the margin rule is taken
BEGUN = {
    "plain": (4, 4, (1, 2), None, (), 8200),
    "enc_batch": (4, 4, (0, 3), None, (), 8300),
    "wide33": (33, 64, (5, 32), None, (), 8400),
    "mixed_delay": (4, 4, (1, 2), (6, 3, 10, 1), (), 8500),
    "alt": (4, 4, (0, 2), None, (0, 1), 8600),
}


def begun_rows(i):
    return 60 + i % 4


def begun_delay(name, i):
    d = BEGUN[name][3]
    return 6 if d is None else d[i % len(d)]


def begun_mels(name, seed=None):
    """[(first mel, grown mel)] per stream; a stream that does not grow gets no second mel"""
    n, _, grow, _, _, s = BEGUN[name]
    rng = np.random.default_rng(s if seed is None else seed)
    out = []
    for i in range(n):
        a = rng.uniform(-0.6, 1.4, size=(FPR * begun_rows(i), TINY.mel_bins)).astype(np.float32)
        b = rng.uniform(-0.6, 1.4, size=(FPR * GROW_ROWS, TINY.mel_bins)).astype(np.float32)
        out.append((a, b if i in grow else None))
    return out


def begun_oracle(name, seed=None):
    """per stream: ids of the start step, of the begun call and of the drain, and the logits of
    every step (the margin rule's input)"""
    key = (name, seed)
    if key not in _REF:
        import vox_oracle
        oms = {}
        out = []
        for i, (a, b) in enumerate(begun_mels(name, seed)):
            d = begun_delay(name, i)
            if d not in oms:
                oms[d] = _oracle_model(TINY, d)
            s = vox_oracle.OracleStream(oms[d])
            assert s.encode_mel(a) == begun_rows(i)
            t0, l0 = s.decode(max_steps=1, stop_at_eos=False, want_logits=True)
            t1, l1 = s.decode(max_steps=BEGUN_STEPS, stop_at_eos=False, want_logits=True)
            t2, l2 = np.zeros(0, np.int32), np.zeros((0, TINY.vocab), np.float32)
            if b is not None:
                assert s.encode_mel(b) == GROW_ROWS
                t2, l2 = s.decode(stop_at_eos=False, want_logits=True)
            out.append(dict(start=t0.tolist(), call=t1.tolist(), drain=t2.tolist(),
                            logits=np.concatenate([l0, l1, l2]), adapter=s.read_adapter()))
            s.close()
        for om in oms.values():
            om.close()
        _REF[key] = out
    return _REF[key]


# ---- d / e. the scheduler ---------------------------------------------------------------------------
# 4 staggered jfk-derived streams of 12..25 s fed in 4 s pieces at -I 0.5: about 50 adapter rows
# per tick against a step cap of 24, so a backlog builds and every run after a stream's first
# begins more than 16 steps for it while the run's pass adds the next 50 rows.  Once every stream
# has finished, the cap is lifted (0) and the remaining backlog drains in one run.
SCHED_PIECE = 64000
SCHED_INTERVAL = 0.5
SCHED_CAP0 = 64
SCHED_STEP_CAP = 24
SCHED_LENS = (12.0, 25.0, 17.5, 21.0)
SCHED_STARTS = (0, 1, 1, 2)


def sched_audios(jfk):
    long = np.concatenate([jfk] * 3)
    return [np.ascontiguousarray(long[int(k * 24000) % 16000:][:int(s * 16000)]) for k, s in enumerate(SCHED_LENS)]


def sched_oracle(jfk):
    """per stream: (ids of the oracle's session on the same pieces, adapter rows after each feed
    and after finish)"""
    if "sched" not in _REF:
        import vox_oracle
        om = _oracle_model(TINY_LONG)
        out = []
        for a in sched_audios(jfk):
            s = vox_oracle.OracleStream(om)
            sess = vox_oracle.OracleAudioSession(s, interval_s=SCHED_INTERVAL)
            rows = []
            for i in range(0, len(a), SCHED_PIECE):
                sess.feed(a[i:i + SCHED_PIECE])
                rows.append(s.adapter_tokens)
            sess.finish()
            rows.append(s.adapter_tokens)
            out.append((list(sess.tokens), rows))
            sess.close()
            s.close()
        om.close()
        _REF["sched"] = out
    return _REF["sched"]


def sched_row_schedule(rows_per_tick, step_cap=SCHED_STEP_CAP, cap0=SCHED_CAP0, delay=6):
    """The overlapped scheduler's step-capped runs on the host, from each stream's adapter rows after each of
    its feeds (the oracle session's, which chunks as vh_stream_feed does): run t begins, for every
    stream, min(step cap, rows complete before the run - rows consumed) steps and then enqueues
    the pass that brings the stream to its rows of tick t.  Returns per stream the list of
    (steps begun, capacity before, capacity after) of the runs whose pass outgrew the buffer
    while the stream had steps begun."""
    prompt = 33 + delay
    out = []
    for rows in rows_per_tick:
        have, used, cap, started, hits = 0, 0, cap0, False, []
        for t in range(len(rows)):
            steps = 0
            if started or have >= prompt + 1:
                if not started:
                    used, started = prompt, True
                steps = min(step_cap, have - used)
                used += steps
            new_cap = cap
            while new_cap < rows[t]:
                new_cap *= 2
            if new_cap > cap and steps > 0:
                hits.append((steps, cap, new_cap))
            cap, have = new_cap, rows[t]
        out.append(hits)
    return out
