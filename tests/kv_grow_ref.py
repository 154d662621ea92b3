"""Growing decoder K/V rings (vox_hip_model_set_kv_grow): the numpy restatement of
the capacity schedule and of the prefix re-pitch copy that the GPU tests compare against, and the
inputs and CPU-oracle sessions those tests share.  tests/test_kv_grow_cpu.py pins the restatement
and, on the oracle alone, the top-2 margin rule on every step whose ids are compared.

A ring below the full size (window + 64) has not wrapped, so slot = position: growing it is a
copy of rows [0, pos) of every layer from pitch cap0 to pitch cap1, nothing else moves."""
import os

import numpy as np

from vox_weights import TINY, TINY_LONG

SLACK = 64           # DEC_SLACK (csrc/vox_hip.hip): the full ring is window + SLACK, the smallest first capacity SLACK
FPR = 8              # mel frames per adapter row
LOGIT_TOL = 5e-5     # of the largest logit magnitude, the project's bar (tests/test_gpu_batch.py)
MARGIN = 4 * LOGIT_TOL
STEP_BATCH = 16      # steps per chunk of a batched call (csrc/vox_hip.hip)
PROMPT = 38          # positions the prefill appends at the model's delay of 6 (32 + delay)


# ---- the schedule ------------------------------------------------------------------------------------
def full_slots(cfg):
    return cfg.dec_window + SLACK


def clamp_slots0(slots0, cfg):
    """what vox_hip_model_set_kv_grow keeps of slots0: 0 = off, else [SLACK, full]"""
    if slots0 == 0:
        return 0
    return min(max(slots0, SLACK), full_slots(cfg))


def grow_cap(slots0, full, need):
    """the smallest slots0 * 2^k that holds `need` positions, capped at the full ring"""
    c = slots0
    while c < need and c < full:
        c *= 2
    return min(c, full)


def schedule(slots0, cfg, needs):
    """capacities after each of the calls whose last position + 1 are `needs`, and the growths"""
    full = full_slots(cfg)
    cap = clamp_slots0(slots0, cfg) or full
    if cap == full:
        return [full] * len(needs), 0
    s0, caps, grows = cap, [], 0
    for need in needs:
        need = min(need, full)
        if need > cap:
            cap = grow_cap(s0, full, need)
            grows += 1
        caps.append(cap)
    return caps, grows


def ring_bytes(cfg, slots, esize):
    """K and V rings of one stream together"""
    return 2 * cfg.dec_layers * slots * cfg.dec_kv_heads * cfg.dec_head_dim * esize


# ---- the copy ----------------------------------------------------------------------------------------
def repitch(old, new, pos):
    """old [L, cap0, C] -> new [L, cap1, C] (cap1 >= cap0): rows [0, pos) of every layer land at
    the same slots of the longer buffer, the rest of `new` stays as it was.  Works on the flat
    buffers the device holds: layer l of a ring of cap slots starts at l * cap * C."""
    L, cap0, C = old.shape
    L1, cap1, C1 = new.shape
    assert L1 == L and C1 == C and cap1 >= cap0 and 0 <= pos <= cap0
    fo, fn = old.reshape(-1), new.reshape(-1)
    for l in range(L):
        fn[l * cap1 * C:l * cap1 * C + pos * C] = fo[l * cap0 * C:l * cap0 * C + pos * C]
    return new


# ---- shared inputs and oracle sessions ------------------------------------------------------------
_W = {}
_REF = {}


def weights():
    """synth_weights(TINY, seed=1), as conftest's tiny_weights; the windows do not enter the tensors"""
    if "w" not in _W:
        from vox_weights import synth_weights
        _W["w"] = synth_weights(TINY, seed=1)
    return _W["w"]


def _oracle_model(cfg):
    import vox_oracle
    vox_oracle.set_threads(min(2, os.cpu_count() or 1))
    return vox_oracle.OracleModel(cfg, weights())


def worst_margin(logits):
    """the smallest (top1 - top2) / max|logit| over the rows of logits [n, vocab]"""
    lg = np.asarray(logits, np.float32)
    top = np.partition(lg, -2, axis=1)[:, -2:]
    return float(np.min((top[:, 1] - top[:, 0]) / np.max(np.abs(lg), axis=1)))


# name -> (config, steps, mel seed).  Seeds scanned on the CPU oracle from each base on; the first
# whose every step keeps the top-2 margin rule is taken (tests/test_kv_grow_cpu.py pins it).
#   long: one TINY_LONG session of 424 steps (positions 38..461: 256 -> 512 and 64 -> .. -> 512)
#   wrap: one TINY session of 200 steps (positions 38..237: 64 -> 112, then the ring wraps twice)
# worst gaps: long 9100 4.10e-3; wrap 9200 1.51e-4 (below the rule), 9201 3.21e-3
SESSIONS = {
    "long": (TINY_LONG, 424, 9100),
    "wrap": (TINY, 200, 9201),
}


def session_mel(name, seed=None):
    cfg, steps, s = SESSIONS[name]
    rng = np.random.default_rng(s if seed is None else seed)
    return rng.uniform(-0.6, 1.4, size=(FPR * (PROMPT + 1 + steps + 4), cfg.mel_bins)).astype(np.float32)


def session_oracle(name, seed=None):
    """ids [steps] and logits [steps, vocab] of the oracle's session on session_mel(name)"""
    key = (name, seed)
    if key not in _REF:
        import vox_oracle
        cfg, steps, _ = SESSIONS[name]
        om = _oracle_model(cfg)
        s = vox_oracle.OracleStream(om)
        s.encode_mel(session_mel(name, seed))
        ids, lg = s.decode(max_steps=steps, stop_at_eos=False, want_logits=True)
        s.close()
        om.close()
        assert len(ids) == steps
        _REF[key] = dict(ids=ids.tolist(), logits=lg)
    return _REF[key]


# ---- the scheduler run ---------------------------------------------------------------------------------
# 6 staggered jfk-derived clips of 4..8 s in 0.5 s pieces under a step cap of 8, then a seventh
# clip on the first stream's slot after vh_stream_reset
SCHED_PIECE = 8000
SCHED_INTERVAL = 0.5
SCHED_STEP_CAP = 8
SCHED_LENS = (4.0, 8.0, 5.5, 7.0, 4.5, 6.0)
SCHED_STARTS = (0, 1, 2, 3, 4, 5)
SCHED_REUSE_LEN = 5.0


def sched_audios(jfk):
    long = np.concatenate([jfk] * 2)
    cut = [np.ascontiguousarray(long[int(k * 21000) % 16000:][:int(s * 16000)]) for k, s in enumerate(SCHED_LENS)]
    return cut, np.ascontiguousarray(long[5000:][:int(SCHED_REUSE_LEN * 16000)])


def sched_oracle(jfk):
    """ids of the oracle's session per clip (the six, then the reused slot's second clip)"""
    if "sched" not in _REF:
        import vox_oracle
        om = _oracle_model(TINY_LONG)
        out = []
        audios, again = sched_audios(jfk)
        for a in audios + [again]:
            s = vox_oracle.OracleStream(om)
            sess = vox_oracle.OracleAudioSession(s, interval_s=SCHED_INTERVAL)
            for i in range(0, len(a), SCHED_PIECE):
                sess.feed(a[i:i + SCHED_PIECE])
            sess.finish()
            out.append(list(sess.tokens))
            sess.close()
            s.close()
        om.close()
        _REF["sched"] = out
    return _REF["sched"]
