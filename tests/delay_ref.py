"""The runs of tests/test_gpu_stream_delay.py (streams of one model at delays of their own) and
their CPU-oracle references, shared with tests/test_stream_delay_cpu.py, which pins on the oracle
alone what makes the GPU comparisons mean something: the top-2 margin rule of
tests/test_gpu_batch_kv8.py on every step of every stream, and that a wrong ada table is visible.

A run is a list of streams; stream i has delay DELAYS[i % 5], frames(i) mel frames (distinct sizes;
8 frames per adapter row, so 70..90 rows: 37..44 steps at delay 1 down to 20..27 at delay 30) and
its mel drawn in turn from one generator, so a shorter run is a prefix with identical mels.  Each
stream's reference is its own oracle session on an OracleModel(cfg, W, its delay).

Seeds (scanned on the CPU oracle, the worst top-2 gap of the whole run as a fraction of the largest
logit beside each; the rule is 4 x the logit bar: 2e-4, half rings 4e-4): see RUNS.
"""
import os
from dataclasses import replace

import numpy as np

from vox_weights import TINY, TINY_LONG

LOGIT_TOL = 5e-5     # of the largest logit magnitude, as tests/test_gpu_batch.py
LOGIT_TOL16 = 1e-4   # half KV rings, as tests/test_gpu_kv16.py
MARGIN_F32 = 4 * LOGIT_TOL
MARGIN_KV16 = 4 * LOGIT_TOL16

KV8 = replace(TINY, dec_heads=32, dec_kv_heads=8, dec_dim=768, dec_hidden=1280)   # tests/test_gpu_batch_kv8.py's
CFGS = {"TINY": TINY, "KV8": KV8, "TINY_LONG": TINY_LONG}

DELAYS = (1, 3, 6, 12, 30)
MODEL_DELAY = 6


def delay_of(i):
    return DELAYS[i % 5]


def frames(i):
    return 560 + 24 * (i % 5) + i


# name -> (config, streams, mel seed, half rings, Q8).
# Scanned on the CPU oracle from each base on; the first seed at which the whole run passes the
# margin rule is taken (worst top-2 gap of the run beside each seed):
#   f32 64    7000: 5.89e-4 (2,388 steps), the first tried
#   kv16 40   7100: 5.11e-4 (1,424 steps; rule 4e-4), the first tried
#   q8 64     7200: 7.53e-5, 7201: 7.28e-7, 7202: 5.18e-5, 7203: 2.01e-4 (2,388 steps)
#   single    7300: 1.80e-2 (TINY; streams 3 and 0 of the pattern, delays 12 and 1, 35 + 37 steps)
RUNS = {
    "f32": ("KV8", 64, 7000, False, False),
    "kv16": ("KV8", 40, 7100, True, False),
    "q8": ("KV8", 64, 7203, False, True),
    "single": ("TINY", 4, 7300, False, False),
}


def mels(name, n=None, seed=None):
    cfg_name, total, s, _, _ = RUNS[name]
    cfg = CFGS[cfg_name]
    rng = np.random.default_rng(s if seed is None else seed)
    out = [rng.uniform(-0.6, 1.4, size=(frames(i), cfg.mel_bins)).astype(np.float32) for i in range(total)]
    return out[:total if n is None else n]


_W = {}
_REF = {}


def weights(cfg, q8=False):
    """synth_weights(cfg, seed=1); the windows do not enter the tensors"""
    from vox_weights import quantize_q8, synth_weights
    key = (cfg.dec_dim, cfg.dec_hidden, cfg.dec_heads, q8)
    if key not in _W:
        if q8:
            _W[key] = quantize_q8(weights(cfg))
        else:
            _W[key] = synth_weights(replace(cfg, enc_window=TINY.enc_window, dec_window=TINY.dec_window), seed=1)
    return _W[key]


def oracle(name, n=None, seed=None, only=None):
    """[(ids, logits [steps, vocab])] of the run's first n streams (only: just those indices, the
    others None), each decoded to the end of its adapter rows on an OracleModel at its own delay.
    Encoder and prefill + first token in turn (the oracle's M > 1 linears share one scratch
    buffer), the greedy decodes side by side in threads, as tests/test_gpu_batch_kv8.py does."""
    from concurrent.futures import ThreadPoolExecutor
    import vox_oracle
    cfg_name, total, s, kv16, q8 = RUNS[name]
    seed = s if seed is None else seed
    n = total if n is None else n
    idx = list(range(n)) if only is None else list(only)
    key = (name, seed)
    have = _REF.setdefault(key, {})
    todo = [i for i in idx if i not in have]
    if todo:
        cfg = CFGS[cfg_name]
        W = weights(cfg, q8)
        ms = mels(name, seed=seed)
        oms = {d: vox_oracle.OracleModel(cfg, W, d) for d in sorted({delay_of(i) for i in todo})}
        vox_oracle.set_kv_fp16(kv16)
        try:
            vox_oracle.set_threads(min(4, os.cpu_count() or 1))
            sts, first = [], []
            for i in todo:
                st = vox_oracle.OracleStream(oms[delay_of(i)])
                st.encode_mel(ms[i])
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
        for om in oms.values():
            om.close()
        for i, (t0, l0), (t1, l1) in zip(todo, first, rest):
            lg = np.concatenate([l0, l1])
            lg.setflags(write=False)
            have[i] = (np.concatenate([t0, t1]).tolist(), lg)
    return [have[i] if i in idx else None for i in range(max(idx) + 1)] if only is not None else [have[i] for i in idx]


def margin(ref):
    """(worst (top1 - top2) / max|logit| over every step of every stream, steps); the ids are the
    logits' first-max argmax"""
    worst, steps = np.inf, 0
    for i, r in enumerate(ref):
        if r is None:
            continue
        ids, lg = r
        assert len(ids) == lg.shape[0] > 0, i
        assert np.array_equal(np.argmax(lg, axis=1), np.asarray(ids)), i
        top = np.partition(lg, -2, axis=1)[:, -2:]
        gap = (top[:, 1] - top[:, 0]) / np.max(np.abs(lg), axis=1)
        worst = min(worst, float(np.min(gap)))
        steps += len(ids)
    return worst, steps


def assert_margin(ref, rule, what):
    worst, steps = margin(ref)
    print(f"{what}: oracle top-2 gap >= {worst:.2e} of the largest logit over {steps} steps (rule: {rule:.0e})")
    assert worst >= rule, (what, worst, rule)


def wrong_table_shift(cfg_name, delay, wrong, seed=7400, steps=6):
    """A delay-`delay` stream decoded with the table of `wrong` after its first token
    (OracleModel.set_delay), against the same stream decoded properly: the largest logit shift of
    `steps` steps, of that step's largest proper logit."""
    import vox_oracle
    cfg = CFGS[cfg_name]
    W = weights(cfg)
    mel = np.random.default_rng(seed).uniform(-0.6, 1.4, size=(560, cfg.mel_bins)).astype(np.float32)
    out = []
    for swap in (False, True):
        om = vox_oracle.OracleModel(cfg, W, delay)
        st = vox_oracle.OracleStream(om)
        st.encode_mel(mel)
        st.decode(max_steps=1, stop_at_eos=False, want_logits=True)
        if swap:
            om.set_delay(wrong)
        out.append(st.decode(max_steps=steps, stop_at_eos=False, want_logits=True)[1])
        st.close()
        om.close()
    good, bad = out
    assert good.shape == bad.shape and good.shape[0] == steps
    return float(np.max(np.max(np.abs(bad - good), axis=1) / np.max(np.abs(good), axis=1)))
