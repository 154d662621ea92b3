"""The batched decoder prefill over compressed KV rings: streams whose decoder
rings are IEEE half or FP8 E4M3 join a batch through the same stacked prefill passes on the batch
queue as f32 streams (k_rope_kv_rows<KT>, k_attn_mf<128, KT, 1>), instead of one single-stream
prefill per stream on its own queue.  vox_hip_batch_set_prefill_kv(b, 0) restores the per-stream
prefills (A/B).

FP8 streams are held to the ring-conditioned replay of tests/test_gpu_kv8.py (the Rings / replay
pattern is copied from there): the reference session of tests/kv8_ref.py recomputes every K/V row
from its own activations, holds the GPU's stored row to check_fp8_rows, adopts it, and then ids
must be equal (the replay's top-2 margin at least MARGIN on every step) and logits within
LOGIT_TOL = 5e-5 of the step's largest magnitude.

Half-ring streams are held to the CPU oracle under set_kv_fp16(True): ids equal, every step's
logits within LOGIT_TOL16 = 1e-4 of that step's largest oracle logit.  An id comparison only means
something where the oracle's own top-2 gap exceeds what the tolerance allows, so each such test
first asserts that gap to be at least 4 x LOGIT_TOL16 on every compared step (the mel seeds and
audio offsets were picked on the CPU so that it is; tests/test_prefill_kv_cpu.py pins that)."""
import ctypes
import os
from dataclasses import replace

import numpy as np
import pytest

from kv8_ref import ACT_TOL, CFGS, MARGIN, RUNS, RefDecoder, check_fp8_rows, oracle_adapter, run_mels

pytestmark = pytest.mark.gpu

LOGIT_TOL = 5e-5      # of the step's largest logit magnitude, as tests/test_gpu_batch.py
LOGIT_TOL16 = 1e-4    # half rings against the rounded-KV oracle, as tests/test_gpu_kv16.py
MARGIN_KV16 = 4 * LOGIT_TOL16
assert LOGIT_TOL == ACT_TOL and MARGIN == 4 * LOGIT_TOL
CHUNK = 4096
MAX_CALL = 64         # steps per decode call between ring read-backs (the ring's slack)
NP = 38               # prefill rows of a prompt (32 + the 6 delay tokens); the step after them reads row 38
PIECE = 8000          # 0.5 s of 16 kHz samples per feed (the served test)

# the half-ring cases: name -> (config, weights kind, mel seed, [tokens per stream]); a stream of n
# tokens gets NP + n adapter rows.  Seeds: picked on the CPU so that the rounded-KV oracle's top-2
# gap is at least MARGIN_KV16 on every step of every stream (each the first tried: gaps 2.8e-3,
# 7.1e-4 and 5.7e-3; the served sessions 5.2e-4).
HALF = {
    "kv8_5": ("KV8", "bf16", 5102, [12, 15, 9, 14, 11]),
    "tiny_3": ("TINY", "bf16", 5200, [20, 14, 17]),
    "tiny_q8_3": ("TINY", "q8", 5300, [16, 19, 13]),
}
# the served case: 5 TINY_LONG streams over pieces of the jfk fixture, (offset s, length s) each,
# two starting per tick; picked under the same rule on the oracle's audio sessions
SERVED = [(0.0, 3.5), (1.5, 4.0), (3.0, 3.0), (4.5, 4.5), (6.0, 3.5)]
SERVED_STARTS = [0, 0, 1, 1, 2]

_M = {}
_W = {}


def _weights(cfg_name, kind="bf16"):
    if (cfg_name, kind) not in _W:
        from vox_weights import quantize_q8, synth_weights
        w = synth_weights(CFGS[cfg_name], seed=1)
        _W[(cfg_name, kind)] = quantize_q8(w) if kind == "q8" else w
    return _W[(cfg_name, kind)]


def _oracle_model(cfg_name, kind="bf16"):
    import vox_oracle
    vox_oracle.set_threads(min(16, os.cpu_count() or 1))
    return vox_oracle.OracleModel(CFGS[cfg_name], _weights(cfg_name, kind))


def _models(cfg_name, kind="bf16"):
    """(hip model, oracle model, weights) per config and weights kind, made once"""
    if (cfg_name, kind) not in _M:
        import vox_hip
        w = _weights(cfg_name, kind)
        _M[(cfg_name, kind)] = (vox_hip.Model(CFGS[cfg_name], w), _oracle_model(cfg_name, kind), w)
    return _M[(cfg_name, kind)]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    import vox_oracle
    vox_oracle.set_kv_fp16(False)
    for hm, om, _ in _M.values():
        hm.close()
        om.close()
    _M.clear()


def _stream(hm, dtype, mel):
    import vox_hip
    hm.set_kv_dtype(dtype)
    s = vox_hip.Stream(hm)
    hm.set_kv_dtype(vox_hip.KV_F32)
    assert s.kv_dtype == dtype
    for i in range(0, mel.shape[0], CHUNK):
        s.encode_mel(mel[i:i + CHUNK])
    return s


class Rings:
    """the decoded ring rows of one GPU stream by logical position, filled after every call"""

    def __init__(self, s):
        c = s.cfg
        self.s, self.n = s, 0
        self.K = [[] for _ in range(c.dec_layers)]
        self.V = [[] for _ in range(c.dec_layers)]

    def pull(self):
        pos = self.s.state()["kv_pos"]
        if pos > self.n:
            for l in range(self.s.cfg.dec_layers):
                k, v = self.s.read_kv(l, self.n, pos - self.n, decoded=True)
                self.K[l].append(k)
                self.V[l].append(v)
            self.n = pos

    def done(self):
        self.K = [np.concatenate(k) for k in self.K]
        self.V = [np.concatenate(v) for v in self.V]


def _replay(cfg_name, mel, ids, logits, rg, what, need_ids=True):
    """the ring-conditioned replay of one stream: every prefill row and every step's row of every
    layer under check_fp8_rows, then adopted; need_ids: the margin rule and id equality on every
    step; logits (where read) within LOGIT_TOL.  Returns (adjacent-code elements, worst logit err)"""
    hm, om, w = _models(cfg_name)
    cfg = CFGS[cfg_name]
    adj = [0]
    seen = [0]

    def hook(k, v, layer, pos):
        n = k.shape[0]
        gk, gv = rg.K[layer][pos:pos + n], rg.V[layer][pos:pos + n]
        assert gk.shape == k.shape, (what, layer, pos, gk.shape, k.shape)
        adj[0] += check_fp8_rows(k, gk, f"{what} K layer {layer} pos {pos}")
        adj[0] += check_fp8_rows(v, gv, f"{what} V layer {layer} pos {pos}")
        seen[0] += n
        return gk, gv

    r = RefDecoder(cfg, w, oracle_adapter(om, mel), om.ada_scale(), round_fn=hook)
    worst, read = 0.0, 0
    for i, gid in enumerate(ids):
        out = r.step(force_token=gid)
        assert out is not None, (what, i)
        rid, rlg = out
        if i == 0:
            assert seen[0] == (NP + 1) * cfg.dec_layers, (what, seen[0])   # the prompt's rows + the step's
        scale = float(np.max(np.abs(rlg)))
        if need_ids:
            s2 = np.sort(rlg)
            margin = float(s2[-1] - s2[-2]) / scale
            assert margin >= MARGIN, (what, i, margin)
            assert rid == gid, (what, i, rid, gid)
        if logits[i] is not None:
            err = float(np.max(np.abs(logits[i] - rlg))) / scale
            worst = max(worst, err)
            read += 1
            assert err < LOGIT_TOL, (what, i, err)
    assert r.pos == rg.n and read > 0, (what, r.pos, rg.n, read)
    print(f"{what}: {len(ids)} ids {'equal' if need_ids else 'forced'}, {r.pos} positions x {cfg.dec_layers} layers, "
          f"{adj[0]} adjacent-code elements, {read} logit rows rel err {worst:.2e}")
    return adj[0], worst


def _fp8_batch(name, passes, prefill_kv=None, bounded=False, cap=None):
    """the FP8 streams of RUNS[name], none of them started, through batched calls only: the first
    call prefills all of them (`passes` passes); every stream replayed on its own.
    bounded: Batch.decode(..., rows=bounds) in ragged pieces (the scheduler's path: the prefill
    on the batch queue whatever the ring type)"""
    import vox_hip
    cfg_name, _, steps = RUNS[name]
    hm, _, _ = _models(cfg_name)
    mels = run_mels(name)
    ss = [_stream(hm, vox_hip.KV_FP8, mel) for mel in mels]
    rgs = [Rings(s) for s in ss]
    ids = [[] for _ in ss]
    lgs = [[] for _ in ss]
    b = vox_hip.Batch(hm, cap or max(4, len(ss)))
    if prefill_kv is not None:
        assert b.set_prefill_kv(prefill_kv) == 0
    first = True

    def took(act, out, n_max):
        nonlocal first
        if first:
            st = b.stats()
            assert st["prefill_passes"] == passes and st["prefilled"] == len(ss), st
            first = False
        for k, t in zip(act, out):
            ids[k] += t.tolist()
            # the last step's logits, for the streams that step advanced
            if len(t):
                lgs[k] += [None] * (len(t) - 1) + [b.read_logits(ss[k]) if len(t) == n_max else None]
            rgs[k].pull()

    if bounded:
        every = list(range(len(ss)))
        out = b.decode(ss, max_steps=1000, stop_at_eos=False, rows=[10, 20, 5][:len(ss)])   # below the prompt
        assert all(len(t) == 0 for t in out) and b.stats()["prefilled"] == 0
        # stream k's first NP + n rows give it exactly its n tokens: ragged bounds, all but the
        # last row, then the last row (one step for every stream: its logits are read)
        for piece in (0.45, 0.8, -1, 0):
            bounds = [NP + n + piece if piece <= 0 else max(1, int(round((NP + n) * piece))) for n in steps]
            out = b.decode(ss, max_steps=1000, stop_at_eos=False, rows=bounds)
            took(every, out, max(len(t) for t in out))
            for k in every:
                gp = ss[k].state()["gen_pos"]
                assert gp <= bounds[k], (k, gp, bounds[k])
    else:
        # all but the last two steps in calls of <= MAX_CALL (graph replays), the last two one by
        # one for their logits; a stream leaves when it has its steps
        def live():
            return [k for k in range(len(ss)) if len(ids[k]) < steps[k]]
        while live():
            act = live()
            left = min(steps[k] - len(ids[k]) for k in act)
            n = 1 if left <= 2 else min(MAX_CALL, left - 2)
            out = b.decode([ss[k] for k in act], max_steps=n, stop_at_eos=False)
            assert all(len(t) == n for t in out)
            took(act, out, n)
    st = b.stats()
    assert st["prefill_passes"] == passes and st["prefilled"] == len(ss), st
    b.close()
    for k, s in enumerate(ss):
        s.close()
        rgs[k].done()
        assert len(ids[k]) == steps[k], (k, len(ids[k]), steps[k])
        _replay(cfg_name, mels[k], ids[k], lgs[k], rgs[k], f"prefill fp8 {name} stream {k}")


# ---- 1, 2: FP8 rings through the stacked pass ----------------------------------------------------
def test_fp8_17_streams_one_stacked_pass():
    """32 query / 8 kv heads, the 17 unstarted streams of RUNS["batch17"] in one Batch.decode: one
    prefill pass for all 17 (17 passes when every stream prefills alone), then the replay of every
    stream.  Each prompt's 38 rows end in a query block of 6 rows, so the partial block of
    k_attn_mf<128, kv8_t, 1> is covered."""
    _fp8_batch("batch17", passes=1, cap=32)


@pytest.mark.parametrize("bounded", [False, True], ids=["decode", "decode_rows"])
def test_fp8_three_streams_4_2_heads(bounded):
    """TINY_LONG (4 / 2 heads), the three streams of RUNS["batch3"] with no single-stream
    pre-steps: one pass; the same through Batch.decode(..., rows=bounds) (the bounded path on the
    batch queue: a bound below the prompt first, then ragged bounds)"""
    _fp8_batch("batch3", passes=1, bounded=bounded)


# ---- 3: groups -----------------------------------------------------------------------------------
def test_fp8_32_streams_two_groups():
    """32 KV8 streams, prompt + one step: two stacked passes (26 prompts of 38 rows fit the 1024
    rows of one pass, then 6).  For every stream the 38 prefill rows and the step's row of every
    layer obey check_fp8_rows against the reference session, which adopts them; the step's logits
    within LOGIT_TOL of the replay's.  No id comparison (the reference is fed the GPU's id), so
    no margin is needed and nothing is exempted."""
    import vox_hip
    hm, _, _ = _models("KV8")
    mels = (run_mels("batch17", seed=4511) + run_mels("batch17", seed=4512))[:32]
    ss = [_stream(hm, vox_hip.KV_FP8, mel) for mel in mels]
    rgs = [Rings(s) for s in ss]
    b = vox_hip.Batch(hm, 32)
    out = b.decode(ss, max_steps=1, stop_at_eos=False)
    st = b.stats()
    assert st["prefill_passes"] == 2 and st["prefilled"] == 32, st
    lgs = [b.read_logits(s) for s in ss]
    b.close()
    for k, s in enumerate(ss):
        assert len(out[k]) == 1
        rgs[k].pull()
        rgs[k].done()
        assert rgs[k].n == NP + 1
        s.close()
        _replay("KV8", mels[k], out[k].tolist(), [lgs[k]], rgs[k], f"prefill fp8 groups stream {k}", need_ids=False)


# ---- 4, 5: half rings against the rounded-KV oracle ----------------------------------------------
def _case_mels(case):
    cfg_name, _, seed, toks = HALF[case]
    rng = np.random.default_rng(seed)
    return [rng.uniform(-0.6, 1.4, size=(8 * (NP + n), CFGS[cfg_name].mel_bins)).astype(np.float32) for n in toks]


def _gaps(lg):
    top = np.partition(lg, -2, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) / np.max(np.abs(lg), axis=1)


def _assert_margin(ref, what):
    """the margin rule, on the oracle's logits alone, every step of every stream"""
    worst, steps = np.inf, 0
    for i, (ids, lg) in enumerate(ref):
        assert len(ids) == lg.shape[0] > 0, (what, i)
        assert np.array_equal(np.argmax(lg, axis=1), np.asarray(ids)), (what, i)
        gap = _gaps(lg)
        k = int(np.argmin(gap))
        assert gap[k] >= MARGIN_KV16, (what, i, k, float(gap[k]), MARGIN_KV16)
        worst = min(worst, float(gap[k]))
        steps += len(ids)
    print(f"{what}: oracle top-2 gap >= {worst:.2e} of the largest logit over {steps} steps (rule: {MARGIN_KV16:.0e})")
    return worst


def half_oracle(case, om=None):
    """[(ids, logits)] of the oracle under set_kv_fp16(True), one session per stream of the case"""
    import vox_oracle
    cfg_name, kind, _, toks = HALF[case]
    own = om is None
    if own:
        om = _oracle_model(cfg_name, kind)
    out = []
    vox_oracle.set_kv_fp16(True)
    try:
        for mel, n in zip(_case_mels(case), toks):
            st = vox_oracle.OracleStream(om)
            st.encode_mel(mel)
            ids, lg = st.decode(stop_at_eos=False, want_logits=True)
            st.close()
            assert len(ids) == n, (case, len(ids), n)
            out.append((ids.tolist(), lg))
    finally:
        vox_oracle.set_kv_fp16(False)
        if own:
            om.close()
    return out


@pytest.mark.parametrize("case", sorted(HALF))
def test_half_rings_one_pass_vs_oracle(case):
    """kv8_5: 32 / 8 heads, 5 streams; tiny_3: 4 / 2 heads, 3 streams (the k_gemmf branch of the
    stacked prefill); tiny_q8_3: the Q8 model, whose prefill takes the launch_gemm branch.  One
    pass for all streams, ids equal to the oracle's fp16-KV sessions, every step's logits within
    LOGIT_TOL16."""
    import vox_hip
    cfg_name, kind, _, toks = HALF[case]
    hm, om, _ = _models(cfg_name, kind)
    ref = half_oracle(case, om)
    _assert_margin(ref, f"half {case}")
    ss = [_stream(hm, vox_hip.KV_F16, mel) for mel in _case_mels(case)]
    b = vox_hip.Batch(hm, max(4, len(ss)))
    got = [[] for _ in ss]
    worst = 0.0
    for step in range(max(toks)):
        act = [k for k in range(len(ss)) if step < toks[k]]
        out = b.decode([ss[k] for k in act], max_steps=1, stop_at_eos=False)
        if step == 0:
            st = b.stats()
            assert st["prefill_passes"] == 1 and st["prefilled"] == len(ss), st
        for k, t in zip(act, out):
            assert len(t) == 1, (case, k, step)
            got[k] += t.tolist()
            rlg = ref[k][1][step]
            err = float(np.max(np.abs(b.read_logits(ss[k]) - rlg))) / float(np.max(np.abs(rlg)))
            worst = max(worst, err)
            assert err < LOGIT_TOL16, (case, k, step, err)
    assert b.stats()["prefill_passes"] == 1
    b.close()
    for k, s in enumerate(ss):
        s.close()
        assert got[k] == ref[k][0], (case, k)
    print(f"half {case}: {sum(toks)} ids equal over {len(ss)} streams, logits rel err {worst:.2e}")


# ---- 6: the switch -------------------------------------------------------------------------------
def test_switch_off_restores_per_stream_prefills():
    """set_prefill_kv(0): the FP8 batch of three streams counts three passes and passes the same
    replay"""
    _fp8_batch("batch3", passes=3, prefill_kv=0)


def _begin(b, ss, max_steps):
    import vox_hip
    n = len(ss)
    arr = (ctypes.c_void_p * n)(*[s.h for s in ss])
    rows = (ctypes.c_int * n)(*[s.adapter_tokens for s in ss])
    toks = np.zeros((n, max_steps), np.int32)
    cnt = np.zeros(n, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    rc = vox_hip.lib().vox_hip_batch_begin_rows(b.h, arr, n, rows, max_steps, 0, toks.ctypes.data_as(ip),
                                                cnt.ctypes.data_as(ip))
    return rc, toks, cnt


def test_switch_setter_env_and_f32(monkeypatch):
    """the setter is refused between begin_rows and finish (and the flag stays); f32 streams take
    one pass under either value; VOX_HIP_BATCH_PREFILL_KV=0 in the environment at Batch(...) gives
    the initial value, and the setter overrides it"""
    import vox_hip
    hm, _, _ = _models("TINY_LONG")
    mels = run_mels("batch3")
    L = vox_hip.lib()

    def passes(b, dtype):
        ss = [_stream(hm, dtype, mel) for mel in mels]
        b.decode(ss, max_steps=1, stop_at_eos=False)
        for s in ss:
            s.close()
        st = b.stats()
        assert st["prefilled"] == 3, st
        return st["prefill_passes"]

    # a begun call: the prefills of three half-ring streams and two steps in flight
    b = vox_hip.Batch(hm, 4)
    ss = [_stream(hm, vox_hip.KV_F16, mel) for mel in mels]
    rc, toks, cnt = _begin(b, ss, 2)
    assert rc == 0
    L.vox_hip_clear_error()
    assert b.set_prefill_kv(0) == -1
    assert b"begun call" in L.vox_hip_last_error()
    assert L.vox_hip_batch_finish(b.h) >= 0
    assert cnt.tolist() == [2, 2, 2] and b.stats()["prefill_passes"] == 1
    for s in ss:
        s.close()
    b.close()
    # f32 streams do not read the flag
    for on in (1, 0):
        b = vox_hip.Batch(hm, 4)
        assert b.set_prefill_kv(on) == 0
        assert passes(b, vox_hip.KV_F32) == 1, on
        b.close()
    # the environment's initial value, for both compressed types; unset and "1": stacked
    for env, want in (("0", 3), ("1", 1), (None, 1)):
        if env is None:
            monkeypatch.delenv("VOX_HIP_BATCH_PREFILL_KV", raising=False)
        else:
            monkeypatch.setenv("VOX_HIP_BATCH_PREFILL_KV", env)
        for dtype in (vox_hip.KV_F16, vox_hip.KV_FP8):
            b = vox_hip.Batch(hm, 4)
            assert passes(b, dtype) == want, (env, dtype)
            b.close()
    monkeypatch.setenv("VOX_HIP_BATCH_PREFILL_KV", "0")
    b = vox_hip.Batch(hm, 4)
    assert b.set_prefill_kv(1) == 0
    assert passes(b, vox_hip.KV_FP8) == 1
    b.close()


# ---- 7: f32 untouched ----------------------------------------------------------------------------
def test_f32_batch_same_bits_under_either_value():
    """a 3-stream f32 batch: ids and first-step logits bit for bit the same with the switch on
    and off (the f32 path does not read it; the float instances of the two kernels are the ones
    the batched encoder pass runs)"""
    import vox_hip
    hm, _, _ = _models("TINY_LONG")
    mels = run_mels("gemv2") + run_mels("batch3")[:1]
    runs = []
    for on in (1, 0):
        ss = [_stream(hm, vox_hip.KV_F32, mel) for mel in mels]
        b = vox_hip.Batch(hm, 4)
        assert b.set_prefill_kv(on) == 0
        first = b.decode(ss, max_steps=1, stop_at_eos=False)
        lg = [b.read_logits(s) for s in ss]
        rest = b.decode(ss, max_steps=20, stop_at_eos=False)
        assert b.stats()["prefill_passes"] == 1
        runs.append(([np.concatenate([a, c]) for a, c in zip(first, rest)], lg))
        b.close()
        for s in ss:
            s.close()
    for k in range(len(mels)):
        assert len(runs[0][0][k]) == 21
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k


# ---- 8: served -----------------------------------------------------------------------------------
class _LogStream:
    """an OracleStream whose decode() also keeps the logits of every step it takes"""

    def __init__(self, s):
        self._s, self.logits = s, []

    def __getattr__(self, name):
        return getattr(self._s, name)

    def decode(self, **kw):
        t, lg = self._s.decode(want_logits=True, **kw)
        self.logits.append(lg)
        return t


def served_audios(jfk):
    return [np.ascontiguousarray(jfk[int(o * 16000):][:int(n * 16000)]) for o, n in SERVED]


def served_oracle(om, audio):
    """(ids, logits) of the oracle's fp16-KV audio session fed in 0.5 s pieces"""
    import vox_oracle
    vox_oracle.set_kv_fp16(True)
    try:
        os_ = _LogStream(vox_oracle.OracleStream(om))
        sess = vox_oracle.OracleAudioSession(os_, interval_s=0.5)
        for i in range(0, len(audio), PIECE):
            sess.feed(audio[i:i + PIECE])
        sess.finish()
        ids = list(sess.tokens)
        lg = np.concatenate([l for l in os_.logits if len(l)])
        sess.close()
        os_.close()
    finally:
        vox_oracle.set_kv_fp16(False)
    return ids, lg


def test_served_half_rings_share_prefill_passes(jfk_samples):
    """a Scheduler over a model with half rings, 5 TINY_LONG streams, two starting per tick: the
    streams whose prompts complete in one tick share a stacked pass on the batch queue (fewer
    passes than prefills; one pass per prefill when every stream prefills alone), and every
    stream's ids equal its oracle fp16-KV session"""
    import vox_hip
    hm, om, _ = _models("TINY_LONG")
    audios = served_audios(jfk_samples)
    ref = [served_oracle(om, a) for a in audios]
    _assert_margin(ref, "served half")
    hm.set_kv_fp16(True)
    try:
        ctx = vox_hip.HostCtx(hm)
        q = vox_hip.Scheduler(ctx, 8)
        ss = [vox_hip.HostStream(ctx, interval_s=0.5) for _ in audios]
    finally:
        hm.set_kv_fp16(False)
    for s in ss:
        q.attach(s)
    pos = [0] * len(audios)
    done = [False] * len(audios)
    ids = [[] for _ in audios]
    tick = 0
    while not all(done) or any(s.pending() for s in ss):
        for k, (a, s) in enumerate(zip(audios, ss)):
            if done[k] or tick < SERVED_STARTS[k]:
                continue
            if pos[k] < len(a):
                s.feed(a[pos[k]:pos[k] + PIECE])
                pos[k] += PIECE
            else:
                s.finish()
                done[k] = True
        q.run()
        for k, s in enumerate(ss):
            ids[k] += s.get()
        tick += 1
    st = q.stats()
    for s in ss:
        s.close()
    q.close()
    ctx.close()
    print("served half-ring scheduler stats", st)
    assert st["prefills"] == len(audios), st
    assert 0 < st["prefill_passes"] < st["prefills"], st
    for k in range(len(audios)):
        assert ids[k] == ref[k][0], (k, len(ids[k]), len(ref[k][0]))
