"""Cross-stream batched decoding (C4) against per-stream decoding and the
CPU oracle.  The batched step shares each weight GEMM across the streams (M = streams), so
logits differ from the single-stream GEMV only in f32 summation order: greedy ids must be
identical per stream, whatever mix of positions, lengths and start states the batch holds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOGIT_TOL = 5e-5   # of the largest logit magnitude, as the single-stream bar


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))


def _mels(cfg, sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-0.6, 1.4, size=(n, cfg.mel_bins)).astype(np.float32) for n in sizes]


def _reference_tokens(om, mel):
    import vox_oracle
    st = vox_oracle.OracleStream(om)
    st.encode_mel(mel)
    t = st.decode(stop_at_eos=False)
    st.close()
    return t.tolist()


@pytest.fixture(scope="module")
def models(tiny_cfg, tiny_weights):
    import vox_hip
    import vox_oracle
    hm = vox_hip.Model(tiny_cfg, tiny_weights)
    om = vox_oracle.OracleModel(tiny_cfg, tiny_weights)
    yield hm, om
    hm.close()
    om.close()


@pytest.mark.parametrize("nstreams", [1, 3, 8])
def test_batch_matches_single_and_oracle(models, tiny_cfg, nstreams):
    import vox_hip
    hm, om = models
    sizes = [400 + 37 * i for i in range(nstreams)]   # ragged lengths: streams drop out
    mels = _mels(tiny_cfg, sizes, 100 + nstreams)
    ss = [vox_hip.Stream(hm) for _ in mels]
    for s, mel in zip(ss, mels):
        s.encode_mel(mel)
    b = vox_hip.Batch(hm, 8)
    got = b.decode(ss, max_steps=1000, stop_at_eos=False)
    for i, mel in enumerate(mels):
        ref = _reference_tokens(om, mel)
        single = vox_hip.Stream(hm)
        single.encode_mel(mel)
        one = single.decode(stop_at_eos=False).tolist()
        assert one == ref, i
        assert got[i].tolist() == ref, (i, len(got[i]), len(ref))
        single.close()
    for s in ss:
        s.close()
    b.close()


def test_batch_logits_per_step_vs_oracle(models, tiny_cfg):
    """The batched path's logit bar: 3 TINY streams advanced one batched step per call (the
    first call prefills all three in one stacked pass and takes their first token in the
    batched step); every step's logits within LOGIT_TOL of the oracle's, ids identical."""
    import vox_hip
    import vox_oracle
    hm, om = models
    mels = _mels(tiny_cfg, [800, 900, 1000], 31)   # 62+ steps of adapter rows each
    ss = [vox_hip.Stream(hm) for _ in mels]
    for s, mel in zip(ss, mels):
        s.encode_mel(mel)
    b = vox_hip.Batch(hm, 3)
    n = 40
    got = [[] for _ in ss]
    lg = [[] for _ in ss]
    for step in range(n):
        for i, t in enumerate(b.decode(ss, max_steps=1, stop_at_eos=False)):
            got[i] += t.tolist()
            lg[i].append(b.read_logits(ss[i]))
    worst = 0.0
    for i, mel in enumerate(mels):
        o = vox_oracle.OracleStream(om)
        o.encode_mel(mel)
        t, ol = o.decode(max_steps=n, stop_at_eos=False, want_logits=True)
        o.close()
        assert got[i] == t.tolist(), i
        r = rel(np.stack(lg[i]), ol)
        worst = max(worst, r)
        assert r < LOGIT_TOL, (i, r)
    print(f"batched logits vs oracle: worst rel err {worst:.2e}")
    for s in ss:
        s.close()
    b.close()


def test_batch_mixed_positions_and_continuation(models, tiny_cfg):
    """streams at different decode positions (one advanced alone first), decoding resumed
    in several batch calls and finished on the single-stream path."""
    import vox_hip
    hm, om = models
    mels = _mels(tiny_cfg, [520, 600, 480, 700], 7)
    refs = [_reference_tokens(om, m) for m in mels]
    ss = [vox_hip.Stream(hm) for _ in mels]
    for s, mel in zip(ss, mels):
        s.encode_mel(mel)
    first = ss[1].decode(max_steps=5, stop_at_eos=False).tolist()   # ahead of the others
    b = vox_hip.Batch(hm, 4)
    out = [[] for _ in ss]
    out[1] += first
    for _ in range(2):
        for i, t in enumerate(b.decode(ss, max_steps=9, stop_at_eos=False)):
            out[i] += t.tolist()
    for i, s in enumerate(ss):
        out[i] += s.decode(stop_at_eos=False).tolist()
        assert out[i] == refs[i], i
        s.close()
    b.close()


def _oracle_tokens_parallel(om, mels, chunks):
    """The oracle's tokens for several streams: each stream's encoder and prefill + first
    token in turn (the oracle's M > 1 linears share one scratch buffer, as the reference's
    bf16_scratch does), then the single-threaded greedy decodes side by side in threads
    (ctypes releases the GIL; the M = 1 path touches no shared state)."""
    from concurrent.futures import ThreadPoolExecutor
    import os
    import vox_oracle
    vox_oracle.set_threads(min(16, os.cpu_count() or 1))
    sts, first = [], []
    for mel in mels:
        st = vox_oracle.OracleStream(om)
        off = 0
        for n in chunks:
            st.encode_mel(mel[off:off + n])
            off += n
        first.append(st.decode(max_steps=1, stop_at_eos=False).tolist())
        sts.append(st)
    vox_oracle.set_threads(1)

    def rest_of(st):
        a = st.decode(max_steps=st.adapter_tokens - 38 - 2, stop_at_eos=False).tolist()
        b, lg = st.decode(stop_at_eos=False, want_logits=True)
        return a + b.tolist(), lg[-1]
    with ThreadPoolExecutor(len(sts)) as ex:
        rest = list(ex.map(rest_of, sts))
    for st in sts:
        st.close()
    return [f + r[0] for f, r in zip(first, rest)], [r[1] for r in rest]


@pytest.mark.slow
def test_batch_full_size_streams_each_vs_oracle():
    """Full Voxtral-4B shapes at the 16-stream bench line's load (config 4's 8 streams per GPU
    run the same kernels: below 256 (stream, kv head) blocks the attention takes the same
    path): 16 streams of 7 s one-shot schedules (700 / 70 / 1 mel-frame chunks, different
    audio) decoded as one batch; EVERY stream's ids equal the CPU oracle's for that stream and
    the final batched step's logits are within LOGIT_TOL.  (A full jfk length per stream
    doubled the oracle's share of the GPU suite's wall time.)"""
    import vox_hip
    import vox_oracle
    from vox_weights import VOXTRAL_4B, synth_weights
    nstreams = 16
    chunks = [700, 70, 1]
    w = synth_weights(VOXTRAL_4B, seed=0)
    hm = vox_hip.Model(VOXTRAL_4B, w)
    mels = _mels(VOXTRAL_4B, [sum(chunks)] * nstreams, 42)
    ss = [vox_hip.Stream(hm) for _ in mels]
    for s, mel in zip(ss, mels):
        off = 0
        for n in chunks:
            s.encode_mel(mel[off:off + n])
            off += n
    b = vox_hip.Batch(hm, nstreams)
    got = [g.tolist() for g in b.decode(ss, max_steps=1000, stop_at_eos=False)]
    last = [b.read_logits(s) for s in ss]   # the final batched step (all 8 streams in it)
    for s in ss:
        s.close()
    b.close()
    hm.close()
    om = vox_oracle.OracleModel(VOXTRAL_4B, w)
    refs, ref_last = _oracle_tokens_parallel(om, mels, chunks)
    om.close()
    worst = 0.0
    nt = len(refs[0])
    assert nt > 40
    for i in range(nstreams):
        assert len(refs[i]) == nt
        assert got[i] == refs[i], (i, next(k for k in range(nt) if got[i][k] != refs[i][k]))
        r = rel(last[i], ref_last[i])
        worst = max(worst, r)
        assert r < LOGIT_TOL, (i, r)
    print(f"{nstreams} full-size streams: ids equal, last-step logits worst rel err {worst:.2e}")
    assert len({tuple(r) for r in refs}) > 1   # the streams really differ


def test_batch_long_context_multiblock(tiny_weights):
    """TINY_LONG (8192-key window): 4 streams decoded past 256 positions, so the batched
    attention runs on several 256-key blocks and the combine kernel writes the wo planes;
    ids equal decoding each stream alone and the CPU oracle."""
    import vox_hip
    import vox_oracle
    from vox_weights import TINY_LONG
    hm = vox_hip.Model(TINY_LONG, tiny_weights)
    om = vox_oracle.OracleModel(TINY_LONG, tiny_weights)
    mels = _mels(TINY_LONG, [2600, 2900, 2500, 2750], 11)
    ss = [vox_hip.Stream(hm) for _ in mels]
    for s, mel in zip(ss, mels):
        s.encode_mel(mel)
    b = vox_hip.Batch(hm, 4)
    got = b.decode(ss, max_steps=1000, stop_at_eos=False)
    assert min(len(g) for g in got) > 256
    for i, mel in enumerate(mels):
        one = vox_hip.Stream(hm)
        one.encode_mel(mel)
        assert got[i].tolist() == one.decode(stop_at_eos=False).tolist(), i
        one.close()
    assert got[0].tolist() == _reference_tokens(om, mels[0])
    for s in ss:
        s.close()
    b.close()
    hm.close()
    om.close()


def test_batch_graph_not_reused_after_stream_churn(models, tiny_cfg):
    """C4 serving churns streams: decode a batch, free one stream, create another (its
    handle may land at the freed address) and decode again with the same Batch.  The
    captured step graph holds per-stream device pointers, so it must be keyed by stream
    identity (uid), not by handle address: every stream still gets the oracle's ids."""
    import vox_hip
    hm, om = models
    mels = _mels(tiny_cfg, [520, 560, 600, 640], 23)
    refs = [_reference_tokens(om, m) for m in mels]
    ss = [vox_hip.Stream(hm) for _ in mels[:3]]
    for s, mel in zip(ss, mels):
        s.encode_mel(mel)
    b = vox_hip.Batch(hm, 4)
    out = [t.tolist() for t in b.decode(ss, max_steps=6, stop_at_eos=False)]
    assert out[1] == refs[1][:6]
    old = ss[1].h
    ss[1].close()
    ss[1] = vox_hip.Stream(hm)
    reused = ss[1].h == old
    ss[1].encode_mel(mels[3])
    got = [t.tolist() for t in b.decode(ss, max_steps=1000, stop_at_eos=False)]
    assert out[0] + got[0] == refs[0]
    assert got[1] == refs[3], reused
    assert out[2] + got[2] == refs[2]
    for s in ss:
        s.close()
    b.close()


def test_batch_churn_device_slots(models, tiny_cfg):
    """Serving churn on one Batch: every call lists a different set of streams -- new ones
    (prefilled together in one stacked pass, first token in the batched step), running ones,
    ones that run out of adapter rows in the middle of a call (they stop on the device while
    the others go on) -- and the step graphs are captured once per slot bucket, not per set.
    Every stream's ids equal the CPU oracle's."""
    import vox_hip
    hm, om = models
    sizes = [430, 520, 470, 610, 400, 560, 505]
    mels = _mels(tiny_cfg, sizes, 77)
    refs = [_reference_tokens(om, m) for m in mels]
    ss = [vox_hip.Stream(hm) for _ in mels]
    for s, mel in zip(ss, mels):
        s.encode_mel(mel)
    b = vox_hip.Batch(hm, 8)
    out = [[] for _ in ss]
    # (streams, max_steps) per call: joins, leaves, re-joins, drop-outs mid-call
    plan = [([0, 1, 2], 5), ([1, 2, 3, 4], 7), ([0, 4, 5], 3), ([6, 3, 0, 2, 5], 11), ([1, 6], 2),
            ([0, 1, 2, 3, 4, 5, 6], 9), ([4, 2], 1000), ([0, 1, 3, 5, 6], 1000)]
    for idx, ms in plan:
        toks = b.decode([ss[i] for i in idx], max_steps=ms, stop_at_eos=False)
        for i, t in zip(idx, toks):
            assert len(t) <= ms
            out[i] += t.tolist()
    st = b.stats()
    for i in range(len(ss)):
        assert out[i] == refs[i], (i, len(out[i]), len(refs[i]))
    # buckets 4 and 8 slots (1-2 streams: 2), one attention split bucket (48-key window)
    assert st["captures"] <= 3, st
    assert st["prefilled"] == len(ss) and st["prefill_passes"] <= 4, st
    assert st["rows"] == sum(len(o) for o in out), st
    print(f"churn: {st}")
    for s in ss:
        s.close()
    b.close()


def test_batch_alternatives_match_stream_fill_alts(models, tiny_cfg):
    """--alt streams stay in the batch (VERDICT r3 missing 1): the batched argmax keeps the
    softmax partials and the top-4 text candidates per row, and each alt stream's records agree
    with the reference rule (stream_fill_alts, voxtral.c:955-1010) on the oracle's logits; a
    stream without alternatives in the same batch is unaffected."""
    import vox_hip
    import vox_oracle
    hm, om = models
    mels = _mels(tiny_cfg, [640, 700, 580], 91)
    settings = [(3, 1.0), (1, 1.0), (4, 0.5)]
    ss = [vox_hip.Stream(hm) for _ in mels]
    for s, mel, (na, co) in zip(ss, mels, settings):
        s.set_alt(na, co)
        s.encode_mel(mel)
    b = vox_hip.Batch(hm, 4)
    got = [g.tolist() for g in b.decode(ss, max_steps=1000, stop_at_eos=False)]
    n_with = 0
    for i, (mel, (na, co)) in enumerate(zip(mels, settings)):
        o = vox_oracle.OracleStream(om)
        o.encode_mel(mel)
        t, ol = o.decode(stop_at_eos=False, want_logits=True)
        o.close()
        assert got[i] == t.tolist(), i
        ids, pr = ss[i].read_alts(0, len(got[i]))
        for k, tok in enumerate(got[i]):
            rid, rpr = vox_oracle.fill_alts(ol[k], tok, na, co)
            assert ids[k].tolist() == rid, (i, k, ids[k], rid)
            np.testing.assert_allclose(pr[k], rpr, rtol=2 * LOGIT_TOL * float(np.max(np.abs(ol[k]))), atol=1e-9)
            n_with += ids[k][1] >= 0
    assert n_with > 0
    for s in ss:
        s.close()
    b.close()


def test_batch_decode_rows_bounds_each_stream(models, tiny_cfg):
    """vox_hip_batch_decode_rows: stream i reads only its first rows[i] adapter rows (the
    scheduler's overlap decodes the rows complete at a run's start while the next encoder
    pass runs); decoding in row-bounded pieces -- a bound below the prompt (no prefill yet),
    the prompt plus a few rows, then everything -- gives the oracle's ids."""
    import vox_hip
    hm, om = models
    mels = _mels(tiny_cfg, [420, 510, 380], 77)
    ss = [vox_hip.Stream(hm) for _ in mels]
    for s, mel in zip(ss, mels):
        s.encode_mel(mel)
    total = [s.adapter_tokens for s in ss]
    b = vox_hip.Batch(hm, 4)
    got = [[] for _ in ss]
    # below the prompt: nothing runs
    out = b.decode(ss, max_steps=1000, stop_at_eos=False, rows=[10, 20, 5])
    assert all(len(t) == 0 for t in out)
    # ragged bounds, then the rest in two more pieces
    for frac in (0.45, 0.8, 1.0):
        bounds = [max(1, int(round(t * frac))) for t in total]
        out = b.decode(ss, max_steps=1000, stop_at_eos=False, rows=bounds)
        for i, t in enumerate(out):
            got[i] += t.tolist()
            gp = ss[i].state()["gen_pos"]
            assert gp <= bounds[i], (i, gp, bounds[i])   # next adapter row within the bound
    for i, mel in enumerate(mels):
        assert got[i] == _reference_tokens(om, mel), i
    with pytest.raises(RuntimeError):
        b.decode(ss, max_steps=10, stop_at_eos=False, rows=[total[0] + 1, 1, 1])  # past the rows
    for s in ss:
        s.close()
    b.close()


def test_batch_32_streams_two_row_blocks(models, tiny_cfg):
    """32 streams in one batch (the bucket of two 16-row MFMA B blocks): the first call
    prefills all of them in stacked passes (32 prompts of 39 rows exceed one 1024-row pass, so
    the prompts go in groups) and takes their first token in the batched steps; every stream's
    ids equal its own oracle session, and streams in the second row block (rows 16-31) keep
    the logit bar step by step.  At TINY's 2 kv heads 32 slots give 64 (slot, kv head) blocks,
    below the 256 the 1024-thread attention grid needs, so this test runs the 128-key split
    grid; the 32-slot default grid (8 kv heads) is pinned by tests/test_gpu_batch_kv8.py."""
    import vox_hip
    import vox_oracle
    hm, om = models
    n = 32
    mels = _mels(tiny_cfg, [420 + 29 * i for i in range(n)], 3200)
    ss = [vox_hip.Stream(hm) for _ in mels]
    for s, mel in zip(ss, mels):
        s.encode_mel(mel)
    b = vox_hip.Batch(hm, n)
    steps = 6
    got = [[] for _ in ss]
    lg = {i: [] for i in (0, 16, 31)}
    for _ in range(steps):
        for i, t in enumerate(b.decode(ss, max_steps=1, stop_at_eos=False)):
            got[i] += t.tolist()
        for i in lg:
            lg[i].append(b.read_logits(ss[i]))
    for i, t in enumerate(b.decode(ss, max_steps=1000, stop_at_eos=False)):
        got[i] += t.tolist()
    for i, mel in enumerate(mels):
        assert got[i] == _reference_tokens(om, mel), i
    for i, l in lg.items():
        o = vox_oracle.OracleStream(om)
        o.encode_mel(mels[i])
        t, ol = o.decode(max_steps=steps, stop_at_eos=False, want_logits=True)
        o.close()
        assert got[i][:steps] == t.tolist(), i
        r = rel(np.stack(l), ol)
        assert r < LOGIT_TOL, (i, r)
    for s in ss:
        s.close()
    b.close()
