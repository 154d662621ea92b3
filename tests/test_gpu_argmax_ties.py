"""GPU: first-max-wins on exact logit ties, on every LM-head argmax path.

The reference scans ids in ascending order with a strict '>' (voxtral_decoder.c:771-779, and
stream_fill_alts voxtral.c:955-1010 for the --alt candidates): among equal logits the lowest id
is chosen, and equally probable alternatives come out in ascending id order.  The device makes
the same choice with multi-level reductions that restate the rule at every level:

  single stream  k_gemv EPI_LOGITS / EPI_LOGITS_ALT (lane 0 over the block's row groups, alt_row)
                 -> k_argmax_final (per thread, wave shuffles, across the 4 waves) -> alt_merge /
                 alt_tree / alt_before over the per-block top-4 lists;
  batched        k_argmax_rows (64 slices x 256 threads, a per-thread stride from vocab 16384)
                 -> k_argmax_batch_final -> alt_merge;
  twin           vox_hip_decoder_full_step: k_gemv EPI_LOGITS -> k_argmax_final.

tests/golden/gen_ties.py builds weights whose largest logit is attained by 2 or 6 ids at every
step, the ids placed on the boundaries of those reductions, for vocab 4096 / 8192 / 65536 (2-, 4-
and 8-row GEMV groups; 64, 128 and 1024 ids per batched slice) and eight rotations that move the
winning class through the eight positions; tests/test_argmax_ties_cpu.py holds the fixture to its
preconditions on the oracle alone.  The reference here is always the oracle on the same weights
and vox_oracle.fill_alts on its logits.  Per step, wherever the path exposes logits:

  (a) the token is the oracle's;
  (b) the token is the first index of the maximum of the device's own logits, and as many device
      logits equal that maximum as the position has members: the tie was exact on the device and
      the tie-break alone decided;
  (c) device logits of one class are bit-identical;
  (d) logits within LOGIT_TOL of the oracle's;
  (e) alternative ids equal fill_alts on the oracle's and on the device's logits, probabilities by
      the rule of test_alternatives_match_stream_fill_alts, a twin's probability bit-equal to
      the chosen token's; with cutoff 0 exactly the winner's twins with id >= 1000 are accepted.

The x16 rows push the tied maximum about 110 above every other logit from the second step on,
so every other probability underflows to 0 in f32 (some land among the subnormals).  The
reference ranks probabilities, not logits: at cutoff 1 its scan then takes the lowest unused
text ids (1000, 1001, ...) at probability 0.  (e) at cutoff 1 therefore also pins that case;
alt_merge used to report the largest remaining logits there instead.
"""
import numpy as np
import pytest

import gen_ties
from gen_ties import EMB, STEPS, TEXT_MIN

pytestmark = pytest.mark.gpu

LOGIT_TOL = 5e-5     # of the largest logit magnitude, as tests/test_gpu_tiny.py
ALL_ROT = tuple(range(8))
ALT_SETTINGS = ((1, 1.0), (4, 1.0), (4, 0.0))
BATCH_SIZES = [400 + 24 * i for i in range(17)]   # mel frames per stream: all different
# mel seed per stream: from 500 on, the seeds at which the oracle's gap from the tied maximum to
# the next distinct logit is at least GAP_MIN at all 12 steps (scanned on the CPU oracle alone,
# vocab 4096 and 65536; 500, 503, 507 and 509 put two classes within 0.03 at the first step)
BATCH_SEEDS = [501, 502, 504, 505, 506, 508, 510, 511, 512, 513, 514, 515, 516, 517, 518, 519, 520]
GAP_MIN = 0.1        # as tests/test_argmax_ties_cpu.py


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))


# ---- weights and oracle runs, computed once per module ------------------------------------------
_BASE = {}
_ORACLE = {}


def _base(V, q8=False):
    """untouched synth_weights for vocab V (and their Q8 quantisation): synthesised once, only
    the embedding rows are rewritten per rotation"""
    from vox_weights import quantize_q8, synth_weights
    if (V, False) not in _BASE:
        _BASE[V, False] = synth_weights(gen_ties.cfg_for(V), seed=1)
    if q8 and (V, True) not in _BASE:
        _BASE[V, True] = quantize_q8(_BASE[V, False])
    return _BASE[V, q8]


def _weights(V, rot, q8=False):
    """rot: 0..7, or "zero" for the all-zero head"""
    cfg = gen_ties.cfg_for(V)
    if rot == "zero":
        w = gen_ties.zero_head(cfg, base=_base(V))
    else:
        w = gen_ties.tie_weights(cfg, rot, base=_base(V))
    return cfg, (gen_ties.requantize_head(_base(V, True), w) if q8 else w)


def _mel(cfg, i=None):
    """the smoke() mel, or batch stream i's own"""
    if i is None:
        return gen_ties.smoke_mel(cfg)
    return np.random.default_rng(BATCH_SEEDS[i]).uniform(-0.6, 1.4, size=(BATCH_SIZES[i], cfg.mel_bins)).astype(np.float32)


def _oracle(V, rot, q8=False, i=None):
    """(ids, logits [STEPS, V]) of the oracle, read-only and shared"""
    import vox_oracle
    key = (V, rot, q8, i)
    if key not in _ORACLE:
        cfg, w = _weights(V, rot, q8)
        vox_oracle.set_threads(1)
        om = vox_oracle.OracleModel(cfg, w)
        st = vox_oracle.OracleStream(om)
        st.encode_mel(_mel(cfg, i))
        toks, lg = st.decode(max_steps=STEPS, stop_at_eos=False, want_logits=True)
        st.close()
        om.close()
        assert len(toks) == STEPS
        lg.setflags(write=False)
        _ORACLE[key] = (toks.tolist(), lg)
    return _ORACLE[key]


# ---- the per-step assertions --------------------------------------------------------------------
def _check_steps(V, rot, toks, lg, ref, alts=None, n_alt=1, cutoff=1.0, what=""):
    """(a)-(e) for one stream's STEPS steps.  lg: device logits [STEPS, V] or None (then (b)-(d)
    and the device side of (e) are left out); alts: read_alts output or None"""
    import vox_oracle
    otoks, olg = ref
    pos = gen_ties.positions(V)
    assert len(toks) == STEPS, (what, len(toks))
    worst = 0.0
    for k in range(STEPS):
        w = (what, k)
        tok = int(toks[k])
        if rot == "zero":
            members = list(range(V))
            assert (olg[k] == 0).all(), w
        else:
            # the precondition, for this stream's own mel: the oracle ties at its maximum
            o_at, which, gap, same = gen_ties.tie_step(olg[k], V, rot)
            assert which is not None and same and gap >= GAP_MIN, (w, o_at, gap)
            members = pos[which]
        assert otoks[k] == members[0], w
        assert tok == otoks[k], (w, tok, otoks[k], members)                       # (a)
        if lg is not None:
            top = lg[k].max()
            assert tok == int(np.argmax(lg[k])), (w, tok, int(np.argmax(lg[k])))    # (b)
            assert np.flatnonzero(lg[k] == top).tolist() == members, w
            if rot != "zero":                                                     # (c)
                bits = lg[k].view(np.uint32)
                for c, m in enumerate(gen_ties.class_members(V, rot)):
                    assert len(set(bits[m].tolist())) == 1, (w, "class", c, lg[k][m])
            err = rel(lg[k], olg[k])                                              # (d)
            worst = max(worst, err)
            assert err < LOGIT_TOL, (w, err)
        if alts is not None:                                                      # (e)
            ids, pr = alts
            rid, rpr = vox_oracle.fill_alts(olg[k], tok, n_alt, cutoff)
            assert ids[k].tolist() == rid, (w, ids[k], rid)
            if lg is not None:
                assert vox_oracle.fill_alts(lg[k], tok, n_alt, cutoff)[0] == rid, w
            np.testing.assert_allclose(pr[k], rpr, rtol=2 * LOGIT_TOL * float(np.max(np.abs(olg[k]))), atol=1e-9)
            twins = [m for m in members[1:] if m >= TEXT_MIN][:3]
            if n_alt == 4 and cutoff == 0.0:
                assert ids[k].tolist() == [tok] + twins + [-1] * (3 - len(twins)), (w, ids[k], twins)
            if n_alt == 4:
                assert ids[k][1:1 + len(twins)].tolist() == twins, (w, ids[k], twins)
                for j in range(1, 1 + len(twins)):
                    assert pr[k][j].tobytes() == pr[k][0].tobytes(), (w, j, pr[k])
            if n_alt == 4 and cutoff == 1.0:
                assert (ids[k] >= 0).all(), (w, ids[k])
            if n_alt == 1:
                assert ids[k].tolist() == [tok, -1, -1, -1], w
    return worst


def _model(V, rot, mode, monkeypatch):
    """a Model in one of the three weight modes, the mode proven by wpack_stats()"""
    import vox_hip
    if mode == "raw":
        monkeypatch.setenv("VOX_HIP_WPACK", "0")   # read in vox_hip_model_create
    else:
        monkeypatch.delenv("VOX_HIP_WPACK", raising=False)
    cfg, w = _weights(V, rot, q8=(mode == "q8"))
    hm = vox_hip.Model(cfg, w)
    s = hm.wpack_stats()
    n = 4 * cfg.dec_layers + 1   # Q|K|V, wo, W1|W3, W2 per decoder layer, and the LM head
    want = {"wpack": (n, 0), "raw": (0, n), "q8": (0, 0)}[mode]
    assert (s["packed_tensors"], s["raw_tensors"]) == want, (mode, s)
    return cfg, hm


def _single(V, rot, mode, monkeypatch):
    """Stream.decode with logits, without alternatives (EPI_LOGITS) and with them at cutoff 1
    and 0 (EPI_LOGITS_ALT)"""
    import vox_hip
    cfg, hm = _model(V, rot, mode, monkeypatch)
    ref = _oracle(V, rot, q8=(mode == "q8"))
    mel = _mel(cfg)
    worst = 0.0
    for n_alt, cutoff in ALT_SETTINGS:
        st = vox_hip.Stream(hm)
        st.set_alt(n_alt, cutoff)
        st.encode_mel(mel)
        toks, lg = st.decode(max_steps=STEPS, stop_at_eos=False, want_logits=True)
        alts = st.read_alts(0, len(toks))
        st.close()
        worst = max(worst, _check_steps(V, rot, toks, lg, ref, alts, n_alt, cutoff,
                                        what=f"{mode} V={V} rot={rot} alt=({n_alt}, {cutoff})"))
    hm.close()
    print(f"{mode} V={V} rot={rot}: worst logit rel {worst:.2e}")


# wpack13 (the default): every vocab size x every rotation
@pytest.mark.parametrize("rot", ALL_ROT)
@pytest.mark.parametrize("V", gen_ties.VOCABS)
def test_single_stream_wpack(V, rot, monkeypatch):
    _single(V, rot, "wpack", monkeypatch)


# raw rows and Q8: vocab 4096 with every rotation; the 4- and 8-row groups at a 2-member and a
# 6-member position
OTHER = [(4096, r) for r in ALL_ROT] + [(8192, 1), (8192, 4), (65536, 1), (65536, 4)]


@pytest.mark.parametrize("V,rot", OTHER)
def test_single_stream_raw(V, rot, monkeypatch):
    _single(V, rot, "raw", monkeypatch)


@pytest.mark.parametrize("V,rot", OTHER)
def test_single_stream_q8(V, rot, monkeypatch):
    _single(V, rot, "q8", monkeypatch)


# ---- batched ------------------------------------------------------------------------------------
def _batch_alt(i):
    """alternatives on for some streams and off for others"""
    return ALT_SETTINGS[(i + 1) % 3]   # stream 0: (4, 1.0), 1: (4, 0.0), 2: off, ...


def _batched(V, rot, n, monkeypatch, settings):
    """Batch.decode one step at a time, every stream's logits read after each step"""
    import vox_hip
    cfg, hm = _model(V, rot, "wpack", monkeypatch)
    ss = [vox_hip.Stream(hm) for _ in range(n)]
    for i, s in enumerate(ss):
        s.set_alt(*settings(i))
        s.encode_mel(_mel(cfg, i))
    b = vox_hip.Batch(hm, n)
    got = [[] for _ in ss]
    lg = [[] for _ in ss]
    for _ in range(STEPS):
        for i, t in enumerate(b.decode(ss, max_steps=1, stop_at_eos=False)):
            assert len(t) == 1, i
            got[i] += t.tolist()
        for i, s in enumerate(ss):
            lg[i].append(b.read_logits(s))
    worst = 0.0
    for i, s in enumerate(ss):
        n_alt, cutoff = settings(i)
        worst = max(worst, _check_steps(V, rot, got[i], np.stack(lg[i]), _oracle(V, rot, i=i), s.read_alts(0, STEPS),
                                        n_alt, cutoff, what=f"batch of {n} V={V} rot={rot} stream {i}"))
        s.close()
    b.close()
    hm.close()
    print(f"batch of {n} V={V} rot={rot}: worst logit rel {worst:.2e}")


@pytest.mark.parametrize("rot", (0, 1, 4, 7))
@pytest.mark.parametrize("n", (3, 17))
@pytest.mark.parametrize("V", (4096, 65536))
def test_batched(V, n, rot, monkeypatch):
    """3 streams (one 16-row block) and 17 (two): k_argmax_rows with 64 and 1024 ids per slice"""
    _batched(V, rot, n, monkeypatch, _batch_alt)


# ---- the reference-boundary twin ---------------------------------------------------------------
def test_twin_decoder_step(monkeypatch):
    """vox_hip_decoder_full_step returns the argmax id (k_gemv EPI_LOGITS + k_argmax_final into
    the twin's own state), driven as test_decoder_twins_tiny drives it: vocab 8192 (4-row
    groups), the 6-member position V/2 - 40"""
    import vox_hip
    import vox_oracle
    from vox_weights import bf16_to_f32
    V, rot, delay = 8192, 4, 6
    cfg, hm = _model(V, rot, "wpack", monkeypatch)
    _, w = _weights(V, rot)
    om = vox_oracle.OracleModel(cfg, w, delay)
    enc = vox_oracle.OracleStream(om)
    enc.encode_mel(_mel(cfg))
    adapter = enc.read_adapter()
    enc.close()
    emb = w.bf16(EMB)

    def embed(row, tok):
        return adapter[row] + bf16_to_f32(emb[tok])

    hs, os_ = vox_hip.Stream(hm), vox_oracle.OracleStream(om)
    prompt = [1] + [32] * (32 + delay)
    npf = len(prompt) - 1
    assert adapter.shape[0] == npf + STEPS
    x = np.stack([embed(i, prompt[i]) for i in range(npf)])
    hs.twin_decoder_prefill_step(x, vox_oracle.rope_freqs(np.arange(npf), cfg.dec_head_dim, cfg.rope_theta), 0)
    os_.decoder_prefill(x)
    prev, toks, lg, otoks, olg = prompt[-1], [], [], [], []
    for p in range(npf, npf + STEPS):
        e = embed(p, prev)
        ht, hl = hs.twin_decoder_step(e, vox_oracle.rope_freqs([p], cfg.dec_head_dim, cfg.rope_theta)[0], p)
        ot, ol = os_.decoder_forward(e)
        toks.append(ht); lg.append(hl); otoks.append(ot); olg.append(ol)
        prev = ot
    hs.close(); os_.close(); hm.close(); om.close()
    # the twin's oracle run is the stream decode's: same prompt, same adapter rows
    assert otoks == _oracle(V, rot)[0]
    worst = _check_steps(V, rot, toks, np.stack(lg), (otoks, np.stack(olg)), what=f"twin V={V} rot={rot}")
    print(f"twin V={V} rot={rot}: worst logit rel {worst:.2e}")


# ---- the all-zero head --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("wpack", "raw"))
@pytest.mark.parametrize("V", gen_ties.VOCABS)
def test_zero_head_single_stream(V, mode, monkeypatch):
    """every logit +-0: every block's partial ties with every other one.  Token 0 at every step,
    alternatives 1000, 1001, 1002, each with the chosen token's probability 1 / V"""
    import vox_hip
    cfg, hm = _model(V, "zero", mode, monkeypatch)
    ref = _oracle(V, "zero")
    assert ref[0] == [0] * STEPS
    for n_alt, cutoff in ALT_SETTINGS:
        st = vox_hip.Stream(hm)
        st.set_alt(n_alt, cutoff)
        st.encode_mel(_mel(cfg))
        toks, lg = st.decode(max_steps=STEPS, stop_at_eos=False, want_logits=True)
        ids, pr = st.read_alts(0, len(toks))
        st.close()
        assert toks.tolist() == [0] * STEPS and (lg == 0).all()
        _check_steps(V, "zero", toks, lg, ref, (ids, pr), n_alt, cutoff, what=f"zero {mode} V={V}")
        if n_alt == 4:
            assert (ids == [0, 1000, 1001, 1002]).all()
            assert (pr == np.float32(1.0 / V)).all()   # 1 / V and the sum V are exact in f32
    hm.close()


@pytest.mark.parametrize("V", (4096, 65536))
def test_zero_head_batched(V, monkeypatch):
    """3 streams, alternatives on: every slice of k_argmax_rows ties with every other one"""
    _batched(V, "zero", 3, monkeypatch, lambda i: (4, (0.0, 1.0, 0.5)[i]))
    import vox_hip
    cfg, hm = _model(V, "zero", "wpack", monkeypatch)
    ss = [vox_hip.Stream(hm) for _ in range(3)]
    for i, s in enumerate(ss):
        s.set_alt(4, 0.0)
        s.encode_mel(_mel(cfg, i))
    b = vox_hip.Batch(hm, 3)
    got = b.decode(ss, max_steps=STEPS, stop_at_eos=False)   # several steps per call
    for i, s in enumerate(ss):
        assert got[i].tolist() == [0] * STEPS, i
        ids, pr = s.read_alts(0, STEPS)
        assert (ids == [0, 1000, 1001, 1002]).all(), (i, ids)
        assert (pr == np.float32(1.0 / V)).all(), (i, pr)
        s.close()
    b.close()
    hm.close()
