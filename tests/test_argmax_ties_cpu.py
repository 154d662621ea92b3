"""CPU: the preconditions of tests/test_gpu_argmax_ties.py, on the oracle alone.

tests/golden/gen_ties.py rewrites rows of the tied embeddings so that the largest logit of
every decode step is attained by several ids at once.  The GPU tests then pin the reference's
rule (ascending scan, strict '>': the lowest id wins, equal alternatives in ascending order)
on every argmax path.  They could pass vacuously if the fixture did not tie, tied somewhere
other than at the maximum, or tied so narrowly that rounding decides; this file rules that out
for every vocab size and rotation, for bf16 and for Q8 weights:

  * at each of the 12 steps the oracle's maximum is attained by exactly the members of one
    position (2 or 6 ids) and its token is that position's first id;
  * the oracle's logits within every class are bit-identical;
  * the next distinct logit lies at least 0.1 of the largest |logit| below the maximum (a
    condition on the fixture, 2000x the 5e-5 logit bar the GPU paths are held to; measured 0.58
    for bf16 and 0.54 for Q8);
  * the rewritten tensor stays inside wpack13's window, so the packed GEMV is the one tested.
"""
import numpy as np
import pytest

import gen_ties
from gen_ties import EMB, STEPS, VOCABS

pytestmark = pytest.mark.cpu

GAP_MIN = 0.1


@pytest.fixture(scope="module", params=VOCABS)
def base(request):
    """(cfg, untouched synthetic weights, their Q8 quantisation, mel) for one vocab size"""
    import vox_oracle
    from vox_weights import quantize_q8, synth_weights
    vox_oracle.set_threads(1)
    cfg = gen_ties.cfg_for(request.param)
    w = synth_weights(cfg, seed=1)
    return cfg, w, quantize_q8(w), gen_ties.smoke_mel(cfg)


def _oracle(cfg, w, mel):
    import vox_oracle
    om = vox_oracle.OracleModel(cfg, w)
    st = vox_oracle.OracleStream(om)
    st.encode_mel(mel)
    toks, lg = st.decode(max_steps=STEPS, stop_at_eos=False, want_logits=True)
    st.close()
    om.close()
    assert len(toks) == STEPS
    return toks, lg


def _check(cfg, w, mel, rot, what):
    V = cfg.vocab
    pos = gen_ties.positions(V)
    toks, lg = _oracle(cfg, w, mel)
    worst, winners = np.inf, set()
    for k in range(STEPS):
        at_max, which, gap, same = gen_ties.tie_step(lg[k], V, rot)
        assert which is not None, (what, k, at_max)
        assert len(at_max) in (2, 6) and len(at_max) == len(pos[which])
        assert int(toks[k]) == pos[which][0] == gen_ties.first_ids(V)[which], (what, k, toks[k], at_max)
        assert same, (what, k)
        assert gap >= GAP_MIN, (what, k, gap)
        worst = min(worst, gap)
        winners.add(which)
    print(f"{what}: winners at positions {sorted(winners)}, gap to the next logit >= {worst:.2f} of max|logit|")
    return winners


@pytest.mark.parametrize("rot", range(8))
def test_bf16_ties_at_the_maximum(base, rot):
    cfg, w0, _, mel = base
    winners = _check(cfg, gen_ties.tie_weights(cfg, rot, base=w0), mel, rot, f"bf16 V={cfg.vocab} rot={rot}")
    # class 0 (+16 x row 3500) holds the maximum at every step of this mel, so rot alone
    # decides the winning position: rot 0..7 cover all eight
    assert winners == {rot}


@pytest.mark.parametrize("rot", range(8))
def test_q8_ties_at_the_maximum(base, rot):
    """identical bf16 rows quantise to identical int8 rows and scales"""
    cfg, w0, q0, mel = base
    w = gen_ties.tie_weights(cfg, rot, base=w0)
    q = gen_ties.requantize_head(q0, w)
    sc, qq = q.q8[EMB]
    for m in gen_ties.class_members(cfg.vocab, rot):
        assert len({sc[i].tobytes() for i in m}) == 1
        assert all(np.array_equal(qq[m[0]], qq[i]) for i in m[1:])
    winners = _check(cfg, q, mel, rot, f"q8 V={cfg.vocab} rot={rot}")
    assert winners == {rot}


def test_requantize_head_is_quantize_q8(base):
    """the shortcut the tests take (only the rewritten tensor is quantised again) gives the
    tensors of a full quantize_q8"""
    from vox_weights import quantize_q8
    cfg, w0, q0, _ = base
    w = gen_ties.tie_weights(cfg, 3, base=w0)
    a, b = gen_ties.requantize_head(q0, w), quantize_q8(w)
    assert a.q8.keys() == b.q8.keys() and a._stored_f32.keys() == b._stored_f32.keys()
    for name in a.q8:
        assert all(np.array_equal(x, y) for x, y in zip(a.q8[name], b.q8[name])), name
    for name in a._stored_f32:
        assert np.array_equal(a._stored_f32[name], b._stored_f32[name]), name


def test_only_the_embedding_rows_change(base):
    cfg, w0, _, _ = base
    before = {n: a.copy() for n, a in w0.t.items()}
    w = gen_ties.tie_weights(cfg, 5, base=w0)
    assert all(np.array_equal(before[n], w0.t[n]) for n in before)   # the shared base is untouched
    assert all(w.t[n] is w0.t[n] for n in before if n != EMB)
    changed = np.flatnonzero((w.t[EMB] != w0.t[EMB]).any(axis=1)).tolist()
    assert changed == sorted(i for m in gen_ties.positions(cfg.vocab) for i in m)


def test_tied_head_stays_in_wpack13_window(base):
    """x16 widens the tensor's exponent span (measured 23 at vocab 4096, 27 at 65536); past 29
    the model would stream the raw rows and the packed LM head would go untested"""
    from test_wpack_cpu import scan
    cfg, w0, _, _ = base
    for rot in range(8):
        ok, lo, hi, d = scan(gen_ties.tie_weights(cfg, rot, base=w0).t[EMB])
        assert ok and hi - lo <= 29 and abs(d) <= 40, (rot, lo, hi, d)
    print(f"V={cfg.vocab}: exponent span {hi - lo}")
    assert scan(gen_ties.zero_head(cfg, base=w0).t[EMB]) == (True, 0, 0, 0)


def test_zero_head(base):
    """every logit +-0: token 0 at every step, and the alternatives are the first three text
    ids, each as probable as the chosen token"""
    import vox_oracle
    cfg, w0, _, mel = base
    w = gen_ties.zero_head(cfg, base=w0)
    emb = w.t[EMB]
    assert (emb[0::2] == 0).all() and (emb[1::2] == 0x8000).all()
    toks, lg = _oracle(cfg, w, mel)
    assert (toks == 0).all()
    assert (lg == 0).all()
    for k in range(STEPS):
        ids, pr = vox_oracle.fill_alts(lg[k], 0, 4, 0.0)
        assert ids == [0, 1000, 1001, 1002]
        assert pr == [pr[0]] * 4 and pr[0] == pytest.approx(1.0 / cfg.vocab, rel=1e-6)
