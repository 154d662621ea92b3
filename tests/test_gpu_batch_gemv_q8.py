"""The opt-in R-row GEMV batched decode step on Q8 weights (k_gemvr<.., WF_Q8, R>,
vox_hip_batch_set_gemv_rows_q8) and its test entries.

Configs, mels, oracle sessions and the step driver are those of tests/test_gpu_batch_gemv.py
(KV8: QKV 6144 rows in 4-row groups at K 768 = 48 chunks of 16 int8, wo K 4096 = one full
round, W1|W3 2560 rows, W2 K 1280; G95: W2 K 9216 = three rounds, which at 4 or 8 rows is the
multi-pass instance), on quantize_q8(synth_weights(cfg, seed=1)).

The entry tests hold the kernel's invariants on int8 rows over the whole int8 range with
log-uniform row scales: 5e-5 of max|y| against float64, row independence in bits, k_gemv<Q8>'s
bits, and the scale taken from the row's own index.  The step tests compare every stream's ids
with its own CPU-oracle session on the same Q8 weights and six single steps' logits at
LOGIT_TOL of that step's largest oracle logit; tests/test_batch_gemv_q8_cpu.py asserts on the
oracle alone that every case in CASES passes the top-2 margin rule."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_batch_gemv as g  # noqa: E402  (configs, mels, the step driver; nothing of it is collected here)

pytestmark = pytest.mark.gpu

ROOT = g.ROOT
LOGIT_TOL, LOGIT_TOL16 = g.LOGIT_TOL, g.LOGIT_TOL16
MARGIN_F32, MARGIN_KV16 = g.MARGIN_F32, g.MARGIN_KV16
KV8, G95 = g.KV8, g.G95

# name -> (config name, sizes, mel seed, fp16 rings): every oracle comparison of this file, all
# on Q8 weights
CASES = {
    "kv8_q8_9": ("kv8", g.SIZES_9, 3303, False),
    "g95_q8_8": ("g95", g.SIZES_G95, 3950, False),
    "kv8_q8_5_kv16": ("kv8", g.SIZES_5, 3500, True),
}
_ORACLE = {}


def _oracle(case):
    """[(ids, logits [steps, vocab])] per stream of CASES[case], as test_gpu_batch_gemv._oracle"""
    from concurrent.futures import ThreadPoolExecutor
    import vox_oracle
    if case in _ORACLE:
        return _ORACLE[case]
    cname, sizes, seed, kv16 = CASES[case]
    cfg = g.CONFIGS[cname]
    om = vox_oracle.OracleModel(cfg, g._weights(cfg, True))
    vox_oracle.set_kv_fp16(kv16)
    try:
        vox_oracle.set_threads(min(4, os.cpu_count() or 1))
        sts, first = [], []
        for mel in g._mels(cfg, sizes, seed):
            st = vox_oracle.OracleStream(om)
            st.encode_mel(mel)
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
    om.close()
    out = []
    for (t0, l0), (t1, l1) in zip(first, rest):
        lg = np.concatenate([l0, l1])
        lg.setflags(write=False)
        out.append((np.concatenate([t0, t1]).tolist(), lg))
    _ORACLE[case] = out
    return out


def _case_mels(case):
    cname, sizes, seed, _ = CASES[case]
    return g._mels(g.CONFIGS[cname], sizes, seed)


def _batch(hm, n, rows):
    import vox_hip
    b = vox_hip.Batch(hm, n)
    assert b.set_gemv_rows_q8(rows) == 0, vox_hip.lib().vox_hip_last_error()
    assert b.gemv_stats()[0] == rows
    return b


def _decode_stepwise(hm, mels, slots, rows=8, steps=6, kv16=False):
    """test_gpu_batch_gemv._decode_stepwise with the Q8 switch"""
    ss = g._open(hm, mels, kv16)
    b = _batch(hm, len(ss), rows)
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
    st, gst = b.stats(), b.gemv_stats()
    for s in ss:
        s.close()
    b.close()
    return got, {i: np.stack(v) for i, v in lg.items()}, st, gst


@pytest.fixture(scope="module")
def q8_model():
    import vox_hip
    hm = vox_hip.Model(KV8, g._weights(KV8, q8=True))
    yield hm
    hm.close()


# ---- the test entries: k_gemvr's Q8 STORE instance against float64, itself and k_gemv<Q8> -----
ENTRY_SHAPES = [(6144, 768), (768, 4096), (768, 3072), (2560, 1280), (768, 9216), (65536, 768)]
ENTRY_R = (1, 2, 3, 5, 8)
_ENTRY = {}


def _entry(shape):
    """every call of the entry tests for one shape, made once: {R: y} over the first R of 8 x
    rows, and k_gemv<Q8> (vox_hip_gemv_q8) on each of the 8 rows"""
    import vox_hip
    if shape in _ENTRY:
        return _ENTRY[shape]
    rows, K = shape
    rng = np.random.default_rng(rows * 31 + K)
    W = rng.integers(-128, 128, size=(rows, K), dtype=np.int16).astype(np.int8)
    W[0, :4] = (-128, 127, -128, 127)
    sc = np.exp(rng.uniform(np.log(1e-3), np.log(1e-1), size=rows)).astype(np.float32)
    x = rng.standard_normal((8, K)).astype(np.float32)
    e = {"W": W, "sc": sc, "x": x, "calls": {R: vox_hip.gemv_rows_q8(W, sc, x[:R]) for R in ENTRY_R},
         "gemv": [vox_hip.gemv_q8(W, sc, x[r]) for r in range(8)]}
    _ENTRY[shape] = e
    return e


_ids = dict(ids=lambda s: f"{s[0]}x{s[1]}")


@pytest.mark.parametrize("shape", ENTRY_SHAPES, **_ids)
def test_entry_against_float64(shape):
    """every row of every call within 5e-5 of max|y| of scale * (W.astype(float64) @ x).
    Measured worst over the six shapes (MI355X): 1.20e-7 at (6144, 768) to 1.76e-7 at (768, 9216),
    k_gemv<Q8> on the same inputs the same figures (the same bits)."""
    e = _entry(shape)
    assert e["W"].min() == -128 and e["W"].max() == 127
    ref = (e["x"].astype(np.float64) @ e["W"].astype(np.float64).T) * e["sc"].astype(np.float64)
    worst = 0.0
    for R, y in e["calls"].items():
        assert y.shape == (R, shape[0]) and np.isfinite(y).all()
        for r in range(R):
            worst = max(worst, float(np.max(np.abs(y[r] - ref[r])) / np.max(np.abs(ref[r]))))
    worst1 = max(float(np.max(np.abs(y - ref[r])) / np.max(np.abs(ref[r]))) for r, y in enumerate(e["gemv"]))
    print(f"gemv_rows_q8 {shape}: worst err {worst:.2e} of max|y| (bar {LOGIT_TOL:.0e}); gemv_q8 {worst1:.2e}")
    assert worst < LOGIT_TOL and worst1 < LOGIT_TOL, (shape, worst, worst1)


@pytest.mark.parametrize("shape", ENTRY_SHAPES, **_ids)
def test_entry_row_independence_bits(shape):
    """y[r] has the same bits for every R, at every position r, and with NaN and 1e30 in the
    other rows"""
    import vox_hip
    e = _entry(shape)
    W, sc, x = e["W"], e["sc"], e["x"]
    y8 = e["calls"][8]
    for R in ENTRY_R:
        assert g._bits_equal(e["calls"][R], y8[:R]), (shape, R)
    ym = vox_hip.gemv_rows_q8(W, sc, x[[5, 0]])
    assert g._bits_equal(ym[0], y8[5]) and g._bits_equal(ym[1], y8[0]), shape
    ym = vox_hip.gemv_rows_q8(W, sc, x[[7, 1, 5]])
    assert g._bits_equal(ym[2], y8[5]) and g._bits_equal(ym[0], y8[7]) and g._bits_equal(ym[1], y8[1]), shape
    ym = vox_hip.gemv_rows_q8(W, sc, x[[6, 5, 4, 3, 2, 1, 0, 7]])
    assert g._bits_equal(ym, y8[[6, 5, 4, 3, 2, 1, 0, 7]]), shape
    # rows 5 and 2 kept (different passes of a multi-pass instance), the others NaN / 1e30
    for fill in (np.nan, 1e30):
        xb = np.full_like(x, fill)
        xb[5], xb[2] = x[5], x[2]
        yb = vox_hip.gemv_rows_q8(W, sc, xb)
        assert g._bits_equal(yb[5], y8[5]) and g._bits_equal(yb[2], y8[2]), (shape, fill)


@pytest.mark.parametrize("shape", ENTRY_SHAPES, **_ids)
def test_entry_matches_single_row_gemv_bits(shape):
    """every row of every call equals vox_hip_gemv_q8 (k_gemv<WF_Q8>) on that row, bit for bit"""
    e = _entry(shape)
    for R, y in e["calls"].items():
        for r in range(R):
            assert g._bits_equal(y[r], e["gemv"][r]), (shape, R, r)


@pytest.mark.parametrize("shape", [(6144, 768), (2560, 1280)], **_ids)
def test_entry_scale_indexing(shape):
    """scales 2^-(row % 7): the result is the unit-scale run times the row's power of two, bit
    for bit (a power-of-two scale is exact), so a scale taken from another row shows at once"""
    import vox_hip
    e = _entry(shape)
    rows = shape[0]
    p2 = (2.0 ** -(np.arange(rows) % 7)).astype(np.float32)
    for R in (1, 4, 8):
        y1 = vox_hip.gemv_rows_q8(e["W"], np.ones(rows, np.float32), e["x"][:R])
        yp = vox_hip.gemv_rows_q8(e["W"], p2, e["x"][:R])
        assert np.abs(y1).min() > 0
        assert g._bits_equal(yp, y1 * p2[None, :]), (shape, R)
    assert g._bits_equal(vox_hip.gemv_q8(e["W"], p2, e["x"][0]), yp[0])


# ---- the step ---------------------------------------------------------------------------------
def _check(got, lg, st, gst, ref, tol, what):
    g._compare(got, lg, ref, tol, what)
    assert gst[1] == st["replays"] > 0, (gst, st)                  # every replay is a GEMV replay
    assert gst[2] == st["rows"] == sum(len(t) for t in got), (gst, st)


def test_kv8_8_streams(q8_model):
    """KV8 Q8, 8 streams in the 8-row bucket: ids of every stream to the end of its rows, logits
    of streams 0, 3 and 7 on the first six steps, every replay on the GEMV path"""
    got, lg, st, gst = _decode_stepwise(q8_model, _case_mels("kv8_q8_9")[:8], (0, 3, 7))
    _check(got, lg, st, gst, _oracle("kv8_q8_9")[:8], LOGIT_TOL, "kv8 q8 8 streams, gemv 8")


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_other_buckets(q8_model, n):
    """1, 2, 3 and 5 streams at rows = 8: the 1-, 2-, 4- and 8-row buckets, the last two with
    empty tail slots; slots go live = 0 as the shorter streams end"""
    got, lg, st, gst = _decode_stepwise(q8_model, _case_mels("kv8_q8_9")[:n], sorted({0, n - 1}))
    _check(got, lg, st, gst, _oracle("kv8_q8_9")[:n], LOGIT_TOL, f"kv8 q8 {n} streams, gemv 8")


@pytest.mark.parametrize("max_rows", [1, 2, 4])
def test_max_rows_selects_the_bucket(q8_model, max_rows):
    """3 streams (the 4-row bucket): max_rows 4 takes the GEMV step, 1 and 2 leave it to the MFMA
    step; max_rows streams (their own bucket) take the GEMV step.  The oracle's ids every time."""
    ref = _oracle("kv8_q8_9")
    mels = _case_mels("kv8_q8_9")
    got, lg, st, gst = _decode_stepwise(q8_model, mels[:3], (2,), rows=max_rows)
    g._compare(got, lg, ref[:3], LOGIT_TOL, f"kv8 q8 3 streams, gemv {max_rows}")
    assert st["replays"] > 0 and (gst[1] == st["replays"] if max_rows == 4 else gst[1] == 0), (gst, st)
    got, lg, st, gst = _decode_stepwise(q8_model, mels[:max_rows], (max_rows - 1,), rows=max_rows)
    _check(got, lg, st, gst, ref[:max_rows], LOGIT_TOL, f"kv8 q8 {max_rows} streams, gemv {max_rows}")


def test_above_max_rows(q8_model):
    """9 streams at rows = 8: the 16-slot bucket takes the MFMA step; single-step calls on the
    streams still live take the GEMV step once 8 or fewer are left.  The oracle's ids throughout."""
    ref = _oracle("kv8_q8_9")
    ss = g._open(q8_model, _case_mels("kv8_q8_9"))
    b = _batch(q8_model, 9, 8)
    short = min(len(ids) for ids, _ in ref)
    got = [t.tolist() for t in b.decode(ss, max_steps=short, stop_at_eos=False)]
    assert b.gemv_stats()[1:] == (0, 0, 0) and b.stats()["replays"] > 0
    mfma = b.stats()["replays"]
    while True:
        live = [i for i in range(9) if len(got[i]) < len(ref[i][0])]
        if not live:
            break
        assert len(live) <= 8
        for i, t in zip(live, b.decode([ss[i] for i in live], max_steps=4, stop_at_eos=False)):
            got[i] += t.tolist()
    assert b.gemv_stats()[1] == b.stats()["replays"] - mfma > 0, (b.gemv_stats(), b.stats())
    for i, (ids, _) in enumerate(ref):
        assert got[i] == ids, (i, len(got[i]), len(ids))
    for s in ss:
        s.close()
    b.close()


def test_g95_8_streams():
    """G95 Q8 (dec_hidden 9216), 8 streams: W1|W3 in 4-row groups and W2's three K rounds, at 8
    rows in four passes of two rows.  Ids, six steps of logits of streams 0, 1 (first pass), 2,
    5 and 7 (later passes)."""
    import vox_hip
    hm = vox_hip.Model(G95, g._weights(G95, q8=True))
    got, lg, st, gst = _decode_stepwise(hm, _case_mels("g95_q8_8"), (0, 1, 2, 5, 7))
    hm.close()
    _check(got, lg, st, gst, _oracle("g95_q8_8"), LOGIT_TOL, "g95 q8 8 streams, gemv 8")


def test_fp16_rings(q8_model):
    """KV8 Q8, 5 ragged streams on IEEE-half K/V rings, at the fp16 bar; slots go live = 0 mid-call"""
    ref = _oracle("kv8_q8_5_kv16")
    assert len({len(ids) for ids, _ in ref}) == 5
    got, lg, st, gst = _decode_stepwise(q8_model, _case_mels("kv8_q8_5_kv16"), (0, 4), kv16=True)
    _check(got, lg, st, gst, ref, LOGIT_TOL16, "kv8 q8 5 streams, gemv 8, fp16 rings")


def test_alternatives(q8_model):
    """set_alt streams in the Q8 GEMV step: ids and candidate ids of the Q8 MFMA step on the same
    streams, probabilities to the logit bar, and the records against the reference rule on the
    oracle's logits (tests/test_gpu_batch_gemv.py::test_alternatives)"""
    import vox_hip
    import vox_oracle
    ref = _oracle("kv8_q8_9")[:3]
    settings = [(3, 1.0), (1, 1.0), (4, 0.5)]
    runs = []
    for rows in (8, 0):
        ss = [vox_hip.Stream(q8_model) for _ in settings]
        for s, mel, (na, co) in zip(ss, _case_mels("kv8_q8_9")[:3], settings):
            s.set_alt(na, co)
            s.encode_mel(mel)
        b = _batch(q8_model, 4, rows)
        got = [t.tolist() for t in b.decode(ss, max_steps=1000, stop_at_eos=False)]
        assert b.gemv_stats()[1] == (b.stats()["replays"] if rows else 0) and b.stats()["replays"] > 0
        runs.append((got, [s.read_alts(0, len(t)) for s, t in zip(ss, got)]))
        for s in ss:
            s.close()
        b.close()
    (got, alts), (got0, alts0) = runs
    n_with = 0
    for i, (na, co) in enumerate(settings):
        t, ol = ref[i]
        assert got[i] == t and got0[i] == t, i
        ids, pr = alts[i]
        assert np.array_equal(ids, alts0[i][0]), i
        for k, tok in enumerate(t):
            rid, rpr = vox_oracle.fill_alts(ol[k], tok, na, co)
            assert ids[k].tolist() == rid, (i, k, ids[k], rid)
            tol = 2 * LOGIT_TOL * float(np.max(np.abs(ol[k])))
            np.testing.assert_allclose(pr[k], rpr, rtol=tol, atol=1e-9)
            np.testing.assert_allclose(pr[k], alts0[i][1][k], rtol=2 * tol, atol=1e-9)
            n_with += ids[k][1] >= 0
    assert n_with > 0


def test_mode_change_between_calls(q8_model):
    """4 streams: three single-step calls on the MFMA step, three on the Q8 GEMV step, then the
    MFMA step to the end, on the same streams, rings and residual rows"""
    import vox_hip
    ref = _oracle("kv8_q8_9")[:4]
    ss = g._open(q8_model, _case_mels("kv8_q8_9")[:4])
    b = vox_hip.Batch(q8_model, 4)
    assert b.gemv_stats() == (0, 0, 0, 0)
    got = [[] for _ in ss]
    lg = []
    for mode, steps in ((0, 3), (8, 3)):
        assert b.set_gemv_rows_q8(mode) == 0
        for _ in range(steps):
            for i, t in enumerate(b.decode(ss, max_steps=1, stop_at_eos=False)):
                assert len(t) == 1
                got[i] += t.tolist()
            lg.append(b.read_logits(ss[2]))
    assert b.gemv_stats()[:3] == (8, 3, 12), b.gemv_stats()
    vox_hip.lib().vox_hip_clear_error()
    assert b.set_gemv_rows_q8(3) == -1 and vox_hip.lib().vox_hip_last_error()
    assert b.gemv_stats()[0] == 8
    assert b.set_gemv_rows_q8(0) == 0
    for i, t in enumerate(b.decode(ss, max_steps=1000, stop_at_eos=False)):
        got[i] += t.tolist()
    assert b.gemv_stats()[1] == 3 and b.stats()["replays"] > 6
    g._compare(got, {2: np.stack(lg)}, ref, LOGIT_TOL, "kv8 q8 4 streams, mode 0 / 8 / 0")
    for s in ss:
        s.close()
    b.close()


def _child_main():
    """in a fresh process (the variable is read at vox_hip_batch_create): gemv_stats()[0] of a
    batch on a Q8 model and on a bf16 one"""
    import vox_hip
    out = []
    for q8 in (True, False):
        hm = vox_hip.Model(KV8, g._weights(KV8, q8=q8))
        b = vox_hip.Batch(hm, 2)
        out.append(b.gemv_stats()[0])
        b.close()
        hm.close()
    print("GEMV_Q8_CHILD", *out)


def test_switches(q8_model):
    """the Q8 switch on a bf16 model and inside a begun call, the bf16 switch on the Q8 model,
    the environment variable on both kinds of model, and the default"""
    import vox_hip
    last = vox_hip.lib().vox_hip_last_error
    clear = vox_hip.lib().vox_hip_clear_error
    # default: nothing set
    ss = g._open(q8_model, _case_mels("kv8_q8_9")[:2])
    b = vox_hip.Batch(q8_model, 2)
    assert b.gemv_stats() == (0, 0, 0, 0)
    # the bf16 switch still refuses the Q8 model
    clear()
    assert b.set_gemv_rows(8) == -1 and last()
    assert b.gemv_stats()[0] == 0
    # inside a begun call
    assert b.set_gemv_rows_q8(8) == 0
    n = len(ss)
    arr = (ctypes.c_void_p * n)(*[s.h for s in ss])
    rows = (ctypes.c_int * n)(*[s.adapter_tokens for s in ss])
    toks = np.zeros((n, 2), np.int32)
    cnt = np.zeros(n, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    L = vox_hip.lib()
    assert L.vox_hip_batch_begin_rows(b.h, arr, n, rows, 2, 0, toks.ctypes.data_as(ip), cnt.ctypes.data_as(ip)) == 0
    clear()
    assert b.set_gemv_rows_q8(0) == -1
    assert b"begun call" in last()
    assert L.vox_hip_batch_finish(b.h) >= 0
    ref = _oracle("kv8_q8_9")
    assert cnt.tolist() == [2, 2] and [toks[i].tolist() for i in range(n)] == [ref[i][0][:2] for i in range(n)]
    assert b.gemv_stats()[:2] == (8, 2)
    assert b.set_gemv_rows_q8(0) == 0
    for s in ss:
        s.close()
    b.close()
    # a bf16 model: refused, the error names the other setter
    hm = vox_hip.Model(KV8, g._weights(KV8))
    b = vox_hip.Batch(hm, 2)
    clear()
    assert b.set_gemv_rows_q8(8) == -1
    assert b"vox_hip_batch_set_gemv_rows" in last()
    assert b.gemv_stats()[0] == 0
    assert b.set_gemv_rows(8) == 0 and b.gemv_stats()[0] == 8
    b.close()
    hm.close()
    # the environment variable, in a child process
    code = ("import sys; sys.path[:0] = [{!r}, {!r}, {!r}]; import test_gpu_batch_gemv_q8 as t; t._child_main()"
            .format(os.path.join(ROOT, "voxtral.c_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")))
    env = dict(os.environ, VOX_HIP_BATCH_GEMV_Q8="8")
    env.pop("VOX_HIP_BATCH_GEMV", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("GEMV_Q8_CHILD")]
    assert line and line[0].split()[1:] == ["8", "0"], r.stdout[-2000:]
