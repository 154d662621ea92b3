"""The opt-in R-row GEMV batched decode step (k_gemvr, batch_step_gemv) and its
test entry, on configs the CPU oracle follows in seconds.

Configs (TINY with 32 query / 8 kv heads, as tests/test_gpu_batch_kv8.py):
  KV8       dec_dim 768, dec_hidden 1280: QKV 6144 rows (4-row groups) at K 768 (one partial
            round), wo K 4096 (two full rounds), W1|W3 2560 rows and W2 K 1280 (2-row groups, one
            round), vocab 4096 (2-row groups);
  G95       KV8 with dec_hidden 9216: W1|W3 18432 rows (4-row groups), W2 K 9216 (five rounds,
            the last half full: the full model's two-pass instance at 8 rows);
  KV8_W48   the 48-key window (ring of 112 slots) for the wrapped ring;
  KV8_LONG  the 8192-key window for contexts past 256 keys (attention splits > 1).
The full model's K 3072 (two rounds, the second half full) is pinned by the entry tests at
(768, 3072).

The entry tests hold the kernel's four invariants (row independence, raw = packed bits,
k_gemv's bits, 5e-5 of max|y| against float64).  The step tests compare every stream's ids with
its own CPU-oracle session and the named steps' logits at LOGIT_TOL of that step's largest
oracle logit; tests/test_batch_gemv_cpu.py asserts on the oracle alone that every case listed
in CASES passes the top-2 margin rule, so an id comparison means something."""
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

from vox_weights import TINY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOGIT_TOL = 5e-5     # of the largest logit magnitude, the project's parity bar
LOGIT_TOL16 = 1e-4   # fp16 KV rings, as tests/test_gpu_kv16.py
MARGIN_F32 = 4 * LOGIT_TOL
MARGIN_KV16 = 4 * LOGIT_TOL16

KV8 = replace(TINY, dec_heads=32, dec_kv_heads=8, dec_dim=768, dec_hidden=1280)
G95 = replace(KV8, dec_hidden=9216)
KV8_W48 = replace(KV8, dec_window=48)
KV8_LONG = replace(KV8, enc_window=750, dec_window=8192)

SIZES_9 = [400 + 24 * i for i in range(9)]       # 8 streams = the first 8 (the mels are drawn in order)
SIZES_5 = [400 + 40 * i for i in range(5)]       # ragged lengths: slots go live = 0 mid-call
SIZES_G95 = [400 + 16 * i for i in range(8)]
SIZES_LONG = [2400, 420, 460]                    # stream 0 passes 256 keys
SIZES_WRAP = [1000, 960, 400, 408, 416]          # streams 0 and 1 pass the 112-slot ring
SIZES_Q8 = [420 + 13 * i for i in range(3)]

# name -> (config name, sizes, mel seed, fp16 rings, Q8): every oracle comparison of this file.
# The seeds are the first tried at which the oracle passes the margin rule on every step
# (tests/test_batch_gemv_cpu.py prints each case's worst gap).
CONFIGS = {"kv8": KV8, "g95": G95, "kv8_w48": KV8_W48, "kv8_long": KV8_LONG}
CASES = {
    "kv8_9": ("kv8", SIZES_9, 900, False, False),
    "kv8_5": ("kv8", SIZES_5, 500, False, False),
    "kv8_5_kv16": ("kv8", SIZES_5, 501, True, False),   # 500: 3.5e-4 under the fp16 rule of 4e-4
    "kv8_long_3": ("kv8_long", SIZES_LONG, 61, False, False),
    "kv8_wrap_5": ("kv8_w48", SIZES_WRAP, 4800, False, False),
    "g95_8": ("g95", SIZES_G95, 950, False, False),
    "kv8_q8_3": ("kv8", SIZES_Q8, 3201, False, True),
}


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))


def _mels(cfg, sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-0.6, 1.4, size=(n, cfg.mel_bins)).astype(np.float32) for n in sizes]


# ---- weights and oracle sessions, computed once per module -----------------------------------
_W = {}
_ORACLE = {}


def _weights(cfg, q8=False):
    """synth_weights(cfg, seed=1); the windows do not enter the tensors"""
    from vox_weights import quantize_q8, synth_weights
    key = (cfg.dec_dim, cfg.dec_hidden, q8)
    if key not in _W:
        if q8:
            _W[key] = quantize_q8(_weights(cfg))
        else:
            _W[key] = synth_weights(replace(cfg, enc_window=TINY.enc_window, dec_window=TINY.dec_window), seed=1)
    return _W[key]


def _oracle(case):
    """[(ids, logits [steps, vocab])] per stream of CASES[case]: each stream's own oracle session
    decoded to the end of its adapter rows (as tests/test_gpu_batch_kv8.py)."""
    from concurrent.futures import ThreadPoolExecutor
    import vox_oracle
    if case in _ORACLE:
        return _ORACLE[case]
    cname, sizes, seed, kv16, q8 = CASES[case]
    cfg = CONFIGS[cname]
    om = vox_oracle.OracleModel(cfg, _weights(cfg, q8))
    vox_oracle.set_kv_fp16(kv16)
    try:
        vox_oracle.set_threads(min(4, os.cpu_count() or 1))
        sts, first = [], []
        for mel in _mels(cfg, sizes, seed):
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
        ids = np.concatenate([t0, t1]).tolist()
        lg = np.concatenate([l0, l1])
        lg.setflags(write=False)
        out.append((ids, lg))
    _ORACLE[case] = out
    return out


def _case_mels(case):
    cname, sizes, seed, _, _ = CASES[case]
    return _mels(CONFIGS[cname], sizes, seed)


def _open(hm, mels, kv16=False):
    import vox_hip
    hm.set_kv_fp16(kv16)
    ss = [vox_hip.Stream(hm) for _ in mels]
    hm.set_kv_fp16(False)
    for s, mel in zip(ss, mels):
        assert s.kv_fp16 == kv16
        s.encode_mel(mel)
    return ss


def _batch(hm, n, rows):
    import vox_hip
    b = vox_hip.Batch(hm, n)
    assert b.set_gemv_rows(rows) == 0
    assert b.gemv_stats()[0] == rows
    return b


def _decode_stepwise(hm, mels, slots, rows=8, steps=6, kv16=False, order=None, alone_first=False):
    """One Batch in GEMV mode `rows` over the streams (listed in `order`): `steps` single-step
    calls reading the logits of `slots` (stream indices) after each, then the drain.
    alone_first: every stream takes its prefill and first token by itself before the batch.
    Returns (ids per stream, {stream: [steps, vocab]}, stats, gemv_stats, states)."""
    ss = _open(hm, mels, kv16)
    order = list(range(len(ss))) if order is None else order
    lst = [ss[i] for i in order]
    b = _batch(hm, len(ss), rows)
    got = [[] for _ in ss]
    if alone_first:
        for i, s in enumerate(ss):
            got[i] += s.decode(max_steps=1, stop_at_eos=False).tolist()
    lg = {i: [] for i in slots}
    for _ in range(steps):
        for i, t in zip(order, b.decode(lst, max_steps=1, stop_at_eos=False)):
            assert len(t) == 1, i
            got[i] += t.tolist()
        for i in lg:
            lg[i].append(b.read_logits(ss[i]))
    for i, t in zip(order, b.decode(lst, max_steps=1000, stop_at_eos=False)):
        got[i] += t.tolist()
    assert all(len(t) == 0 for t in b.decode(lst, max_steps=1000, stop_at_eos=False))
    st, gst = b.stats(), b.gemv_stats()
    states = [s.state() for s in ss]
    for s in ss:
        s.close()
    b.close()
    return got, {i: np.stack(v) for i, v in lg.items()}, st, gst, states


def _compare(got, lg, ref, tol, what):
    """ids of every stream, and the first steps' logits of the streams read, against the oracle"""
    for i, g in enumerate(got):
        ids = ref[i][0]
        first_diff = next((k for k in range(min(len(ids), len(g))) if g[k] != ids[k]), None)
        assert first_diff is None and len(g) == len(ids), (what, i, first_diff, len(g), len(ids))
    worst = 0.0
    for i, l in lg.items():
        for k in range(l.shape[0]):
            r = rel(l[k], ref[i][1][k])
            worst = max(worst, r)
            assert r < tol, (what, i, k, r)
    print(f"{what}: {sum(len(g) for g in got)} ids equal, worst logit err {worst:.2e} (bar {tol:.0e})")
    return worst


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def kv8_model():
    import vox_hip
    hm = vox_hip.Model(KV8, _weights(KV8))
    yield hm
    hm.close()


# ---- the test entry: k_gemvr's STORE instance against float64, itself and k_gemv --------------
ENTRY_SHAPES = [(6144, 768), (768, 4096), (768, 3072), (2560, 768), (18432, 768), (768, 9216), (65536, 768)]
ENTRY_R = (1, 2, 3, 5, 8)
_ENTRY = {}


def _w(rows, K, seed):
    import ctypes
    from vox_weights import synth_lib
    out = np.zeros((rows, K), np.uint16)
    synth_lib().vox_synth_bf16(ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(out.size), ctypes.c_uint64(seed),
                               ctypes.c_float(1.0 / np.sqrt(K)), ctypes.c_float(0.0))
    return out


def _entry(shape):
    """every call of the entry tests for one shape, made once: {(R, packed): (y, flags)} over
    the first R of 8 x rows, and k_gemv (vox_hip_gemv_wpack) on each of the 8 rows"""
    import vox_hip
    if shape in _ENTRY:
        return _ENTRY[shape]
    rows, K = shape
    W = _w(rows, K, seed=rows + K)
    W[1, ::7] = 0x8000   # signed zeros
    W[2, ::5] = 0
    x = np.random.default_rng(K + rows).standard_normal((8, K)).astype(np.float32)
    x[3] *= 1e-3         # rows of different scale: a leak from a neighbour would show
    x[6] *= 40.0
    e = {"W": W, "x": x, "calls": {}, "gemv": {}}
    for R in ENTRY_R:
        for packed in (False, True):
            e["calls"][R, packed] = vox_hip.gemv_rows(W, x[:R], packed)
    for packed in (False, True):
        e["gemv"][packed] = [vox_hip.gemv_wpack(W, x[r], packed) for r in range(8)]
    _ENTRY[shape] = e
    return e


@pytest.mark.parametrize("shape", ENTRY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_entry_against_float64(shape):
    """invariant (d): every row of every call within 5e-5 of max|y| of the float64 dot product
    of the exact bf16 weights.  Measured worst over the seven shapes (MI355X): k_gemvr 1.72e-7
    at (768, 9216), 1.10e-7 to 1.37e-7 on the others; k_gemv on the same inputs the same figures
    (the same bits)."""
    e = _entry(shape)
    Wf = (e["W"].astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    ref = e["x"].astype(np.float64) @ Wf.T
    worst = 0.0
    for (R, packed), (y, _) in e["calls"].items():
        assert y.shape == (R, shape[0]) and np.isfinite(y).all()
        for r in range(R):
            err = float(np.max(np.abs(y[r] - ref[r])) / np.max(np.abs(ref[r])))
            worst = max(worst, err)
            assert err < LOGIT_TOL, (shape, R, packed, r, err)
    worst1 = max(float(np.max(np.abs(y - ref[r])) / np.max(np.abs(ref[r])))
                 for packed in (False, True) for r, (y, _) in enumerate(e["gemv"][packed]))
    print(f"gemv_rows {shape}: worst err {worst:.2e} of max|y| (bar {LOGIT_TOL:.0e}); gemv_wpack {worst1:.2e}")
    assert worst1 < LOGIT_TOL


@pytest.mark.parametrize("shape", ENTRY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_entry_row_independence_bits(shape):
    """invariant (a): row r of the 8-row call = the 1-row call on that x = the same x at
    another index and in other buckets = the same call with every other row NaN, and 1e30"""
    import vox_hip
    e = _entry(shape)
    x = e["x"]
    for packed in (False, True):
        y8 = e["calls"][8, packed][0]
        for R in ENTRY_R:   # the buckets 1, 2, 4, 8 (and 8 again), rows at the same index
            assert _bits_equal(e["calls"][R, packed][0], y8[:R]), (shape, R, packed)
        # x[5] alone, x[5] at index 0 of a 2-row call and index 2 of a 3-row call
        y1, _ = vox_hip.gemv_rows(e["W"], x[5:6], packed)
        assert _bits_equal(y1[0], y8[5]), (shape, packed)
        ym, _ = vox_hip.gemv_rows(e["W"], x[[5, 0]], packed)
        assert _bits_equal(ym[0], y8[5]) and _bits_equal(ym[1], y8[0]), (shape, packed)
        ym, _ = vox_hip.gemv_rows(e["W"], x[[7, 1, 5]], packed)
        assert _bits_equal(ym[2], y8[5]) and _bits_equal(ym[0], y8[7]), (shape, packed)
        # neighbours full of NaN / 1e30 (row 5 kept; row 2 kept in the other half of a two-pass instance)
        for fill in (np.nan, 1e30):
            xb = np.full_like(x, fill)
            xb[5], xb[2] = x[5], x[2]
            yb, _ = vox_hip.gemv_rows(e["W"], xb, packed)
            assert _bits_equal(yb[5], y8[5]) and _bits_equal(yb[2], y8[2]), (shape, packed, fill)


@pytest.mark.parametrize("shape", ENTRY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_entry_raw_and_packed_bits(shape):
    """invariant (b): the WF_BF16 and WF_P13 instances give the same bits; flag bit 0 says which ran"""
    e = _entry(shape)
    for R in ENTRY_R:
        (y0, f0), (y1, f1) = e["calls"][R, False], e["calls"][R, True]
        assert (f0 & 1, f1 & 1) == (0, 1), (shape, R, f0, f1)
        assert _bits_equal(y0, y1), (shape, R)


@pytest.mark.parametrize("shape", ENTRY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_entry_matches_single_row_gemv_bits(shape):
    """invariant (c): flag bit 1 (the per-row summation order is k_gemv's) is set for every
    shape with K <= 4096, and wherever it is set every row equals vox_hip_gemv_wpack on that
    row, raw and packed"""
    e = _entry(shape)
    for (R, packed), (y, flags) in e["calls"].items():
        if shape[1] <= 4096:
            assert flags & 2, (shape, R, packed, flags)
        if flags & 2:
            for r in range(R):
                for p1 in (False, True):
                    y1, ran = e["gemv"][p1][r]
                    assert ran == p1
                    assert _bits_equal(y[r], y1), (shape, R, packed, r, p1)


# ---- the step ---------------------------------------------------------------------------------
def _kv8_8_run(hm):
    mels = _case_mels("kv8_9")[:8]
    return _decode_stepwise(hm, mels, (0, 3, 7))


def _check_kv8_8(got, lg, st, gst, what):
    ref = _oracle("kv8_9")[:8]
    _compare(got, lg, ref, LOGIT_TOL, what)
    assert gst[1] == st["replays"] > 0, (gst, st)
    assert gst[2] == st["rows"] == sum(len(g) for g in got), (gst, st)
    assert gst[3] == st["captures"], (gst, st)


def test_kv8_8_streams(kv8_model):
    """KV8, 8 streams of 11 to 32 tokens in the 8-row bucket: ids of every stream to the end of
    its rows, logits of streams 0, 3 and 7 on the first six steps, every replay on the GEMV path.
    The model streams wpack13 planes (every decoder tensor packed)."""
    ws = kv8_model.wpack_stats()
    assert ws["packed_tensors"] == 4 * KV8.dec_layers + 1 and ws["raw_tensors"] == 0, ws
    got, lg, st, gst, _ = _kv8_8_run(kv8_model)
    _check_kv8_8(got, lg, st, gst, "kv8 8 streams, gemv 8")


def _child_main(out_path):
    """in a fresh process (VOX_HIP_WPACK is read at model creation), on the GPU only"""
    import vox_hip
    hm = vox_hip.Model(KV8, _weights(KV8))
    ws = hm.wpack_stats()
    got, lg, st, gst, _ = _kv8_8_run(hm)
    hm.close()
    np.savez(out_path, n=np.array([len(g) for g in got]), ids=np.concatenate([np.asarray(g, np.int32) for g in got]),
             lg0=lg[0], lg3=lg[3], lg7=lg[7], st=np.array([st["replays"], st["rows"], st["captures"]]),
             gst=np.array(gst), packed=np.array([ws["packed_tensors"], ws["raw_tensors"]]))


def test_kv8_8_streams_raw_weights(kv8_model, tmp_path):
    """the same in a child process with VOX_HIP_WPACK=0: the WF_BF16 instances run in the step;
    same assertions, and the logits are bit-identical to the packed run's"""
    code = ("import sys; sys.path[:0] = [{!r}, {!r}, {!r}]; import test_gpu_batch_gemv as t; t._child_main(sys.argv[1])"
            .format(os.path.join(ROOT, "voxtral.c_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")))
    env = dict(os.environ, VOX_HIP_WPACK="0")
    env.pop("VOX_HIP_BATCH_GEMV", None)
    out = str(tmp_path / "raw.npz")
    r = subprocess.run([sys.executable, "-c", code, out], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    z = np.load(out)
    assert z["packed"].tolist() == [0, 4 * KV8.dec_layers + 1]
    ends = np.cumsum(z["n"])
    got = [z["ids"][e - k:e].tolist() for e, k in zip(ends, z["n"])]
    lg = {0: z["lg0"], 3: z["lg3"], 7: z["lg7"]}
    st = dict(zip(("replays", "rows", "captures"), z["st"].tolist()))
    _check_kv8_8(got, lg, st, tuple(z["gst"].tolist()), "kv8 8 streams, gemv 8, raw bf16 weights")
    _, lgp, _, _, _ = _kv8_8_run(kv8_model)
    for i in lg:
        assert _bits_equal(lg[i], lgp[i]), i


def _alone_states(hm, mels):
    """each stream decoded alone through the single-stream path: its state() afterwards"""
    out = []
    for s in _open(hm, mels):
        s.decode(max_steps=1000, stop_at_eos=False)
        out.append(s.state())
        s.close()
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_other_buckets(kv8_model, n):
    """1, 2, 3 and 5 streams of ragged lengths: the 1-, 2-, 4- and 8-row buckets, the last two
    with empty tail slots (null rings), slots going live = 0 mid-call.  Ids of every stream, the
    first six steps' logits of the first and last stream, each stream's state() as decoded alone."""
    ref = _oracle("kv8_5")[:n]
    assert len({len(ids) for ids, _ in _oracle("kv8_5")}) == 5
    mels = _case_mels("kv8_5")[:n]
    got, lg, st, gst, states = _decode_stepwise(kv8_model, mels, sorted({0, n - 1}))
    _compare(got, lg, ref, LOGIT_TOL, f"kv8 {n} streams, gemv 8")
    assert gst[1] == st["replays"] > 0
    assert states == _alone_states(kv8_model, mels)


def test_max_rows_selects_the_bucket(kv8_model):
    """3 streams (the 4-row bucket): max_rows 4 takes the GEMV step, max_rows 2 leaves it to the
    MFMA step; both give the oracle's ids"""
    ref = _oracle("kv8_5")[:3]
    mels = _case_mels("kv8_5")[:3]
    got, lg, st, gst, _ = _decode_stepwise(kv8_model, mels, (2,), rows=4)
    _compare(got, lg, ref, LOGIT_TOL, "kv8 3 streams, gemv 4")
    assert gst[1] == st["replays"] > 0
    got, lg, st, gst, _ = _decode_stepwise(kv8_model, mels, (2,), rows=2)
    _compare(got, lg, ref, LOGIT_TOL, "kv8 3 streams, gemv 2 (MFMA step)")
    assert gst[1] == 0 and st["replays"] > 0


def test_slot_order_bits(kv8_model):
    """5 streams in two list orders: every stream's logits on six steps are bit-identical (a
    row's bits do not depend on its slot).  Each stream takes its prefill and first token by
    itself first: the batch's stacked prefill is an M > 1 GEMM over the listed streams' rows,
    whose summation order depends on where a row stands in the stack (measured: without this,
    stream 0's first-step logits differ in the last bits between the two orders)."""
    mels = _case_mels("kv8_5")
    got_a, lg_a, _, gst, _ = _decode_stepwise(kv8_model, mels, range(5), alone_first=True)
    got_b, lg_b, _, _, _ = _decode_stepwise(kv8_model, mels, range(5), order=[3, 0, 4, 2, 1], alone_first=True)
    assert gst[1] > 0
    assert got_a == got_b == [ids for ids, _ in _oracle("kv8_5")]
    for i in range(5):
        assert _bits_equal(lg_a[i], lg_b[i]), i


def test_fp16_rings(kv8_model):
    """KV8, 5 streams on IEEE-half K/V rings (kv_st2_rt's other branch), at the fp16 bar"""
    ref = _oracle("kv8_5_kv16")
    got, lg, st, gst, _ = _decode_stepwise(kv8_model, _case_mels("kv8_5_kv16"), (0, 4), kv16=True)
    _compare(got, lg, ref, LOGIT_TOL16, "kv8 5 streams, gemv 8, fp16 rings")
    assert gst[1] == st["replays"] > 0


def test_past_256_keys():
    """KV8_LONG, 3 streams (the 4-row bucket), stream 0 from 39 keys to about 300: the call that
    passes 256 keys takes the 2-split attention and a GEMV graph of its own.  Stream 0's logits
    on every single-step call from position 253 to 258; ids of every stream."""
    import vox_hip
    ref = _oracle("kv8_long_3")
    assert len(ref[0][0]) + 38 > 290, len(ref[0][0])
    hm = vox_hip.Model(KV8_LONG, _weights(KV8_LONG))
    ss = _open(hm, _case_mels("kv8_long_3"))
    b = _batch(hm, len(ss), 8)
    got = [[] for _ in ss]
    checked, worst = [], 0.0
    caps_below, caps_past = None, None
    while True:
        pos = ss[0].state()["kv_pos"] if got[0] else 38   # position of stream 0's next step
        steps = 1 if 253 <= pos <= 258 else min(16, 253 - pos) if pos < 253 else 16
        out = b.decode(ss, max_steps=steps, stop_at_eos=False)
        if not any(len(t) for t in out):
            break
        for i, t in enumerate(out):
            got[i] += t.tolist()
        caps = b.gemv_stats()[3]
        if pos + len(out[0]) <= 256:
            caps_below = caps
        elif caps_past is None:
            caps_past = caps
        last = pos + len(out[0]) - 1
        if len(out[0]) == steps and 253 <= last <= 258:
            r = rel(b.read_logits(ss[0]), ref[0][1][len(got[0]) - 1])
            checked.append(last)
            worst = max(worst, r)
            assert r < LOGIT_TOL, (last, r)
    assert checked == [253, 254, 255, 256, 257, 258], checked
    assert caps_below is not None and caps_past is not None and caps_past > caps_below, (caps_below, caps_past)
    for i, (ids, _) in enumerate(ref):
        assert got[i] == ids, (i, len(got[i]), len(ids))
    assert b.gemv_stats()[1] == b.stats()["replays"] > 0
    print(f"kv8 long: {sum(len(g) for g in got)} ids equal, stream 0 to position {ss[0].state()['kv_pos']}, "
          f"gemv captures {caps_below} -> {caps_past}, worst logit err {worst:.2e}")
    for s in ss:
        s.close()
    b.close()
    hm.close()


def test_wrapped_ring():
    """48-key window (ring of 112 slots), 5 streams, two of them decoding past position 112:
    the QKV epilogue appends at pos % cap behind the attention's window.  Ids of every stream,
    stream 0's logits on its last 8 steps (all past the wrap)."""
    import vox_hip
    ref = _oracle("kv8_wrap_5")
    n0 = len(ref[0][0])
    assert n0 + 38 > KV8_W48.dec_window + 64 + 8 and n0 > len(ref[1][0]) and len(ref[1][0]) + 38 > 112
    hm = vox_hip.Model(KV8_W48, _weights(KV8_W48))
    ss = _open(hm, _case_mels("kv8_wrap_5"))
    b = _batch(hm, len(ss), 8)
    tail = 8
    got = [t.tolist() for t in b.decode(ss, max_steps=n0 - tail, stop_at_eos=False)]
    assert len(got[0]) == n0 - tail
    worst = 0.0
    for k in range(tail):
        for i, t in enumerate(b.decode(ss, max_steps=1, stop_at_eos=False)):
            got[i] += t.tolist()
        r = rel(b.read_logits(ss[0]), ref[0][1][n0 - tail + k])
        worst = max(worst, r)
        assert r < LOGIT_TOL, (k, r)
    assert all(len(t) == 0 for t in b.decode(ss, max_steps=1000, stop_at_eos=False))
    for i, (ids, _) in enumerate(ref):
        assert got[i] == ids, (i, len(got[i]), len(ids))
    assert ss[0].state()["kv_pos"] == 38 + n0
    assert b.gemv_stats()[1] == b.stats()["replays"] > 0
    print(f"kv8 wrap: {sum(len(g) for g in got)} ids equal, stream 0 to position {38 + n0} of a 112-slot ring, "
          f"worst logit err on its last 8 steps {worst:.2e}")
    for s in ss:
        s.close()
    b.close()
    hm.close()


def test_g95_8_streams():
    """G95 (dec_hidden 9216), 8 streams: W1|W3 in 4-row groups and W2's five K rounds, which at
    8 rows is the two-pass instance (rows 0-3, then 4-7).  Ids, six steps of logits of streams
    0, 3 (first pass), 4 and 7 (second pass)."""
    import vox_hip
    ref = _oracle("g95_8")
    hm = vox_hip.Model(G95, _weights(G95))
    got, lg, st, gst, _ = _decode_stepwise(hm, _case_mels("g95_8"), (0, 3, 4, 7))
    hm.close()
    _compare(got, lg, ref, LOGIT_TOL, "g95 8 streams, gemv 8")
    assert gst[1] == st["replays"] > 0


def test_mode_change_in_flight(kv8_model):
    """KV8, 4 streams: three single-step calls in mode 0, three in mode 8, then mode 0 to the
    end -- the two steps alternate on the same streams, rings and b->x.  set_gemv_rows(3) fails."""
    import vox_hip
    ref = _oracle("kv8_9")[:4]
    ss = _open(kv8_model, _case_mels("kv8_9")[:4])
    b = vox_hip.Batch(kv8_model, 4)
    assert b.gemv_stats() == (0, 0, 0, 0)
    got = [[] for _ in ss]
    lg = []
    for mode, steps in ((0, 3), (8, 3)):
        assert b.set_gemv_rows(mode) == 0
        for _ in range(steps):
            for i, t in enumerate(b.decode(ss, max_steps=1, stop_at_eos=False)):
                assert len(t) == 1
                got[i] += t.tolist()
            lg.append(b.read_logits(ss[2]))
    assert b.gemv_stats()[:3] == (8, 3, 12), b.gemv_stats()
    vox_hip.lib().vox_hip_clear_error()
    assert b.set_gemv_rows(3) == -1
    assert vox_hip.lib().vox_hip_last_error()
    assert b.gemv_stats()[0] == 8
    assert b.set_gemv_rows(0) == 0
    for i, t in enumerate(b.decode(ss, max_steps=1000, stop_at_eos=False)):
        got[i] += t.tolist()
    assert b.gemv_stats()[1] == 3 and b.stats()["replays"] > 6
    _compare(got, {2: np.stack(lg)}, ref, LOGIT_TOL, "kv8 4 streams, mode 0 / 8 / 0")
    for s in ss:
        s.close()
    b.close()


def test_above_max_rows(kv8_model):
    """9 streams with max_rows 8 (the 16-slot bucket) keep the MFMA step; the first 8 of them
    in a second batch then count GEMV replays.  Ids of streams 0 and 7 (the oracle sessions of
    test_kv8_8_streams) both times."""
    ref = _oracle("kv8_9")
    ss = _open(kv8_model, _case_mels("kv8_9"))
    b = _batch(kv8_model, 9, 8)
    got = [t.tolist() for t in b.decode(ss, max_steps=1000, stop_at_eos=False)]
    assert b.gemv_stats()[1:] == (0, 0, 0) and b.stats()["replays"] > 0
    assert got[0] == ref[0][0] and got[7] == ref[7][0]
    b.close()
    for s in ss:
        s.close()
    ss = _open(kv8_model, _case_mels("kv8_9")[:8])
    b = _batch(kv8_model, 8, 8)
    got = [t.tolist() for t in b.decode(ss, max_steps=1000, stop_at_eos=False)]
    assert b.gemv_stats()[1] == b.stats()["replays"] > 0
    assert got[0] == ref[0][0] and got[7] == ref[7][0]
    b.close()
    for s in ss:
        s.close()


def test_alternatives(kv8_model):
    """streams with alternatives on in an 8-mode batch (launch_argmax_batch on the GEMV step's
    logits rows): records against the reference rule on the oracle's logits, by the method and
    tolerances of tests/test_gpu_batch.py::test_batch_alternatives_match_stream_fill_alts"""
    import vox_hip
    import vox_oracle
    ref = _oracle("kv8_5")[:3]
    settings = [(3, 1.0), (1, 1.0), (4, 0.5)]
    ss = [vox_hip.Stream(kv8_model) for _ in settings]
    for s, mel, (na, co) in zip(ss, _case_mels("kv8_5")[:3], settings):
        s.set_alt(na, co)
        s.encode_mel(mel)
    b = _batch(kv8_model, 4, 8)
    got = [g.tolist() for g in b.decode(ss, max_steps=1000, stop_at_eos=False)]
    assert b.gemv_stats()[1] == b.stats()["replays"] > 0
    n_with = 0
    for i, (na, co) in enumerate(settings):
        t, ol = ref[i]
        assert got[i] == t, i
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


def test_q8_model_keeps_the_mfma_step():
    """a Q8 model: set_gemv_rows(8) fails with an error, the mode stays 0 and a short decode
    still gives the oracle's ids"""
    import vox_hip
    ref = _oracle("kv8_q8_3")
    hm = vox_hip.Model(KV8, _weights(KV8, q8=True))
    ss = _open(hm, _case_mels("kv8_q8_3"))
    b = vox_hip.Batch(hm, 3)
    vox_hip.lib().vox_hip_clear_error()
    assert b.set_gemv_rows(8) == -1
    assert vox_hip.lib().vox_hip_last_error()
    assert b.gemv_stats()[0] == 0
    got = [t.tolist() for t in b.decode(ss, max_steps=6, stop_at_eos=False)]
    for i, (ids, _) in enumerate(ref):
        assert got[i] == ids[:6], i
    assert b.gemv_stats() == (0, 0, 0, 0) and b.stats()["replays"] > 0
    for s in ss:
        s.close()
    b.close()
    hm.close()
