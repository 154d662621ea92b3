"""The R-row GEMV batched decode step on the wmx4 GEMV planes (k_gemvr<.., WF_MX4, R>,
vox_hip_batch_set_gemv_wmx4) and its test entry (vox_hip_gemv_rows, packed = 2).

The wmx4 instances decode every weight to the f32 its bf16 form widens to and run the bf16
instance's FMA chains, so the step on the wpack13 planes (set_gemv_wmx4(0)) is the bit-exact
twin, and the unchanged CPU oracle on the MXFP4-rounded weights (vox_weights.quantize_mxfp4, what
wmx4 mode 2 makes of a checkpoint at load) the exact reference.

Configs, sizes and helpers are tests/test_gpu_batch_gemv.py's (KV8, G95).  Group sizes of the
wmx4 plane at these shapes: QKV 6144 rows and G95's W1|W3 18432 rows 4 (as bf16); wo, W2, KV8's
W1|W3 2560 rows and the LM head's 4096 rows 4 where the bf16 instances run 2.  8-row groups
(65,536 rows and up) are reached by the entry test alone.

tests/test_batch_gemv_wmx4_cpu.py asserts on the oracle alone that every case in CASES keeps the
top-2 margin on every compared step, so an id comparison means something."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_batch_gemv as g   # configs, sizes, mels and comparison helpers (nothing of it is collected here)

pytestmark = pytest.mark.gpu

ROOT = g.ROOT
LOGIT_TOL, LOGIT_TOL16 = g.LOGIT_TOL, g.LOGIT_TOL16
MARGIN_F32, MARGIN_KV16 = g.MARGIN_F32, g.MARGIN_KV16
KV8, G95 = g.KV8, g.G95
CONFIGS = {"kv8": KV8, "g95": G95}
UNROUNDED = "layers.1.attention.wo.weight"   # the tensor the `mixed` weights leave off the MXFP4 grid
FP8_STEPS = [8, 11]                          # steps per stream of the FP8-ring case (39 + n + 5 adapter rows)

# name -> (config name, weights, sizes, mel seed, ring): every oracle comparison of this file.
# The seeds are the first from the base on at which the oracle (for fp8: the unforced FP8 reference
# session of tests/kv8_ref.py) on these weights passes the margin rule on every step of every
# stream; scanned on the CPU, asserted by tests/test_batch_gemv_wmx4_cpu.py.
CASES = {
    "kv8_8": ("kv8", "rounded", g.SIZES_9[:8], 900, "f32"),
    "kv8_5": ("kv8", "rounded", g.SIZES_5, 500, "f32"),
    "kv8_5_kv16": ("kv8", "rounded", g.SIZES_5, 500, "f16"),
    "g95_8": ("g95", "rounded", g.SIZES_G95, 950, "f32"),
    "kv8_mixed_3": ("kv8", "mixed", g.SIZES_5[:3], 500, "f32"),
    "kv8_fp8_2": ("kv8", "rounded", [8 * (39 + n + 5) for n in FP8_STEPS], 4600, "fp8"),
}

_W = {}
_ORACLE = {}


def _weights(cname, kind):
    """tests/test_gpu_batch_gemv.py's synth_weights(cfg, seed=1) (`plain`), their quantize_mxfp4
    rounding (`rounded`), or that with UNROUNDED put back as it was (`mixed`)"""
    from vox_weights import Weights, quantize_mxfp4
    key = (cname, kind)
    if key not in _W:
        plain = g._weights(CONFIGS[cname])
        if kind == "plain":
            _W[key] = plain
        elif kind == "rounded":
            _W[key] = quantize_mxfp4(plain)
        else:
            base = _weights(cname, "rounded")
            t = dict(base.t)
            t[UNROUNDED] = plain.t[UNROUNDED]
            assert not np.array_equal(t[UNROUNDED], base.t[UNROUNDED])
            _W[key] = Weights(base.cfg, t, keep=base._keep)
    return _W[key]


def _case_mels(case):
    cname, _, sizes, seed, _ = CASES[case]
    return g._mels(CONFIGS[cname], sizes, seed)


def _oracle(case):
    """[(ids, logits [steps, vocab])] per stream of an f32 / f16 case: each stream's own oracle
    session on the case's weights, decoded to the end of its adapter rows"""
    from concurrent.futures import ThreadPoolExecutor
    import vox_oracle
    if case in _ORACLE:
        return _ORACLE[case]
    cname, kind, sizes, seed, ring = CASES[case]
    assert ring in ("f32", "f16")
    cfg = CONFIGS[cname]
    om = vox_oracle.OracleModel(cfg, _weights(cname, kind))
    vox_oracle.set_kv_fp16(ring == "f16")
    try:
        vox_oracle.set_threads(min(4, os.cpu_count() or 1))
        sts, first = [], []
        for mel in _case_mels(case):
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


def _model(cname, kind="plain", mode=2):
    """a model created in wmx4 mode `mode` (2: the plain weights rounded at load; 1: detect)"""
    import vox_hip
    old = vox_hip.wmx4()
    vox_hip.set_wmx4(mode)
    try:
        return vox_hip.Model(CONFIGS[cname], _weights(cname, kind))
    finally:
        vox_hip.set_wmx4(old)


@pytest.fixture(scope="module")
def kv8_model():
    hm = _model("kv8")
    yield hm
    hm.close()


def _batch(hm, n, wmx4, rows=8):
    import vox_hip
    b = vox_hip.Batch(hm, n)
    assert b.set_gemv_rows(rows) == 0
    assert b.set_gemv_wmx4(wmx4) == 0
    assert b.gemv_wmx4_stats()[0] == int(wmx4)
    return b


def _decode_stepwise(hm, mels, slots, wmx4=1, steps=6, kv16=False):
    """tests/test_gpu_batch_gemv.py's _decode_stepwise with the weight-source flag: one Batch in
    GEMV mode 8 over the streams, `steps` single-step calls reading the logits of `slots` after
    each, then the drain.  Returns (ids per stream, {stream: [steps, vocab]}, gemv_stats,
    gemv_wmx4_stats)."""
    ss = g._open(hm, mels, kv16)
    b = _batch(hm, len(ss), wmx4)
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
    gst, mst = b.gemv_stats(), b.gemv_wmx4_stats()
    assert gst[1] == b.stats()["replays"] > 0, (gst, b.stats())     # every replay on the GEMV path
    for s in ss:
        s.close()
    b.close()
    return got, {i: np.stack(v) for i, v in lg.items()}, gst, mst


# ---- the test entry: k_gemvr<NONE, STORE, RB, KQ, WF_MX4, R> ------------------------------------
# (512, 768): one partial K round, 4-row groups where bf16 runs 2; (256, 3072): two rounds, the
# second half full (the full model's dec_dim); (256, 4096): wo's K, two full rounds; (128, 9216):
# five rounds, two passes at R = 8; (6144, 768): QKV's group count; (65536, 768): 8-row groups
ENTRY_SHAPES = [(512, 768), (256, 3072), (256, 4096), (128, 9216), (6144, 768), (65536, 768)]
ENTRY_R = (1, 2, 3, 5, 8)
_ENTRY = {}


def _entry_r(shape):
    return (1, 8) if shape[0] >= 65536 else ENTRY_R


def _entry(shape):
    """every shared call of the entry tests for one shape, made once: {(R, packed): (y, flags)}
    over the first R of 8 x rows, and k_gemv's wmx4 instance (gemv_wpack(.., 2)) on each row"""
    import vox_hip
    from vox_weights import mxfp4_round
    if shape in _ENTRY:
        return _ENTRY[shape]
    rows, K = shape
    W = g._w(rows, K, seed=rows + K)
    W[1, ::7] = 0x8000   # signed zeros
    W[2, ::5] = 0
    W = mxfp4_round(W)
    W.setflags(write=False)
    x = np.random.default_rng(K + rows).standard_normal((8, K)).astype(np.float32)
    x[3] *= 1e-3         # rows of different scale: a leak from a neighbour would show
    x[6] *= 40.0
    e = {"W": W, "x": x, "calls": {}, "gemv": []}
    for R in _entry_r(shape):
        for packed in (0, 1, 2):
            e["calls"][R, packed] = vox_hip.gemv_rows(W, x[:R], packed)
    e["gemv"] = [vox_hip.gemv_wpack(W, x[r], 2) for r in range(8)]
    _ENTRY[shape] = e
    return e


@pytest.mark.parametrize("shape", ENTRY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_entry_bits(shape):
    """packed = 2 returns bit 2 (the wmx4 instance ran) and bit 1; its y is bit-equal to the
    wpack13 instance's, to the raw one's and, row by row, to k_gemv<WF_MX4>'s; every row is within
    5e-5 of max|y| of the float64 product of the exact bf16 weights.  Measured worst (MI355X)
    over the six shapes: 1.87e-7 at (128, 9216), 1.14e-7 to 1.44e-7 on the others."""
    e = _entry(shape)
    ref = e["x"].astype(np.float64) @ ((e["W"].astype(np.uint32) << 16).view(np.float32).astype(np.float64)).T
    worst = 0.0
    for R in _entry_r(shape):
        (y0, f0), (y1, f1), (y2, f2) = (e["calls"][R, p] for p in (0, 1, 2))
        assert (f0 & 5, f1 & 5, f2 & 5) == (0, 1, 4), (shape, R, f0, f1, f2)
        assert f2 & 2, (shape, R, f2)
        assert y2.shape == (R, shape[0]) and np.isfinite(y2).all()
        assert g._bits_equal(y2, y1), (shape, R, "wpack13")
        assert g._bits_equal(y2, y0), (shape, R, "raw")
        for r in range(R):
            y1r, ran = e["gemv"][r]
            assert ran == 2, (shape, r, ran)
            assert g._bits_equal(y2[r], y1r), (shape, R, r, "k_gemv wmx4")
            err = float(np.max(np.abs(y2[r] - ref[r])) / np.max(np.abs(ref[r])))
            worst = max(worst, err)
            assert err < LOGIT_TOL, (shape, R, r, err)
    print(f"gemv_rows wmx4 {shape}: worst err {worst:.2e} of max|y| (bar {LOGIT_TOL:.0e})")


@pytest.mark.parametrize("shape", ENTRY_SHAPES[:5], ids=lambda s: f"{s[0]}x{s[1]}")
def test_entry_row_independence_bits(shape):
    """row r's bits do not change with R, with r's index, or with NaN / 1e30 in the other rows"""
    import vox_hip
    e = _entry(shape)
    x, W = e["x"], e["W"]
    y8 = e["calls"][8, 2][0]
    for R in ENTRY_R:   # the buckets 1, 2, 4, 8 (and 8 again), rows at the same index
        assert g._bits_equal(e["calls"][R, 2][0], y8[:R]), (shape, R)
    ym, _ = vox_hip.gemv_rows(W, x[[5, 0]], 2)
    assert g._bits_equal(ym[0], y8[5]) and g._bits_equal(ym[1], y8[0]), shape
    ym, _ = vox_hip.gemv_rows(W, x[[7, 1, 5]], 2)
    assert g._bits_equal(ym[2], y8[5]) and g._bits_equal(ym[0], y8[7]), shape
    # neighbours full of NaN / 1e30 (row 5 kept; row 2 kept in the other half of a two-pass instance)
    for fill in (np.nan, 1e30):
        xb = np.full_like(x, fill)
        xb[5], xb[2] = x[5], x[2]
        yb, f = vox_hip.gemv_rows(W, xb, 2)
        assert f & 4
        assert g._bits_equal(yb[5], y8[5]) and g._bits_equal(yb[2], y8[2]), (shape, fill)


def test_entry_refusal():
    """a W that is not MXFP4-valued: packed = 2 returns with bit 2 clear and gives the raw bits"""
    import vox_hip
    W = g._w(512, 768, seed=7)
    x = np.random.default_rng(7).standard_normal((5, 768)).astype(np.float32)
    y2, f2 = vox_hip.gemv_rows(W, x, 2)
    y0, f0 = vox_hip.gemv_rows(W, x, 0)
    assert f2 & 4 == 0 and f2 & 2, f2
    assert f0 & 5 == 0
    assert g._bits_equal(y2, y0)


# ---- the step -----------------------------------------------------------------------------------
def test_step_is_its_twin_and_the_oracle(kv8_model):
    """KV8 in wmx4 mode 2, 8 streams in the 8-row bucket: set_gemv_wmx4(0) (the wpack13 planes of
    the rounded model), then the same streams reopened with set_gemv_wmx4(1).  Ids and every read
    step's logits are array_equal between the two; ids equal the oracle's on the rounded weights to
    the end of every stream, logits of streams 0, 3 and 7 on six steps within 5e-5."""
    ws = kv8_model.wmx4_stats()
    assert ws["wmx4_tensors"] == 4 * KV8.dec_layers + 1, ws
    mels = _case_mels("kv8_8")
    got0, lg0, gst0, mst0 = _decode_stepwise(kv8_model, mels, (0, 3, 7), wmx4=0)
    got1, lg1, gst1, mst1 = _decode_stepwise(kv8_model, mels, (0, 3, 7), wmx4=1)
    assert got0 == got1
    for i in lg0:
        assert np.array_equal(lg0[i].view(np.uint32), lg1[i].view(np.uint32)), i
    g._compare(got1, lg1, _oracle("kv8_8"), LOGIT_TOL, "kv8 8 streams, gemv 8 on wmx4 planes")
    assert mst0 == (0, 0, 4 * KV8.dec_layers + 1, 0), mst0
    assert mst1 == (1, gst1[1], 4 * KV8.dec_layers + 1, 0) and gst1[1] > 0, (mst1, gst1)


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_other_buckets(kv8_model, n):
    """1, 2, 3 and 5 streams of ragged lengths: the 1-, 2-, 4- and 8-row instances, the last two
    with empty tail slots, slots going live = 0 mid-call.  Ids of every stream, six steps' logits
    of the first and last stream."""
    ref = _oracle("kv8_5")[:n]
    assert len({len(ids) for ids, _ in _oracle("kv8_5")}) == 5
    got, lg, gst, mst = _decode_stepwise(kv8_model, _case_mels("kv8_5")[:n], sorted({0, n - 1}))
    g._compare(got, lg, ref, LOGIT_TOL, f"kv8 {n} streams, gemv 8 on wmx4 planes")
    assert mst[1] == gst[1] > 0


def test_g95_8_streams():
    """G95 (dec_hidden 9216), 8 streams: W2 with K = 9216, five K rounds and at 8 rows two passes
    (rows 0-3, then 4-7) over 4-row groups; logits of streams 0, 3, 4 and 7"""
    hm = _model("g95")
    try:
        assert hm.wmx4_stats()["wmx4_tensors"] == 4 * G95.dec_layers + 1
        got, lg, gst, mst = _decode_stepwise(hm, _case_mels("g95_8"), (0, 3, 4, 7))
    finally:
        hm.close()
    g._compare(got, lg, _oracle("g95_8"), LOGIT_TOL, "g95 8 streams, gemv 8 on wmx4 planes")
    assert mst[1] == gst[1] > 0 and mst[3] == 0


def test_fp16_rings(kv8_model):
    """5 streams on IEEE-half K/V rings (kv_st2_rt's half branch in the wmx4 QKV instance), at the
    fp16 bar against the oracle that rounds every K/V append to half"""
    got, lg, gst, mst = _decode_stepwise(kv8_model, _case_mels("kv8_5_kv16"), (0, 4), kv16=True)
    g._compare(got, lg, _oracle("kv8_5_kv16"), LOGIT_TOL16, "kv8 5 streams, gemv 8 on wmx4 planes, fp16 rings")
    assert mst[1] == gst[1] > 0


def test_fp8_rings(kv8_model):
    """2 streams on FP8 (E4M3) rings in the 2-row bucket, stream 1 after 3 steps of its own: the
    GPU runs first, then the ring-conditioned replay of tests/kv8_ref.py (on the rounded weights)
    checks every stored K/V row by the adjacent-code rule, adopts it, and holds every id, the
    replay's own 2e-4 top-2 margin, and the logits of each call's last step at 5e-5"""
    import vox_hip
    import vox_oracle
    from kv8_ref import MARGIN, RefDecoder, check_fp8_rows, oracle_adapter
    assert MARGIN == MARGIN_F32
    mels = _case_mels("kv8_fp8_2")
    hm = kv8_model
    ss = []
    for mel in mels:
        hm.set_kv_dtype(vox_hip.KV_FP8)
        s = vox_hip.Stream(hm)
        hm.set_kv_dtype(vox_hip.KV_F32)
        assert s.kv_dtype == vox_hip.KV_FP8
        s.encode_mel(mel)
        ss.append(s)
    ids = [[] for _ in ss]
    lgs = [[] for _ in ss]
    t, lg = ss[1].decode(max_steps=3, stop_at_eos=False, want_logits=True)
    ids[1] += t.tolist()
    lgs[1] += list(lg)
    b = _batch(hm, 2, 1, rows=2)
    while any(len(ids[k]) < FP8_STEPS[k] for k in range(2)):
        act = [k for k in range(2) if len(ids[k]) < FP8_STEPS[k]]
        left = min(FP8_STEPS[k] - len(ids[k]) for k in act)
        n = 1 if left <= 2 else left - 2
        for k, t in zip(act, b.decode([ss[k] for k in act], max_steps=n, stop_at_eos=False)):
            assert len(t) == n
            ids[k] += t.tolist()
            lgs[k] += [None] * (n - 1) + [b.read_logits(ss[k])]
    mst = b.gemv_wmx4_stats()
    assert mst[1] == b.gemv_stats()[1] > 0
    b.close()
    w = _weights("kv8", "rounded")
    om = vox_oracle.OracleModel(KV8, w)
    try:
        for k, s in enumerate(ss):
            pos = s.state()["kv_pos"]
            assert pos == 38 + FP8_STEPS[k]
            rk = [s.read_kv(l, 0, pos, decoded=True) for l in range(KV8.dec_layers)]
            adj = [0]

            def hook(kk, vv, layer, p0):
                gk, gv = rk[layer][0][p0:p0 + kk.shape[0]], rk[layer][1][p0:p0 + kk.shape[0]]
                adj[0] += check_fp8_rows(kk, gk, f"stream {k} K layer {layer} pos {p0}")
                adj[0] += check_fp8_rows(vv, gv, f"stream {k} V layer {layer} pos {p0}")
                return gk, gv

            r = RefDecoder(KV8, w, oracle_adapter(om, mels[k]), om.ada_scale(), round_fn=hook)
            worst = 0.0
            for i, gid in enumerate(ids[k]):
                rid, rlg = r.step(force_token=gid)
                scale = float(np.max(np.abs(rlg)))
                s2 = np.sort(rlg)
                assert float(s2[-1] - s2[-2]) / scale >= MARGIN, (k, i)
                assert rid == gid, (k, i, rid, gid)
                if lgs[k][i] is not None:
                    err = float(np.max(np.abs(lgs[k][i] - rlg))) / scale
                    worst = max(worst, err)
                    assert err < LOGIT_TOL, (k, i, err)
            assert r.pos == pos
            print(f"fp8 rings stream {k}: {len(ids[k])} ids equal, {adj[0]} adjacent-code elements, logits rel err {worst:.2e}")
    finally:
        om.close()
        for s in ss:
            s.close()


def test_mixed_tensors():
    """detect mode (wmx4 mode 1) on a rounded KV8 checkpoint whose layer-1 wo is left unrounded:
    that tensor keeps its wpack13 launch inside the same step; ids and logits match the oracle on
    those weights"""
    hm = _model("kv8", "mixed", mode=1)
    try:
        ws = hm.wmx4_stats()
        assert ws["wmx4_tensors"] == 4 * KV8.dec_layers and ws["refused_tensors"] == 1, ws
        got, lg, gst, mst = _decode_stepwise(hm, _case_mels("kv8_mixed_3"), (0, 2))
    finally:
        hm.close()
    g._compare(got, lg, _oracle("kv8_mixed_3"), LOGIT_TOL, "kv8 3 streams, one tensor without a wmx4 plane")
    assert mst == (1, gst[1], 4 * KV8.dec_layers, 1) and gst[1] > 0, (mst, gst)


def test_mode_change_between_calls(kv8_model):
    """4 streams: the flag alternates 1, 0, 1, 0, 1, 0 over six single-step calls, then 1 to the
    end; the oracle's ids and stream 2's logits throughout.  Inside a begun call the setter
    returns -1 and the flag stays."""
    import vox_hip
    ref = _oracle("kv8_8")[:4]
    ss = g._open(kv8_model, _case_mels("kv8_8")[:4])
    b = _batch(kv8_model, 4, 0)
    got = [[] for _ in ss]
    lg = []
    for k in range(6):
        assert b.set_gemv_wmx4(1 - k % 2) == 0
        for i, t in enumerate(b.decode(ss, max_steps=1, stop_at_eos=False)):
            assert len(t) == 1
            got[i] += t.tolist()
        lg.append(b.read_logits(ss[2]))
    assert b.gemv_wmx4_stats()[:2] == (0, 3) and b.gemv_stats()[1] == 6
    assert b.gemv_stats()[3] == 2                       # one graph per weight source
    # a begun call: two steps in flight
    n = len(ss)
    arr = (ctypes.c_void_p * n)(*[s.h for s in ss])
    rows = (ctypes.c_int * n)(*[s.adapter_tokens for s in ss])
    toks = np.zeros((n, 2), np.int32)
    cnt = np.zeros(n, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    L = vox_hip.lib()
    assert L.vox_hip_batch_begin_rows(b.h, arr, n, rows, 2, 0, toks.ctypes.data_as(ip), cnt.ctypes.data_as(ip)) == 0
    L.vox_hip_clear_error()
    assert b.set_gemv_wmx4(1) == -1
    assert b"begun call" in L.vox_hip_last_error()
    assert L.vox_hip_batch_finish(b.h) >= 0
    assert b.gemv_wmx4_stats()[0] == 0
    for i in range(n):
        assert cnt[i] == 2
        got[i] += toks[i, :2].tolist()
    assert b.set_gemv_wmx4(1) == 0
    for i, t in enumerate(b.decode(ss, max_steps=1000, stop_at_eos=False)):
        got[i] += t.tolist()
    g._compare(got, {2: np.stack(lg)}, ref, LOGIT_TOL, "kv8 4 streams, wmx4 flag alternating")
    for s in ss:
        s.close()
    b.close()


def _alts_run(hm, wmx4):
    import vox_hip
    settings = [(3, 1.0), (1, 1.0), (4, 0.5)]
    ss = [vox_hip.Stream(hm) for _ in settings]
    for s, mel, (na, co) in zip(ss, _case_mels("kv8_5")[:3], settings):
        s.set_alt(na, co)
        s.encode_mel(mel)
    b = _batch(hm, 4, wmx4)
    got = [t.tolist() for t in b.decode(ss, max_steps=1000, stop_at_eos=False)]
    assert b.gemv_stats()[1] == b.stats()["replays"] > 0
    alts = [s.read_alts(0, len(t)) for s, t in zip(ss, got)]
    for s in ss:
        s.close()
    b.close()
    return got, alts


def test_alternatives(kv8_model):
    """streams with alternatives on: ids and alternative records of the step on the wmx4 planes
    are those of the wpack13 GEMV step (array_equal), and the ids the oracle's"""
    got0, alts0 = _alts_run(kv8_model, 0)
    got1, alts1 = _alts_run(kv8_model, 1)
    assert got1 == got0 == [ids for ids, _ in _oracle("kv8_5")[:3]]
    n_with = 0
    for (i0, p0), (i1, p1) in zip(alts0, alts1):
        assert np.array_equal(i0, i1) and np.asarray(p0).tobytes() == np.asarray(p1).tobytes()
        n_with += int(np.sum(np.asarray(i1)[:, 1] >= 0))
    assert n_with > 0


# ---- off is off ---------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[2], sys.argv[3], sys.argv[4]]
import vox_hip
import test_gpu_batch_gemv_wmx4 as t

out = {"mode": np.array(vox_hip.wmx4())}
hm = vox_hip.Model(t.KV8, t._weights("kv8", "plain"))
ss = t.g._open(hm, t._case_mels("kv8_8")[:2])
b = vox_hip.Batch(hm, 2)
out["rows"] = np.array(b.gemv_stats()[0])
out["before"] = np.array(b.gemv_wmx4_stats())
ids = [x.tolist() for x in b.decode(ss, max_steps=6, stop_at_eos=False)]
out["ids"] = np.array(ids)
out["after"] = np.array(b.gemv_wmx4_stats())
out["gemv"] = np.array(b.gemv_stats())
b.close()
for s in ss:
    s.close()
hm.close()
vox_hip.set_wmx4(0)
hm = vox_hip.Model(t.KV8, t._weights("kv8", "plain"))
b = vox_hip.Batch(hm, 2)
vox_hip.lib().vox_hip_clear_error()
out["set0"] = np.array(b.set_gemv_wmx4(1))
out["err0"] = np.array(vox_hip.lib().vox_hip_last_error().decode())
out["stats0"] = np.array(b.gemv_wmx4_stats())
b.close()
hm.close()
np.savez(sys.argv[1], **out)
"""


def test_off_is_off(tmp_path):
    """a child process with VOX_HIP_WMX4=2 VOX_HIP_BATCH_GEMV=8 and VOX_HIP_BATCH_GEMV_WMX4 unset:
    the flag is 0 and no replay streams a wmx4 plane (the GEMV step runs, on the wpack13 planes,
    and gives the oracle's ids); on a model in mode 0 the setter returns -1 with the documented
    message"""
    path = str(tmp_path / "off.npz")
    env = dict(os.environ, VOX_HIP_WMX4="2", VOX_HIP_BATCH_GEMV="8")
    for k in ("VOX_HIP_BATCH_GEMV_WMX4", "VOX_HIP_WMX4_BATCH", "VOX_HIP_WPACK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CHILD, path, os.path.join(ROOT, "voxtral.c_amd"), os.path.join(ROOT, "oracle"),
                        os.path.join(ROOT, "tests")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    z = np.load(path)
    assert int(z["mode"]) == 2 and int(z["rows"]) == 8
    assert z["before"].tolist() == [0, 0, 4 * KV8.dec_layers + 1, 0]
    assert z["after"].tolist()[:2] == [0, 0]
    assert z["gemv"][1] == 6
    ref = _oracle("kv8_8")[:2]
    for i in range(2):
        assert z["ids"][i].tolist() == ref[i][0][:6], i
    assert int(z["set0"]) == -1 and "no wmx4 GEMV plane" in str(z["err0"])
    assert z["stats0"].tolist() == [0, 0, 0, 4 * KV8.dec_layers + 1]
