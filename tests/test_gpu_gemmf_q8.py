"""k_gemmf over the int8 fragment copies of Q8 tensors (vox_hip_set_gemmf_q8).

1. The kernel: gemmf_q8_rows(fmt = 1) (int8 blocks, row scales in the epilogue) against
   gemmf_q8_rows(fmt = 0) (the bf16 fragment copy of the same integers through the bf16 instance of
   the same tile) times the scales in f32 on the host: equal bits, with the owner waiting and under
   the owner-recompute backstop; and both within the plane count's bar of an f64 statement of
   x @ (q * scale)^T (2e-6 of the largest magnitude with three planes, 5e-5 with two: the bars of
   tests/test_gpu_gemm_planes.py).  The two-plane instances run in child processes (the plane
   count is read once per process), at 64-row and, forced, 128-row tiles.
2. TINY quantised with the switch on: the jfk one-shot schedule (677-row encoder pass, 38-row
   prefill) against the Q8 oracle at the bars of tests/test_gpu_q8.py, and the same ids with it off.
3. The wide step at 64 and 33 streams: the model, sizes, seed and margin rule of
   tests/test_gpu_batch_wide.py::test_wide_q8_64_streams (imported, not copied).
4. The stacked prefill of three streams with f32 and IEEE-half rings: the tiny_q8_3 case of
   tests/test_gpu_prefill_kv.py (its mels and oracle helper imported).  The f32 oracle's top-2 gap
   with those mels is 5.6e-3, the half one's 5.6e-3 (rules 2e-4 and 4e-4, asserted before any
   comparison).
A Q8 weight set with one tensor left bf16 is not something vox_hip.Model can be given (the weight
table carries the scale arrays for all tensors or none), so the per-launch dispatch is covered by
the engine's two formats in one process (case 1) only."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 5e-5            # adapter rows and logits, of the largest magnitude (tests/test_gpu_q8.py)
SHAPES = [(5, 128, 768), (70, 256, 1280), (16, 128, 64), (130, 384, 512)]
F64_BAR = {3: 2e-6, 2: 5e-5}


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))


def q8_case(M, N, K):
    """int8 from the full range with -128 and 127 in every row, scales in [2^-10, 2^-3] (no
    subnormal product), standard normal rows"""
    rng = np.random.default_rng(1000 * M + N + K)
    q = rng.integers(-128, 128, size=(N, K), dtype=np.int8)
    q[:, 3] = -128
    q[:, K - 5] = 127
    sc = rng.uniform(2.0 ** -10, 2.0 ** -3, size=N).astype(np.float32)
    x = rng.standard_normal((M, K)).astype(np.float32)
    return x, q, sc


def check_shape(vox_hip, M, N, K, what):
    x, q, sc = q8_case(M, N, K)
    y1 = vox_hip.gemmf_q8_rows(x, q, sc, 1)
    y0 = vox_hip.gemmf_q8_rows(x, q, sc, 0)
    want = np.float32(y0) * sc[None, :]
    ref = x.astype(np.float64) @ (q.astype(np.float64) * sc.astype(np.float64)[:, None]).T
    e1, e0 = rel(y1, ref), rel(want, ref)
    bad = int(np.count_nonzero(y1 != want))
    print(f"{what} M {M} N {N} K {K}: {bad} of {y1.size} differ from f32(bf16 instance) * scale; "
          f"f64 err int8 {e1:.2e} bf16 {e0:.2e}")
    assert np.all(np.isfinite(y1)) and float(np.max(np.abs(y1))) > 0
    assert np.array_equal(y1, want), (what, M, N, K, bad)
    bar = F64_BAR[vox_hip.gemm_planes()]
    assert e1 < bar and e0 < bar, (what, M, N, K, e1, e0, bar)


# ---- 1: the kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("wait", [None, -1], ids=["handoff", "owner_recompute"])
def test_int8_instance_has_the_bf16_instances_accumulators(wait):
    import vox_hip
    old = vox_hip.set_gemmf_wait(wait) if wait is not None else None
    try:
        for M, N, K in SHAPES:
            check_shape(vox_hip, M, N, K, "wait %s" % wait)
    finally:
        if wait is not None:
            vox_hip.set_gemmf_wait(old)


def test_refused_shape_reports_an_error():
    import vox_hip
    x, q, sc = q8_case(4, 192, 64)  # N % 128 != 0
    with pytest.raises(RuntimeError, match="gemmf_q8_rows"):
        vox_hip.gemmf_q8_rows(x, q, sc, 1)


CHILD = r"""
import sys
sys.path.insert(0, {pkg!r})
sys.path.insert(0, {tests!r})
import vox_hip
import test_gpu_gemmf_q8 as t
assert vox_hip.gemm_planes() == 2
for M, N, K in ((130, 384, 512), (5, 128, 768)):
    t.check_shape(vox_hip, M, N, K, "two planes")
print("two planes ok")
"""


@pytest.mark.parametrize("rb", ["", "8"], ids=["rb4", "rb8"])
def test_two_plane_instances_in_a_child_process(rb):
    """VOX_HIP_GEMM_PLANES=2: the int8 instances run 8 waves (WR = 2) where the bf16 ones run 16,
    at 64-row tiles by shape and 128-row tiles with VOX_HIP_GEMMF_RB=8: the same bits."""
    code = CHILD.format(pkg=os.path.join(ROOT, "voxtral.c_amd"), tests=os.path.join(ROOT, "tests"))
    env = dict(os.environ, VOX_HIP_GEMM_PLANES="2")
    env.pop("VOX_HIP_GEMMF_RB", None)
    if rb:
        env["VOX_HIP_GEMMF_RB"] = rb
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "two planes ok" in r.stdout, r.stdout
    print(r.stdout)


# ---- models with the switch on ----------------------------------------------------------------------
def model_with_switch(cfg, w, on):
    """the switch is read at creation: set, create, restore"""
    import vox_hip
    old = vox_hip.gemmf_q8()
    vox_hip.set_gemmf_q8(on)
    try:
        return vox_hip.Model(cfg, w)
    finally:
        vox_hip.set_gemmf_q8(bool(old))


# ---- 2: encoder and single-stream prefill ------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_q8(tiny_cfg, tiny_weights):
    from vox_weights import quantize_q8
    return quantize_q8(tiny_weights)


@pytest.fixture(scope="module")
def jfk_oracle(tiny_cfg, tiny_q8, jfk_samples):
    """(events, ids, adapter rows, logits) of the Q8 oracle on the jfk one-shot schedule, once"""
    import vox_oracle
    om = vox_oracle.OracleModel(tiny_cfg, tiny_q8)
    events = vox_oracle.transcribe_mel_schedule(jfk_samples)
    st = vox_oracle.OracleStream(om)
    ids, logs, done = [], [], 0
    for _, mel in events:
        st.encode_mel(mel[done:])
        t, lg = st.decode(stop_at_eos=False, want_logits=True)
        ids += t.tolist()
        logs.append(lg)
        done = mel.shape[0]
    ad = st.read_adapter().copy()
    st.close()
    om.close()
    lg = np.concatenate(logs)
    ad.setflags(write=False)
    lg.setflags(write=False)
    return events, ids, ad, lg


def run_jfk(hm, events):
    import vox_hip
    hs = vox_hip.Stream(hm)
    ids, logs, done = [], [], 0
    for _, mel in events:
        hs.encode_mel(mel[done:])
        t, lg = hs.decode(stop_at_eos=False, want_logits=True)
        ids += t.tolist()
        logs.append(lg)
        done = mel.shape[0]
    ad = hs.read_adapter()
    hs.close()
    return ids, ad, np.concatenate(logs)


def test_jfk_encoder_and_prefill_on_int8_fragments(tiny_cfg, tiny_q8, jfk_oracle):
    events, oids, oad, olg = jfk_oracle
    hm = model_with_switch(tiny_cfg, tiny_q8, True)
    try:
        st0 = hm.gemmf_q8_stats()
        # 4 matrices per encoder and decoder layer and the LM head, every shape accepted
        assert st0[0] == 1 and st0[1] == 0 and st0[3] == 0, st0
        assert st0[2] == 4 * (tiny_cfg.enc_layers + tiny_cfg.dec_layers) + 1, st0
        ids, ad, lg = run_jfk(hm, events)
        st1 = hm.gemmf_q8_stats()
    finally:
        hm.close()
    ra, rl = rel(ad, oad), rel(lg, olg)
    print(f"jfk on int8 fragments: {len(ids)} ids, adapter rel err {ra:.2e}, logits rel err {rl:.2e}, stats {st1}")
    assert len(oids) > 100 and ids == oids
    assert ra < TOL and rl < TOL, (ra, rl)
    assert st1[1] > 0 and st1[3] == 0, st1


def test_switch_off_counts_nothing_and_gives_the_same_ids(tiny_cfg, tiny_q8, jfk_oracle):
    events, oids, oad, olg = jfk_oracle
    hm = model_with_switch(tiny_cfg, tiny_q8, False)
    try:
        ids, ad, lg = run_jfk(hm, events)
        st = hm.gemmf_q8_stats()
    finally:
        hm.close()
    assert st[0] == 0 and st[1] == 0, st
    assert ids == oids
    assert rel(ad, oad) < TOL and rel(lg, olg) < TOL


# ---- 3: the wide step ---------------------------------------------------------------------------------
def wide_stepwise(hm, mels, slots, steps=6):
    """test_gpu_batch_kv8._decode_stepwise's call pattern, returning the batch's counters too"""
    import test_gpu_batch_kv8 as g
    import vox_hip
    ss = g._open(hm, mels)
    b = vox_hip.Batch(hm, len(ss))
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
    st = b.stats()
    for s in ss:
        s.close()
    b.close()
    return got, {i: np.stack(v) for i, v in lg.items()}, st


def test_wide_step_64_and_33_streams_on_int8_fragments():
    import test_gpu_batch_kv8 as g
    import test_gpu_batch_wide as wide
    import vox_hip
    from test_gpu_batch_kv8 import KV8, LOGIT_TOL, MARGIN_F32
    ref = g._oracle("kv8", KV8, wide.SIZES[:64], 6417, q8=True)
    g._assert_margin(ref, MARGIN_F32, "wide q8 64 streams")
    mels = wide._mels(64, 6417)
    hm = model_with_switch(KV8, g._weights(KV8, q8=True), True)
    try:
        n0 = hm.gemmf_q8_stats()[1]
        got, lg, st64 = wide_stepwise(hm, mels, (0, 31, 32, 63))
        n1 = hm.gemmf_q8_stats()[1]
        got33, lg33, st33 = wide_stepwise(hm, mels[:33], ())
        n2 = hm.gemmf_q8_stats()[1]
        assert hm.gemmf_q8_stats()[3] == 0
    finally:
        hm.close()
    g._compare(got, lg, ref, LOGIT_TOL, "wide q8 gemmf 64 streams")
    g._compare(got33, lg33, ref[:33], LOGIT_TOL, "wide q8 gemmf 33 streams")
    # every wide step launches 4 projections per layer and the LM head on int8 fragments
    per_step = 4 * KV8.dec_layers + 1
    assert n1 - n0 >= per_step * st64["replays"] > 0, (n0, n1, st64)
    assert n2 > n1, (n1, n2)
    # the same call pattern on the bf16 model: no more captures than it needs
    hb = vox_hip.Model(KV8, g._weights(KV8))
    try:
        _, _, sb64 = wide_stepwise(hb, mels, ())
        _, _, sb33 = wide_stepwise(hb, mels[:33], ())
        assert hb.gemmf_q8_stats()[1] == 0
    finally:
        hb.close()
    print(f"wide q8 gemmf: int8 launches {n1 - n0} + {n2 - n1}; captures {st64['captures']} / {st33['captures']} "
          f"(bf16 {sb64['captures']} / {sb33['captures']})")
    assert st64["captures"] <= sb64["captures"] and st33["captures"] <= sb33["captures"], (st64, sb64, st33, sb33)


# ---- 4: the stacked prefill ----------------------------------------------------------------------------
@pytest.mark.parametrize("kv16", [False, True], ids=["f32", "kv16"])
def test_stacked_prefill_of_three_streams_on_int8_fragments(kv16):
    import test_gpu_prefill_kv as pk
    import vox_hip
    import vox_oracle
    case = "tiny_q8_3"
    cfg_name, kind, _, toks = pk.HALF[case]
    cfg, w = pk.CFGS[cfg_name], pk._weights(cfg_name, kind)
    mels = pk._case_mels(case)
    om = pk._oracle_model(cfg_name, kind)
    try:
        if kv16:
            ref = pk.half_oracle(case, om)
        else:
            ref = []
            for mel, n in zip(mels, toks):
                st = vox_oracle.OracleStream(om)
                st.encode_mel(mel)
                ids, lg = st.decode(stop_at_eos=False, want_logits=True)
                st.close()
                assert len(ids) == n
                ref.append((ids.tolist(), lg))
    finally:
        om.close()
    margin, tol = (pk.MARGIN_KV16, pk.LOGIT_TOL16) if kv16 else (pk.MARGIN, pk.LOGIT_TOL)
    for i, (ids, lg) in enumerate(ref):
        assert np.array_equal(np.argmax(lg, axis=1), np.asarray(ids)), i
        gap = float(pk._gaps(lg).min())
        assert gap >= margin, (i, gap, margin)
    hm = model_with_switch(cfg, w, True)
    try:
        ss = [pk._stream(hm, vox_hip.KV_F16 if kv16 else vox_hip.KV_F32, mel) for mel in mels]
        n_enc = hm.gemmf_q8_stats()[1]
        b = vox_hip.Batch(hm, max(4, len(ss)))
        got = [[] for _ in ss]
        worst = 0.0
        for step in range(max(toks)):
            act = [k for k in range(len(ss)) if step < toks[k]]
            out = b.decode([ss[k] for k in act], max_steps=1, stop_at_eos=False)
            if step == 0:
                st = b.stats()
                assert st["prefill_passes"] == 1 and st["prefilled"] == len(ss), st
                # the stacked pass: 4 projections per layer on int8 fragments
                assert hm.gemmf_q8_stats()[1] - n_enc == 4 * cfg.dec_layers, (n_enc, hm.gemmf_q8_stats())
            for k, t in zip(act, out):
                assert len(t) == 1, (k, step)
                got[k] += t.tolist()
                rlg = ref[k][1][step]
                err = float(np.max(np.abs(b.read_logits(ss[k]) - rlg))) / float(np.max(np.abs(rlg)))
                worst = max(worst, err)
                assert err < tol, (k, step, err)
        assert b.stats()["prefill_passes"] == 1
        b.close()
        for k, s in enumerate(ss):
            s.close()
            assert got[k] == ref[k][0], k
    finally:
        hm.close()
    print(f"stacked prefill on int8 fragments (kv16 {kv16}): {sum(toks)} ids equal, logits rel err {worst:.2e}")
