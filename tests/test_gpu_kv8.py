"""The opt-in FP8 (E4M3) decoder KV rings (vox_hip_model_set_kv_dtype(m, 2), VOX_HIP_KV_FP8).

Convert: the kernels' own store / load helpers (vox_hip_kv8_convert) against the host rule of
csrc/vox_kv8.h, byte for byte and bit for bit.

Ring-conditioned parity: with 3 mantissa bits a GPU K/V element that differs from the CPU's in
the last f32 bit can land on the neighbouring code (6-12 % of the element), after which every
later activation decorrelates at ~1e-3 and a comparison against a rounded oracle means nothing.
So the GPU stream runs first, its ring codes are read back (Stream.read_kv), and the reference
session (tests/kv8_ref.py, pinned bit for bit to the oracle in tests/test_kv8_cpu.py) is
replayed position by position: at every layer it computes its own K/V rows from its own
activations, compares them with what the GPU stored --

    a GPU element equals the reference's rounding (as decoded values), or it is the adjacent
    code across a midpoint that lies within ACT_TOL = 5e-5 x max|row| of the reference's
    unrounded value; anything else fails

-- and then adopts the GPU's stored rows before that layer's attention (prefill rows the same
way).  Both sides then attend identical rings, so every step's logits are held to the f32 ring's
LOGIT_TOL = 5e-5, every id must be equal, and the replay's top-2 margin must be at least
4 x LOGIT_TOL on every step (the mel seeds were picked on the CPU with the unforced FP8
reference so that it is; test_kv8_cpu.py pins that).  ACT_TOL is the project's f32 activation
bar: test_f32_ring_within_act_tol checks the unchanged f32 path's ring against the oracle's K/V
at the same bar and prints what it measures."""
import numpy as np
import pytest

import kv8_ref
from kv8_ref import ACT_TOL, CFGS, MARGIN, RUNS, RefDecoder, check_fp8_rows, oracle_adapter, run_mels, top2_margin

pytestmark = pytest.mark.gpu

LOGIT_TOL = 5e-5     # of the step's largest logit magnitude, as tests/test_gpu_batch.py
CHUNK = 4096
MAX_CALL = 64        # steps per decode call between ring read-backs (the ring's slack)

_M = {}


def _models(cfg_name):
    """(hip model, oracle model, weights) per config, made once"""
    if cfg_name not in _M:
        import os

        import vox_hip
        import vox_oracle
        from vox_weights import synth_weights
        vox_oracle.set_threads(min(16, os.cpu_count() or 1))
        cfg = CFGS[cfg_name]
        w = synth_weights(cfg, seed=1)
        _M[cfg_name] = (vox_hip.Model(cfg, w), vox_oracle.OracleModel(cfg, w), w)
    return _M[cfg_name]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
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


def _gpu_single(hm, dtype, mel, steps):
    """ids, logits and ring rows of a single-stream decode in calls of <= MAX_CALL steps"""
    s = _stream(hm, dtype, mel)
    rg = Rings(s)
    ids, lgs = [], []
    while len(ids) < steps:
        t, lg = s.decode(max_steps=min(MAX_CALL, steps - len(ids)), stop_at_eos=False, want_logits=True)
        assert len(t) > 0
        ids += t.tolist()
        lgs.append(lg)
        rg.pull()
    rg.done()
    if rg.n > s.cfg.dec_window + 64:
        with pytest.raises(RuntimeError, match="overwritten"):     # position 0 left the ring at the wrap
            s.read_kv(0, 0, 1)
    s.close()
    return ids, np.concatenate(lgs), rg


def _replay(cfg_name, mel, ids, logits, rg, what, f32_logits=None):
    """the ring-conditioned replay of one stream; returns (adjacent-code elements, worst logit err)"""
    hm, om, w = _models(cfg_name)
    cfg = CFGS[cfg_name]
    adj = [0]

    def hook(k, v, layer, pos):
        n = k.shape[0]
        gk, gv = rg.K[layer][pos:pos + n], rg.V[layer][pos:pos + n]
        assert gk.shape == k.shape, (what, layer, pos, gk.shape, k.shape)
        adj[0] += check_fp8_rows(k, gk, f"{what} K layer {layer} pos {pos}")
        adj[0] += check_fp8_rows(v, gv, f"{what} V layer {layer} pos {pos}")
        return gk, gv

    r = RefDecoder(cfg, w, oracle_adapter(om, mel), om.ada_scale(), round_fn=hook)
    worst, rlgs = 0.0, []
    for i, gid in enumerate(ids):
        out = r.step(force_token=gid)
        assert out is not None, (what, i)
        rid, rlg = out
        rlgs.append(rlg)
        scale = float(np.max(np.abs(rlg)))
        s2 = np.sort(rlg)
        margin = float(s2[-1] - s2[-2]) / scale
        assert margin >= MARGIN, (what, i, margin)
        assert rid == gid, (what, i, rid, gid)
        if logits is not None and logits[i] is not None:
            err = float(np.max(np.abs(logits[i] - rlg))) / scale
            worst = max(worst, err)
            assert err < LOGIT_TOL, (what, i, err)
    assert r.pos == rg.n, (what, r.pos, rg.n)
    if f32_logits is not None:
        # the rounding is applied: the FP8 logits are nearer the replay than the f32 oracle
        rl = np.stack(rlgs)
        have = [i for i in range(len(ids)) if logits[i] is not None]
        g = np.stack([logits[i] for i in have])
        d_replay = float(np.max(np.abs(g - rl[have])))
        d_f32 = float(np.max(np.abs(g - f32_logits[have])))
        assert d_replay < d_f32, (what, d_replay, d_f32)
    print(f"{what}: {len(ids)} ids equal, {r.pos} positions x {cfg.dec_layers} layers, "
          f"{adj[0]} adjacent-code elements, logits rel err {worst:.2e}")
    return adj[0], worst


def _f32_oracle_logits(cfg_name, mel, n):
    import vox_oracle
    _, om, _ = _models(cfg_name)
    st = vox_oracle.OracleStream(om)
    for i in range(0, mel.shape[0], CHUNK):
        st.encode_mel(mel[i:i + CHUNK])
    ids, lg = st.decode(max_steps=n, stop_at_eos=False, want_logits=True)
    st.close()
    return lg


# ---- convert ---------------------------------------------------------------------------------
def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_kv8_convert_equals_host_rule():
    """every code value, every midpoint and its two f32 neighbours, saturation, zeros, NaNs and
    1e5 random values over 2^+-12, each at all 8 positions of the kernel's 8-element group (pair
    store, single store, word / pair / single load)"""
    import vox_hip
    rng = np.random.default_rng(17)
    mid = kv8_ref.kv8_midpoints()
    mid = np.concatenate([mid, np.float32([464.0])])
    parts = [kv8_ref.c_kv8_decode(np.arange(256, dtype=np.uint8))]
    for m in (mid, -mid):
        parts += [m, np.nextafter(m, np.float32(0)), np.nextafter(m, np.float32(np.inf) * np.sign(m))]
    big = np.float32([448, 463.99997, 464, 464.00003, 480, 1e9, 3.4e38, np.inf])
    parts += [big, -big, np.float32([0.0, -0.0, 1e-45, -1e-45, 1e-38, 2.0 ** -10, -(2.0 ** -10)])]
    parts.append(np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffc12345], np.uint32).view(np.float32))
    parts.append(np.linspace(0, 2.0 ** -6, 1025).astype(np.float32))
    parts.append((rng.choice([-1.0, 1.0], 100000) * 2.0 ** rng.uniform(-12, 12, 100000)).astype(np.float32))
    x = np.concatenate(parts).astype(np.float32)
    want_c, want_b = kv8_ref.c_kv8_encode(x)
    assert np.array_equal(want_c, kv8_ref.np_kv8_encode(x))
    for shift in range(8):
        xs = np.concatenate([np.zeros(shift, np.float32), x])
        codes, back = vox_hip.kv8_convert(xs)
        codes, back = codes[shift:], back[shift:]
        bad = np.nonzero(codes != want_c)[0]
        assert bad.size == 0, (shift, bad.size, x[bad[:5]], codes[bad[:5]], want_c[bad[:5]])
        nb = np.nonzero(_bits(back) != _bits(want_b))[0]
        # the two NaN codes: v_cvt_pk_f32_fp8 returns a NaN of its own sign and payload where
        # vox_kv8_decode gives the quiet NaN with the code's sign; a NaN has no value to be exact
        # about, so there both sides only have to be NaN (every other code: bit for bit)
        nanb = sorted({hex(int(b)) for b in _bits(back[np.isnan(back)])})
        nb = [i for i in nb if not (np.isnan(back[i]) and np.isnan(want_b[i]))]
        assert not nb, (shift, len(nb), x[nb[:5]], back[nb[:5]], want_b[nb[:5]])
    print(f"kv8 convert: {x.size} values x 8 group positions equal the host rule; device NaN bits {nanb}")
    assert np.array_equal(vox_hip.kv8_decode(np.arange(256, dtype=np.uint8))[:0x7f], kv8_ref.np_kv8_decode(np.arange(0x7f)))


# ---- defaults, memory, mixing ----------------------------------------------------------------
def test_kv8_default_memory_and_mixing():
    import vox_hip
    hm, _, _ = _models("TINY_LONG")
    L = vox_hip.lib()
    m0 = L.vox_hip_memory_used()
    s32 = vox_hip.Stream(hm)
    m1 = L.vox_hip_memory_used()
    assert s32.kv_dtype == vox_hip.KV_F32 and not s32.kv_fp16          # nothing set: f32
    hm.set_kv_dtype(vox_hip.KV_FP8)
    s8 = vox_hip.Stream(hm)
    m2 = L.vox_hip_memory_used()
    hm.set_kv_fp16(True)
    s16 = vox_hip.Stream(hm)
    hm.set_kv_fp16(False)
    s32b = vox_hip.Stream(hm)
    assert (s8.kv_dtype, s8.kv_fp16) == (vox_hip.KV_FP8, False)
    assert (s16.kv_dtype, s16.kv_fp16) == (vox_hip.KV_F16, True)
    assert (s32b.kv_dtype, s32b.kv_fp16) == (vox_hip.KV_F32, False)
    c = hm.cfg
    ring32 = 2 * c.dec_layers * (c.dec_window + 64) * c.dec_kv_heads * c.dec_head_dim * 4
    # everything but the rings is the same: the FP8 stream's rings are exactly a quarter
    assert (m1 - m0) - (m2 - m1) == ring32 - ring32 // 4, (m1 - m0, m2 - m1, ring32)
    with pytest.raises(RuntimeError):
        hm.set_kv_dtype(3)
    mel = run_mels("gemv2")[0]
    for s in (s8, s16, s32):
        s.encode_mel(mel[:800])
    b = vox_hip.Batch(hm, 4)
    for other in (s16, s32):
        with pytest.raises(RuntimeError, match="set_kv_dtype"):
            b.decode([s8, other], max_steps=1, stop_at_eos=False)
    # read_kv: nothing appended yet -> an error, as for positions already overwritten
    with pytest.raises(RuntimeError):
        s8.read_kv(0, 0, 1)
    # read_kv in the half mode: raw float16 rows of the positions a short decode appended
    s16.decode(max_steps=2, stop_at_eos=False)
    n = s16.state()["kv_pos"]
    k16, v16 = s16.read_kv(1, 0, n)
    assert k16.dtype == np.float16 and k16.shape == v16.shape == (n, c.dec_kv_heads * c.dec_head_dim)
    assert np.all(np.isfinite(k16)) and np.any(k16 != 0) and np.any(v16 != 0)
    b.close()
    for s in (s32, s8, s16, s32b):
        s.close()


# ---- single stream ---------------------------------------------------------------------------
def test_f32_ring_within_act_tol():
    """the unchanged f32 path: its ring rows over prefill + 300 steps are within ACT_TOL x max|row|
    of the oracle's K/V (the identity session: the oracle bit for bit) -- the window the FP8
    comparison rule allows a midpoint to sit in"""
    import vox_hip
    name = "long300"
    cfg_name, _, (steps,) = RUNS[name]
    hm, om, w = _models(cfg_name)
    mel = run_mels(name)[0]
    ids, lg, rg = _gpu_single(hm, vox_hip.KV_F32, mel, steps)
    r = RefDecoder(CFGS[cfg_name], w, oracle_adapter(om, mel), om.ada_scale())
    rids, rlg = r.decode(steps)
    assert ids == rids.tolist()
    worst = 0.0
    for l in range(CFGS[cfg_name].dec_layers):
        for ref, gpu in ((r.K[l][:r.pos], rg.K[l]), (r.V[l][:r.pos], rg.V[l])):
            assert gpu.shape == ref.shape
            worst = max(worst, float(np.max(np.max(np.abs(gpu - ref), axis=1) / np.max(np.abs(ref), axis=1))))
    print(f"f32 ring vs oracle K/V: worst |diff| / max|row| = {worst:.2e} (bar {ACT_TOL:.1e})")
    assert worst < ACT_TOL, worst


@pytest.mark.parametrize("name", ["long300", "wrap320", "tiny48"])
def test_kv8_single_stream_ring_conditioned(name):
    """long300: TINY_LONG, prefill (k_rope_kv, k_attn_mf) + 300 steps -- k_attn_short up to 256
    keys, then the split path with the merge.  wrap320: a 320-key window (ring of 384) over 450
    steps in calls of <= 64 -- the ring wraps with more than 256 keys in the split path.  tiny48:
    TINY's 48-key window (ring of 112): the wrap inside the one-block kernel."""
    import vox_hip
    cfg_name, _, (steps,) = RUNS[name]
    hm, _, _ = _models(cfg_name)
    mel = run_mels(name)[0]
    ids, lg, rg = _gpu_single(hm, vox_hip.KV_FP8, mel, steps)
    assert rg.n == 38 + steps                             # 38 prefill rows + one append per step
    if name != "long300":
        assert rg.n > CFGS[cfg_name].dec_window + 64       # past the ring's wrap
    _replay(cfg_name, mel, ids, list(lg), rg, f"kv8 {name}", f32_logits=_f32_oracle_logits(cfg_name, mel, steps))


# ---- batched ---------------------------------------------------------------------------------
def _batched(name, pre, gemv_rows=0, cap=None):
    """streams of RUNS[name] decoded by batched steps (stream k first takes pre[k] single-stream
    steps, so the batch's rows sit at different positions); every stream replayed on its own"""
    import vox_hip
    cfg_name, _, steps = RUNS[name]
    hm, _, _ = _models(cfg_name)
    mels = run_mels(name)
    ss = [_stream(hm, vox_hip.KV_FP8, mel) for mel in mels]
    rgs = [Rings(s) for s in ss]
    ids = [[] for _ in ss]
    lgs = [[] for _ in ss]
    for k, s in enumerate(ss):
        while len(ids[k]) < pre[k]:
            t, lg = s.decode(max_steps=min(MAX_CALL, pre[k] - len(ids[k])), stop_at_eos=False, want_logits=True)
            ids[k] += t.tolist()
            lgs[k] += list(lg)
            rgs[k].pull()
    b = vox_hip.Batch(hm, cap or max(4, len(ss)))
    if gemv_rows:
        assert b.set_gemv_rows(gemv_rows) == 0
    # batched steps: all but the last two in calls of <= MAX_CALL (graph replays), the last two one
    # by one for their logits; a stream leaves when it has its steps
    def live():
        return [k for k in range(len(ss)) if len(ids[k]) < steps[k]]
    while live():
        act = live()
        left = min(steps[k] - len(ids[k]) for k in act)
        n = 1 if left <= 2 else min(MAX_CALL, left - 2)
        for k, t in zip(act, b.decode([ss[k] for k in act], max_steps=n, stop_at_eos=False)):
            assert len(t) == n
            ids[k] += t.tolist()
            lgs[k] += [None] * (n - 1) + [b.read_logits(ss[k])]
            rgs[k].pull()
    if gemv_rows:
        assert b.gemv_stats()[1] > 0                        # GEMV step replays
    b.close()
    for k, s in enumerate(ss):
        s.close()
        rgs[k].done()
        assert len(ids[k]) == steps[k]
        _replay(cfg_name, mels[k], ids[k], lgs[k], rgs[k], f"kv8 {name} stream {k}")


def test_kv8_batch_three_streams():
    """the default batched step (RoPE + append fused into the attention) over three FP8 streams at
    different positions, one of them past 256 keys (the 128-key blocks and the merge)"""
    _batched("batch3", pre=[0, 230, 17])


def test_kv8_batch_17_streams_kv8_config():
    """32 query / 8 kv heads, 17 streams (the 32-slot bucket: two row blocks): the 1024-thread
    block per (slot, kv head) that shares the new key through LDS"""
    _batched("batch17", pre=[0] * 17, cap=32)


def test_kv8_batch_gemv_step():
    """the R-row GEMV step (k_gemvr: RoPE + append in the QKV epilogue, element type at run time)"""
    _batched("gemv2", pre=[0, 9], gemv_rows=2)
