"""Decode attention over FP8 KV rings on the matrix pipe (k_attn_decode_mf8).

The kernel against numpy float64 softmax attention over the decoded codes, at ACT_TOL = 5e-5 of
max |out| per row (the default kernel runs against the same reference, so the record shows both
distances); its FP8 -> bf16 convert on all 256 codes; the fused forms in the product under the
ring-conditioned replay of tests/test_gpu_kv8.py with the switch on; the mode change between
calls, the default and the refusal inside a begun call.  Fails without the feature:
vox_hip.attn_decode_kv8 and vox_hip.set_attn_mf8 do not exist."""
import ctypes

import numpy as np
import pytest

import test_gpu_kv8 as T
from kv8_ref import ACT_TOL, CFGS, FRAMES_PER_ROW, RUNS, c_kv8_decode, np_kv8_decode, np_kv8_encode, run_mels

pytestmark = pytest.mark.gpu

WINDOW, CAP = 1024, 1088


@pytest.fixture(autouse=True)
def _switch_off():
    import vox_hip
    yield
    vox_hip.set_attn_mf8(False)


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for hm, om, _ in T._M.values():
        hm.close()
        om.close()
    T._M.clear()


def _ref64(q, kc, vc, pos):
    """float64 softmax attention of each stream's last min(pos + 1, WINDOW) keys"""
    nb, H, hd = q.shape
    KVH = kc.shape[2]
    K, V = np_kv8_decode(kc).astype(np.float64), np_kv8_decode(vc).astype(np.float64)
    out = np.zeros(q.shape)
    for b in range(nb):
        L = min(pos[b] + 1, WINDOW)
        sl = np.arange(pos[b] - L + 1, pos[b] + 1) % CAP
        for h in range(H):
            kvh = h // (H // KVH)
            s = K[b, sl, kvh] @ q[b, h].astype(np.float64) / np.sqrt(hd)
            p = np.exp(s - s.max())
            out[b, h] = (p / p.sum()) @ V[b, sl, kvh]
    return out


@pytest.mark.parametrize("heads", [(4, 1), (6, 3)])
@pytest.mark.parametrize("pos", [(256,), (299,), (511,), (999,), (1024 + 37,), (1088 + 37,), (0, 39, 700)])
def test_kernel_against_float64(heads, pos):
    """contexts of 257 / 300 / 512 / 1000 keys, the full window before and after the ring's wrap (the
    wrap inside a tile), and one call of three streams at 1 / 40 / 701 keys (empty ranges and waves);
    a 4-head group and 2-head groups (rows 2..3 of the A operand stay zero)"""
    import vox_hip
    H, KVH = heads
    nb = len(pos)
    rng = np.random.default_rng(1000 * H + pos[0])
    q = rng.standard_normal((nb, H, 128)).astype(np.float32)
    kc = np_kv8_encode(rng.standard_normal((nb, CAP, KVH, 128)).astype(np.float32))
    vc = np_kv8_encode(rng.standard_normal((nb, CAP, KVH, 128)).astype(np.float32))
    ref = _ref64(q, kc, vc, pos)
    bar = ACT_TOL * np.max(np.abs(ref), axis=2, keepdims=True)
    d = [float(np.max(np.abs(vox_hip.attn_decode_kv8(q, kc, vc, pos, WINDOW, mode) - ref) / bar)) for mode in (0, 1)]
    print(f"H {H} KVH {KVH} pos {pos}: distance / bar: default kernel {d[0]:.4f}, mf8 {d[1]:.4f}")
    assert d[0] < 1.0 and d[1] < 1.0, d


def test_convert_all_codes():
    """every code through the kernel's FP8 -> bf16 convert is vox_kv8_decode's value, bit for bit; the
    two NaN codes are NaN"""
    import vox_hip
    bits = vox_hip.attn_mf8_codes()
    got = (bits.astype(np.uint32) << 16).view(np.float32)
    want = c_kv8_decode(np.arange(256, dtype=np.uint8))
    nan = np.isnan(want)
    assert nan.sum() == 2 and np.all(np.isnan(got[nan]))
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


# name -> (config, mels, steps per replayed stream, single-stream steps taken first, filler streams,
# kv_grow slots): batch3 is test_gpu_kv8's run (one stream past 256 keys); wrap3 is three streams on
# wrap320's mel (its margin holds on every step), one of them through the wrap of the 384-slot ring
FORMS = {
    "ptrs": ("batch3", RUNS["batch3"][2], [0, 230, 17], 0, 0),
    "ptrs_wrap": ("wrap320", [450, 120, 60], [150, 0, 40], 0, 0),
    "ptrs_rag": ("batch3", RUNS["batch3"][2], [0, 230, 17], 0, 256),
    "slots": ("batch3", RUNS["batch3"][2], [0, 230, 17], 30, 0),
    "slots_rag": ("batch3", RUNS["batch3"][2], [0, 230, 17], 30, 256),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_fused_forms_ring_conditioned(form):
    """the batched steps with the switch on: the GPU runs first, its stored codes are checked and
    adopted by the replay, logits at ACT_TOL, ids equal, top-2 margin >= MARGIN; the wide cases
    (33 slots) replay three streams, the others only fill slots for their first steps"""
    import vox_hip
    run, steps, pre, fill, grow = FORMS[form]
    cfg_name = RUNS[run][0]
    hm, _, _ = T._models(cfg_name)
    mels = run_mels(run)
    mels = mels if len(mels) == len(steps) else mels * len(steps)
    rng = np.random.default_rng(7)
    fmels = [rng.uniform(-0.6, 1.4, size=(FRAMES_PER_ROW * 52, CFGS[cfg_name].mel_bins)).astype(np.float32)
             for _ in range(fill)]
    hm.set_kv_grow(grow)
    try:
        ss = [T._stream(hm, vox_hip.KV_FP8, mel) for mel in mels + fmels]
    finally:
        hm.set_kv_grow(0)
    n = len(steps)
    want = list(steps) + [8] * fill
    rgs = [T.Rings(s) for s in ss[:n]]
    ids, lgs = [[] for _ in ss], [[] for _ in ss]
    for k in range(n):
        while len(ids[k]) < pre[k]:
            t, lg = ss[k].decode(max_steps=min(T.MAX_CALL, pre[k] - len(ids[k])), stop_at_eos=False, want_logits=True)
            ids[k] += t.tolist()
            lgs[k] += list(lg)
            rgs[k].pull()
    vox_hip.set_attn_mf8(True)
    before = vox_hip.attn_mf8_stats()
    b = vox_hip.Batch(hm, 64 if fill else 4)
    while True:
        act = [k for k in range(len(ss)) if len(ids[k]) < want[k]]
        if not act:
            break
        left = min(want[k] - len(ids[k]) for k in act)
        m = 1 if left <= 2 else min(T.MAX_CALL, left - 2)
        for k, t in zip(act, b.decode([ss[k] for k in act], max_steps=m, stop_at_eos=False)):
            assert len(t) == m
            ids[k] += t.tolist()
            if k < n:
                lgs[k] += [None] * (m - 1) + [b.read_logits(ss[k])]
                rgs[k].pull()
    after = vox_hip.attn_mf8_stats()
    b.close()
    key = form.replace("_wrap", "")
    assert after[key] > before[key], (form, before, after)
    for k, s in enumerate(ss):
        s.close()
    for k in range(n):
        rgs[k].done()
        T._replay(cfg_name, mels[k], ids[k], lgs[k], rgs[k], f"mf8 {form} stream {k}")


def test_mode_change_default_and_refusal():
    """nothing set: the mode is 0 and no count moves over a batched run past 256 keys; off -> on -> off
    between calls on live streams moves the counts only while on, and a second call in the same mode
    captures no graph; inside a begun call the setter is refused"""
    import vox_hip
    hm, _, _ = T._models("TINY_LONG")
    mels = run_mels("batch3")[1:]                       # 290 and 100 steps of adapter rows
    ss = [T._stream(hm, vox_hip.KV_FP8, mel) for mel in mels]
    assert vox_hip.attn_mf8() == 0
    zero = vox_hip.attn_mf8_stats()
    ss[0].decode(max_steps=230, stop_at_eos=False)      # 268 keys: every later step is past 256
    b = vox_hip.Batch(hm, 4)

    def call():
        c0, s0 = b.stats()["captures"], vox_hip.attn_mf8_stats()["ptrs"]
        assert all(len(t) == 3 for t in b.decode(ss, max_steps=3, stop_at_eos=False))
        return b.stats()["captures"] - c0, vox_hip.attn_mf8_stats()["ptrs"] - s0

    assert call()[1] == 0 and vox_hip.attn_mf8_stats() == zero
    vox_hip.set_attn_mf8(True)
    cap, n = call()
    assert cap == 1 and n == ss[0].cfg.dec_layers
    assert call() == (0, 0)                              # same mode: a replay, nothing captured
    vox_hip.set_attn_mf8(False)
    assert call() == (1, 0)
    assert call() == (0, 0)
    # a begun call: the setter is refused, the mode stays
    L = vox_hip.lib()
    IP = ctypes.POINTER(ctypes.c_int)
    arr = (ctypes.c_void_p * 2)(*[s.h for s in ss])
    rows = np.array([s.adapter_tokens for s in ss], np.int32)
    toks, cnt = np.zeros((2, 2), np.int32), np.zeros(2, np.int32)
    assert L.vox_hip_batch_begin_rows(b.h, arr, 2, rows.ctypes.data_as(IP), 2, 0, toks.ctypes.data_as(IP),
                                      cnt.ctypes.data_as(IP)) == 0, L.vox_hip_last_error()
    with pytest.raises(RuntimeError, match="begun"):
        vox_hip.set_attn_mf8(True)
    assert L.vox_hip_batch_finish(b.h) >= 0
    assert vox_hip.attn_mf8() == 0
    vox_hip.set_attn_mf8(True)
    vox_hip.set_attn_mf8(False)
    b.close()
    for s in ss:
        s.close()
