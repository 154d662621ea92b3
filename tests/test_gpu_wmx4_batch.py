"""GPU: opt-in MXFP4 fragment planes for the batched MFMA decode step (csrc/vox_wmx4.h's fragment
plane, the WF_MX4 instances of k_skl / k_skl2 / k_sklx / k_skf).

The mx4 instances form, in registers, the very bf16 A fragments the bf16 instances load, with the
same waves, splits, slabs and summation order, so the step on the bf16 fragment copies is the
bit-exact twin, and the unchanged CPU oracle on the rounded weights the exact reference.

Entry tests (vox_hip.skinny_wmx4, the step's own launchers on one matrix): fmt 1 (mx4 plane) is
array_equal to fmt 0 (bf16 fragments) as uint32, and both are within 5e-5 of max|y| of a float64
product, for the four projection shapes of KV8, MID and WIDE (tests/test_gpu_batch_kv8.py's
configs: ks = 4, 6 and 8, 4- and 8-wave blocks) and three LM-head shapes, at 1, 5, 16, 17 and 32
rows; an unrounded matrix is refused.

Step tests.  The modes are read at model creation, so each decodes in a fresh child process:
  on     VOX_HIP_WMX4=1 VOX_HIP_WMX4_BATCH=1 on quantize_mxfp4 weights: Batch.decode of 3, 16, 17
         and 32 streams with set_wmx4(1) and again with set_wmx4(0) -- array_equal ids, logits and
         alternatives (KV8, and WIDE at 17 streams for the 8-wave variants); a mode change between
         two calls; the oracle's ids and logits (KV8 with 3 and 17 streams, fp16 rings, MID); a
         model with one spoiled tensor;
  round  VOX_HIP_WMX4=2 VOX_HIP_WMX4_BATCH=1 on the unrounded weights: the bits of `on`; a Q8
         model builds no planes;
  off    VOX_HIP_WMX4=2 alone: no planes, set_wmx4(1) fails, the bits of set_wmx4(0).
tests/test_wmx4_frag_cpu.py asserts on the oracle alone that every run in ORACLE_RUNS keeps the
top-2 margin on every compared step, so an id comparison means something."""
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
STEPS = 6            # decode steps compared per stream (single-step calls, logits read after each)

KV8 = replace(TINY, dec_heads=32, dec_kv_heads=8, dec_dim=768, dec_hidden=1280)
MID = replace(KV8, dec_dim=1536, dec_hidden=3072)
WIDE = replace(KV8, dec_dim=2048, dec_hidden=6144)
CONFIGS = {"kv8": KV8, "mid": MID, "wide": WIDE}
SPOILED = "layers.0.feed_forward.w2.weight"   # the tensor the `spoiled` weights make unrepresentable

# oracle run -> (config name, weights, streams, fp16 rings, mel seed).  The seed is the first of
# 1, 2, ... at which the oracle on these weights passes the margin rule on every step of every
# stream (scanned on the CPU; tests/test_wmx4_frag_cpu.py asserts it)
ORACLE_RUNS = {
    "kv8": ("kv8", "rounded", 17, False, 1),
    "kv8_kv16": ("kv8", "rounded", 17, True, 1),
    "mid": ("mid", "rounded", 17, False, 1),
    "kv8_spoiled": ("kv8", "spoiled", 3, False, 1),
}
TWIN_STREAMS = (3, 16, 17, 32)
TWIN_SEED = ORACLE_RUNS["kv8"][4]   # the twin runs of 3 and 17 streams are the ones compared with the oracle
# slots whose logits are read after every step
SLOTS = {3: (0, 2), 16: (0, 15), 17: (0, 16), 32: (0, 15, 16, 31)}
ALT_SLOT = 1         # the stream of every batch that has alternatives on


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))


def _mels(cname, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-0.6, 1.4, size=(400 + 8 * (i % 7), CONFIGS[cname].mel_bins)).astype(np.float32) for i in range(n)]


_W = {}
_ORACLE = {}


def _weights(cname, kind):
    """synth_weights(cfg, seed=1) (`plain`), its quantize_mxfp4 rounding (`rounded`), that with one
    weight of SPOILED moved off the MXFP4 grid (`spoiled`), or quantize_q8 (`q8`)"""
    from vox_weights import Weights, quantize_mxfp4, quantize_q8, synth_weights
    key = (cname, kind)
    if key in _W:
        return _W[key]
    if kind == "plain":
        w = synth_weights(CONFIGS[cname], seed=1)
    elif kind == "rounded":
        w = quantize_mxfp4(_weights(cname, "plain"))
    elif kind == "q8":
        w = quantize_q8(_weights(cname, "plain"))
    else:
        base = _weights(cname, "rounded")
        t = dict(base.t)
        a = t[SPOILED].copy()
        r, k = np.argwhere((a & 0x7fff) != 0)[0]
        a[r, k] ^= 1          # the mantissa's last bit: no e2m1 value has it
        t[SPOILED] = a
        w = Weights(base.cfg, t, keep=base._keep)
    _W[key] = w
    return w


def _oracle(run, seed=None):
    """[(ids, logits [STEPS, vocab])] per stream: the CPU oracle on the run's weights"""
    import vox_oracle
    cname, kind, n, kv16, s0 = ORACLE_RUNS[run]
    seed = s0 if seed is None else seed
    if (run, seed) in _ORACLE:
        return _ORACLE[run, seed]
    om = vox_oracle.OracleModel(CONFIGS[cname], _weights(cname, kind))
    vox_oracle.set_kv_fp16(kv16)
    out = []
    try:
        vox_oracle.set_threads(min(4, os.cpu_count() or 1))
        for mel in _mels(cname, n, seed):
            st = vox_oracle.OracleStream(om)
            st.encode_mel(mel)
            ids, lg = st.decode(max_steps=STEPS, stop_at_eos=False, want_logits=True)
            st.close()
            lg = np.asarray(lg)
            lg.setflags(write=False)
            out.append((np.asarray(ids).tolist(), lg))
    finally:
        vox_oracle.set_kv_fp16(False)
        vox_oracle.set_threads(1)
    om.close()
    _ORACLE[run, seed] = out
    return out


# ---- MXFP4-valued test matrices (shared with tests/test_wmx4_frag_cpu.py) -----------------------
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def mx4_matrix(N, K, seed):
    """bf16 bits [N, K] of a random MXFP4-valued matrix, built from codes and block exponents:
    even rows draw every block's exponent from -64..64 (the whole window, both ends present), odd
    rows from -10..-2; one block in 8 is all zero (of both signs), one in 8 has a single nonzero
    weight; the others hold random codes with one weight of magnitude 4 or 6, which makes the
    block's rule exponent the drawn one."""
    rng = np.random.default_rng(seed)
    nb = K // 32
    code = rng.integers(0, 16, size=(N, nb, 32))
    kind = rng.integers(0, 8, size=(N, nb))
    kind[0, :2] = 2                                             # the blocks that take the window's two ends
    code[kind <= 1] &= 8                                        # zeros, signs kept
    pos = rng.integers(0, 32, size=(N, nb))
    top = rng.integers(6, 8, size=(N, nb)) | (rng.integers(0, 2, size=(N, nb)) << 3)
    ii, jj = np.nonzero(kind >= 1)                              # kind 1: the single nonzero weight
    code[ii, jj, pos[ii, jj]] = top[ii, jj]
    e = rng.integers(-64, 65, size=(N, nb))
    e[1::2] = rng.integers(-10, -1, size=e[1::2].shape)
    e[0, :2] = (-64, 64)
    v = np.where(code & 8, -1.0, 1.0) * E2M1[code & 7] * np.exp2(e.astype(np.float64))[:, :, None]
    bits = (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).reshape(N, K)
    return bits


def bf16_f64(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# ---- the children ---------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2])
sys.path.insert(0, sys.argv[3])
import vox_hip
import test_gpu_wmx4_batch as t

out_path, job = sys.argv[1], sys.argv[4]
out = {"mode": np.array([vox_hip.wmx4(), vox_hip.wmx4_batch()])}


def stats(model, key):
    s = model.wmx4_batch_stats()
    out[key + "_stats"] = np.array([s["tensors"], s["plane_bytes"], s["bf16_bytes"]], np.int64)


def run(model, cname, n, seed, modes, key, kv16=False):
    # STEPS single-step calls of one Batch over n fresh streams; modes[k]: set_wmx4 before step k
    # (None: leave it); stream ALT_SLOT has alternatives on
    model.set_kv_fp16(kv16)
    ss = [vox_hip.Stream(model) for _ in range(n)]
    model.set_kv_fp16(False)
    for s, mel in zip(ss, t._mels(cname, n, seed)):
        assert s.kv_fp16 == kv16
        s.encode_mel(mel)
    ss[t.ALT_SLOT].set_alt(3, 1.0)
    b = vox_hip.Batch(model, n)
    got = [[] for _ in ss]
    lg = {i: [] for i in t.SLOTS[n]}
    for k in range(t.STEPS):
        if modes[k] is not None:
            assert b.set_wmx4(modes[k]) == 0, k
        for i, ids in enumerate(b.decode(ss, max_steps=1, stop_at_eos=False)):
            assert len(ids) == 1, (k, i)
            got[i] += ids.tolist()
        for i in lg:
            lg[i].append(b.read_logits(ss[i]))
    out[key + "_ids"] = np.array(got)
    for i, v in lg.items():
        out["%s_lg%d" % (key, i)] = np.stack(v)
    aid, apr = ss[t.ALT_SLOT].read_alts(0, t.STEPS)
    out[key + "_alt_ids"], out[key + "_alt_p"] = np.asarray(aid), np.asarray(apr)
    b.close()
    for s in ss:
        s.close()


ON, OFF = [1] + [None] * (t.STEPS - 1), [0] + [None] * (t.STEPS - 1)
LEAVE = [None] * t.STEPS
if job == "on":
    m = vox_hip.Model(t.KV8, t._weights("kv8", "rounded"))
    stats(m, "kv8")
    b = vox_hip.Batch(m, 3)
    out["starts_on"] = np.array(b.set_wmx4(1) == 0)
    b.close()
    for n in t.TWIN_STREAMS:
        run(m, "kv8", n, t.TWIN_SEED, LEAVE if n == 3 else ON, "on%d" % n)     # a new batch starts with it on
        run(m, "kv8", n, t.TWIN_SEED, OFF, "off%d" % n)
    half = t.STEPS // 2
    run(m, "kv8", 17, t.TWIN_SEED, [1] + [None] * (half - 1) + [0] + [None] * (t.STEPS - half - 1), "switch17")
    run(m, "kv8", 17, t.ORACLE_RUNS["kv8_kv16"][4], ON, "kv16_17", kv16=True)
    m.close()
    m = vox_hip.Model(t.MID, t._weights("mid", "rounded"))
    stats(m, "mid")
    run(m, "mid", 17, t.ORACLE_RUNS["mid"][4], ON, "mid17")
    m.close()
    # WIDE: the 8-wave variants the full-size widths select (k_sklx<8, 8>, k_skl2<., 8, 8>), twin only
    m = vox_hip.Model(t.WIDE, t._weights("wide", "rounded"))
    stats(m, "wide")
    run(m, "wide", 17, t.TWIN_SEED, ON, "wide_on17")
    run(m, "wide", 17, t.TWIN_SEED, OFF, "wide_off17")
    m.close()
    m = vox_hip.Model(t.KV8, t._weights("kv8", "spoiled"))
    stats(m, "spoiled")
    run(m, "kv8", 3, t.ORACLE_RUNS["kv8_spoiled"][4], ON, "spoiled3")
    m.close()
elif job == "round":
    m = vox_hip.Model(t.KV8, t._weights("kv8", "plain"))
    stats(m, "kv8")
    run(m, "kv8", 17, t.TWIN_SEED, LEAVE, "on17")
    m.close()
    m = vox_hip.Model(t.KV8, t._weights("kv8", "q8"))
    stats(m, "q8")
    b = vox_hip.Batch(m, 2)
    out["q8_set"] = np.array(b.set_wmx4(1))
    b.close()
    m.close()
else:
    m = vox_hip.Model(t.KV8, t._weights("kv8", "plain"))
    stats(m, "kv8")
    b = vox_hip.Batch(m, 2)
    out["set_on"] = np.array(b.set_wmx4(1))
    out["set_off"] = np.array(b.set_wmx4(0))
    b.close()
    run(m, "kv8", 17, t.TWIN_SEED, LEAVE, "off17")
    m.close()
np.savez(out_path, **out)
"""


def _child(tmp, job, wmx4, batch):
    path = os.path.join(tmp, job + ".npz")
    env = dict(os.environ, VOX_HIP_WMX4=str(wmx4))
    for k in ("VOX_HIP_WMX4_BATCH", "VOX_HIP_WPACK", "VOX_HIP_BATCH_GEMV"):
        env.pop(k, None)
    if batch:
        env["VOX_HIP_WMX4_BATCH"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD, path, os.path.join(ROOT, "voxtral.c_amd"),
                        os.path.join(ROOT, "tests"), job], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(path))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("wmx4_batch"))


@pytest.fixture(scope="module")
def on(tmp):
    return _child(tmp, "on", 1, True)


@pytest.fixture(scope="module")
def rounding(tmp):
    return _child(tmp, "round", 2, True)


@pytest.fixture(scope="module")
def off(tmp):
    return _child(tmp, "off", 2, False)


# ---- the test entry: the mx4 instances against their bf16 twins and float64 ----------------------
def _proj_shapes(c):
    dq, dkv = c.dec_heads * c.dec_head_dim, c.dec_kv_heads * c.dec_head_dim
    return [(dq + 2 * dkv, c.dec_dim), (c.dec_dim, dq), (2 * c.dec_hidden, c.dec_dim), (c.dec_dim, c.dec_hidden)]


ENTRY = sorted({(N, K, 0) for c in (KV8, MID, WIDE) for N, K in _proj_shapes(c)}) + \
    [(4096, 768, 1), (4096, 1536, 1), (4096, 2048, 1)]
ENTRY_ROWS = (1, 5, 16, 17, 32)


def _x(nb, K, seed):
    """rows of magnitudes over 2^-20 .. 2^20"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nb, K)) * np.exp2(rng.integers(-20, 21, size=(nb, K)))
    return x.astype(np.float32)


@pytest.mark.parametrize("N,K,head", ENTRY)
def test_entry_bits(N, K, head):
    import vox_hip
    W = mx4_matrix(N, K, seed=N + K + head)
    Wf = bf16_f64(W)
    for nb in ENTRY_ROWS:
        x = _x(nb, K, seed=K + nb)
        y0 = vox_hip.skinny_wmx4(W, x, fmt=0, head=bool(head))
        y1 = vox_hip.skinny_wmx4(W, x, fmt=1, head=bool(head))
        ref = x.astype(np.float64) @ Wf.T
        e0 = float(np.max(np.abs(y0 - ref)) / np.max(np.abs(ref)))
        e1 = float(np.max(np.abs(y1 - ref)) / np.max(np.abs(ref)))
        print(f"skinny_wmx4 ({N}, {K}) head={head} nb={nb}: err bf16 {e0:.2e} mx4 {e1:.2e} of max|y| (bar {LOGIT_TOL:.0e}), "
              f"{int((y0.view(np.uint32) != y1.view(np.uint32)).sum())} words differ")
        assert np.array_equal(y1.view(np.uint32), y0.view(np.uint32)), nb
        assert e0 < LOGIT_TOL and e1 < LOGIT_TOL, nb


def test_entry_refusal():
    import ctypes
    import vox_hip
    from vox_weights import synth_lib
    W = np.zeros((768, 1280), np.uint16)
    synth_lib().vox_synth_bf16(ctypes.c_void_p(W.ctypes.data), ctypes.c_size_t(W.size), ctypes.c_uint64(5),
                               ctypes.c_float(0.03), ctypes.c_float(0.0))
    x = _x(5, 1280, seed=5)
    with pytest.raises(RuntimeError, match="MXFP4"):
        vox_hip.skinny_wmx4(W, x, fmt=1)
    y0 = vox_hip.skinny_wmx4(W, x, fmt=0)
    ref = x.astype(np.float64) @ bf16_f64(W).T
    assert float(np.max(np.abs(y0 - ref)) / np.max(np.abs(ref))) < LOGIT_TOL


# ---- the step -----------------------------------------------------------------------------------
def _same(a, b, keys):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _keys(tag, n):
    return [tag + "_ids", tag + "_alt_ids", tag + "_alt_p"] + ["%s_lg%d" % (tag, i) for i in SLOTS[n]]


@pytest.mark.parametrize("n", TWIN_STREAMS)
def test_step_is_its_twin(on, n):
    assert on["mode"].tolist() == [1, 1] and bool(on["starts_on"])
    a, b = {k: on[k] for k in _keys("on%d" % n, n)}, {k.replace("off", "on", 1): on[k] for k in _keys("off%d" % n, n)}
    assert a["on%d_ids" % n].shape == (n, STEPS)
    _same(a, b, sorted(a))


def test_step_is_its_twin_wide(on):
    """WIDE (tests/test_gpu_batch_kv8.py): k_sklx<8, 8, SCALE, SWIGLU, MX4> and k_skl2<MX4, 8, 8>, the variants
    the full-size W1|W3, wo and W2 take"""
    a, b = {k: on[k] for k in _keys("wide_on17", 17)}, {k.replace("_off", "_on", 1): on[k] for k in _keys("wide_off17", 17)}
    assert a["wide_on17_ids"].shape == (17, STEPS) and on["wide_stats"][0] == 4 * WIDE.dec_layers + 1
    _same(a, b, sorted(a))


def test_mode_change_between_calls(on):
    got = {k.replace("switch", "on", 1): on[k] for k in _keys("switch17", 17)}
    _same(got, on, sorted(got))


def _against_oracle(res, tag, run, n, slots):
    cname, _, _, kv16, _ = ORACLE_RUNS[run]
    ref = _oracle(run)
    tol = LOGIT_TOL16 if kv16 else LOGIT_TOL
    ids = res[tag + "_ids"]
    for i in range(n):
        assert ids[i].tolist() == ref[i][0], (tag, i)
    worst = max(rel(res["%s_lg%d" % (tag, i)][k], ref[i][1][k]) for i in slots for k in range(STEPS))
    print(f"{tag}: {n} streams x {STEPS} ids equal the oracle's on the rounded weights, worst logit err {worst:.2e} (bar {tol:.0e})")
    assert worst < tol
    assert res[tag + "_alt_ids"][:, 0].tolist() == ids[ALT_SLOT].tolist()


@pytest.mark.parametrize("tag,run,n", [("on3", "kv8", 3), ("on17", "kv8", 17), ("kv16_17", "kv8_kv16", 17), ("mid17", "mid", 17)])
def test_step_is_the_oracle(on, tag, run, n):
    _against_oracle(on, tag, run, n, SLOTS[n])


def test_round_mode(on, rounding):
    assert rounding["mode"].tolist() == [2, 1]
    _same(rounding, on, _keys("on17", 17))
    assert np.array_equal(rounding["kv8_stats"], on["kv8_stats"])


def test_off_is_off(on, rounding, off):
    assert off["mode"].tolist() == [2, 0]
    assert not off["kv8_stats"].any()
    assert int(off["set_on"]) == -1 and int(off["set_off"]) == 0
    _same(off, on, _keys("off17", 17))
    # a Q8 model with both variables set builds no planes
    assert not rounding["q8_stats"].any() and int(rounding["q8_set"]) == -1


def _frag_words(N, K):
    return N // 16 * (K // 64) * 144


def test_stats(on):
    for cname in ("kv8", "mid"):
        c = CONFIGS[cname]
        shapes = _proj_shapes(c) * c.dec_layers + [(c.vocab, c.dec_dim)]
        n, pbytes, bbytes = on[cname + "_stats"]
        assert n == 4 * c.dec_layers + 1 == len(shapes)
        assert pbytes == sum(_frag_words(N, K) * 4 for N, K in shapes)
        assert bbytes == sum(N * K * 2 for N, K in shapes)
        assert pbytes * 8 / (bbytes / 2) == 4.5
    # one tensor spoiled with a single unrepresentable weight: not planed, decoded from its bf16 copy
    c = KV8
    shapes = _proj_shapes(c) * c.dec_layers + [(c.vocab, c.dec_dim)]
    shapes.remove((c.dec_dim, c.dec_hidden))
    n, pbytes, bbytes = on["spoiled_stats"]
    assert n == 4 * c.dec_layers and pbytes == sum(_frag_words(N, K) * 4 for N, K in shapes)
    _against_oracle(on, "spoiled3", "kv8_spoiled", 3, SLOTS[3])
