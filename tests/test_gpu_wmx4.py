"""GPU: opt-in MXFP4 weight streaming for the single-stream decode GEMVs (wmx4: csrc/vox_wmx4.h,
k_gemv's WF_MX4 instances).

An MXFP4-valued model is a bf16 model, so the unchanged CPU oracle on the rounded weights is the
exact reference of the wmx4 step, and the raw-bf16 kernel on the same weights its bit-exact twin.

Entry tests: on rounded random matrices the wmx4, wpack13 and raw instances of k_gemv give
array_equal outputs, within 5e-5 of max|y| of a float64 product; an unrounded matrix is refused.

Step tests, on configs the oracle follows in seconds (tests/test_gpu_batch_gemv.py's KV8: dec_dim
768, hidden 1280, 32/8 heads, vocab 4096; G95: hidden 9216).  VOX_HIP_WMX4 is read at model
creation, so each mode decodes in a fresh child process:
  detect  VOX_HIP_WMX4=1 on quantize_mxfp4 weights: ids = the oracle's, logits within 5e-5 (1e-4
          with fp16 rings), also with set_alt on (LOGITS_ALT);
  raw     the same with VOX_HIP_WPACK=0: array_equal ids and logits;
  round   VOX_HIP_WMX4=2 on the unrounded weights: the bits of detect mode, and a 3-stream
          Batch.decode with the oracle's ids (prefill and the batched step read the rounded values).
tests/test_wmx4_cpu.py asserts on the oracle alone that every run in ORACLE_RUNS keeps the top-2
margin on every compared step, so an id comparison means something."""
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
STEPS = 10           # decode steps compared per stream

KV8 = replace(TINY, dec_heads=32, dec_kv_heads=8, dec_dim=768, dec_hidden=1280)
G95 = replace(KV8, dec_hidden=9216)
CONFIGS = {"kv8": KV8, "g95": G95}
# config name -> (mel sizes, mel seed): the first seeds tried (1, 2, ...) at which the oracle on
# the rounded weights passes the margin rule on every step of every run below
MELS = {"kv8": ([400, 424, 448], 1), "g95": ([400], 1)}
# oracle run -> (config name, fp16 rings); f32 runs follow every stream of MELS, fp16 stream 0
ORACLE_RUNS = {"kv8": ("kv8", False), "kv8_kv16": ("kv8", True), "g95": ("g95", False)}
# single-stream scenarios of a child: name -> (config name, n_alt, fp16 rings, oracle run)
SCENARIOS = {"kv8": ("kv8", 1, False, "kv8"), "kv8_alt": ("kv8", 3, False, "kv8"),
             "kv8_kv16": ("kv8", 1, True, "kv8_kv16"), "g95": ("g95", 1, False, "g95")}


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))


def _mels(cname):
    sizes, seed = MELS[cname]
    rng = np.random.default_rng(seed)
    return [rng.uniform(-0.6, 1.4, size=(n, CONFIGS[cname].mel_bins)).astype(np.float32) for n in sizes]


_W = {}
_ORACLE = {}


def _weights(cname, rounded):
    """synth_weights(cfg, seed=1), and its quantize_mxfp4 rounding"""
    from vox_weights import quantize_mxfp4, synth_weights
    if (cname, rounded) not in _W:
        _W[cname, rounded] = quantize_mxfp4(_weights(cname, False)) if rounded else synth_weights(CONFIGS[cname], seed=1)
    return _W[cname, rounded]


def _oracle(run):
    """[(ids, logits [STEPS, vocab])] per stream: the CPU oracle on the rounded weights"""
    import vox_oracle
    if run in _ORACLE:
        return _ORACLE[run]
    cname, kv16 = ORACLE_RUNS[run]
    om = vox_oracle.OracleModel(CONFIGS[cname], _weights(cname, True))
    vox_oracle.set_kv_fp16(kv16)
    out = []
    try:
        vox_oracle.set_threads(min(4, os.cpu_count() or 1))
        for mel in _mels(cname)[:1 if kv16 else None]:
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
    _ORACLE[run] = out
    return out


# ---- the child: one process per (VOX_HIP_WMX4, VOX_HIP_WPACK, weights) --------------------------
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2])
sys.path.insert(0, sys.argv[3])
import vox_hip
import test_gpu_wmx4 as t

out_path, rounded, scenarios, batch, extra = sys.argv[1], sys.argv[4] == "rounded", sys.argv[5], sys.argv[6], sys.argv[7]
out = {"mode": np.array(vox_hip.wmx4())}
STAT = ("wmx4_tensors", "refused_tensors", "plane_bytes", "bf16_bytes")


def stats(model, key):
    s = model.wmx4_stats()
    out[key + "_wmx4"] = np.array([s[k] for k in STAT], np.int64)
    out[key + "_bits"] = np.array(s["bits_per_weight"])
    out[key + "_ms"] = np.array([s["scan_ms"], s["round_ms"], s["pack_ms"]])
    p = model.wpack_stats()
    out[key + "_wpack"] = np.array([p[k] for k in ("packed_tensors", "raw_tensors", "packed_bytes",
                                                   "packed_raw_bytes", "raw_bytes")], np.int64)


models = {}
for name in [s for s in scenarios.split(",") if s]:
    cname, n_alt, kv16, _ = t.SCENARIOS[name]
    if cname not in models:
        models[cname] = vox_hip.Model(t.CONFIGS[cname], t._weights(cname, rounded))
        stats(models[cname], cname)
    model = models[cname]
    model.set_kv_fp16(kv16)
    st = vox_hip.Stream(model)
    model.set_kv_fp16(False)
    assert st.kv_fp16 == kv16
    st.encode_mel(t._mels(cname)[0])
    if n_alt > 1:
        st.set_alt(n_alt, 1.0)
    toks, logits = st.decode(max_steps=t.STEPS, stop_at_eos=False, want_logits=True)
    out[name + "_tokens"], out[name + "_logits"] = np.asarray(toks), np.asarray(logits)
    if n_alt > 1:
        ids, pr = st.read_alts(0, len(toks))
        out[name + "_alt_ids"], out[name + "_alt_p"] = np.asarray(ids), np.asarray(pr)
    st.close()
if batch:
    model = models[batch]
    ss = [vox_hip.Stream(model) for _ in t._mels(batch)]
    for s, mel in zip(ss, t._mels(batch)):
        s.encode_mel(mel)
    b = vox_hip.Batch(model, len(ss))
    for i, ids in enumerate(b.decode(ss, max_steps=t.STEPS, stop_at_eos=False)):
        out["batch_%d" % i] = np.asarray(ids)
    b.close()
    for s in ss:
        s.close()
for m in models.values():
    m.close()
if extra:
    # ordinary synthetic weights in this process's mode, then in mode 0
    m = vox_hip.Model(t.KV8, t._weights("kv8", False))
    stats(m, "plain")
    m.close()
    vox_hip.set_wmx4(0)
    assert vox_hip.wmx4() == 0
    m = vox_hip.Model(t.KV8, t._weights("kv8", False))
    stats(m, "plain_off")
    m.close()
    m = vox_hip.Model(t.KV8, t._weights("kv8", True))
    stats(m, "rounded_off")
    m.close()
np.savez(out_path, **out)
"""


def _child(tmp, tag, wmx4, wpack, rounded, scenarios, batch="", extra=False):
    path = os.path.join(tmp, tag + ".npz")
    env = dict(os.environ, VOX_HIP_WMX4=str(wmx4))
    env.pop("VOX_HIP_WPACK", None)
    if wpack is not None:
        env["VOX_HIP_WPACK"] = str(wpack)
    r = subprocess.run([sys.executable, "-c", CHILD, path, os.path.join(ROOT, "voxtral.c_amd"),
                        os.path.join(ROOT, "tests"), "rounded" if rounded else "plain", ",".join(scenarios), batch,
                        "1" if extra else ""], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(path))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("wmx4"))


@pytest.fixture(scope="module")
def detect(tmp):
    return _child(tmp, "detect", 1, None, True, sorted(SCENARIOS), extra=True)


@pytest.fixture(scope="module")
def raw(tmp):
    return _child(tmp, "raw", 1, 0, True, sorted(SCENARIOS))


@pytest.fixture(scope="module")
def rounding(tmp):
    return _child(tmp, "round", 2, None, False, ["kv8"], batch="kv8")


# ---- the test entry: the WF_MX4 STORE instance against its twins and float64 -------------------
# (rows, K): one partial K round; second round half full; two full rounds; five rounds; many
# groups per block (the early loads and the zero-length-descriptor tail run)
ENTRY_SHAPES = [(512, 768), (256, 3072), (256, 4096), (128, 9216), (4096, 768)]


def _w(rows, K, seed):
    import ctypes
    from vox_weights import synth_lib
    out = np.zeros((rows, K), np.uint16)
    synth_lib().vox_synth_bf16(ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(out.size), ctypes.c_uint64(seed),
                               ctypes.c_float(1.0 / np.sqrt(K)), ctypes.c_float(0.0))
    return out


@pytest.mark.parametrize("rows,K", ENTRY_SHAPES)
def test_entry_bits(rows, K):
    import vox_hip
    from vox_weights import mxfp4_round
    W = _w(rows, K, seed=rows + K)
    W[1, ::7] = 0x8000   # signed zeros
    W[2, ::5] = 0
    W[3, 32:96] = 0      # all-zero blocks
    W[5] = (W[5].astype(np.uint32) + (9 << 7)).astype(np.uint16)   # a row 2^9 larger: other scale bytes
    W = mxfp4_round(W)
    x = np.random.default_rng(K).standard_normal(K).astype(np.float32)
    y2, p2 = vox_hip.gemv_wpack(W, x, packed=2)
    y1, p1 = vox_hip.gemv_wpack(W, x, packed=1)
    y0, p0 = vox_hip.gemv_wpack(W, x, packed=0)
    assert (p2, p1, p0) == (2, True, False)
    assert np.array_equal(y2.view(np.uint32), y0.view(np.uint32))
    assert np.array_equal(y1.view(np.uint32), y0.view(np.uint32))
    Wf = (W.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    ref = Wf @ x.astype(np.float64)
    err = float(np.max(np.abs(y2 - ref)) / np.max(np.abs(ref)))
    print(f"gemv_wpack packed=2 ({rows}, {K}): err {err:.2e} of max|y| (bar {LOGIT_TOL:.0e})")
    assert err < LOGIT_TOL


def test_entry_refusal():
    import vox_hip
    W = _w(512, 768, seed=5)
    x = np.random.default_rng(5).standard_normal(768).astype(np.float32)
    y2, p2 = vox_hip.gemv_wpack(W, x, packed=2)
    y0, p0 = vox_hip.gemv_wpack(W, x, packed=0)
    assert (p2, p0) == (0, False)
    assert np.array_equal(y2.view(np.uint32), y0.view(np.uint32))


# ---- the step -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_step_detect(detect, raw, name):
    _, n_alt, kv16, run = SCENARIOS[name]
    assert int(detect["mode"]) == 1 and int(raw["mode"]) == 1
    ids, lg = _oracle(run)[0]
    tol = LOGIT_TOL16 if kv16 else LOGIT_TOL
    got, glg = detect[name + "_tokens"], detect[name + "_logits"]
    assert got.tolist() == ids
    worst = max(rel(glg[k], lg[k]) for k in range(STEPS))
    print(f"{name}: {len(ids)} ids equal the oracle's on the rounded weights, worst logit err {worst:.2e} (bar {tol:.0e})")
    assert worst < tol
    # the raw-bf16 kernels on the same weights: the same bits
    keys = [name + s for s in ("_tokens", "_logits") + (("_alt_ids",) if n_alt > 1 else ())]
    for k in keys:
        assert detect[k].dtype == raw[k].dtype and detect[k].tobytes() == raw[k].tobytes(), k
    if n_alt > 1:
        # The alternatives' probabilities are exp(l - max) / S with S summed per block and then
        # over blocks.  At vocab 4096 the wmx4 LM head runs 4-row groups where bf16 runs 2-row
        # groups (at 65536 rows and more both run 8), so S is the same n = 4096 positive terms
        # added in another grouping: two f32 summation orders of n positive terms differ by at
        # most 2 n 2^-24 of the sum.  The ids come from bit-equal logits: equal.
        assert detect[name + "_alt_ids"].shape[0] == STEPS
        vocab = CONFIGS[SCENARIOS[name][0]].vocab
        np.testing.assert_allclose(detect[name + "_alt_p"], raw[name + "_alt_p"], rtol=2 * vocab * 2.0 ** -24, atol=0)


def test_step_round(detect, rounding):
    assert int(rounding["mode"]) == 2
    assert np.array_equal(rounding["kv8_tokens"], detect["kv8_tokens"])
    assert np.array_equal(rounding["kv8_logits"].view(np.uint32), detect["kv8_logits"].view(np.uint32))
    ref = _oracle("kv8")
    for i, (ids, _) in enumerate(ref):
        assert rounding["batch_%d" % i].tolist() == ids, i
    # the same planes as detect mode on the rounded checkpoint, and some rounding time
    assert np.array_equal(rounding["kv8_wmx4"], detect["kv8_wmx4"])
    assert rounding["kv8_ms"][1] > 0 and detect["kv8_ms"][1] == 0


def _eligible(c):
    dq, dkv = c.dec_heads * c.dec_head_dim, c.dec_kv_heads * c.dec_head_dim
    return [(dq + 2 * dkv, c.dec_dim), (c.dec_dim, dq), (2 * c.dec_hidden, c.dec_dim),
            (c.dec_dim, c.dec_hidden)] * c.dec_layers + [(c.vocab, c.dec_dim)]


def test_stats(detect, raw):
    for cname in ("kv8", "g95"):
        shapes = _eligible(CONFIGS[cname])
        n, refused, pbytes, bbytes = detect[cname + "_wmx4"]
        assert (n, refused) == (len(shapes), 0)
        assert bbytes == sum(r * k * 2 for r, k in shapes)
        bits = float(detect[cname + "_bits"])
        assert bits == pbytes * 8 / (bbytes / 2) and 4.25 <= bits <= 5.0
        # VOX_HIP_WPACK=0 streams raw rows everywhere: no planes are built
        assert not raw[cname + "_wmx4"].any()
    # mode 1 on ordinary weights: every tensor scanned and refused, wpack13 as in mode 0
    assert tuple(detect["plain_wmx4"]) == (0, len(_eligible(KV8)), 0, 0)
    assert np.array_equal(detect["plain_wpack"], detect["plain_off_wpack"])
    assert detect["plain_wpack"][0] == len(_eligible(KV8))
    # mode 0: all zero, whatever the weights; wpack13 of the rounded weights as in mode 1
    for key in ("plain_off", "rounded_off"):
        assert not detect[key + "_wmx4"].any() and float(detect[key + "_bits"]) == 0 and not detect[key + "_ms"].any()
    assert np.array_equal(detect["rounded_off_wpack"], detect["kv8_wpack"])
