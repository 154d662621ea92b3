"""GPU: the opt-in lossless wpack13 fragment planes of the batched MFMA decode step (the WF_P13 instances of k_skl /
k_skl2 / k_sklx / k_skf): the bits of the step on the bf16 fragment copies, and the CPU oracle's ids.
The modes are read at model creation, so each step case decodes in a fresh child process.  Configs, mels, rows and
comparisons are tests/test_gpu_wmx4_batch.py's."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import test_gpu_wmx4_batch as t
from test_gpu_wmx4_batch import KV8, WIDE, LOGIT_TOL, MARGIN_F32, SLOTS, STEPS, _keys, _same
from test_wpack_frag_cpu import _matrix

pytestmark = pytest.mark.gpu

# the first mel seed of 1, 2, ... at which the oracle on synth_weights(KV8, seed=1) keeps a top-2 gap of MARGIN_F32
ORACLE_SEED = 1
W2 = "layers.0.feed_forward.w2.weight"
# t's projection shapes and LM heads of 256 row groups (skf_cfg's R = 1), and heads of 512 (R = 2) and 2048 (R = 4)
ENTRY = t.ENTRY + [(8192, 320, 1), (32768, 320, 1)]


def _far():
    """synth_weights(KV8, seed=1) with the largest weight of one W2 times 2^40: that tensor leaves the window"""
    from vox_weights import Weights
    base = t._weights("kv8", "plain")
    a = base.t[W2].copy()
    a.flat[np.argmax(a & 0x7fff)] += 40 << 7
    return Weights(base.cfg, dict(base.t, **{W2: a}), keep=base._keep)


CHILD = r"""
import sys
import numpy as np
sys.path[:0] = sys.argv[2:4]
import vox_hip
import test_gpu_wmx4_batch as t
import test_gpu_wpack_batch as p
out = {"mode": np.array(vox_hip.wpack_batch())}

def model(cfg, w, key):
    m = vox_hip.Model(cfg, w)
    s = m.wpack_batch_stats()
    out[key + "_stats"] = np.array([s["tensors"], s["plane_bytes"], s["bf16_bytes"]], np.int64)
    b = vox_hip.Batch(m, 2)
    out[key + "_set"] = np.array([b.wpack(), b.set_wpack(1), b.set_wpack(0)])   # a new batch's mode; on; off
    b.close()
    return m

def run(m, cname, n, modes, key):
    # STEPS single-step calls of one Batch over n fresh streams; modes: {step: set_wpack before it}
    ss = [vox_hip.Stream(m) for _ in range(n)]
    for s, mel in zip(ss, t._mels(cname, n, p.ORACLE_SEED)):
        s.encode_mel(mel)
    ss[t.ALT_SLOT].set_alt(3, 1.0)
    b = vox_hip.Batch(m, n)
    got, lg = [[] for _ in ss], {i: [] for i in t.SLOTS[n]}
    for k in range(t.STEPS):
        if k in modes:
            assert b.set_wpack(modes[k]) == 0, k
        for i, ids in enumerate(b.decode(ss, max_steps=1, stop_at_eos=False)):
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

m = model(t.KV8, t._weights("kv8", "plain"), "kv8")
if sys.argv[4] == "off":
    run(m, "kv8", 17, {}, "off17")
else:
    for n in t.TWIN_STREAMS:
        run(m, "kv8", n, {} if n == 3 else {0: 1}, "on%d" % n)   # a new batch starts with it on
        run(m, "kv8", n, {0: 0}, "off%d" % n)
    run(m, "kv8", 17, {0: 1, t.STEPS // 2: 0}, "switch17")
    for key, cname, w, n in (("wide", "wide", t._weights("wide", "plain"), 17), ("far", "kv8", p._far(), 3)):
        m.close()
        m = model(t.CONFIGS[cname], w, key)
        run(m, cname, n, {0: 1}, "%s_on%d" % (key, n))
        run(m, cname, n, {0: 0}, "%s_off%d" % (key, n))
    m.close()
    m = model(t.KV8, t._weights("kv8", "q8"), "q8")
m.close()
np.savez(sys.argv[1], **out)
"""


_RES = {}


def _res(job):
    """what the child of that job saved: `on` runs under VOX_HIP_WPACK_BATCH=1, `off` with it unset"""
    if job not in _RES:
        env = {k: v for k, v in os.environ.items() if not k.startswith(("VOX_HIP_W", "VOX_HIP_BATCH_GEMV"))}
        if job == "on":
            env["VOX_HIP_WPACK_BATCH"] = "1"
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, job + ".npz")
            r = subprocess.run([sys.executable, "-c", CHILD, path, os.path.join(t.ROOT, "voxtral.c_amd"),
                                os.path.join(t.ROOT, "tests"), job], env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            _RES[job] = dict(np.load(path))
    return _RES[job]


@pytest.mark.parametrize("N,K,head", ENTRY)
def test_entry_bits(N, K, head):
    import vox_hip
    W = _matrix(N, K, 100, seed=N + K + head)   # the whole 30-binade window, zeros of both signs
    Wf = t.bf16_f64(W)
    for nb in t.ENTRY_ROWS:
        x = t._x(nb, K, seed=K + nb)
        y0 = vox_hip.skinny_wpack(W, x, fmt=0, head=bool(head))
        y1 = vox_hip.skinny_wpack(W, x, fmt=1, head=bool(head))
        ref = x.astype(np.float64) @ Wf.T
        e0, e1 = (float(np.max(np.abs(y - ref)) / np.max(np.abs(ref))) for y in (y0, y1))
        print(f"skinny_wpack ({N}, {K}) head={head} nb={nb}: err bf16 {e0:.2e} p13 {e1:.2e} of max|y| (bar {LOGIT_TOL:.0e})")
        assert np.array_equal(y1.view(np.uint32), y0.view(np.uint32)), nb
        assert e0 < LOGIT_TOL and e1 < LOGIT_TOL, nb


def test_entry_refusal():
    import vox_hip
    W = _matrix(768, 1280, 100, seed=3)
    W[5, 7] = (W[0, 1] & 0x7fff) + (40 << 7)   # the top of the window times 2^40
    with pytest.raises(RuntimeError, match="window"):
        vox_hip.skinny_wpack(W, t._x(5, 1280, seed=5), fmt=1)


@pytest.mark.parametrize("a,b,n", [("on3", "off3", 3), ("on16", "off16", 16), ("on17", "off17", 17), ("on32", "off32", 32),
                                   ("wide_on17", "wide_off17", 17), ("switch17", "on17", 17), ("far_on3", "far_off3", 3)])
def test_step_is_its_twin(a, b, n):
    """set_wpack(1) against set_wpack(0): KV8, WIDE (8-wave variants), a switch between two calls on live streams
    against the unswitched run, and a model whose one unplaned tensor goes through its bf16 copy"""
    on = _res("on")
    assert int(on["mode"]) == 1 and on["kv8_set"].tolist() == [1, 0, 0]   # a new batch starts in the p13 mode
    assert on[a + "_ids"].shape == (n, STEPS)
    _same({k.replace(a, b, 1): on[k] for k in _keys(a, n)}, on, _keys(b, n))


def test_step_is_the_oracle():
    t.ORACLE_RUNS["p13"] = ("kv8", "plain", 17, False, ORACLE_SEED)   # t._oracle's run on the unrounded weights
    for ids, lg in t._oracle("p13"):
        top = np.sort(lg, axis=1)
        gap = (top[:, -1] - top[:, -2]) / np.max(np.abs(lg), axis=1)
        assert gap.min() >= MARGIN_F32, gap.min()
    t._against_oracle(_res("on"), "on17", "p13", 17, SLOTS[17])   # every id, logits within LOGIT_TOL


def test_off_refusal_stats():
    on, off = _res("on"), _res("off")
    assert int(off["mode"]) == 0 and not off["kv8_stats"].any() and off["kv8_set"].tolist() == [0, -1, 0]
    _same(off, on, _keys("off17", 17))   # variable unset: no planes, the switch fails, the switched-off run's bits
    for key, c, skip in (("kv8", KV8, 0), ("wide", WIDE, 0), ("far", KV8, 1)):   # 13 bits per weight of every plane
        shapes = t._proj_shapes(c) * c.dec_layers + [(c.vocab, c.dec_dim)]
        shapes = shapes[:3] + shapes[3 + skip:]   # without layer 0's W2
        n, pbytes, bbytes = on[key + "_stats"]
        assert n == len(shapes) == 4 * c.dec_layers + 1 - skip and pbytes * 16 == bbytes * 13 == sum(N * K * 26 for N, K in shapes)
    assert not on["q8_stats"].any() and on["q8_set"].tolist() == [0, -1, 0]
