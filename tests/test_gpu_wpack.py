"""GPU: the single-stream decode step from wpack13 planes (csrc/vox_wpack.h, 13 bits per
bf16 weight, lossless) computes the same bits as from the raw bf16 rows.

VOX_HIP_WPACK is read once at model creation, so each mode decodes in a fresh child process
(one per mode, every scenario in it); token ids, every step's logits and the alternatives
must be identical.  The scenarios cover every converted epilogue (QKV, RESID, SWIGLU, LOGITS,
and LOGITS_ALT through n_alt > 1) and both decoder KV ring types (f32, IEEE half).  TINY's
matrices all have 2-row groups and one K round, so single GEMVs through the test entry add
the 4- and 8-row groups, two full K rounds, and W2's ragged fifth round.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 12
RAW_TENSOR = "layers.1.feed_forward.w2.weight"   # given one out-of-window weight in "window"

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import vox_hip
from vox_weights import TINY, TINY_LONG, synth_weights

steps, raw_tensor = int(sys.argv[3]), sys.argv[4]
out = {}
rng = np.random.default_rng(0)
mel = rng.uniform(-0.5, 1.5, size=(400, TINY.mel_bins)).astype(np.float32)
# (name, config, half KV ring, n_alt, one out-of-window weight)
for name, cfg, kv16, n_alt, window in (("f32", TINY, 0, 1, 0), ("half_alt", TINY, 1, 3, 0),
                                       ("long_alt", TINY_LONG, 0, 3, 0), ("window", TINY, 0, 1, 1)):
    w = synth_weights(cfg, seed=1)
    if window:
        w.t[raw_tensor][5, 17] = 60 << 7   # 2^-67: the tensor's exponents now span > 30 binades
    model = vox_hip.Model(cfg, w)
    if kv16:
        model.set_kv_fp16(True)
    st = vox_hip.Stream(model)
    assert st.kv_fp16 == bool(kv16)
    st.encode_mel(mel)
    if n_alt > 1:
        st.set_alt(n_alt, 1.0)
    toks, logits = st.decode(max_steps=steps, stop_at_eos=False, want_logits=True)
    out[name + "_tokens"] = np.asarray(toks)
    out[name + "_logits"] = np.asarray(logits)
    if n_alt > 1:
        ids, pr = st.read_alts(0, len(toks))
        out[name + "_alt_ids"], out[name + "_alt_p"] = np.asarray(ids), np.asarray(pr)
    s = model.wpack_stats()
    out[name + "_stats"] = np.array([s["packed_tensors"], s["raw_tensors"], s["packed_bytes"],
                                     s["packed_raw_bytes"], s["raw_bytes"]], np.int64)
    st.close()
    model.close()
np.savez(sys.argv[1], **out)
"""


def _child(tmp, mode):
    path = os.path.join(tmp, f"wpack{mode}.npz")
    env = dict(os.environ, VOX_HIP_WPACK=str(mode))
    r = subprocess.run([sys.executable, "-c", CHILD, path, os.path.join(ROOT, "voxtral.c_amd"), str(STEPS), RAW_TENSOR],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(path))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("wpack"))
    return _child(tmp, 1), _child(tmp, 0)


@pytest.mark.parametrize("name", ["f32", "half_alt", "long_alt", "window"])
def test_decode_bits(runs, name):
    on, off = runs
    assert len(on[name + "_tokens"]) == STEPS
    for k in on:
        if k.startswith(name + "_") and not k.endswith("_stats"):
            assert np.array_equal(on[k], off[k]), k
    assert np.isfinite(on[name + "_logits"]).all()


def test_stats(runs, tiny_cfg):
    on, off = runs
    c = tiny_cfg
    n = 4 * c.dec_layers + 1   # Q|K|V, wo, W1|W3, W2 per decoder layer, and the LM head
    dq, dkv = c.dec_heads * c.dec_head_dim, c.dec_kv_heads * c.dec_head_dim
    shapes = [(dq + 2 * dkv, c.dec_dim), (c.dec_dim, dq), (2 * c.dec_hidden, c.dec_dim),
              (c.dec_dim, c.dec_hidden)] * c.dec_layers + [(c.vocab, c.dec_dim)]
    # 12 B per 8 weights, and one side dword per thread of each 2-row group (one K round)
    want_planes = sum(r * k // 8 * 12 + r // 2 * 256 * 4 for r, k in shapes)
    want_bf16 = sum(r * k * 2 for r, k in shapes)
    for name in ("f32", "half_alt", "long_alt"):
        packed, raw, pbytes, prbytes, rbytes = on[name + "_stats"]
        assert (packed, raw, rbytes) == (n, 0, 0)
        assert (pbytes, prbytes) == (want_planes, want_bf16)
        assert tuple(off[name + "_stats"]) == (0, n, 0, 0, want_bf16)
    packed, raw, _, _, rbytes = on["window_stats"]
    assert (packed, raw) == (n - 1, 1)
    assert rbytes == tiny_cfg.dec_dim * tiny_cfg.dec_hidden * 2


def _w(rows, K, seed):
    import ctypes
    from vox_weights import synth_lib
    out = np.zeros((rows, K), np.uint16)
    synth_lib().vox_synth_bf16(ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(out.size), ctypes.c_uint64(seed),
                               ctypes.c_float(1.0 / np.sqrt(K)), ctypes.c_float(0.0))
    return out


# rows pick the row group (2 / 4 / 8 rows), K the rounds of 256 chunks: 4.5 (W2's ragged fifth
# round), 2 full, a fraction of one; 72 = 9 chunks
@pytest.mark.parametrize("rows,K", [(6, 9216), (6144, 4096), (6148, 72), (65536, 72), (65544, 264)])
def test_single_gemv_bits(rows, K):
    import vox_hip
    W = _w(rows, K, seed=rows + K)
    W[1, ::7] = 0x8000   # signed zeros
    W[2, ::5] = 0
    x = np.random.default_rng(K).standard_normal(K).astype(np.float32)
    y0, p0 = vox_hip.gemv_wpack(W, x, packed=False)
    y1, p1 = vox_hip.gemv_wpack(W, x, packed=True)
    assert (p0, p1) == (False, True)
    assert np.array_equal(y0, y1)
    # against float64: a lane's chain is at most 5 x 8 FMAs, then 6 shuffle adds and 3 adds
    # across waves, each rounding to 2^-24 relative of a partial sum bounded by sum |w x|
    Wf = (W.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    ref, mag = Wf @ x.astype(np.float64), np.abs(Wf) @ np.abs(x).astype(np.float64)
    assert (np.abs(y1 - ref) <= 49 * 2.0 ** -24 * mag + 1e-30).all()
    # an out-of-window weight: the raw kernel runs instead, same bits again
    W[0, 0] = 60 << 7
    y2, p2 = vox_hip.gemv_wpack(W, x, packed=True)
    y3, _ = vox_hip.gemv_wpack(W, x, packed=False)
    assert p2 is False and np.array_equal(y2, y3)
