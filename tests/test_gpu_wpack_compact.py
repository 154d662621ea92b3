"""GPU: the compact wpack13 side plane (csrc/vox_wpack.h) and the lanes that fetch nothing.

A packed GEMV whose rows end inside their last K round of 256 chunks reads side slots only for
the chunks that exist, and its lanes past the row end take their weights and side dwords as
zeros from the range check instead of re-loading chunk 0.  Its outputs must be the bits of the
raw bf16 GEMV and of the padded side plane.  Chunk 0 of every row and of x holds large values:
a lane that still fetched chunk 0 and met a nonzero x, or a nonzero weight against x it should
not see, would move every output.

Shapes: 1.5 rounds in 4-row groups (QKV, W1|W3) and in the LM head's 8-row groups, W2's 4.5
rounds in 2-row groups, and a last round of a single wave (K = 2560); one group per block.
The knob (VOX_HIP_WPACK_COMPACT, read when a model is created) decodes TINY_LONG in a fresh
process per value: same ids, same logits at every step.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 8

# (rows, K, rows per group, the shape has a compact plane)
SHAPES = [(64, 3072, 4, True), (64, 3072, 8, True), (32, 9216, 2, True), (64, 2560, 4, True),
          (64, 3072, 2, False), (64, 4096, 4, False)]


def _w(rows, K, seed):
    from vox_weights import synth_lib
    out = np.zeros((rows, K), np.uint16)
    synth_lib().vox_synth_bf16(ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(out.size), ctypes.c_uint64(seed),
                               ctypes.c_float(1.0 / np.sqrt(K)), ctypes.c_float(0.0))
    return out


@pytest.mark.parametrize("rows,K,rb,compact", SHAPES)
def test_gemv_bits(rows, K, rb, compact):
    import vox_hip
    from vox_weights import synth_lib
    L = synth_lib()
    L.vox_wpack13_side_compact_of.restype = ctypes.c_int
    L.vox_wpack13_side_compact_of.argtypes = [ctypes.c_longlong, ctypes.c_int]
    assert bool(L.vox_wpack13_side_compact_of(K, rb)) == compact
    W = _w(rows, K, seed=rows + K + rb)
    W[:, :8] = 0x3e00                     # 0.125 in chunk 0 of every row (|w| elsewhere < 2^-5)
    W[1::2, 1:8:2] = 0xbe00
    W[1, 8::7] = 0x8000                   # signed zeros
    x = np.random.default_rng(K + rb).standard_normal(K).astype(np.float32)
    x[:8] = [3.0, -5.0, 7.0, 11.0, -13.0, 17.0, 19.0, -23.0]
    raw, p0 = vox_hip.gemv_wpack_rb(W, x, packed=False, rb=rb)
    new, p1 = vox_hip.gemv_wpack_rb(W, x, packed=True, rb=rb, compact=True)
    pad, p2 = vox_hip.gemv_wpack_rb(W, x, packed=True, rb=rb, compact=False)
    assert (p0, p1, p2) == (False, True, True)
    assert np.array_equal(new, raw)
    assert np.array_equal(pad, raw)
    # the row group does not enter a row's arithmetic
    own, p3 = vox_hip.gemv_wpack(W, x, packed=True)
    assert p3 is True and np.array_equal(own, raw)
    # and the values are the product's: a lane's chain is at most 5 x 8 FMAs, then 6 shuffle
    # adds and 3 adds across waves, each rounding to 2^-24 relative of a partial sum bounded by
    # sum |w x| (tests/test_gpu_wpack.py)
    Wf = (W.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    ref, mag = Wf @ x.astype(np.float64), np.abs(Wf) @ np.abs(x).astype(np.float64)
    assert (np.abs(new - ref) <= 49 * 2.0 ** -24 * mag + 1e-30).all()


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import vox_hip
from vox_weights import TINY_LONG, synth_weights

steps = int(sys.argv[3])
cfg = TINY_LONG
w = synth_weights(cfg, seed=1)
mel = np.random.default_rng(0).uniform(-0.5, 1.5, size=(400, cfg.mel_bins)).astype(np.float32)
model = vox_hip.Model(cfg, w)
st = vox_hip.Stream(model)
st.encode_mel(mel)
toks, logits = st.decode(max_steps=steps, stop_at_eos=False, want_logits=True)
s = model.wpack_stats()
np.savez(sys.argv[1], tokens=np.asarray(toks), logits=np.asarray(logits), compact=np.int64(vox_hip.lib().vox_hip_wpack_compact()),
         stats=np.array([s["packed_tensors"], s["packed_bytes"]], np.int64))
st.close()
model.close()
"""


def _child(tmp, knob):
    path = os.path.join(tmp, f"compact{knob}.npz")
    env = dict(os.environ)
    env.pop("VOX_HIP_WPACK_COMPACT", None)
    if knob is not None:
        env["VOX_HIP_WPACK_COMPACT"] = str(knob)
    r = subprocess.run([sys.executable, "-c", CHILD, path, os.path.join(ROOT, "voxtral.c_amd"), str(STEPS)],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(path))


def test_knob_decode_bits(tmp_path):
    on, off = _child(str(tmp_path), None), _child(str(tmp_path), 0)
    assert (int(on["compact"]), int(off["compact"])) == (1, 0)
    assert len(on["tokens"]) == STEPS
    assert np.array_equal(on["tokens"], off["tokens"])
    assert np.array_equal(on["logits"], off["logits"])
    assert np.isfinite(on["logits"]).all()
    # TINY_LONG's rows take one K round: both arms stream the same planes
    assert on["stats"][0] > 0 and np.array_equal(on["stats"], off["stats"])
