"""CPU: the reference the GPU tests of the 16-bit encoder K/V rings compare against
(tests/enc_kv_ref.py, a restatement of the oracle's incremental encoder with a hook at the K/V
append) is pinned to the oracle itself, and the library declares and exports the new entry points.
No GPU work here."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.cpu

# mel frames per chunk: 1 row, 2 rows, odd frame counts (a conv0 column carried over), a single
# frame, a chunk of more than 80 rows, and chunks that leave 1..3 rows for the next adapter group
SCHEDULE = [2, 4, 7, 1, 50, 170, 33, 3, 200, 51]


def _mel(cfg, seed, frames):
    return np.random.default_rng(seed).uniform(-0.6, 1.4, size=(frames, cfg.mel_bins)).astype(np.float32)


@pytest.fixture(scope="module")
def sessions(tiny_cfg, tiny_weights):
    """(oracle adapter rows, added per chunk, identity restatement, f16-hook restatement)"""
    import enc_kv_ref
    import vox_oracle
    mel = _mel(tiny_cfg, 5100, sum(SCHEDULE))
    pieces = enc_kv_ref.chunks(mel, SCHEDULE)
    om = vox_oracle.OracleModel(tiny_cfg, tiny_weights)
    os_ = vox_oracle.OracleStream(om)
    o_added = [os_.encode_mel(p) for p in pieces]
    o_rows = os_.read_adapter()
    os_.close()
    om.close()
    ident = enc_kv_ref.RefEncoder(tiny_cfg, tiny_weights)
    i_added = [ident.encode_mel(p) for p in pieces]
    half = enc_kv_ref.RefEncoder(tiny_cfg, tiny_weights, enc_kv_ref.f16_hook)
    for p in pieces:
        half.encode_mel(p)
    return o_rows, o_added, ident, i_added, half


def test_identity_hook_is_the_oracle_bit_for_bit(sessions, tiny_cfg):
    o_rows, o_added, ident, i_added, _ = sessions
    assert i_added == o_added and sum(o_added) > 0
    rows = ident.adapter()
    assert rows.shape == o_rows.shape and rows.shape[0] == sum(SCHEDULE) // 2 // 4
    assert ident.pos > tiny_cfg.enc_window + 80          # the window slid, a chunk had > 80 rows
    assert np.array_equal(rows.view(np.uint32), o_rows.view(np.uint32))


def test_identity_hook_is_the_oracle_on_q8_weights(tiny_cfg, tiny_weights):
    """the Q8 checkpoint (the GPU's slab path is reached through it): same pin, fewer chunks"""
    import enc_kv_ref
    import vox_oracle
    from vox_weights import quantize_q8
    w8 = quantize_q8(tiny_weights)
    pieces = enc_kv_ref.chunks(_mel(tiny_cfg, 5101, 190), [50, 2, 87])
    om = vox_oracle.OracleModel(tiny_cfg, w8)
    os_ = vox_oracle.OracleStream(om)
    for p in pieces:
        os_.encode_mel(p)
    o_rows = os_.read_adapter()
    os_.close()
    om.close()
    ident = enc_kv_ref.RefEncoder(tiny_cfg, w8)
    for p in pieces:
        ident.encode_mel(p)
    assert o_rows.shape[0] > 0 and np.array_equal(ident.adapter().view(np.uint32), o_rows.view(np.uint32))


def test_f16_hook_is_applied(sessions):
    o_rows, _, _, _, half = sessions
    import enc_kv_ref
    import vox_oracle
    rows = half.adapter()
    assert rows.shape == o_rows.shape
    d = enc_kv_ref.rel(rows, o_rows)
    print(f"f16-hook restatement against the f32 oracle: rel {d:.3e}")
    assert d > 0, d
    for l in range(len(half.K)):
        assert np.array_equal(vox_oracle.f16_round(half.K[l]).reshape(half.K[l].shape), half.K[l])
        assert np.array_equal(vox_oracle.f16_round(half.V[l]).reshape(half.V[l].shape), half.V[l])


NEW = ["vox_hip_model_set_enc_kv_fp16", "vox_hip_stream_enc_kv_fp16", "vox_hip_stream_read_enc_kv",
       "vox_hip_stream_enc_kv_bytes", "vox_hip_stream_enc_paths"]


def test_abi_declares_and_exports_the_encoder_ring_calls():
    import vox_hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voxtral_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in vox_hip.EXPORTS, n
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vox_hip_host.h")).read(), flags=re.S)
    hl = ctypes.CDLL(os.path.join(ROOT, "voxtral.c_amd", "libvox_hip_host.so"))
    for n in ["vh_set_enc_kv_fp16", "vh_stream_enc_kv_fp16"]:
        assert re.search(r"\b%s\s*\(" % n, host), n
        assert hasattr(hl, n), n
    for name in ["set_enc_kv_fp16"]:
        assert hasattr(vox_hip.Model, name)
    for name in ["enc_kv_fp16", "read_enc_kv", "enc_kv_bytes", "enc_paths"]:
        assert hasattr(vox_hip.Stream, name)
