"""CPU: what the GPU tests of the FP8 (E4M3) encoder K/V rings compare against -- the restatement
of the oracle's incremental encoder (tests/enc_kv_ref.py, pinned to the oracle by
tests/test_enc_kv16_cpu.py) with a hook at the K/V append built on vox_kv8_round of
csrc/vox_kv8.h (through libvox_synth.so) -- really rounds, the library declares and exports the
new entry points, and the CLI takes --enc-kv8.  No GPU work here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.cpu

# mel frames per chunk: one-row and odd chunks, a chunk of more than 80 rows, the window slides
SCHEDULE = [2, 7, 50, 170, 33, 200, 51]


def _mel(cfg, seed, frames):
    return np.random.default_rng(seed).uniform(-0.6, 1.4, size=(frames, cfg.mel_bins)).astype(np.float32)


def _kv8_round(x):
    """vox_kv8_round of csrc/vox_kv8.h over an array, shape kept"""
    from vox_weights import synth_lib
    L = synth_lib()
    L.vox_kv8_round.argtypes = [ctypes.c_float]
    L.vox_kv8_round.restype = ctypes.c_float
    x = np.ascontiguousarray(x, np.float32)
    return np.array([L.vox_kv8_round(float(v)) for v in x.ravel()], np.float32).reshape(x.shape)


def fp8_hook(k, v, layer, pos):
    return _kv8_round(k), _kv8_round(v)


@pytest.fixture(scope="module")
def sessions(tiny_cfg, tiny_weights):
    import enc_kv_ref
    pieces = enc_kv_ref.chunks(_mel(tiny_cfg, 5200, sum(SCHEDULE)), SCHEDULE)
    ident = enc_kv_ref.RefEncoder(tiny_cfg, tiny_weights)
    fp8 = enc_kv_ref.RefEncoder(tiny_cfg, tiny_weights, fp8_hook)
    added = [(ident.encode_mel(p), fp8.encode_mel(p)) for p in pieces]
    assert all(a == b for a, b in added) and sum(a for a, _ in added) > 0
    return ident, fp8


def test_fp8_hook_session_differs_from_the_identity_session(sessions, tiny_cfg):
    import enc_kv_ref
    ident, fp8 = sessions
    assert ident.pos == fp8.pos > tiny_cfg.enc_window + 80
    a, b = ident.adapter(), fp8.adapter()
    assert a.shape == b.shape and a.shape[0] > 0
    d = enc_kv_ref.rel(b, a)
    print(f"fp8-hook restatement against the identity session: rel {d:.3e}")
    # three mantissa bits: the session sits far above the f32 bar, not merely off it
    assert d > 100 * enc_kv_ref.ACT_TOL, d
    # layer-0 K/V do not depend on the ring: the fp8 session holds the rounding of the identity's
    assert np.array_equal(fp8.K[0], _kv8_round(ident.K[0])) and np.array_equal(fp8.V[0], _kv8_round(ident.V[0]))
    assert not np.array_equal(fp8.K[0], ident.K[0])


def test_fp8_hook_is_idempotent(sessions):
    _, fp8 = sessions
    for l in range(len(fp8.K)):
        assert np.array_equal(_kv8_round(fp8.K[l]), fp8.K[l]) and np.array_equal(_kv8_round(fp8.V[l]), fp8.V[l])
        assert float(np.max(np.abs(fp8.K[l]))) < 448 and float(np.max(np.abs(fp8.V[l]))) < 448     # nothing saturated
    x = np.array([0.0, -0.0, 1e-4, 2.0 ** -10, 0.3, -17.3, 447.9, 448.0, 1e9, -1e9, np.inf], np.float32)
    r = _kv8_round(x)
    assert np.array_equal(_kv8_round(r), r) and float(np.max(np.abs(r))) == 448.0


NEW = ["vox_hip_model_set_enc_kv_dtype", "vox_hip_stream_enc_kv_dtype"]


def test_abi_declares_and_exports_the_encoder_dtype_calls():
    import vox_hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voxtral_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in vox_hip.EXPORTS, n
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vox_hip_host.h")).read(), flags=re.S)
    hl = ctypes.CDLL(os.path.join(ROOT, "voxtral.c_amd", "libvox_hip_host.so"))
    for n in ["vh_set_enc_kv_dtype", "vh_stream_enc_kv_dtype"]:
        assert re.search(r"\b%s\s*\(" % n, host), n
        assert hasattr(hl, n), n
    assert hasattr(vox_hip.Model, "set_enc_kv_dtype") and hasattr(vox_hip.Stream, "enc_kv_dtype")
    # the earlier names stay
    assert hasattr(vox_hip.Model, "set_enc_kv_fp16") and hasattr(vox_hip.Stream, "enc_kv_fp16")


def test_cli_names_enc_kv8_and_refuses_it_together_with_enc_kv16():
    exe = os.path.join(ROOT, "voxtral.c_amd", "vox_hip_transcribe")

    def run(*args):
        p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
        return p.returncode, p.stderr

    rc, err = run()
    assert rc == 2 and "--enc-kv8" in err and "--enc-kv16" in err
    rc, err = run("-d", "/nonexistent/model", "-i", "/nonexistent/a.wav", "--enc-kv16", "--enc-kv8")
    assert rc == 2 and "usage" in err and "exclude" in err
    for flag in ("--enc-kv8", "--enc-kv16"):
        # accepted alone: the run gets as far as the checkpoint, which does not exist
        rc, err = run("-d", "/nonexistent/model", "-i", "/nonexistent/a.wav", flag)
        assert rc == 1 and "usage" not in err, (flag, rc, err)
