"""k_attn_rows_mf16 without a GPU: the new names are exported and wrapped
(tests/test_abi.py holds EXPORTS to the header's declarations)."""
import ctypes
import os

import pytest

pytestmark = pytest.mark.cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vox_hip_set_enc_attn_mf16", "vox_hip_enc_attn_mf16", "vox_hip_enc_attn_mf16_stats", "vox_hip_enc_attn_kv16",
         "vox_hip_enc_attn_mf16_probe"]


def test_exports():
    import vox_hip
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n) and n in vox_hip.EXPORTS, n
    host = ctypes.CDLL(os.path.join(ROOT, "voxtral.c_amd", "libvox_hip_host.so"))
    assert hasattr(host, "vh_set_enc_attn_mf16")
    for f in ("set_enc_attn_mf16", "enc_attn_mf16", "enc_attn_mf16_stats", "enc_attn_kv16", "enc_attn_mf16_probe"):
        assert callable(getattr(vox_hip, f))
