"""k_attn_rows_mf8 without a GPU: the new names are exported, declared and wrapped."""
import ctypes
import os
import re

import pytest

pytestmark = pytest.mark.cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vox_hip_set_enc_attn_mf8", "vox_hip_enc_attn_mf8", "vox_hip_enc_attn_mf8_stats", "vox_hip_enc_attn_kv8"]


def test_exports():
    import vox_hip
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "voxtral_hip.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in vox_hip.EXPORTS and re.search(rf"\b{n}\s*\(", hdr), n
    host = ctypes.CDLL(os.path.join(ROOT, "voxtral.c_amd", "libvox_hip_host.so"))
    assert hasattr(host, "vh_set_enc_attn_mf8")
    assert re.search(r"\bvh_set_enc_attn_mf8\s*\(", open(os.path.join(ROOT, "include", "vox_hip_host.h")).read())
    for f in ("set_enc_attn_mf8", "enc_attn_mf8", "enc_attn_mf8_stats", "enc_attn_kv8"):
        assert callable(getattr(vox_hip, f))
