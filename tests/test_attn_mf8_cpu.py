"""k_attn_decode_mf8 without a GPU: the exports, and the two exactness claims the
kernel rests on -- every finite E4M3 value is a bf16 value, and the project's hi + mid + lo bf16
split reproduces an f32 exactly."""
import ctypes
import os
import re

import numpy as np

from kv8_ref import np_kv8_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vox_hip_set_attn_mf8", "vox_hip_attn_mf8", "vox_hip_attn_mf8_stats", "vox_hip_attn_decode_kv8",
         "vox_hip_attn_mf8_codes"]


def _bf16(x):
    """f32 -> bf16 (round to nearest even) -> f32"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def test_exports():
    import vox_hip
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "voxtral_hip.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in vox_hip.EXPORTS and re.search(rf"\b{n}\s*\(", hdr), n
    host = ctypes.CDLL(os.path.join(ROOT, "voxtral.c_amd", "libvox_hip_host.so"))
    assert hasattr(host, "vh_set_attn_mf8")
    for f in ("set_attn_mf8", "attn_mf8", "attn_mf8_stats", "attn_decode_kv8", "attn_mf8_codes"):
        assert callable(getattr(vox_hip, f))


def test_every_finite_e4m3_value_is_a_bf16():
    v = np_kv8_values()
    fin = v[~np.isnan(v)].astype(np.float32)
    assert fin.size == 254 and np.array_equal(fin.astype(np.float64), v[~np.isnan(v)])
    assert np.array_equal(_bf16(fin).view(np.uint32), fin.view(np.uint32))


def test_split3_reproduces_f32_over_the_normal_range():
    """split3 of vox_hip_dev.h: hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid), every
    difference exact in f32; hi + mid + lo == v for normal f32 whose lo plane stays normal (24
    mantissa bits in three 8-bit pieces)"""
    rng = np.random.default_rng(35)
    e = rng.integers(-100, 100, 1 << 16)
    v = (rng.uniform(1.0, 2.0, e.size) * np.where(rng.integers(0, 2, e.size), -1.0, 1.0)).astype(np.float32)
    v = np.ldexp(v, e).astype(np.float32)
    v = np.concatenate([v, np.float32([1.0, -1.0, 448.0, 3.4028235e38 / 2, 1.1754944e-38 * 2 ** 20, 0.0])])
    hi = _bf16(v)
    r1 = v - hi
    mid = _bf16(r1)
    r2 = r1 - mid
    lo = _bf16(r2)
    assert np.array_equal(lo, r2)                         # nothing is left after three planes
    assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64), v.astype(np.float64))
