"""Python host-side mirror of the voxtral.c streaming API over the MI355X backend.

Loads libvoxtral_hip.so (built in-tree by __graft_entry__.build()) and exposes the same
objects the reference's C API has (voxtral.h:251-337): a model loaded once, streams fed
incrementally, greedy token ids out.  Streams take log-mel frames (host or device
arrays), or raw 16 kHz samples through AudioSession, whose incremental log-mel (Mel,
vox_mel_ctx_t) runs on the device.

There is no CPU fallback: if the HIP library or a GPU is missing every entry point
raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from vox_weights import (VoxConfig, Weights, build_weights_struct, config_struct_class,
                         weights_struct_class)

_HERE = os.path.dirname(os.path.abspath(__file__))
# VOX_HIP_LIB: another build of the same library (developer A/B of two builds on one box)
LIB_PATH = os.environ.get("VOX_HIP_LIB") or os.path.join(_HERE, "libvoxtral_hip.so")

TOKEN_BOS, TOKEN_EOS, TOKEN_STREAMING_PAD = 1, 2, 32
STREAM_FIRST_CHUNK_MIN_MEL = 312          # voxtral.c:405
STREAM_DEFAULT_INTERVAL = 2.0             # voxtral.c:408
RAW_AUDIO_LENGTH_PER_TOK = 1280           # voxtral.c:400
OFFLINE_STREAMING_BUFFER_TOKENS = 10      # voxtral.c:401

ConfigC = config_struct_class()
WeightsC = weights_struct_class()

class WPackStatsC(ctypes.Structure):
    """vox_hip_wpack_stats_t"""
    _fields_ = [("packed_tensors", ctypes.c_int), ("raw_tensors", ctypes.c_int),
                ("packed_bytes", ctypes.c_longlong), ("packed_raw_bytes", ctypes.c_longlong),
                ("raw_bytes", ctypes.c_longlong), ("pack_ms", ctypes.c_double)]


class WMx4StatsC(ctypes.Structure):
    """vox_hip_wmx4_stats_t"""
    _fields_ = [("wmx4_tensors", ctypes.c_int), ("refused_tensors", ctypes.c_int),
                ("plane_bytes", ctypes.c_longlong), ("bf16_bytes", ctypes.c_longlong),
                ("bits_per_weight", ctypes.c_double), ("scan_ms", ctypes.c_double),
                ("round_ms", ctypes.c_double), ("pack_ms", ctypes.c_double)]


def gemv_wpack(W_bf16, x, packed):
    """Test entry: (y, ran_packed) of y = W x for one bf16 matrix [rows, K] through the M = 1
    GEMV, from wpack13 planes (packed True / 1), from the wmx4 plane (packed=2) or from the raw
    rows.  ran_packed is a bool for packed False / True, and for packed=2 the kernel that ran:
    2 (wmx4) or 0 (raw: the matrix is not MXFP4-valued)"""
    init()
    W = np.ascontiguousarray(W_bf16, np.uint16)
    xv = np.ascontiguousarray(x, np.float32)
    rows, K = W.shape
    assert xv.shape == (K,)
    y = np.empty(rows, np.float32)
    rc = lib().vox_hip_gemv_wpack(rows, K, W.ctypes.data, fptr(xv), fptr(y), int(packed))
    if rc < 0:
        _err("gemv_wpack")
    return y, (rc if int(packed) == 2 else bool(rc))


def gemv_rows(W_bf16, x, packed):
    """Test entry: (y [R, rows], flags) of y[r] = W x[r] for R <= 8 rows through the R-row GEMV
    (vox_hip_gemv_rows); packed: 0 raw rows, 1 (or True) wpack13 planes, 2 the wmx4 plane.
    flags bit 0: the wpack13 instance ran, bit 1: the per-row summation order is the single-row
    GEMV's, bit 2: the wmx4 instance ran"""
    init()
    W = np.ascontiguousarray(W_bf16, np.uint16)
    xv = np.ascontiguousarray(x, np.float32)
    rows, K = W.shape
    assert xv.ndim == 2 and xv.shape[1] == K
    R = xv.shape[0]
    y = np.empty((R, rows), np.float32)
    rc = lib().vox_hip_gemv_rows(rows, K, W.ctypes.data, fptr(xv), R, fptr(y), int(packed))
    if rc < 0:
        _err("gemv_rows")
    return y, rc


def _q8_args(W_i8, scales, x):
    W = np.ascontiguousarray(W_i8, np.int8)
    sc = np.ascontiguousarray(scales, np.float32)
    xv = np.ascontiguousarray(x, np.float32)
    rows, K = W.shape
    assert sc.shape == (rows,) and xv.shape[-1] == K
    return W, sc, xv, rows, K


def gemv_rows_q8(W_i8, scales, x):
    """Test entry: y [R, rows] of y[r] = scales * (W x[r]) for R <= 8 rows through the R-row
    GEMV's Q8 instance (vox_hip_gemv_rows_q8); W int8 [rows, K], scales f32 [rows]"""
    init()
    W, sc, xv, rows, K = _q8_args(W_i8, scales, x)
    assert xv.ndim == 2
    R = xv.shape[0]
    y = np.empty((R, rows), np.float32)
    if lib().vox_hip_gemv_rows_q8(rows, K, W.ctypes.data, fptr(sc), fptr(xv), R, fptr(y)) < 0:
        _err("gemv_rows_q8")
    return y


def gemv_q8(W_i8, scales, x):
    """Test entry: y [rows] = scales * (W x) through the single-row Q8 GEMV (vox_hip_gemv_q8)"""
    init()
    W, sc, xv, rows, K = _q8_args(W_i8, scales, x)
    assert xv.ndim == 1
    y = np.empty(rows, np.float32)
    if lib().vox_hip_gemv_q8(rows, K, W.ctypes.data, fptr(sc), fptr(xv), fptr(y)) < 0:
        _err("gemv_q8")
    return y


# exported symbols, as declared in include/voxtral_hip.h
EXPORTS = [
    "vox_hip_init", "vox_hip_available", "vox_hip_shutdown", "vox_hip_memory_used",
    "vox_hip_last_error", "vox_hip_clear_error", "vox_hip_set_device", "vox_hip_config_voxtral_4b",
    "vox_hip_model_create", "vox_hip_model_free", "vox_hip_model_set_delay",
    "vox_hip_model_ada_scale", "vox_hip_model_set_kv_fp16", "vox_hip_stream_kv_fp16",
    "vox_hip_model_set_kv_dtype", "vox_hip_stream_kv_dtype", "vox_hip_stream_read_kv", "vox_hip_kv8_convert",
    "vox_hip_model_set_enc_kv_fp16", "vox_hip_stream_enc_kv_fp16", "vox_hip_stream_read_enc_kv",
    "vox_hip_stream_enc_kv_bytes", "vox_hip_stream_enc_paths",
    "vox_hip_model_set_enc_kv_dtype", "vox_hip_stream_enc_kv_dtype",
    "vox_hip_model_set_kv_grow", "vox_hip_stream_kv_slots", "vox_hip_stream_kv_bytes",
    "vox_hip_stream_kv_grow_stats", "vox_hip_stream_reserve_kv", "vox_hip_batch_kv_grow_stats",
    "vox_hip_model_wpack_stats", "vox_hip_gemv_wpack",
    "vox_hip_set_wmx4", "vox_hip_wmx4", "vox_hip_model_wmx4_stats",
    "vox_hip_set_wmx4_batch", "vox_hip_wmx4_batch", "vox_hip_model_wmx4_batch_stats", "vox_hip_batch_set_wmx4",
    "vox_hip_skinny_wmx4",
    "vox_hip_set_gemm_planes", "vox_hip_gemm_planes", "vox_hip_set_gemmf_wait",
    "vox_hip_set_gemmf_q8", "vox_hip_gemmf_q8", "vox_hip_model_gemmf_q8_stats", "vox_hip_gemmf_q8_rows",
    "vox_hip_stream_create", "vox_hip_stream_free",
    "vox_hip_stream_reset", "vox_hip_stream_reset_decoder", "vox_hip_stream_encode_mel",
    "vox_hip_stream_set_delay", "vox_hip_stream_delay", "vox_hip_stream_ada_scale",
    "vox_hip_stream_adapter_tokens", "vox_hip_stream_read_adapter", "vox_hip_stream_decode",
    "vox_hip_set_adapter_rows0", "vox_hip_stream_adapter_stats",
    "vox_hip_batch_create", "vox_hip_batch_free", "vox_hip_batch_decode", "vox_hip_batch_decode_rows",
    "vox_hip_batch_begin_rows", "vox_hip_batch_finish",
    "vox_hip_batch_read_logits",
    "vox_hip_batch_stats", "vox_hip_batch_set_gemv_rows", "vox_hip_batch_gemv_stats", "vox_hip_gemv_rows",
    "vox_hip_batch_set_gemv_wmx4", "vox_hip_batch_gemv_wmx4_stats", "vox_hip_batch_set_prefill_kv",
    "vox_hip_batch_set_gemv_rows_q8", "vox_hip_gemv_rows_q8", "vox_hip_gemv_q8",
    "vox_hip_stream_state", "vox_hip_stream_set_alt", "vox_hip_stream_read_alts", "vox_hip_sgemm_bf16", "vox_hip_sgemm_q8", "vox_hip_fused_qkv_bf16",
    "vox_hip_fused_ffn_bf16", "vox_hip_encoder_attention", "vox_hip_encoder_full_step",
    "vox_hip_decoder_prefill_step", "vox_hip_decoder_start", "vox_hip_decoder_end",
    "vox_hip_decoder_full_step", "vox_hip_stream_set_profiling", "vox_hip_stream_profile",
    "vox_hip_stream_sync", "vox_hip_stream_set_async_encode", "vox_hip_stream_encode_mel_batch", "vox_hip_device_upload", "vox_hip_device_free",
    "vox_hip_mel_create", "vox_hip_mel_feed", "vox_hip_mel_finish", "vox_hip_mel_frames",
    "vox_hip_mel_frame_ptr", "vox_hip_mel_discard_before", "vox_hip_mel_read", "vox_hip_mel_free", "vox_hip_mel_reset",
]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fp = ctypes.POINTER(ctypes.c_float)
    ip = ctypes.POINTER(ctypes.c_int)
    sig = {
        "vox_hip_init": (I, []), "vox_hip_available": (I, []), "vox_hip_shutdown": (None, []),
        "vox_hip_memory_used": (ctypes.c_size_t, []), "vox_hip_last_error": (ctypes.c_char_p, []),
        "vox_hip_clear_error": (None, []),
        "vox_hip_set_device": (I, [I]),
        "vox_hip_config_voxtral_4b": (None, [P]),
        "vox_hip_model_create": (P, [P, P, I]), "vox_hip_model_free": (None, [P]),
        "vox_hip_model_set_delay": (I, [P, I]), "vox_hip_model_ada_scale": (I, [P, fp]),
        "vox_hip_model_set_kv_fp16": (I, [P, I]), "vox_hip_stream_kv_fp16": (I, [P]),
        "vox_hip_model_set_kv_dtype": (I, [P, I]), "vox_hip_stream_kv_dtype": (I, [P]),
        "vox_hip_stream_read_kv": (I, [P, I, I, I, P, P]),
        "vox_hip_model_set_enc_kv_fp16": (I, [P, I]), "vox_hip_stream_enc_kv_fp16": (I, [P]),
        "vox_hip_stream_read_enc_kv": (I, [P, I, I, I, P, P]),
        "vox_hip_model_set_enc_kv_dtype": (I, [P, I]), "vox_hip_stream_enc_kv_dtype": (I, [P]),
        "vox_hip_stream_enc_kv_bytes": (ctypes.c_longlong, [P]),
        "vox_hip_stream_enc_paths": (I, [P, ctypes.POINTER(ctypes.c_longlong)]),
        "vox_hip_model_set_kv_grow": (I, [P, I]), "vox_hip_stream_kv_slots": (I, [P]),
        "vox_hip_stream_kv_bytes": (ctypes.c_longlong, [P]),
        "vox_hip_stream_kv_grow_stats": (I, [P, ctypes.POINTER(ctypes.c_longlong)]),
        "vox_hip_stream_reserve_kv": (I, [P, I]),
        "vox_hip_batch_kv_grow_stats": (I, [P, ctypes.POINTER(ctypes.c_longlong)]),
        "vox_hip_kv8_convert": (I, [fp, I, P, fp]),
        "vox_hip_model_wpack_stats": (I, [P, P]),
        "vox_hip_gemv_wpack": (I, [I, I, P, fp, fp, I]),
        "vox_hip_set_wmx4": (I, [I]), "vox_hip_wmx4": (I, []), "vox_hip_model_wmx4_stats": (I, [P, P]),
        "vox_hip_set_wmx4_batch": (I, [I]), "vox_hip_wmx4_batch": (I, []),
        "vox_hip_model_wmx4_batch_stats": (I, [P, ctypes.POINTER(ctypes.c_longlong)]),
        "vox_hip_batch_set_wmx4": (I, [P, I]),
        "vox_hip_skinny_wmx4": (I, [I, I, P, fp, I, fp, I, I]),
        "vox_hip_set_gemm_planes": (I, [I]), "vox_hip_gemm_planes": (I, []),
        "vox_hip_set_gemmf_wait": (I, [I]),
        "vox_hip_set_gemmf_q8": (I, [I]), "vox_hip_gemmf_q8": (I, []),
        "vox_hip_model_gemmf_q8_stats": (I, [P, ctypes.POINTER(ctypes.c_longlong)]),
        "vox_hip_gemmf_q8_rows": (I, [I, I, I, fp, P, fp, fp, I]),
        "vox_hip_stream_create": (P, [P]), "vox_hip_stream_free": (None, [P]),
        "vox_hip_stream_reset": (I, [P]), "vox_hip_stream_reset_decoder": (I, [P]),
        "vox_hip_stream_set_delay": (I, [P, I]), "vox_hip_stream_delay": (I, [P]),
        "vox_hip_stream_ada_scale": (I, [P, fp]),
        "vox_hip_stream_encode_mel": (I, [P, P, I, I]),
        "vox_hip_stream_adapter_tokens": (I, [P]),
        "vox_hip_set_adapter_rows0": (I, [I]),
        "vox_hip_stream_adapter_stats": (I, [P, ctypes.POINTER(ctypes.c_longlong)]),
        "vox_hip_stream_read_adapter": (I, [P, I, I, fp]),
        "vox_hip_stream_decode": (I, [P, I, I, ip, fp]),
        "vox_hip_stream_state": (I, [P, ip]),
        "vox_hip_batch_create": (P, [P, I]), "vox_hip_batch_free": (None, [P]),
        "vox_hip_batch_decode": (I, [P, ctypes.POINTER(ctypes.c_void_p), I, I, I, ip, ip]),
        "vox_hip_batch_decode_rows": (I, [P, ctypes.POINTER(ctypes.c_void_p), I, ip, I, I, ip, ip]),
        "vox_hip_batch_begin_rows": (I, [P, ctypes.POINTER(ctypes.c_void_p), I, ip, I, I, ip, ip]),
        "vox_hip_batch_finish": (I, [P]),
        "vox_hip_batch_read_logits": (I, [P, P, fp]),
        "vox_hip_batch_stats": (I, [P, ctypes.POINTER(ctypes.c_longlong)]),
        "vox_hip_batch_set_gemv_rows": (I, [P, I]),
        "vox_hip_batch_gemv_stats": (I, [P, ctypes.POINTER(ctypes.c_longlong)]),
        "vox_hip_gemv_rows": (I, [I, I, P, fp, I, fp, I]),
        "vox_hip_batch_set_gemv_wmx4": (I, [P, I]),
        "vox_hip_batch_gemv_wmx4_stats": (I, [P, ctypes.POINTER(ctypes.c_longlong)]),
        "vox_hip_batch_set_prefill_kv": (I, [P, I]),
        "vox_hip_batch_set_gemv_rows_q8": (I, [P, I]),
        "vox_hip_gemv_rows_q8": (I, [I, I, P, fp, fp, I, fp]),
        "vox_hip_gemv_q8": (I, [I, I, P, fp, fp, fp]),
        "vox_hip_stream_set_alt": (I, [P, I, F]),
        "vox_hip_stream_read_alts": (I, [P, I, I, ip, fp]),
        "vox_hip_sgemm_bf16": (None, [I, I, I, fp, P, fp]),
        "vox_hip_sgemm_q8": (None, [I, I, I, fp, P, fp, fp]),
        "vox_hip_fused_qkv_bf16": (None, [I, I, fp, P, I, P, I, P, I, fp, fp, fp]),
        "vox_hip_fused_ffn_bf16": (None, [I, I, I, fp, P, P, P, fp]),
        "vox_hip_encoder_attention": (None, [fp, fp, fp, fp, I, I, I, I, I, F, I, I]),
        "vox_hip_encoder_full_step": (I, [P, fp, I, fp, I]),
        "vox_hip_decoder_prefill_step": (I, [P, fp, I, fp, I]),
        "vox_hip_decoder_start": (None, [P, fp, I]), "vox_hip_decoder_end": (None, [P]),
        "vox_hip_decoder_full_step": (I, [P, fp, I, fp]),
        "vox_hip_stream_set_profiling": (I, [P, I]),
        "vox_hip_stream_profile": (I, [P, ctypes.POINTER(ctypes.c_double)]),
        "vox_hip_stream_sync": (I, [P]),
        "vox_hip_stream_set_async_encode": (I, [P, I]),
        "vox_hip_stream_encode_mel_batch": (I, [P, P, P, I, I, P]),
        "vox_hip_device_upload": (P, [P, ctypes.c_size_t]),
        "vox_hip_device_free": (I, [P]),
        "vox_hip_mel_create": (P, [P, I]), "vox_hip_mel_feed": (I, [P, fp, I]),
        "vox_hip_mel_finish": (I, [P, I]), "vox_hip_mel_frames": (I, [P, ip]),
        "vox_hip_mel_frame_ptr": (P, [P, I]), "vox_hip_mel_discard_before": (I, [P, I]),
        "vox_hip_mel_read": (I, [P, I, I, fp]), "vox_hip_mel_free": (None, [P]), "vox_hip_mel_reset": (I, [P, I]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def fptr(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _err(what):
    msg = lib().vox_hip_last_error()
    raise RuntimeError(f"{what}: {msg.decode() if msg else 'unknown error'}")


KV_F32, KV_F16, KV_FP8 = 0, 1, 2                       # decoder KV ring element types
MAX_DELAY_TOKENS = 30                                  # VOX_HIP_MAX_DELAY_TOKENS (2400 ms)
KV_NP_DTYPE = {KV_F32: np.float32, KV_F16: np.float16, KV_FP8: np.uint8}


def kv8_decode(codes) -> np.ndarray:
    """FP8 E4M3 codes (uint8; csrc/vox_kv8.h) -> their f32 values, exactly"""
    c = np.arange(256)
    e, m = (c >> 3) & 15, (c & 7).astype(np.float64)
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10.0))
    v[(c & 0x7f) == 0x7f] = np.nan
    lut = np.where(c & 0x80, -v, v).astype(np.float32)
    return lut[np.asarray(codes, np.uint8)]


def kv8_convert(x):
    """vox_hip_kv8_convert: the kernels' FP8 ring store and load helpers on the device over x
    -> (codes uint8, the f32 values read back)"""
    x = np.ascontiguousarray(x, np.float32).ravel()
    codes = np.empty(x.size, np.uint8)
    back = np.empty(x.size, np.float32)
    if lib().vox_hip_kv8_convert(fptr(x), x.size, codes.ctypes.data, fptr(back)) != 0:
        _err("kv8_convert")
    return codes, back


def set_gemm_planes(planes: int):
    """bf16 activation planes of the M > 1 GEMMs: 3 (default, exact f32 activations) or 2 (hi + lo)"""
    if lib().vox_hip_set_gemm_planes(int(planes)) != 0:
        _err("set_gemm_planes")


def gemm_planes() -> int:
    return lib().vox_hip_gemm_planes()


def set_wmx4(mode: int):
    """MXFP4 weight streaming of models created from now on: 0 off (default), 1 stream the
    decode-step matrices that are already MXFP4-valued, 2 round them first (include/voxtral_hip.h)"""
    if lib().vox_hip_set_wmx4(int(mode)) != 0:
        _err("set_wmx4")


def wmx4() -> int:
    return lib().vox_hip_wmx4()


def set_wmx4_batch(on: bool):
    """wmx4 fragment planes for the batched MFMA step, for models created from now on (on top
    of wmx4 mode 1 or 2; include/voxtral_hip.h)"""
    if lib().vox_hip_set_wmx4_batch(int(bool(on))) != 0:
        _err("set_wmx4_batch")


def wmx4_batch() -> int:
    return lib().vox_hip_wmx4_batch()


def skinny_wmx4(W_bf16, x, fmt: int, head: bool = False) -> np.ndarray:
    """Test entry: y [nb, N] = x [nb, K] @ W^T for nb <= 32 rows through the batched step's
    launchers (vox_hip_skinny_wmx4): the projection kernels and their slab sum, or the LM-head
    kernel (head).  fmt 0: the bf16 fragment-major copy, fmt 1: the wmx4 fragment plane (raises
    for a matrix that is not MXFP4-valued)"""
    init()
    W = np.ascontiguousarray(W_bf16, np.uint16)
    xv = np.ascontiguousarray(x, np.float32)
    N, K = W.shape
    assert xv.ndim == 2 and xv.shape[1] == K
    nb = xv.shape[0]
    y = np.empty((nb, N), np.float32)
    if lib().vox_hip_skinny_wmx4(N, K, W.ctypes.data, fptr(xv), nb, fptr(y), int(fmt), int(bool(head))) != 0:
        _err("skinny_wmx4")
    return y


def set_gemmf_wait(ticks: int) -> int:
    """the encoder GEMM owner's wait per partial tile (100 MHz ticks; < 0: always recompute);
    returns the previous value (a diagnostic knob for the tests)"""
    return lib().vox_hip_set_gemmf_wait(int(ticks))


def set_gemmf_q8(on: bool):
    """k_gemmf over the int8 fragment copies of Q8 tensors, for models created from now on
    (vox_hip_set_gemmf_q8; off by default, VOX_HIP_GEMMF_Q8=1 gives the initial value)"""
    if lib().vox_hip_set_gemmf_q8(int(bool(on))) != 0:
        _err("set_gemmf_q8")


def gemmf_q8() -> int:
    return lib().vox_hip_gemmf_q8()


def gemmf_q8_rows(x, W_i8, scales, fmt: int) -> np.ndarray:
    """Test entry: y [M, N] = x [M, K] against the Q8 matrix (W int8 [N, K], scales f32 [N])
    through the plane writer and k_gemmf (vox_hip_gemmf_q8_rows).  fmt 1: the int8 fragment copy
    with the scales; fmt 0: the bf16 fragment copy of the same integers, unscaled"""
    init()
    W, sc, xv, N, K = _q8_args(W_i8, scales, x)
    assert xv.ndim == 2
    M = xv.shape[0]
    y = np.empty((M, N), np.float32)
    if lib().vox_hip_gemmf_q8_rows(M, N, K, fptr(xv), W.ctypes.data, fptr(sc), fptr(y), int(fmt)) != 0:
        _err("gemmf_q8_rows")
    return y


def set_adapter_rows0(rows: int):
    """vox_hip_set_adapter_rows0: the first adapter-buffer capacity (rows) of streams created from
    now on, a power of two in 16..1024; 0 restores the default of 1024.  Needs no device."""
    if lib().vox_hip_set_adapter_rows0(int(rows)) != 0:
        _err("set_adapter_rows0")


def init(device: int | None = None):
    L = lib()
    if device is not None and L.vox_hip_set_device(device) != 0:
        _err("set_device")
    if not L.vox_hip_init():
        _err("vox_hip_init (no GPU?)")


class Model:
    """vox_load (voxtral.c:131-383) for the HIP backend: weights uploaded once into HBM."""

    def __init__(self, cfg: VoxConfig, weights: Weights, delay_tokens: int = 6):
        init()
        self.cfg = cfg
        self.delay_tokens = delay_tokens
        self._cfg_c = cfg.ctypes_struct(ConfigC)
        wstruct, keep = build_weights_struct(weights, WeightsC)
        self.h = lib().vox_hip_model_create(ctypes.byref(self._cfg_c), ctypes.byref(wstruct), delay_tokens)
        if not self.h:
            _err("vox_hip_model_create")

    def set_delay(self, delay_ms: int):
        """vox_set_delay (voxtral.c:1681-1687)"""
        delay_ms = min(max(delay_ms, 80), 2400)
        self.delay_tokens = delay_ms // 80
        if lib().vox_hip_model_set_delay(self.h, self.delay_tokens) != 0:
            _err("set_delay")

    def set_kv_fp16(self, on: bool):
        """VOX_DECODER_KV_FP16 (voxtral.c:189-190): streams created afterwards keep their
        decoder K/V rings in IEEE half"""
        if lib().vox_hip_model_set_kv_fp16(self.h, int(on)) != 0:
            _err("set_kv_fp16")

    def set_kv_dtype(self, dtype: int):
        """vox_hip_model_set_kv_dtype: streams created afterwards keep their decoder K/V rings
        in f32 (KV_F32 = 0), IEEE half (KV_F16 = 1) or FP8 E4M3 (KV_FP8 = 2: no scale,
        saturating at 448, quality not evaluated)"""
        if lib().vox_hip_model_set_kv_dtype(self.h, int(dtype)) != 0:
            _err("set_kv_dtype")

    def set_enc_kv_fp16(self, on: bool):
        """vox_hip_model_set_enc_kv_fp16: streams created afterwards keep their encoder K/V rings
        in IEEE half (half the ring's bytes; f32 arithmetic; quality not evaluated)"""
        if lib().vox_hip_model_set_enc_kv_fp16(self.h, int(on)) != 0:
            _err("set_enc_kv_fp16")

    def set_enc_kv_dtype(self, dtype: int):
        """vox_hip_model_set_enc_kv_dtype: the encoder K/V ring element of streams created
        afterwards: 0 f32, 1 IEEE half, 2 FP8 E4M3 (a quarter of the f32 rings' bytes, no scale;
        f32 arithmetic; quality not evaluated)"""
        if lib().vox_hip_model_set_enc_kv_dtype(self.h, int(dtype)) != 0:
            _err("set_enc_kv_dtype")

    def set_kv_grow(self, slots0: int):
        """vox_hip_model_set_kv_grow: streams created afterwards start with decoder K/V rings of
        slots0 slots (clamped to [64, dec_window + 64]) that double as their position needs them,
        up to the full ring; lossless.  0: full rings from the start (the default)"""
        if lib().vox_hip_model_set_kv_grow(self.h, int(slots0)) != 0:
            _err("set_kv_grow")

    def wpack_stats(self) -> dict:
        """What the single-stream decode GEMV streams as wpack13 planes (13 bits per bf16
        weight, lossless) and what stayed raw: tensor counts, bytes, host packing time"""
        st = WPackStatsC()
        if lib().vox_hip_model_wpack_stats(self.h, ctypes.byref(st)) != 0:
            _err("wpack_stats")
        return {name: getattr(st, name) for name, _ in WPackStatsC._fields_}

    def wmx4_stats(self) -> dict:
        """What the single-stream decode GEMV streams as wmx4 planes (MXFP4, 5 stored bits per
        weight): tensors streamed and refused, bytes, bits per weight, host scan / round / pack ms"""
        st = WMx4StatsC()
        if lib().vox_hip_model_wmx4_stats(self.h, ctypes.byref(st)) != 0:
            _err("wmx4_stats")
        return {name: getattr(st, name) for name, _ in WMx4StatsC._fields_}

    def wmx4_batch_stats(self) -> dict:
        """The wmx4 fragment planes the batched step may stream (vox_hip_model_wmx4_batch_stats):
        tensors, plane bytes, the bf16 bytes they stand for, host microseconds"""
        out = (ctypes.c_longlong * 4)()
        if lib().vox_hip_model_wmx4_batch_stats(self.h, out) != 0:
            _err("wmx4_batch_stats")
        return dict(zip(("tensors", "plane_bytes", "bf16_bytes", "host_us"), (int(v) for v in out)))

    def gemmf_q8_stats(self) -> list:
        """vox_hip_model_gemmf_q8_stats: [the switch the model took, k_gemmf launches on int8
        fragments since creation (captured ones once at capture and once per replay), Q8 matrices
        k_gemmf accepts, Q8 matrices whose shape it refuses]"""
        out = (ctypes.c_longlong * 4)()
        if lib().vox_hip_model_gemmf_q8_stats(self.h, out) != 0:
            _err("gemmf_q8_stats")
        return [int(v) for v in out]

    def ada_scale(self):
        c = self.cfg
        out = np.empty(c.dec_layers * c.dec_dim, np.float32)
        lib().vox_hip_model_ada_scale(self.h, fptr(out))
        return out.reshape(c.dec_layers, c.dec_dim)

    def close(self):
        if self.h:
            lib().vox_hip_model_free(self.h)
            self.h = None


def encode_mel_batch(streams, mels):
    """vox_hip_stream_encode_mel_batch: each stream's new host mel frames, one encoder pass
    over all of their rows; returns the adapter rows added per stream."""
    n = len(streams)
    assert n == len(mels) and n > 0
    arrs = [np.ascontiguousarray(m, dtype=np.float32) for m in mels]
    for s, a in zip(streams, arrs):
        # the C side copies n * mel_bins floats per stream: shapes are checked here
        assert a.ndim == 2 and a.shape[1] == s.cfg.mel_bins, (a.shape, s.cfg.mel_bins)
        assert s.model is streams[0].model, "encode_mel_batch: streams of one model"
    hs = (ctypes.c_void_p * n)(*[s.h for s in streams])
    ps = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
    ns = np.array([a.shape[0] for a in arrs], np.int32)
    added = np.zeros(n, np.int32)
    if lib().vox_hip_stream_encode_mel_batch(hs, ps, ns.ctypes.data, n, 0, added.ctypes.data) != 0:
        _err("encode_mel_batch")
    return added.tolist()


class Stream:
    """Per-stream device state (rolling KV, conv tails, adapter buffer) + decode loop."""

    def __init__(self, model: Model):
        self.model = model
        self.cfg = model.cfg
        self.h = lib().vox_hip_stream_create(model.h)
        if not self.h:
            _err("vox_hip_stream_create")

    def reset(self):
        if lib().vox_hip_stream_reset(self.h) != 0:
            _err("reset")

    def set_delay(self, delay_tokens: int | None):
        """vox_hip_stream_set_delay: the stream's own delay in tokens (0..MAX_DELAY_TOKENS, 80 ms
        each); None or -1: follow the model (the default).  Refused once the decoder has started."""
        if lib().vox_hip_stream_set_delay(self.h, -1 if delay_tokens is None else int(delay_tokens)) != 0:
            _err("stream_set_delay")

    @property
    def delay_tokens(self) -> int:
        """the delay in effect: the stream's own, or the model's"""
        return lib().vox_hip_stream_delay(self.h)

    def ada_scale(self):
        """the stream's ada table (Model.ada_scale's twin)"""
        c = self.cfg
        out = np.empty(c.dec_layers * c.dec_dim, np.float32)
        if lib().vox_hip_stream_ada_scale(self.h, fptr(out)) != 0:
            _err("stream_ada_scale")
        return out.reshape(c.dec_layers, c.dec_dim)

    @property
    def kv_fp16(self) -> bool:
        return bool(lib().vox_hip_stream_kv_fp16(self.h))

    @property
    def kv_dtype(self) -> int:
        """the decoder KV ring element: KV_F32, KV_F16 or KV_FP8"""
        return lib().vox_hip_stream_kv_dtype(self.h)

    def read_kv(self, layer: int, first: int, n: int, decoded: bool = False):
        """vox_hip_stream_read_kv: the K and V ring elements of logical positions
        [first, first + n) of one decoder layer, [n, kv_heads * head_dim] each: raw (float32,
        float16 or uint8 codes by kv_dtype) or, decoded, widened to float32"""
        dt = KV_NP_DTYPE[self.kv_dtype]
        kvd = self.cfg.dec_kv_heads * self.cfg.dec_head_dim
        k, v = np.empty((n, kvd), dt), np.empty((n, kvd), dt)
        if lib().vox_hip_stream_read_kv(self.h, int(layer), int(first), int(n), k.ctypes.data, v.ctypes.data) != 0:
            _err("read_kv")
        if not decoded:
            return k, v
        if dt is np.uint8:
            return kv8_decode(k), kv8_decode(v)
        return k.astype(np.float32), v.astype(np.float32)

    @property
    def kv_slots(self) -> int:
        """slots of the decoder K/V rings now (dec_window + 64 unless Model.set_kv_grow)"""
        return lib().vox_hip_stream_kv_slots(self.h)

    @property
    def kv_bytes(self) -> int:
        """bytes of the stream's decoder K and V rings together"""
        return int(lib().vox_hip_stream_kv_bytes(self.h))

    def kv_grow_stats(self) -> dict:
        """vox_hip_stream_kv_grow_stats: growths of the decoder rings, bytes copied, slots now"""
        out = (ctypes.c_longlong * 3)()
        if lib().vox_hip_stream_kv_grow_stats(self.h, out) != 0:
            _err("kv_grow_stats")
        return dict(zip(("grows", "copied", "slots"), (int(v) for v in out)))

    def reserve_kv(self, positions: int):
        """vox_hip_stream_reserve_kv: grow the decoder rings ahead of time to hold `positions`
        positions (the full ring at most); raises when they cannot be allocated or the stream is
        held by a begun batched call"""
        if lib().vox_hip_stream_reserve_kv(self.h, int(positions)) != 0:
            _err("reserve_kv")

    @property
    def enc_kv_fp16(self) -> bool:
        """True when the stream's encoder K/V rings hold IEEE half (Model.set_enc_kv_fp16)"""
        return bool(lib().vox_hip_stream_enc_kv_fp16(self.h))

    @property
    def enc_kv_dtype(self) -> int:
        """the stream's encoder K/V ring element: 0 f32, 1 IEEE half, 2 FP8 E4M3 (Model.set_enc_kv_dtype)"""
        return int(lib().vox_hip_stream_enc_kv_dtype(self.h))

    @property
    def enc_kv_bytes(self) -> int:
        """bytes of the stream's encoder K and V rings together"""
        return int(lib().vox_hip_stream_enc_kv_bytes(self.h))

    def enc_paths(self) -> dict:
        """vox_hip_stream_enc_paths: this stream's encoder passes by the path they took"""
        out = (ctypes.c_longlong * 5)()
        if lib().vox_hip_stream_enc_paths(self.h, out) != 0:
            _err("enc_paths")
        return dict(zip(("gemv_row", "fused", "slab", "rows", "fused_split"), (int(v) for v in out)))

    def read_enc_kv(self, layer: int, first: int, n: int, decoded: bool = False):
        """vox_hip_stream_read_enc_kv: the K and V ring elements of logical encoder positions
        [first, first + n) of one encoder layer, [n, enc_kv_heads * enc_head_dim] each: raw
        (float32, float16 on a half stream, uint8 E4M3 codes on an FP8 stream) or, decoded,
        widened to float32 (exactly: kv8_decode for the codes)"""
        dt = KV_NP_DTYPE[self.enc_kv_dtype]
        kvd = self.cfg.enc_kv_heads * self.cfg.enc_head_dim
        k, v = np.empty((n, kvd), dt), np.empty((n, kvd), dt)
        if lib().vox_hip_stream_read_enc_kv(self.h, int(layer), int(first), int(n), k.ctypes.data, v.ctypes.data) != 0:
            _err("read_enc_kv")
        if not decoded:
            return k, v
        if dt is np.uint8:
            return kv8_decode(k), kv8_decode(v)
        return k.astype(np.float32), v.astype(np.float32)

    def encode_mel(self, mel: np.ndarray) -> int:
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        assert mel.ndim == 2 and mel.shape[1] == self.cfg.mel_bins
        n = lib().vox_hip_stream_encode_mel(self.h, mel.ctypes.data, mel.shape[0], 0)
        if n < 0:
            _err("encode_mel")
        return n

    def encode_mel_device(self, dev_ptr: int, n_frames: int) -> int:
        n = lib().vox_hip_stream_encode_mel(self.h, ctypes.c_void_p(dev_ptr), n_frames, 1)
        if n < 0:
            _err("encode_mel")
        return n

    def set_async_encode(self, on: bool):
        """encode_mel returns once the pass is enqueued (vox_hip_stream_set_async_encode);
        host mel arrays must outlive the next sync()."""
        if lib().vox_hip_stream_set_async_encode(self.h, int(on)) != 0:
            _err("set_async_encode")

    def sync(self):
        if lib().vox_hip_stream_sync(self.h) != 0:
            _err("sync")

    @property
    def adapter_tokens(self) -> int:
        return lib().vox_hip_stream_adapter_tokens(self.h)

    def adapter_stats(self) -> dict:
        """vox_hip_stream_adapter_stats: the adapter buffer's capacity in rows, its growths, and
        those of them that happened inside a begun, unfinished batched call"""
        out = (ctypes.c_longlong * 3)()
        if lib().vox_hip_stream_adapter_stats(self.h, out) != 0:
            _err("adapter_stats")
        return dict(zip(("cap", "grows", "grows_held"), (int(v) for v in out)))

    def read_adapter(self, first: int = 0, n: int | None = None) -> np.ndarray:
        if n is None:
            n = self.adapter_tokens - first
        out = np.empty((n, self.cfg.dec_dim), np.float32)
        if n and lib().vox_hip_stream_read_adapter(self.h, first, n, fptr(out)) != 0:
            _err("read_adapter")
        return out

    def decode(self, max_steps: int = 1 << 30, stop_at_eos: bool = True, want_logits: bool = False):
        max_steps = min(max_steps, 1 << 20)
        cap = min(max_steps, max(self.adapter_tokens + 1, 1))
        toks = np.zeros(cap, np.int32)
        logits = np.zeros((cap, self.cfg.vocab), np.float32) if want_logits else None
        n = lib().vox_hip_stream_decode(self.h, cap, int(stop_at_eos),
                                        toks.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                        fptr(logits) if want_logits else None)
        if n < 0:
            _err("decode")
        return (toks[:n], logits[:n]) if want_logits else toks[:n]

    def state(self):
        o = np.zeros(6, np.int32)
        lib().vox_hip_stream_state(self.h, o.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        return dict(zip(["kv_pos", "gen_pos", "prev_token", "started", "eos_seen", "generated"], o.tolist()))

    def set_alt(self, n_alt: int, cutoff: float):
        """vox_stream_set_alt: keep up to n_alt candidates per step (1 = off)."""
        if lib().vox_hip_stream_set_alt(self.h, n_alt, cutoff) != 0:
            _err("set_alt")

    def read_alts(self, first: int, n: int):
        """(ids [n, 4] with -1 for none, probs [n, 4]) for generated steps [first, first+n)."""
        ids = np.empty((n, 4), np.int32)
        pr = np.empty((n, 4), np.float32)
        if lib().vox_hip_stream_read_alts(self.h, first, n, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                          fptr(pr)) != 0:
            _err("read_alts")
        return ids, pr

    # ---- reference-boundary twins on this stream's device state (host arrays in / out;
    # the calls INTEGRATION.md sections 4-5 bind into voxtral_encoder.c / voxtral_decoder.c)
    def twin_encoder_full_step(self, x: np.ndarray, rope: np.ndarray, logical_start: int) -> np.ndarray:
        """vox_metal_encoder_full_step twin: all encoder layers + final norm on x [n, enc_dim]
        (a copy is returned), K/V appended at logical positions logical_start.."""
        x = np.array(x, np.float32, copy=True, order="C")
        rope = np.ascontiguousarray(rope, np.float32)
        if lib().vox_hip_encoder_full_step(self.h, fptr(x), x.shape[0], fptr(rope), logical_start) != 0:
            _err("encoder_full_step")
        return x

    def twin_decoder_prefill_step(self, x: np.ndarray, rope: np.ndarray, logical_start: int) -> np.ndarray:
        """vox_metal_decoder_prefill_step twin: decoder layers on x [n, dec_dim], KV written."""
        x = np.array(x, np.float32, copy=True, order="C")
        rope = np.ascontiguousarray(rope, np.float32)
        if lib().vox_hip_decoder_prefill_step(self.h, fptr(x), x.shape[0], fptr(rope), logical_start) != 0:
            _err("decoder_prefill_step")
        return x

    def twin_decoder_step(self, x: np.ndarray, rope_row: np.ndarray, logical_pos: int, want_logits=True):
        """decoder_start + decoder_full_step + decoder_end, as voxtral_decoder.c:686-699
        drives the Metal twins: returns (token, logits or None)."""
        x = np.ascontiguousarray(x, np.float32)
        rope_row = np.ascontiguousarray(rope_row, np.float32)
        L = lib()
        L.vox_hip_clear_error()
        L.vox_hip_decoder_start(self.h, fptr(x), x.shape[-1])
        if L.vox_hip_last_error():
            _err("decoder_start")
        logits = np.empty(self.cfg.vocab, np.float32) if want_logits else None
        tok = L.vox_hip_decoder_full_step(self.h, fptr(rope_row), logical_pos,
                                          fptr(logits) if want_logits else None)
        L.vox_hip_decoder_end(self.h)
        if tok < 0:
            _err("decoder_full_step")
        return tok, logits

    def set_profiling(self, on: bool):
        lib().vox_hip_stream_set_profiling(self.h, int(on))

    def profile(self):
        o = (ctypes.c_double * 8)()
        lib().vox_hip_stream_profile(self.h, o)
        # kind 0: the events bracket the W1|W3 GEMV of every layer
        return {"ms": o[0], "bytes": o[1], "launches": int(o[2]), "avg_ms": o[3], "kind": int(o[4]),
                "bytes_per_launch": o[5], "gemmf_recomputes": int(o[6])}

    def sync(self):
        lib().vox_hip_stream_sync(self.h)

    def close(self):
        if self.h:
            lib().vox_hip_stream_free(self.h)
            self.h = None


class Session:
    """vox_stream_t's chunk scheduling over log-mel input (voxtral.c:827-851, 1242-1316,
    1640-1667).  The caller supplies the mel frames produced so far (vox_mel_feed /
    vox_mel_finish output); the session decides when the encoder runs and drains the
    decoder, exactly as stream_run_encoder / stream_run_decoder do."""

    def __init__(self, stream: Stream, interval_s: float = STREAM_DEFAULT_INTERVAL):
        self.s = stream
        self.mel_cursor = 0
        self.conv_started = False
        self.finished = False
        self.min_new_mel = max(1, int(interval_s * 100.0))
        self.tokens: list[int] = []
        self.chunks: list[int] = []

    def _run_encoder(self, mel_all, min_new: int):
        """stream_run_encoder's chunk decision (voxtral.c:827-851); mel_all is the host
        frame array so far, or a device Mel (frames stay in HBM, discarded once encoded)."""
        dev = isinstance(mel_all, Mel)
        total = mel_all.total if dev else mel_all.shape[0]
        if dev:
            self.mel_cursor = max(self.mel_cursor, mel_all.offset)
        new = total - self.mel_cursor
        need = STREAM_FIRST_CHUNK_MIN_MEL if not self.conv_started else min_new
        if new < need and not self.finished:
            return
        if new <= 0:
            return
        self.chunks.append(new)
        if dev:
            self.s.encode_mel_device(mel_all.ptr(self.mel_cursor), new)
        else:
            self.s.encode_mel(mel_all[self.mel_cursor:total])
        self.conv_started = True
        self.mel_cursor = total
        if dev:
            mel_all.discard_before(self.mel_cursor)

    def _run_decoder(self, stop_at_eos=True):
        self.tokens += self.s.decode(stop_at_eos=stop_at_eos).tolist()

    def feed(self, mel_all: np.ndarray, stop_at_eos=True):
        """vox_stream_feed after vox_mel_feed produced mel_all (all frames so far)."""
        self._run_encoder(mel_all, self.min_new_mel)
        self._run_decoder(stop_at_eos)

    def flush(self, mel_all: np.ndarray, stop_at_eos=True):
        """vox_stream_flush (mel_all includes the right-pad frames)."""
        self._run_encoder(mel_all, 1)
        self._run_decoder(stop_at_eos)

    def finish(self, mel_all: np.ndarray, stop_at_eos=True):
        """vox_stream_finish's final pass after vox_mel_finish."""
        self.finished = True
        self._run_encoder(mel_all, self.min_new_mel)
        self._run_decoder(stop_at_eos)


class Mel:
    """Incremental log-mel on the device (vox_mel_ctx_t twin, voxtral_audio.c:405-671):
    samples in, frames kept in HBM for encode_mel_device.  Frame indices are global."""

    def __init__(self, stream: Stream, left_pad_samples: int = 32 * 1280):
        self.h = lib().vox_hip_mel_create(stream.h, left_pad_samples)
        if not self.h:
            _err("vox_hip_mel_create")

    def feed(self, samples: np.ndarray) -> int:
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        n = lib().vox_hip_mel_feed(self.h, fptr(samples), samples.shape[0])
        if n < 0:
            _err("mel_feed")
        return n

    def finish(self, right_pad: int = 0) -> int:
        n = lib().vox_hip_mel_finish(self.h, right_pad)
        if n < 0:
            _err("mel_finish")
        return n

    @property
    def offset(self) -> int:
        off = ctypes.c_int(0)
        lib().vox_hip_mel_frames(self.h, ctypes.byref(off))
        return off.value

    @property
    def total(self) -> int:
        off = ctypes.c_int(0)
        n = lib().vox_hip_mel_frames(self.h, ctypes.byref(off))
        return off.value + n

    def ptr(self, frame: int) -> int:
        p = lib().vox_hip_mel_frame_ptr(self.h, frame)
        if not p:
            _err("mel_frame_ptr")
        return p

    def discard_before(self, frame: int):
        if lib().vox_hip_mel_discard_before(self.h, frame) != 0:
            _err("mel_discard_before")

    def read(self, first: int, n: int) -> np.ndarray:
        out = np.empty((n, 128), np.float32)
        if n and lib().vox_hip_mel_read(self.h, first, n, fptr(out)) != 0:
            _err("mel_read")
        return out

    def close(self):
        if self.h:
            lib().vox_hip_mel_free(self.h)
            self.h = None


class AudioSession(Session):
    """vox_stream_feed / vox_stream_flush / vox_stream_finish (voxtral.c:1288-1316,
    1640-1667) over raw 16 kHz samples: the log-mel is computed on the device (Mel) and
    encoded from HBM, so only the samples cross PCIe."""

    def __init__(self, stream: Stream, interval_s: float = STREAM_DEFAULT_INTERVAL):
        super().__init__(stream, interval_s)
        self.mel = Mel(stream, 32 * RAW_AUDIO_LENGTH_PER_TOK)
        self.real_samples = 0
        # the stream itself: a caller may put a wrapper with the encode / decode calls in self.s
        # (bench.py --streaming times them that way), and the right pad needs the stream's delay
        self.stream = stream

    def feed_samples(self, samples: np.ndarray, stop_at_eos=True):
        self.mel.feed(samples)
        self.real_samples += int(samples.shape[0])
        self.feed(self.mel, stop_at_eos)

    def flush_samples(self, stop_at_eos=True):
        pad = right_pad_samples(self.real_samples, self.stream.delay_tokens)
        self.mel.feed(np.zeros(pad, np.float32))
        self.flush(self.mel, stop_at_eos)

    def finish_samples(self, stop_at_eos=True):
        self.flush_samples(stop_at_eos)
        self.mel.finish(0)
        self.finish(self.mel, stop_at_eos)

    def close(self):
        self.mel.close()


def right_pad_samples(n_real_samples: int, delay_tokens: int) -> int:
    """vox_stream_flush padding (voxtral.c:1645-1649)."""
    align = (RAW_AUDIO_LENGTH_PER_TOK - (n_real_samples % RAW_AUDIO_LENGTH_PER_TOK)) % RAW_AUDIO_LENGTH_PER_TOK
    return align + ((delay_tokens + 1) + OFFLINE_STREAMING_BUFFER_TOKENS) * RAW_AUDIO_LENGTH_PER_TOK


class DeviceArray:
    """A host array copied once into HBM (inputs resident before a timed region)."""

    def __init__(self, a: np.ndarray):
        a = np.ascontiguousarray(a)
        self.shape, self.dtype = a.shape, a.dtype
        self.ptr = lib().vox_hip_device_upload(a.ctypes.data, a.nbytes)
        if not self.ptr:
            _err("device_upload")

    def free(self):
        if self.ptr:
            lib().vox_hip_device_free(self.ptr)
            self.ptr = None


# ---------------------------------------------------------------------------
# reference-boundary twins (voxtral_metal.h), host arrays in / out
# ---------------------------------------------------------------------------
BATCH_MAX_SLOTS = 128   # VOX_HIP_BATCH_MAX_SLOTS (voxtral_hip.h)
SCHED_MAX = 128         # VH_SCHED_MAX (vox_hip_host.h)


class Batch:
    """Cross-stream batched greedy decoding (C4): one weight read per step for all streams.

    max_streams: 1..BATCH_MAX_SLOTS (128).  Calls with up to 32 streams run the skinny MFMA step
    (or the opt-in R-row GEMV step, which the set_gemv_* / set_wmx4 switches act on); calls with
    33..128 streams run the wide k_gemmf step over the bf16 fragment-major copies.  Decoder KV
    rings at 128 streams: ~225 GB f32, ~113 GB half, ~56 GB FP8 (Model.set_kv_dtype) as full rings;
    with Model.set_kv_grow they follow each session's length instead (~28 GB f32 one minute in).
    Streams of any ring capacities share a call (kv_grow_stats counts the ragged steps)."""

    def __init__(self, model: "Model", max_streams: int):
        if not 1 <= int(max_streams) <= BATCH_MAX_SLOTS:
            raise ValueError(f"Batch: max_streams must be 1..{BATCH_MAX_SLOTS}")
        self.h = lib().vox_hip_batch_create(model.h, max_streams)
        if not self.h:
            _err("vox_hip_batch_create")

    def decode(self, streams, max_steps: int, stop_at_eos: bool = True, rows=None):
        """Returns one int32 token array per stream.  rows: each stream reads only its first
        rows[i] adapter rows (vox_hip_batch_decode_rows; the streams' queues are not waited for)."""
        n = len(streams)
        arr = (ctypes.c_void_p * n)(*[s.h for s in streams])
        toks = np.zeros((n, max(1, max_steps)), np.int32)
        cnt = np.zeros(n, np.int32)
        tp = toks.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        cp = cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        if rows is None:
            r = lib().vox_hip_batch_decode(self.h, arr, n, max_steps, int(stop_at_eos), tp, cp)
        else:
            rw = np.ascontiguousarray(rows, np.int32)
            assert rw.shape == (n,), "one row bound per stream"
            r = lib().vox_hip_batch_decode_rows(self.h, arr, n, rw.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                max_steps, int(stop_at_eos), tp, cp)
        if r < 0:
            _err("vox_hip_batch_decode")
        return [toks[i, :cnt[i]].copy() for i in range(n)]

    def read_logits(self, stream: "Stream") -> np.ndarray:
        """logits of the last batched step for a stream that step advanced"""
        out = np.empty(stream.cfg.vocab, np.float32)
        if lib().vox_hip_batch_read_logits(self.h, stream.h, fptr(out)) != 0:
            _err("vox_hip_batch_read_logits")
        return out

    def stats(self) -> dict:
        """vox_hip_batch_stats: counters since creation"""
        out = (ctypes.c_longlong * 6)()
        if lib().vox_hip_batch_stats(self.h, out) != 0:
            _err("vox_hip_batch_stats")
        keys = ("calls", "replays", "rows", "captures", "prefill_passes", "prefilled")
        return dict(zip(keys, (int(v) for v in out)))

    def kv_grow_stats(self) -> dict:
        """vox_hip_batch_kv_grow_stats: calls with a decoder ring shorter than the full size
        (Model.set_kv_grow), their step replays and step-graph captures"""
        out = (ctypes.c_longlong * 3)()
        if lib().vox_hip_batch_kv_grow_stats(self.h, out) != 0:
            _err("vox_hip_batch_kv_grow_stats")
        return dict(zip(("ragged_calls", "ragged_replays", "ragged_captures"), (int(v) for v in out)))

    def set_gemv_rows(self, max_rows: int) -> int:
        """vox_hip_batch_set_gemv_rows: steps of up to max_rows slots (0, 1, 2, 4, 8) take the
        R-row GEMV step.  Returns 0, or -1 with last_error() set (another value, a Q8 model, a
        begun call)."""
        return lib().vox_hip_batch_set_gemv_rows(self.h, int(max_rows))

    def set_gemv_rows_q8(self, max_rows: int) -> int:
        """vox_hip_batch_set_gemv_rows_q8: the same switch for a model with Q8 step tensors (the
        step streams their int8 rows).  Returns 0, or -1 with last_error() set (another value, a
        model with no Q8 step tensor, a begun call)."""
        return lib().vox_hip_batch_set_gemv_rows_q8(self.h, int(max_rows))

    def set_wmx4(self, on: bool) -> int:
        """vox_hip_batch_set_wmx4: the MFMA step streams the wmx4 fragment planes (on) or the bf16
        fragment copies (off); the same bits.  Returns 0, or -1 with last_error() set (the model
        has no fragment planes, a begun call)."""
        return lib().vox_hip_batch_set_wmx4(self.h, int(bool(on)))

    def set_gemv_wmx4(self, on: bool) -> int:
        """vox_hip_batch_set_gemv_wmx4: the R-row GEMV step streams the wmx4 GEMV plane of every
        tensor that has one (on) or the wpack13 planes / raw rows (off); same bits.  0, or -1
        (vox_hip.last_error()) when the model has no wmx4 GEMV plane or inside a begun call."""
        return lib().vox_hip_batch_set_gemv_wmx4(self.h, int(bool(on)))

    def set_prefill_kv(self, on: bool) -> int:
        """vox_hip_batch_set_prefill_kv: joining streams with half or FP8 decoder KV rings are
        prefilled in the stacked passes on the batch queue (on, the default) or one by one on
        their own queues (off); f32 streams ignore it.  0, or -1 (vox_hip.last_error()) inside a
        begun call."""
        return lib().vox_hip_batch_set_prefill_kv(self.h, int(bool(on)))

    def gemv_wmx4_stats(self) -> tuple:
        """vox_hip_batch_gemv_wmx4_stats: (flag, GEMV step replays on wmx4 planes, step tensors
        with a wmx4 GEMV plane, step tensors without)"""
        out = (ctypes.c_longlong * 4)()
        if lib().vox_hip_batch_gemv_wmx4_stats(self.h, out) != 0:
            _err("vox_hip_batch_gemv_wmx4_stats")
        return tuple(int(v) for v in out)

    def gemv_stats(self) -> tuple:
        """vox_hip_batch_gemv_stats: (max_rows, GEMV step replays, live rows, GEMV captures)"""
        out = (ctypes.c_longlong * 4)()
        if lib().vox_hip_batch_gemv_stats(self.h, out) != 0:
            _err("vox_hip_batch_gemv_stats")
        return tuple(int(v) for v in out)

    def close(self):
        if self.h:
            lib().vox_hip_batch_free(self.h)
            self.h = None


def _void_call(what, fn, *args):
    """The reference-boundary twins return void (voxtral_metal.h); a failure is reported
    through vox_hip_last_error(), cleared before the call."""
    L = lib()
    L.vox_hip_clear_error()
    fn(*args)
    msg = L.vox_hip_last_error()
    if msg:
        raise RuntimeError(f"{what}: {msg.decode()}")


def sgemm_bf16(A: np.ndarray, B_bf16: np.ndarray) -> np.ndarray:
    """C = A @ B^T (vox_metal_sgemm_bf16 twin); B is cached on the device by host pointer
    and shape, so keep it alive and unmodified."""
    A = np.ascontiguousarray(A, np.float32)
    B_bf16 = np.ascontiguousarray(B_bf16, np.uint16)
    M, K = A.shape
    N = B_bf16.shape[0]
    assert B_bf16.shape[1] == K
    C = np.empty((M, N), np.float32)
    _void_call("sgemm_bf16", lib().vox_hip_sgemm_bf16, M, N, K, fptr(A), B_bf16.ctypes.data, fptr(C))
    return C


def sgemm_q8(A: np.ndarray, B_q8: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """C = A @ (scales[:, None] * B_q8)^T (vox_metal_sgemm_q8 twin); B/scales are cached
    on the device by host pointer, so keep them alive and unmodified."""
    A = np.ascontiguousarray(A, np.float32)
    M, K = A.shape
    N = B_q8.shape[0]
    C = np.empty((M, N), np.float32)
    _void_call("sgemm_q8", lib().vox_hip_sgemm_q8, M, N, K, fptr(A), B_q8.ctypes.data, fptr(scales), fptr(C))
    return C


def fused_qkv_bf16(x: np.ndarray, wq: np.ndarray, wk: np.ndarray, wv: np.ndarray):
    """vox_metal_fused_qkv_bf16 twin: (x wq^T, x wk^T, x wv^T), biases left to the caller."""
    x = np.ascontiguousarray(x, np.float32)
    M, K = x.shape
    outs = [np.empty((M, w.shape[0]), np.float32) for w in (wq, wk, wv)]
    _void_call("fused_qkv_bf16", lib().vox_hip_fused_qkv_bf16, M, K, fptr(x), wq.ctypes.data, wq.shape[0],
               wk.ctypes.data, wk.shape[0], wv.ctypes.data, wv.shape[0], *[fptr(o) for o in outs])
    return tuple(outs)


def fused_ffn_bf16(x: np.ndarray, w1: np.ndarray, w3: np.ndarray, w2: np.ndarray) -> np.ndarray:
    """vox_metal_fused_ffn_bf16 twin: (silu(x w1^T) * x w3^T) w2^T, w2 bias left to the caller."""
    x = np.ascontiguousarray(x, np.float32)
    M, dim = x.shape
    hidden = w1.shape[0]
    out = np.empty((M, dim), np.float32)
    _void_call("fused_ffn_bf16", lib().vox_hip_fused_ffn_bf16, M, dim, hidden, fptr(x), w1.ctypes.data,
               w3.ctypes.data, w2.ctypes.data, fptr(out))
    return out


def encoder_attention(Q, K, V, n_heads, n_kv_heads, head_dim, window, q_offset):
    Q, K, V = (np.ascontiguousarray(x, np.float32) for x in (Q, K, V))
    out = np.empty_like(Q)
    _void_call("encoder_attention", lib().vox_hip_encoder_attention, fptr(out), fptr(Q), fptr(K), fptr(V),
               Q.shape[0], K.shape[0], n_heads, n_kv_heads, head_dim, float(1.0 / np.sqrt(head_dim)),
               window, q_offset)
    return out


# ---------------------------------------------------------------------------
# the C host side (include/vox_hip_host.h, libvox_hip_host.so): vh_stream_* and the per-GPU
# stream scheduler, over a model this process created
# ---------------------------------------------------------------------------
HOST_LIB_PATH = os.path.join(_HERE, "libvox_hip_host.so")
_host = None


class SchedStats(ctypes.Structure):
    _fields_ = [("runs", ctypes.c_int), ("prefills", ctypes.c_int), ("batch_calls", ctypes.c_int),
                ("tokens", ctypes.c_longlong), ("run_ms", ctypes.c_double), ("batch_ms", ctypes.c_double),
                ("enc_batches", ctypes.c_int), ("steps", ctypes.c_longlong), ("captures", ctypes.c_longlong),
                ("prefill_passes", ctypes.c_longlong), ("enc_ms", ctypes.c_double)]


def host_lib():
    global _host
    if _host is not None:
        return _host
    lib()  # the C ABI library first (the host library links it)
    if not os.path.exists(HOST_LIB_PATH):
        raise RuntimeError(f"{HOST_LIB_PATH} not built (run __graft_entry__.build())")
    H = ctypes.CDLL(HOST_LIB_PATH)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    ip = ctypes.POINTER(ctypes.c_int)
    sig = {
        "vh_ctx_wrap": (P, [P, P, I]), "vh_free": (None, [P]), "vh_last_error": (ctypes.c_char_p, []),
        "vh_stream_init": (P, [P]), "vh_stream_free": (None, [P]), "vh_stream_reset": (I, [P]),
        "vh_set_processing_interval": (None, [P, F]), "vh_stream_set_continuous": (None, [P, I]),
        "vh_stream_feed": (I, [P, ctypes.POINTER(ctypes.c_float), I]), "vh_stream_flush": (I, [P]),
        "vh_stream_finish": (I, [P]), "vh_stream_get": (I, [P, ip, I]),
        "vh_stream_get_alt": (I, [P, ip, I]), "vh_stream_set_alt": (I, [P, I, F]),
        "vh_sched_create": (P, [P, I]), "vh_sched_free": (None, [P]), "vh_sched_attach": (I, [P, P]),
        "vh_sched_detach": (I, [P, P]), "vh_sched_run": (I, [P]),
        "vh_sched_stats": (None, [P, ctypes.POINTER(SchedStats)]),
        "vh_sched_set_step_cap": (None, [P, I]), "vh_stream_pending": (I, [P]),
        "vh_stream_set_delay": (I, [P, I]), "vh_stream_delay_ms": (I, [P]),
        "vh_set_enc_kv_fp16": (I, [P, I]), "vh_stream_enc_kv_fp16": (I, [P]),
        "vh_set_enc_kv_dtype": (I, [P, I]), "vh_stream_enc_kv_dtype": (I, [P]),
        "vh_set_kv_grow": (I, [P, I]), "vh_stream_kv_slots": (I, [P]),
        "vh_sched_debug_fail_next_encode": (None, [P]),
        "vh_stream_adapter_stats": (I, [P, ctypes.POINTER(ctypes.c_longlong)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(H, name)
        fn.restype = res
        fn.argtypes = args
    _host = H
    return H


def _herr(what):
    msg = host_lib().vh_last_error()
    raise RuntimeError(f"{what}: {msg.decode() if msg else 'unknown error'}")


class HostCtx:
    """vh_ctx_t over a Model of this process (vh_ctx_wrap: the model stays the Model's)."""

    def __init__(self, model: Model):
        self.model = model
        self.h = host_lib().vh_ctx_wrap(model.h, ctypes.byref(model._cfg_c), model.delay_tokens)
        if not self.h:
            _herr("vh_ctx_wrap")

    def set_kv_grow(self, slots0: int):
        """vh_set_kv_grow: streams initialised afterwards start with decoder rings of slots0 slots"""
        if host_lib().vh_set_kv_grow(self.h, int(slots0)) != 0:
            _herr("vh_set_kv_grow")

    def set_enc_kv_dtype(self, dtype: int):
        """vh_set_enc_kv_dtype: the encoder K/V ring element of streams initialised afterwards
        (0 f32, 1 IEEE half, 2 FP8 E4M3)"""
        if host_lib().vh_set_enc_kv_dtype(self.h, int(dtype)) != 0:
            _herr("vh_set_enc_kv_dtype")

    def close(self):
        if self.h:
            host_lib().vh_free(self.h)
            self.h = None


class HostStream:
    """vh_stream_t: vox_stream_feed / flush / finish / get of the C host (voxtral.c:1242-1327)."""

    def __init__(self, ctx: HostCtx, interval_s: float = STREAM_DEFAULT_INTERVAL, continuous: bool = False):
        H = host_lib()
        self.h = H.vh_stream_init(ctx.h)
        if not self.h:
            _herr("vh_stream_init")
        H.vh_set_processing_interval(self.h, interval_s)
        H.vh_stream_set_continuous(self.h, int(continuous))

    def feed(self, samples: np.ndarray):
        samples = np.ascontiguousarray(samples, np.float32)
        if host_lib().vh_stream_feed(self.h, fptr(samples), samples.shape[0]) != 0:
            _herr("vh_stream_feed")

    def flush(self):
        if host_lib().vh_stream_flush(self.h) != 0:
            _herr("vh_stream_flush")

    def finish(self):
        if host_lib().vh_stream_finish(self.h) != 0:
            _herr("vh_stream_finish")

    def reset(self):
        """vh_stream_reset: new audio on this (detached) stream, its buffers and settings kept"""
        if host_lib().vh_stream_reset(self.h) != 0:
            _herr("vh_stream_reset")

    def set_delay(self, delay_ms: int):
        """vh_stream_set_delay: this stream's own delay (clamped to 80..2400 ms, 80 ms per token)"""
        if host_lib().vh_stream_set_delay(self.h, int(delay_ms)) != 0:
            _herr("vh_stream_set_delay")

    def delay_ms(self) -> int:
        return host_lib().vh_stream_delay_ms(self.h)

    def get(self) -> list[int]:
        out, buf = [], np.empty(4096, np.int32)
        while True:
            n = host_lib().vh_stream_get(self.h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 4096)
            out += buf[:n].tolist()
            if n < 4096:
                return out

    def set_alt(self, n_alt: int, cutoff: float):
        """vox_stream_set_alt (voxtral.c:1329-1337)"""
        if host_lib().vh_stream_set_alt(self.h, n_alt, cutoff) != 0:
            _herr("vh_stream_set_alt")

    def pending(self) -> int:
        """adapter rows not decoded yet (vh_stream_pending)"""
        return host_lib().vh_stream_pending(self.h)

    def kv_slots(self) -> int:
        """vh_stream_kv_slots: slots of the decoder K/V rings of the stream behind this one"""
        return host_lib().vh_stream_kv_slots(self.h)

    def adapter_stats(self) -> dict:
        """vh_stream_adapter_stats: as Stream.adapter_stats, for the stream behind this one"""
        out = (ctypes.c_longlong * 3)()
        if host_lib().vh_stream_adapter_stats(self.h, out) != 0:
            _herr("vh_stream_adapter_stats")
        return dict(zip(("cap", "grows", "grows_held"), (int(v) for v in out)))

    def get_alt(self) -> np.ndarray:
        """queued records [n, 4]: the chosen id, then the accepted alternatives, -1 padded"""
        out, buf = [], np.empty((1024, 4), np.int32)
        while True:
            n = host_lib().vh_stream_get_alt(self.h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1024)
            out.append(buf[:n].copy())
            if n < 1024:
                return np.concatenate(out)

    def close(self):
        if self.h:
            host_lib().vh_stream_free(self.h)
            self.h = None


class Scheduler:
    """vh_sched_t: up to 128 HostStreams (VH_SCHED_MAX) of one model on this GPU; run() decodes every
    attached stream's pending adapter rows with batched greedy steps (more than 32 streams with
    rows: the wide step; their deferred chunks are encoded in groups of 32)."""

    def __init__(self, ctx: HostCtx, max_streams: int):
        self.h = host_lib().vh_sched_create(ctx.h, max_streams)
        if not self.h:
            _herr("vh_sched_create")

    def attach(self, s: HostStream):
        if host_lib().vh_sched_attach(self.h, s.h) != 0:
            _herr("vh_sched_attach")

    def detach(self, s: HostStream):
        if host_lib().vh_sched_detach(self.h, s.h) != 0:
            _herr("vh_sched_detach")

    def run(self) -> int:
        n = host_lib().vh_sched_run(self.h)
        if n < 0:
            _herr("vh_sched_run")
        return n

    def set_step_cap(self, cap: int):
        """vh_sched_set_step_cap: at most `cap` steps per stream and run (0: drain every run)"""
        host_lib().vh_sched_set_step_cap(self.h, int(cap))

    def fail_next_encode(self):
        """vh_sched_debug_fail_next_encode (test hook): the next run's encoder pass returns an
        error before it enqueues anything, so that run() raises after finishing its steps"""
        host_lib().vh_sched_debug_fail_next_encode(self.h)

    def stats(self) -> dict:
        st = SchedStats()
        host_lib().vh_sched_stats(self.h, ctypes.byref(st))
        return {f: getattr(st, f) for f, _ in SchedStats._fields_}

    def close(self):
        if self.h:
            host_lib().vh_sched_free(self.h)
            self.h = None
