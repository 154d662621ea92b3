/*
 * voxtral_hip.h -- C ABI of the MI355X (gfx950 / CDNA4) backend for voxtral.c.
 *
 * This header is the drop-in boundary.  It replaces the reference's Metal backend
 * interface (voxtral_metal.h, SeungheonOh/voxtral.c @ 2026-02-20); every entry point
 * below cites the reference declaration it replaces.  Signatures use plain pointers and
 * sizes only.  All functions are synchronous with respect to host pointers they are
 * given, like the Metal backend (voxtral_metal.m waits on every command buffer).
 *
 * Differences from voxtral_metal.h that the discrete-GPU design forces (see
 * INTEGRATION.md for the call-site patch):
 *   - the Metal backend read weights and KV state out of the reference's vox_ctx_t via
 *     `void *ctx` (voxtral_metal.m:2888-3174).  Here weights are handed over once as a
 *     table of host pointers (vox_hip_weights_t, filled from vox_ctx_t at vox_load) and
 *     per-stream device state lives in an opaque vox_hip_stream_t;
 *   - the decoder/encoder KV caches live in HBM as rolling buffers indexed by LOGICAL
 *     position (slot = pos mod capacity), so the host-side memmove compaction of
 *     voxtral_decoder.c:354-384 / voxtral_encoder.c:431-449 becomes unnecessary.  The
 *     step functions therefore take the logical start position instead of the physical
 *     cache length.  Attention semantics are unchanged: the last `window` logical
 *     positions are visible (identical to the CPU path after compaction).
 *
 * Errors: functions returning int return a negative value on failure (the reference's
 * step functions return -1 to request the CPU fallback; this backend never falls back
 * silently -- a failure is reported and the caller decides).
 */
#ifndef VOXTRAL_HIP_H
#define VOXTRAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * Runtime (voxtral_metal.h:20-26)
 * ------------------------------------------------------------------------ */
int vox_hip_init(void);          /* voxtral_metal.h:20  vox_metal_init: 1 on success */
int vox_hip_available(void);     /* voxtral_metal.h:23  vox_metal_available */
void vox_hip_shutdown(void);     /* voxtral_metal.h:26  vox_metal_shutdown */
size_t vox_hip_memory_used(void);/* voxtral_metal.h:282 vox_metal_memory_used */
const char *vox_hip_last_error(void);  /* "" when no error since the last clear */
void vox_hip_clear_error(void);          /* the void twins below report only through last_error */
int vox_hip_set_device(int device);

/* ------------------------------------------------------------------------
 * Model dimensions (voxtral.h:18-50 are compile-time #defines in the reference;
 * here they are a runtime record so test configurations can shrink the model).
 * ------------------------------------------------------------------------ */
typedef struct {
    int enc_dim, enc_layers, enc_heads, enc_kv_heads, enc_head_dim, enc_hidden, enc_window;
    int dec_dim, dec_layers, dec_heads, dec_kv_heads, dec_head_dim, dec_hidden, dec_window;
    int vocab, mel_bins, downsample, ada_dim;
    float rope_theta, enc_eps, dec_eps;
    int gelu_erf; /* 0: tanh GELU (voxtral_kernels.c:505-513), the default */
} vox_hip_config_t;

void vox_hip_config_voxtral_4b(vox_hip_config_t *cfg); /* voxtral.h:26-50 values */

/* Weight table: host pointers, exactly the views vox_ctx_t holds after vox_load
 * (voxtral.h:56-239): bf16 matrices straight off the safetensors mmap, small tensors
 * already converted to f32.  Per-layer tensors are arrays of `layers` pointers. */
typedef struct {
    const float *conv0_w, *conv0_b, *conv1_w, *conv1_b;
    const uint16_t **enc_wq, **enc_wk, **enc_wv, **enc_wo, **enc_w1, **enc_w2, **enc_w3;
    const float **enc_wq_b, **enc_wv_b, **enc_wo_b, **enc_w2_b, **enc_attn_norm, **enc_ffn_norm;
    const float *enc_norm;
    const uint16_t *ad0, *ad1;
    const uint16_t *tok_emb;
    const uint16_t **dec_wq, **dec_wk, **dec_wv, **dec_wo, **dec_w1, **dec_w2, **dec_w3;
    const float **dec_attn_norm, **dec_ffn_norm, **dec_ada_down, **dec_ada_up;
    const float *dec_norm;
    /* Q8 checkpoints (quantize.py output; voxtral_safetensors.c:393-408, 457-468).  A
     * non-NULL per-row scale array (safetensors_get_q8_scales_direct) selects int8 for that
     * matrix, whose pointer above then carries safetensors_get_q8_data_direct, cast
     * (int8 [out, in]).  Q/K/V of a layer and its w1/w3 must agree.  ada_down/up and the
     * conv weights stay f32 (load_f32 dequantises / quantize.py keeps 3-D tensors f32).
     * Leave all NULL (zero-initialise the struct) for a bf16 checkpoint. */
    const float **enc_wq_s, **enc_wk_s, **enc_wv_s, **enc_wo_s, **enc_w1_s, **enc_w2_s, **enc_w3_s;
    const float *ad0_s, *ad1_s, *tok_emb_s;
    const float **dec_wq_s, **dec_wk_s, **dec_wv_s, **dec_wo_s, **dec_w1_s, **dec_w2_s, **dec_w3_s;
} vox_hip_weights_t;

typedef struct vox_hip_model vox_hip_model_t;
typedef struct vox_hip_stream vox_hip_stream_t;

/* Upload + pack all weights into HBM once (replaces the Metal warm-up and weight
 * caches, voxtral.c:186-284 / voxtral_metal.m:133-501: QKV and W1|W3 are merged here).
 * delay_tokens sets the time conditioning (voxtral.c:47-80). */
vox_hip_model_t *vox_hip_model_create(const vox_hip_config_t *cfg, const vox_hip_weights_t *w,
                                      int delay_tokens);
void vox_hip_model_free(vox_hip_model_t *m);
/* vox_set_delay (voxtral.c:1681-1687): recompute ada_scale and re-upload it (the Metal
 * backend's pointer-keyed f32 cache went stale here, voxtral_metal.m:471-501). */
int vox_hip_model_set_delay(vox_hip_model_t *m, int delay_tokens);
/* ada_scale [dec_layers*dec_dim] as computed on the host (for tests). */
int vox_hip_model_ada_scale(vox_hip_model_t *m, float *out);
/* The reference's fp16 decoder KV cache (VOX_DECODER_KV_FP16, voxtral.c:189-190, the Metal
 * default; voxtral_decoder.c:180-243 allocates the dual-format cache): streams created after
 * this call keep their decoder K/V rings in IEEE half (stores round to nearest even, all
 * attention arithmetic f32), halving the ring's HBM bytes per decode step.  Opt-in here: off
 * unless VOX_DECODER_KV_FP16 is set nonzero at model creation or on = 1 is passed; the
 * default f32 ring is the CPU reference's (voxtral_decoder.c:232-234).  head_dim 128 only
 * (Voxtral's); returns 0, or -1 (vox_hip_last_error) for another head_dim. */
int vox_hip_model_set_kv_fp16(vox_hip_model_t *m, int on);
/* The decoder KV ring element of streams created after this call: 0 f32 (the default), 1 IEEE
 * half (what vox_hip_model_set_kv_fp16(m, 1) selects), 2 FP8 E4M3 (no reference counterpart).
 * FP8: one byte per element, OCP "e4m3fn" (the gfx950 native format) by the rule of
 * csrc/vox_kv8.h -- stores clamp to +-448 (the ring saturates; there is NO scale, a per-layer
 * power-of-two scale needs a real checkpoint to calibrate against and is not built), round to
 * nearest with ties to even, keep subnormals; loads widen exactly; all attention arithmetic
 * stays f32 in the f32 ring's order.  A quarter of the f32 ring's bytes per step and per
 * stream.  Its effect on transcripts is NOT evaluated.  Opt-in: off unless VOX_HIP_KV_FP8 is
 * set nonzero at model creation (it wins over VOX_DECODER_KV_FP16) or dtype = 2 is passed.
 * The encoder KV is not touched by this call (vox_hip_model_set_enc_kv_fp16).  Every decoder
 * path honours the element type, the batch's stacked
 * prefill of joining streams included (vox_hip_batch_set_prefill_kv).  head_dim 128 only for 1
 * and 2; returns 0, or -1 (vox_hip_last_error) for another head_dim or dtype. */
int vox_hip_model_set_kv_dtype(vox_hip_model_t *m, int dtype);
/* The encoder's K/V rings (no reference counterpart: the reference's VOX_DECODER_KV_FP16 is
 * decoder-only): streams created after this call with on = 1 keep their encoder rings in IEEE
 * half -- stores round with the decoder ring's rule (nearest even, overflow to infinity), loads
 * widen to f32, the windowed attention keeps its f32 MFMA, f32 queries and the f32 ring's
 * accumulation order.  Half the ring's bytes: (enc_window + 1088) slots x 32 layers x 2048
 * columns x K and V = 0.96 GB per stream as f32, 0.48 GB as half; 123 / 62 GB at 128 streams.
 * Its effect on transcripts is NOT evaluated.  Opt-in: off unless VOX_HIP_ENC_KV_FP16 is set
 * nonzero at model creation or on = 1 is passed.  Every encoder path honours the stream's type
 * (one-row GEMV, the skinny chains, the long passes, the batched pass, vox_hip_encoder_full_step).
 * (FP8 encoder rings: vox_hip_model_set_enc_kv_dtype.)  head_dim 64 only (Voxtral's encoder); returns 0, or -1
 * (vox_hip_last_error) for another head_dim. */
int vox_hip_model_set_enc_kv_fp16(vox_hip_model_t *m, int on);
/* The encoder ring element of the streams created after this call (no reference counterpart):
 * dtype 0 f32 (default), 1 IEEE half (what vox_hip_model_set_enc_kv_fp16(m, 1) selects), 2 FP8
 * E4M3 bytes by the decoder ring's rule (csrc/vox_kv8.h): no scale, each store clamps to +-448
 * in f32 and rounds to nearest even, NaN is 0x7f | sign; loads widen exactly, the windowed
 * attention keeps its f32 MFMA, f32 queries and the f32 ring's accumulation order.  A quarter
 * of the f32 rings' bytes: 0.24 GB per stream, 31 GB at 128 streams.  Its effect on transcripts
 * is NOT evaluated.  Opt-in: off unless VOX_HIP_ENC_KV_FP8 is set nonzero at model creation (it
 * wins over VOX_HIP_ENC_KV_FP16; ignored unless the encoder's head_dim is 64) or dtype = 2 is
 * passed.  Every encoder path honours the stream's type, and one batched call or scheduler
 * serves streams of all three.  head_dim 64 only for 1 and 2; returns 0, or -1
 * (vox_hip_last_error) for another head_dim or dtype. */
int vox_hip_model_set_enc_kv_dtype(vox_hip_model_t *m, int dtype);
/* Decoder K/V rings that grow with the stream (no reference counterpart; lossless).  A stream
 * created after this call with slots0 > 0 starts with decoder rings of slots0 slots (clamped to
 * [64, dec_window + 64]; 64 holds the longest prompt) in its own element type instead of the
 * full dec_window + 64.  Before any call appends decoder positions the rings are made to hold
 * min(dec_window + 64, the last position the call can reach + 1): the new capacity is the
 * smallest slots0 * 2^k that does, capped at the full size, and each layer's first rows are
 * copied into the longer buffer (a ring below the full size has not wrapped: slot = position).
 * Stored values, arithmetic and tokens are those of a full ring; a ring that reached the full
 * size is the full ring.  A growth that cannot be allocated fails its call (< 0,
 * vox_hip_last_error names the growth) before anything is enqueued, the stream intact at its
 * old capacity.  vox_hip_stream_reset returns the rings to slots0, vox_hip_stream_reset_decoder
 * keeps their capacity; vox_hip_memory_used follows both.  One decoder position is 80 ms of
 * audio: 2 x dec_layers x slots x kv_heads x head_dim x element bytes per stream, e.g. 0.22 GB
 * as f32 after one minute (1024 slots) against 1.76 GB.  Batched calls take streams of any
 * capacities together (vox_hip_batch_kv_grow_stats).  A single stream below 256 slots runs
 * the general decode attention where a full ring runs the short-context kernel (same values,
 * another summation order).  slots0 = 0 (the default): full rings from the start, nothing
 * changes.  VOX_HIP_KV_GROW=<slots> gives the initial value.  Returns 0, or -1 for slots0 < 0. */
int vox_hip_model_set_kv_grow(vox_hip_model_t *m, int slots0);
/* wpack13 (no reference counterpart): at creation every bf16 matrix of the single-stream
 * decode step (Q|K|V, wo, W1|W3, W2 per decoder layer, and the LM head) whose nonzero
 * exponents span at most 30 binades also gets a 13-bit-per-weight copy that the M = 1 GEMV
 * streams instead (0.8125 of the bytes, decoded without loss: same bits out).  The others,
 * and every tensor when VOX_HIP_WPACK=0 is set at creation or the model is Q8, stay raw. */
typedef struct {
    int packed_tensors;         /* tensors the decode GEMV streams from wpack13 planes */
    int raw_tensors;            /* bf16 tensors of the same set that stayed raw */
    long long packed_bytes;     /* bytes of the planes (main + side) */
    long long packed_raw_bytes; /* bf16 bytes of the packed tensors (the raw copies kept) */
    long long raw_bytes;        /* bf16 bytes of the tensors that stayed raw */
    double pack_ms;             /* host time spent scanning, packing and uploading the planes */
} vox_hip_wpack_stats_t;
int vox_hip_model_wpack_stats(const vox_hip_model_t *m, vox_hip_wpack_stats_t *out);
/* Test entry: y[rows] = W x for one bf16 matrix W [rows, K] (host pointers) through the
 * M = 1 GEMV, from wpack13 planes (packed = 1), from the wmx4 plane (packed = 2) or from the
 * raw rows.  Returns 1 when the wpack13 kernel ran, 2 when the wmx4 kernel ran, 0 when the raw
 * one did (packed = 0, W outside the wpack13 window, or W refused by the wmx4 scan), -1 on
 * error. */
int vox_hip_gemv_wpack(int rows, int K, const uint16_t *W, const float *x, float *y, int packed);
/* wmx4 (no reference counterpart; opt-in): MXFP4 weight streaming for the single-stream decode
 * GEMVs, 5 stored bits per weight.
 *
 * Format.  A block is 32 consecutive k of one row: 32 e2m1 values ({0, 0.5, 1, 1.5, 2, 3, 4, 6}
 * with a sign) times one scale 2^e, e = floor(log2(amax)) - 2 for the block's largest
 * magnitude amax, stored as the e8m0 byte e + 127 (127 for an all-zero block).  Every such
 * weight is exactly a bf16, so an MXFP4-valued model is an ordinary bf16 model: the kernel
 * rebuilds the same f32 weight (v_cvt_scalef32_pk_f32_fp4) and runs the bf16 kernel's FMAs in
 * the same order -- bit-identical outputs on the same (rounded) weights.
 * Rounding rule (the only lossy step; on the host, never in a kernel): v / 2^e to the nearest
 * e2m1 value, ties to the even mantissa, saturating at +-6; the sign of zero is kept;
 * idempotent.  What this rounding does to transcription quality has not been evaluated.
 * Exponent window: a tensor is streamed as wmx4 only when K % 32 == 0, it holds no Inf, NaN
 * or subnormal, every block is representable under its own e, and every |e| <= 64: scales
 * and weights are then normal f32 in [2^-65, 1.5 * 2^66] (csrc/vox_wmx4.h).
 *
 * Mode (process-wide, read at vox_hip_model_create; VOX_HIP_WMX4 gives the initial value):
 *   0 (default)  nothing changes: no scan, no planes, every path and statistic as without it.
 *   1 (detect)   each bf16 matrix of the single-stream decode step (Q|K|V, wo, W1|W3, W2 per
 *                decoder layer, and the LM head) that passes the scan also gets a wmx4 plane,
 *                which the M = 1 GEMV streams in preference to wpack13 or raw.  A tensor that
 *                fails the scan is treated exactly as in mode 0.
 *   2 (round)    the host first rounds those matrices (tok_emb included, as LM head and as
 *                embedding table) by the rule above; the rounded values feed every upload
 *                (raw rows, fragment-major copies, wpack13, wmx4), so prefill, the batched
 *                steps and the single-stream step see one model.  Then as mode 1.
 * Q8 tensors ignore the mode; VOX_HIP_WPACK=0 still streams raw bf16 everywhere.  The wpack13
 * or raw copies are kept for the paths that need them, so vox_hip_model_wpack_stats reports
 * what it reports in mode 0 (on the same weights).
 * vox_hip_set_wmx4 returns 0, or -1 for another mode. */
int vox_hip_set_wmx4(int mode);
int vox_hip_wmx4(void);
typedef struct {
    int wmx4_tensors;        /* tensors the decode GEMV streams from wmx4 planes */
    int refused_tensors;     /* tensors scanned and refused (not MXFP4-valued, window, shape) */
    long long plane_bytes;   /* bytes of the wmx4 planes */
    long long bf16_bytes;    /* bf16 bytes of the tensors they stand for */
    double bits_per_weight;  /* plane_bytes * 8 / weights (0 when there are none) */
    double scan_ms;          /* host time: scanning, */
    double round_ms;         /* rounding (mode 2), */
    double pack_ms;          /* packing, laying out and uploading the planes */
} vox_hip_wmx4_stats_t;
int vox_hip_model_wmx4_stats(const vox_hip_model_t *m, vox_hip_wmx4_stats_t *out);
/* wmx4 for the batched MFMA step (opt-in on top of wmx4 mode 1 or 2; process-wide, read at
 * vox_hip_model_create; VOX_HIP_WMX4_BATCH=1 gives the initial value).  When on, every bf16
 * decoder matrix that gets a wmx4 GEMV plane (Q|K|V, wo, W1|W3, W2 per layer, the LM head) also
 * gets a wmx4 fragment plane (csrc/vox_wmx4.h: 4.5 stored bits per weight, in the MFMA A
 * operand's order), built on the host from the same nibbles and scales.  The batched step's
 * projections and LM head then stream that plane instead of the 16-bit fragment-major copy
 * and form the very bf16 fragments in registers (v_cvt_scalef32_pk_bf16_fp4): same waves,
 * splits, slabs and summation order, so the step's logits and ids are bit-identical to the
 * step on the bf16 copies.  A tensor the scan refuses keeps only its bf16 copy; Q8 models and
 * VOX_HIP_WPACK=0 build nothing; the bf16 fragment copies stay (prefill reads them).  Off
 * (default), or wmx4 mode 0: nothing changes.  Prefill, the encoder and the single-stream step
 * are untouched; the R-row GEMV step has a switch of its own (vox_hip_batch_set_gemv_wmx4: it
 * streams the wmx4 GEMV planes, not these fragment planes).  What MXFP4 rounding does to transcription quality
 * has not been evaluated.
 * vox_hip_set_wmx4_batch returns 0. */
int vox_hip_set_wmx4_batch(int on);
int vox_hip_wmx4_batch(void);
/* out4: [0] tensors with a fragment plane, [1] bytes of the planes, [2] bf16 bytes of the
 * tensors they stand for, [3] host microseconds spent laying them out and uploading them. */
int vox_hip_model_wmx4_batch_stats(const vox_hip_model_t *m, long long out4[4]);
/* Test entry: nb (1..32) rows x [nb][K] against one bf16 matrix W [N][K] (host pointers)
 * through the batched step's own launchers: the rows are split into planes by the step's plane
 * writer; head = 0 runs the projection launcher (k_skl up to 16 rows, k_skl2 from 17) and sums
 * its split-K slabs in slab order into y [nb][N]; head = 1 runs the LM-head launcher (k_skf)
 * into y.  fmt = 0 streams the bf16 fragment-major copy, fmt = 1 the wmx4 fragment plane.
 * Returns 0; -1 (vox_hip_last_error) on a bad shape, or with fmt = 1 for a matrix the wmx4 scan
 * refuses. */
int vox_hip_skinny_wmx4(int N, int K, const uint16_t *W, const float *x, int nb, float *y, int fmt, int head);
/* Arithmetic of the M > 1 GEMMs (encoder, adapter, prefill; no reference counterpart: the
 * CPU path's cblas_sgemm, voxtral_kernels.c:197-240, is f32): every f32 activation is split
 * into bf16 planes that multiply the exact bf16 weights on MFMA.  planes = 3 (hi + mid + lo,
 * the default) reproduces the f32 activation exactly (only the summation order differs from
 * sgemm); planes = 2 (or VOX_HIP_GEMM_PLANES=2) keeps ~2^-18 of it and issues 2/3 of the
 * MFMAs (measured against the 5e-5 parity bar in tests/test_gpu_gemm_planes.py).
 * Process-wide; returns 0, or -1 for another value. */
int vox_hip_set_gemm_planes(int planes);
int vox_hip_gemm_planes(void);
/* Diagnostic (no reference counterpart): the encoder GEMM's stream-K owner waits up to
 * `ticks` (100 MHz) for each later part of a tile before computing that stage range itself
 * (same code and order: same bits); ticks < 0 never waits, so the tests can force that
 * backstop.  Default 5000 (50 us).  Process-wide; returns the previous value. */
int vox_hip_set_gemmf_wait(int ticks);
/* Opt-in (no reference counterpart): the stream-K MFMA GEMM (k_gemmf) over the int8
 * fragment-major copies of Q8 tensors, for models created from now on.  Off (the default), a
 * model with a Q8 tensor in the encoder or decoder layers runs its M > 1 passes on the row-major
 * GEMM: nothing changes.  On, such a model takes the k_gemmf paths of a bf16 model -- the
 * encoder's long passes and the batched encoder pass, the single-stream and the stacked decoder
 * prefill at every KV ring type, and the wide batched step (33..128 streams) with its LM head
 * and step graphs -- each launch streaming its own tensor's copy: int8 blocks (half the bytes
 * of the bf16 copy) with the tensor's row scales, or the bf16 copy of a tensor that is not Q8.
 * The adapter and conv GEMMs stay on the row-major GEMM, and VOX_HIP_GEMMF=0 /
 * VOX_HIP_PREFILL_GEMMF=0 keep their meaning.  Exact: int8 -> bf16, and with three planes every
 * product; each finished f32 sum is multiplied once by its weight row's f32 scale, before bias,
 * residual, GELU or SwiGLU (the scale * sum rule of the other Q8 kernels).  Against the
 * row-major GEMM only the f32 summation order differs; against the bf16 k_gemmf instance of the
 * same tile the accumulators are the same bits.  VOX_HIP_GEMMF_Q8=1 gives the initial value.
 * vox_hip_set_gemmf_q8 returns 0. */
int vox_hip_set_gemmf_q8(int on);
int vox_hip_gemmf_q8(void);
/* out4: [0] the switch the model took at creation, [1] k_gemmf launches issued on int8
 * fragments for this model since creation (a launch captured into a wide step graph counts
 * once at capture and once more at every replay of that graph), [2] Q8 matrices whose shape
 * k_gemmf accepts (their int8 fragment copy is what it streams; merged Q|K|V and W1|W3 count
 * once each, the LM head once), [3] Q8 matrices whose shape it refuses (N % 128 or K % 64). */
int vox_hip_model_gemmf_q8_stats(const vox_hip_model_t *m, long long out4[4]);
/* Test entry: y[M][N] = x[M][K] against one Q8 matrix (Wq int8 [N][K], scales [N]; host
 * pointers) through the engine's plane writer and k_gemmf's launcher with the STORE epilogue,
 * no bias, at the process's plane count.  fmt = 1 streams the int8 fragment copy and applies
 * `scales`; fmt = 0 streams the bf16 fragment copy of the same integers through the bf16
 * instance of the same tile configuration and applies no scale (`scales` may be null), so
 * fmt 1 == f32(fmt 0) * scales[n], bit for bit.  Returns 0; -1 (vox_hip_last_error) for a shape
 * k_gemmf refuses (M 1..1024, N % 128 == 0, K % 64 == 0). */
int vox_hip_gemmf_q8_rows(int M, int N, int K, const float *x, const int8_t *Wq, const float *scales, float *y,
                          int fmt);

/* Per-stream device state: encoder/decoder rolling KV, conv-stem tails, adapter buffer,
 * scratch and a HIP stream.  One model serves many streams. */
vox_hip_stream_t *vox_hip_stream_create(vox_hip_model_t *m);
void vox_hip_stream_free(vox_hip_stream_t *s);
/* 1 if the stream's decoder KV rings hold IEEE half (vox_hip_model_set_kv_fp16), else 0 */
int vox_hip_stream_kv_fp16(const vox_hip_stream_t *s);
/* the stream's decoder KV ring element: 0 f32, 1 IEEE half, 2 FP8 E4M3 (vox_hip_model_set_kv_dtype) */
int vox_hip_stream_kv_dtype(const vox_hip_stream_t *s);
/* 1 if the stream's encoder KV rings hold IEEE half (vox_hip_model_set_enc_kv_fp16), else 0 */
int vox_hip_stream_enc_kv_fp16(const vox_hip_stream_t *s);
/* the stream's encoder KV ring element: 0 f32, 1 IEEE half, 2 FP8 E4M3 (vox_hip_model_set_enc_kv_dtype) */
int vox_hip_stream_enc_kv_dtype(const vox_hip_stream_t *s);
/* Tests / diagnostics: the stream's own encoder passes since creation, by the path they took:
 * out5[0] one-row GEMV passes, [1] fused skinny chains (k_sklx), [2] slab skinny chains,
 * [3] M > 1 rows passes (GEMM), [4] fused-chain passes whose attention took a split key grid and
 * the combine kernel.  Passes of a batched call that stacks several streams are not counted. */
int vox_hip_stream_enc_paths(const vox_hip_stream_t *s, long long out5[5]);
/* bytes of the stream's encoder K and V rings together (all layers) */
long long vox_hip_stream_enc_kv_bytes(const vox_hip_stream_t *s);
/* slots of the stream's decoder K/V rings now (dec_window + 64 unless vox_hip_model_set_kv_grow) */
int vox_hip_stream_kv_slots(const vox_hip_stream_t *s);
/* bytes of the stream's decoder K and V rings together (all layers) */
long long vox_hip_stream_kv_bytes(const vox_hip_stream_t *s);
/* out3: [0] growths of the stream's decoder rings since creation, [1] bytes their copies moved,
 * [2] slots now */
int vox_hip_stream_kv_grow_stats(const vox_hip_stream_t *s, long long out3[3]);
/* Grow ahead: the stream's decoder rings hold `positions` positions (the full ring at most) from
 * now on, so the calls up to that position grow nothing; a server's admission test (-1 when the
 * rings cannot be allocated, the stream unchanged).  A stream with full rings: 0, nothing done.
 * Refused for a stream held by a begun batched call. */
int vox_hip_stream_reserve_kv(vox_hip_stream_t *s, int positions);
/* Tests / diagnostics: the raw ring elements of decoder layer `layer` at logical positions
 * [first_logical_pos, first_logical_pos + n), [n][dec_kv_heads * dec_head_dim] in the stream's
 * element type (4, 2 or 1 bytes each) to k_out / v_out (either may be null).  Waits for the
 * stream's queue.  -1 (vox_hip_last_error) for positions not appended yet or already
 * overwritten by the ring's wrap. */
int vox_hip_stream_read_kv(vox_hip_stream_t *s, int layer, int first_logical_pos, int n, void *k_out, void *v_out);
/* Tests / diagnostics: the encoder twin of vox_hip_stream_read_kv -- the raw ring elements of
 * encoder layer `layer` at logical encoder positions [first_logical_pos, first_logical_pos + n),
 * [n][enc_kv_heads * enc_head_dim] in the stream's element type (4, 2 or 1 bytes each) to k_out /
 * v_out (either may be null).  Waits for the stream's queue.  -1 (vox_hip_last_error) for
 * positions beyond the rows encoded so far or already overwritten by the ring's wrap. */
int vox_hip_stream_read_enc_kv(vox_hip_stream_t *s, int layer, int first_logical_pos, int n, void *k_out, void *v_out);
/* Tests: the kernels' own FP8 ring store and load helpers run on the device over x[0..n):
 * codes[i] = the byte a ring slot would hold, back[i] = the f32 the attention kernels read from
 * it (either may be null).  Must equal csrc/vox_kv8.h for every input. */
int vox_hip_kv8_convert(const float *x, int n, uint8_t *codes, float *back);
/* stream_reset_full_state (voxtral.c:786-814) / stream_reset_decoder_state (:766-783) */
int vox_hip_stream_reset(vox_hip_stream_t *s);
int vox_hip_stream_reset_decoder(vox_hip_stream_t *s);
/* A stream's own transcription delay, so streams of one model (one copy of the weights, one batch,
 * one scheduler) serve clients at different latencies.  delay_tokens 0..VOX_HIP_MAX_DELAY_TOKENS
 * (80 ms per token; 30 is the host's 2400 ms clamp), or -1: follow the model (the default: the
 * model's delay and table are read at every use, as before).  The delay sets the stream's prompt
 * length (1 + 32 + delay_tokens) and the ada table of its FFN norms; the model keeps one table per
 * delay, built on first use by vox_hip_model_set_delay's host arithmetic (bit-equal to it) and
 * kept at one address until vox_hip_model_free.  Refused (-1, vox_hip_last_error) outside that
 * range and once the stream's decoder has started; allowed again after vox_hip_stream_reset /
 * _reset_decoder, which keep the stream's delay.  Drops the stream's own step graphs.
 * A batched call (vox_hip_batch_decode and kin) in which no stream has a delay of its own is a
 * plain call and runs exactly what it ran before.  Any other call is mixed: its steps take per-slot
 * instances of the FFN norm kernels (same products in the same order, the ada row fetched through
 * the slot table) with step graphs of their own, its new streams are prefilled in one stacked pass
 * per distinct delay, and it never takes the R-row GEMV step (below).  Transcript quality at each
 * delay is the model's property; it is not evaluated on synthetic weights. */
#define VOX_HIP_MAX_DELAY_TOKENS 30
int vox_hip_stream_set_delay(vox_hip_stream_t *s, int delay_tokens);
/* the delay in effect, in tokens (the stream's own, or the model's) */
int vox_hip_stream_delay(const vox_hip_stream_t *s);
/* the stream's ada table [dec_layers*dec_dim] as computed on the host (vox_hip_model_ada_scale's twin) */
int vox_hip_stream_ada_scale(vox_hip_stream_t *s, float *out);

/* ------------------------------------------------------------------------
 * Device-resident streaming pipeline (the fast path).  Inputs are log-mel frames
 * [n, mel_bins] as produced by vox_mel_feed/vox_mel_finish (voxtral_audio.c:560-633).
 * ------------------------------------------------------------------------ */
/* stream_run_encoder body (voxtral.c:845-951): incremental conv stem (voxtral.c:581-759),
 * 32-layer encoder with rolling KV (voxtral_encoder.c:495-693), 4x downsample with the
 * leftover-row residual, adapter (voxtral_encoder.c:699-737); adapter rows stay in HBM.
 * mel is a host pointer (mel_on_device=0) or a device pointer (1).
 * Returns the number of adapter tokens appended, <0 on error. */
int vox_hip_stream_encode_mel(vox_hip_stream_t *s, const float *mel, int n_frames,
                              int mel_on_device);
int vox_hip_stream_adapter_tokens(vox_hip_stream_t *s);
/* The adapter buffer of a stream starts at 1024 rows (about 82 s of audio) and doubles when an
 * encoder pass needs more: a larger buffer is allocated, the rows are copied, the stream's step
 * graphs are captured again on the new address.  vox_hip_set_adapter_rows0 sets the first
 * capacity of streams created from now on, process-wide: a power of two in 16..1024, or 0 for
 * the default of 1024 (for tests, which reach a growth within seconds of audio; the rows and ids
 * do not depend on it).  Host state only, callable without a device.  Returns 0; -1
 * (vox_hip_last_error) for any other value, which leaves the setting as it was.
 * vox_hip_stream_adapter_stats: out3[0] the stream's capacity in rows, [1] its growths so far,
 * [2] those of them that happened while the stream was listed in a begun, unfinished batched
 * call (vox_hip_batch_begin_rows below), where the outgrown buffer outlives the call. */
int vox_hip_set_adapter_rows0(int rows);
int vox_hip_stream_adapter_stats(const vox_hip_stream_t *s, long long out3[3]);
/* on != 0: vox_hip_stream_encode_mel returns once the pass is enqueued on the stream's HIP
 * queue (its adapter-row count is known on the host); everything later on the same stream
 * (decode, read_adapter, reset) is ordered behind it and the batched step waits for every
 * member stream, so a scheduler can have several streams' encoder chunks in flight at once.
 * Host mel pointers must stay valid until vox_hip_stream_sync.  Default 0 (synchronous). */
int vox_hip_stream_set_async_encode(vox_hip_stream_t *s, int on);
/* stream_run_encoder for B streams at once: each stream's conv stem on its own queue, the
 * stacked new rows of all of them through the 32 encoder layers in one pass (projections
 * over all rows: every weight byte read once for the batch; RoPE, K/V append and attention
 * per stream against its own ring), then each stream's downsample + adapter.  The same
 * results as B vox_hip_stream_encode_mel calls up to summation order.  added[b] = adapter
 * rows appended to stream b.  Synchronous unless every stream is in async-encode mode.
 * Returns 0, <0 on error. */
int vox_hip_stream_encode_mel_batch(vox_hip_stream_t *const *streams, const float *const *mels,
                                    const int *n_frames, int B, int mel_on_device, int *added);

/* Incremental log-mel on the device: a vox_mel_ctx_t
 * (voxtral_audio.c:405-671) whose padded sample buffer and frames live in HBM, computed on
 * the stream's HIP queue ahead of the encoder (one block per frame: Hann window, direct
 * 201 x 400 DFT, Slaney filters, log10 clamp).  Frame indices are global, as in the
 * reference (vox_mel_frame_offset + position); a frame's device pointer feeds
 * vox_hip_stream_encode_mel(..., mel_on_device = 1) directly. */
typedef struct vox_hip_mel vox_hip_mel_t;
/* vox_mel_ctx_init (voxtral_audio.c:515-558): 200 + left_pad_samples zeros of padding */
vox_hip_mel_t *vox_hip_mel_create(vox_hip_stream_t *s, int left_pad_samples);
/* vox_mel_feed (voxtral_audio.c:560-582): returns the frames added, <0 on error */
int vox_hip_mel_feed(vox_hip_mel_t *m, const float *samples, int n_samples);
/* vox_mel_finish (voxtral_audio.c:584-633): right_pad zeros, 200-sample reflect, last frame
 * dropped; returns the live frame count */
int vox_hip_mel_finish(vox_hip_mel_t *m, int right_pad_samples);
/* vox_mel_data's count and vox_mel_frame_offset (voxtral_audio.c:635-643) */
int vox_hip_mel_frames(const vox_hip_mel_t *m, int *frame_offset);
/* device pointer of global frame f (frame_offset <= f <= frame_offset + frames) */
const float *vox_hip_mel_frame_ptr(const vox_hip_mel_t *m, int global_frame);
/* vox_mel_discard_before (voxtral_audio.c:645-662) */
int vox_hip_mel_discard_before(vox_hip_mel_t *m, int keep_from_frame);
/* copy live frames [first, first + n) to the host (tests) */
int vox_hip_mel_read(vox_hip_mel_t *m, int global_first, int n, float *out);
/* vox_mel_free (voxtral_audio.c:664-671) */
void vox_hip_mel_free(vox_hip_mel_t *m);
/* The state vox_hip_mel_create leaves (200 + left_pad_samples zeros, no frames), keeping the
 * context's device tables and buffers: a reused stream's new audio (vh_stream_reset). */
int vox_hip_mel_reset(vox_hip_mel_t *m, int left_pad_samples);
/* Copy adapter rows [first, first+n) to host (tests). */
int vox_hip_stream_read_adapter(vox_hip_stream_t *s, int first, int n, float *out);

/* stream_run_decoder (voxtral.c:1013-1145), non-continuous part: prefill when enough
 * adapter tokens exist (prompt BOS + STREAMING_PAD x (32+delay)), then greedy steps
 * while adapter tokens remain.  Generates at most max_steps tokens; stop_at_eos stops
 * after token 2 (EOS).  tokens_out receives the ids; logits_out (may be NULL) receives
 * [n, vocab] logits.  Returns the number of tokens generated (<0 on error). */
int vox_hip_stream_decode(vox_hip_stream_t *s, int max_steps, int stop_at_eos,
                          int *tokens_out, float *logits_out);
/* Alternative tokens (--alt, voxtral.h:294-304).  vox_stream_set_alt (voxtral.c:1329-1337):
 * n_alt clamped to 1..VOX_HIP_MAX_ALT, cutoff to [0,1]; n_alt > 1 makes every later step
 * also keep the softmax candidates of stream_fill_alts (voxtral.c:955-1010) on the device
 * (no logits download).  read_alts returns, for generated steps [first, first+n), the
 * chosen id and the accepted alternatives ([n][VOX_HIP_MAX_ALT], -1 = none) and optionally
 * their probabilities.  Callers apply it to text tokens only, as the reference does. */
#define VOX_HIP_MAX_ALT 4
int vox_hip_stream_set_alt(vox_hip_stream_t *s, int n_alt, float cutoff);
int vox_hip_stream_read_alts(vox_hip_stream_t *s, int first, int n, int *ids_out, float *probs_out);
/* Cross-stream batched greedy decoding (C4; the reference decodes each
 * vox_stream_t separately, voxtral.c:1105-1145).  A batch object holds scratch for up to
 * max_streams (1..VOX_HIP_BATCH_MAX_SLOTS = 128) streams of one model; its slot-indexed buffers
 * are sized for 32, 64 or 128 rows, whichever first holds max_streams (a batch of <= 32
 * allocates what it always did).  Calls with up to 32 streams run the skinny MFMA step (two
 * 16-row blocks; or the opt-in R-row GEMV step); calls with 33..64 and 65..128 streams run the
 * wide step: the stacked prefill's k_gemmf layers over the fragment-major copies (bf16; the int8
 * copies of Q8 step tensors with vox_hip_set_gemmf_q8, without it the row-major GEMM where the
 * model has Q8 step tensors), a slot-table decode attention and the LM
 * head through k_gemmf, with step graphs of their own.  Per-stream decoder KV rings at 128
 * streams take ~225 GB as f32, ~113 GB as IEEE half and ~56 GB as FP8 of the 288 GB
 * (vox_hip_model_set_kv_dtype); transcript quality on FP8 rings and MXFP4 weights remains
 * unevaluated.  vox_hip_batch_decode advances every listed
 * stream that has adapter rows left by one greedy token per step; the weights are streamed
 * once per step for all of them, attention / KV / argmax use each stream's own state.
 * Streams not started yet whose prompt is complete are prefilled first (several of them in
 * one stacked pass) and take their first token in the batched steps.  The stacked prefill
 * covers all three decoder KV ring types (f32, IEEE half, FP8 E4M3; vox_hip_batch_set_prefill_kv).  Every stream stops on
 * the device when it has used its adapter rows, after max_steps tokens or (stop_at_eos) after
 * EOS, while the others go on; streams join and leave a batch without a graph capture (the
 * step graphs read a device slot table).  Streams with alternatives on
 * (vox_hip_stream_set_alt) stay in the batch and get their stream_fill_alts records.
 * Results and device state are those of vox_hip_stream_decode on each stream (up to f32
 * summation order of the shared GEMMs).  tokens_out: [n][max_steps]; counts_out[n].
 * Returns the total number of tokens, < 0 on error. */
#define VOX_HIP_BATCH_MAX_SLOTS 128
typedef struct vox_hip_batch vox_hip_batch_t;
vox_hip_batch_t *vox_hip_batch_create(vox_hip_model_t *m, int max_streams);
void vox_hip_batch_free(vox_hip_batch_t *b);
int vox_hip_batch_decode(vox_hip_batch_t *b, vox_hip_stream_t **streams, int n, int max_steps,
                         int stop_at_eos, int *tokens_out, int *counts_out);
/* The same with stream i reading only its first rows[i] adapter rows (<= its count), which the
 * caller guarantees are complete; the streams' own queues are not waited for, so an encoder
 * pass enqueued on them after those rows (async encode, vox_hip_stream_encode_mel_batch) runs
 * beside the batched steps (the per-GPU scheduler's overlap, vh_sched_run). */
int vox_hip_batch_decode_rows(vox_hip_batch_t *b, vox_hip_stream_t **streams, int n, const int *rows,
                              int max_steps, int stop_at_eos, int *tokens_out, int *counts_out);
/* vox_hip_batch_decode_rows in two halves: begin enqueues the call's prefills and its first
 * 16 steps on the batch queue and returns without waiting (0, or <0 on error); finish waits,
 * runs any further steps and fills tokens_out / counts_out (which must stay valid in between),
 * returning the total as decode_rows does.  In between the caller may enqueue work on other
 * queues -- the per-GPU scheduler enqueues the cross-stream encoder pass there, after the
 * steps, so the steps are on the device first -- but must not touch the listed streams'
 * decoder state or call another batch function on b.
 * The library enforces that window.  The call's slot table names each listed stream's state,
 * token ring, adapter buffer, KV rings, alternatives ring and ada table and is uploaded once, so
 * between begin and finish none of them is freed or moved: encoding a listed stream
 * (vox_hip_stream_encode_mel, _encode_mel_batch, the mel feed) stays allowed, and an adapter
 * buffer it outgrows is kept for the call -- which reads only its rows[i] first rows, all of
 * them in the old buffer -- and freed by finish after its last wait (or by
 * vox_hip_batch_free).  Every entry point that would free or rewrite what the call reads, or
 * move a listed stream's decoder, returns -1 with vox_hip_last_error naming the begun call
 * and changes nothing: vox_hip_stream_free (void: the error only; free the stream after
 * finish), vox_hip_stream_reset, _reset_decoder, vox_hip_stream_decode,
 * vox_hip_decoder_prefill_step, vox_hip_decoder_full_step, vox_hip_stream_set_alt,
 * vox_hip_stream_set_delay, listing the stream in a call of another batch object, and
 * vox_hip_model_set_delay on the model of any begun call. */
int vox_hip_batch_begin_rows(vox_hip_batch_t *b, vox_hip_stream_t **streams, int n, const int *rows,
                             int max_steps, int stop_at_eos, int *tokens_out, int *counts_out);
int vox_hip_batch_finish(vox_hip_batch_t *b);
/* Logits [vocab] of the last batched step, for a stream that step advanced (the logits the
 * reference's vox_decoder_forward returns, voxtral_decoder.c:762-779; for tests and --alt
 * style callers).  Returns 0, or <0 if s was not in that step. */
int vox_hip_batch_read_logits(vox_hip_batch_t *b, vox_hip_stream_t *s, float *out);
/* Counters since creation: [0] calls, [1] step replays, [2] live rows over those steps,
 * [3] step-graph captures, [4] batched prefill passes, [5] prefilled streams. */
int vox_hip_batch_stats(const vox_hip_batch_t *b, long long *out6);
/* Growing decoder rings in batched calls (vox_hip_model_set_kv_grow).  A call grows every listed
 * stream's rings for the whole call -- its position, the prompt if it joins, min(max_steps, the
 * rows it may read) steps -- before its prefills and slot table, copies on the batch queue; if
 * one growth cannot be allocated the call returns -1 with nothing enqueued.  Nothing moves
 * between begin and finish (vox_hip_stream_reserve_kv is refused there).  A call in which every
 * listed stream has full rings is plain: today's kernels, arguments and step graphs.  A call with
 * a shorter ring is ragged: its attention instances take each slot's ring capacity (slot modulo
 * and layer stride) from a per-slot table, on step graphs of their own; it runs the MFMA step
 * (<= 32 streams) or the wide step, never the R-row GEMV steps.  Same bits as the same streams
 * on full rings.  out3: [0] ragged calls, [1] ragged step replays, [2] ragged step-graph captures
 * (all also counted in vox_hip_batch_stats). */
int vox_hip_batch_kv_grow_stats(const vox_hip_batch_t *b, long long out3[3]);
/* The prefill of joining streams whose decoder KV rings are IEEE half or FP8: on = 1 (the
 * default) stacks their prompts into the shared passes on the batch queue exactly as f32
 * streams' are -- the layers' weights read once per pass of up to 26 prompts, no wait on the
 * members' queues in vox_hip_batch_decode_rows / begin_rows --, with the RoPE + K/V append and
 * the causal attention at the ring's element type (same stores, same f32 arithmetic and order as
 * the single-stream prefill).  on = 0 prefills each such stream on its own queue, one pass and
 * one host wait per stream (what the batch did before; for measurements).  f32 streams ignore
 * the flag.  VOX_HIP_BATCH_PREFILL_KV=0 sets the initial value at vox_hip_batch_create.  Returns
 * 0; -1 (vox_hip_last_error) between vox_hip_batch_begin_rows and vox_hip_batch_finish. */
int vox_hip_batch_set_prefill_kv(vox_hip_batch_t *b, int on);
/* Opt-in step for small batches: the R-row GEMV (k_gemvr) streams each weight matrix once per
 * step for the whole bucket -- bf16 rows or the model's wpack13 planes, as the single-stream
 * step does -- in five launches per layer, instead of the skinny MFMA GEMMs over the
 * fragment-major copies.
 * Steps whose slot bucket is <= max_rows (0 = off, the default; 1, 2, 4 or 8) take the R-row
 * GEMV path; larger buckets keep the MFMA step.  Tokens, logits (to f32 summation order),
 * alternatives, rings and stream state are those of the MFMA step, and the mode may change
 * between calls.  Like vox_hip_batch_set_gemv_rows_q8, vox_hip_batch_set_gemv_wmx4 and
 * vox_hip_batch_set_wmx4 it acts on calls of <= 32 streams only: the wide step of 33..128
 * streams always streams the bf16 fragment-major copies (on a wmx4-rounded model they hold the
 * planes' values, so the tokens are the model's).  VOX_HIP_BATCH_GEMV=<0|1|2|4|8> sets the
 * initial value at vox_hip_batch_create (ignored for a Q8 model).  Returns 0; -1 (vox_hip_last_error) for
 * another value, for a Q8 model, or between vox_hip_batch_begin_rows and vox_hip_batch_finish.
 * A mixed call (a stream with a delay of its own, vox_hip_stream_set_delay) takes the MFMA step
 * whatever this switch, _q8 and _wmx4 say, as calls of more than 8 slots do: k_gemvr has no
 * per-slot prologue.  vox_hip_batch_gemv_stats does not count its steps; vox_hip_batch_stats does. */
int vox_hip_batch_set_gemv_rows(vox_hip_batch_t *b, int max_rows);
/* The same opt-in for a model with Q8 step tensors (int8 rows and one f32 scale per row; buckets
 * <= 8 as above): the
 * step's k_gemvr launches stream each Q8 tensor's int8 rows once for the bucket, in the
 * single-stream Q8 GEMV's order per row -- exact int8 -> f32, f32 FMAs, the row's scale times
 * the reduced sum before the epilogue -- and a tensor without scales keeps its bf16 / wpack13
 * launch.  max_rows as above (0 = off, the default); it sets the value that
 * vox_hip_batch_gemv_stats reports, and the bucket dispatch, graphs and counters are the same.
 * VOX_HIP_BATCH_GEMV_Q8=<0|1|2|4|8> sets the initial value at vox_hip_batch_create (ignored for
 * a model with no Q8 step tensor).  Returns 0; -1 (vox_hip_last_error) for another value, for a
 * model with no Q8 step tensor (vox_hip_batch_set_gemv_rows is its switch), for a model shape
 * without a kernel instance, or between vox_hip_batch_begin_rows and vox_hip_batch_finish. */
int vox_hip_batch_set_gemv_rows_q8(vox_hip_batch_t *b, int max_rows);
/* [0] max_rows in effect, [1] step replays on the GEMV path, [2] live rows over those,
 * [3] GEMV step-graph captures.  ([1]..[3] are also counted in vox_hip_batch_stats.) */
int vox_hip_batch_gemv_stats(const vox_hip_batch_t *b, long long *out4);
/* The R-row GEMV step's weight source (opt-in, on top of wmx4 mode 1 or 2; buckets <= 8, so calls
 * of <= 32 streams only): on = 1 makes the
 * step stream the wmx4 GEMV plane of every tensor that has one -- the plane the single-stream
 * step reads, 5 bits per weight, no second copy -- through k_gemvr's wmx4 instances, which
 * decode each weight once for the bucket's rows and run the bf16 instance's FMA chains: same
 * bits as on = 0.  A tensor the scan refused keeps its wpack13 or raw launch, so a step may mix
 * formats per tensor.  The two modes keep step graphs of their own, so the flag may change
 * between calls.  VOX_HIP_BATCH_GEMV_WMX4=1 sets the initial value at vox_hip_batch_create
 * (ignored where this call would fail).  Default off.  Returns 0; -1 (vox_hip_last_error) when
 * the model has no wmx4 GEMV plane (wmx4 mode 0, Q8, VOX_HIP_WPACK=0), or between
 * vox_hip_batch_begin_rows and vox_hip_batch_finish. */
int vox_hip_batch_set_gemv_wmx4(vox_hip_batch_t *b, int on);
/* [0] the flag in effect, [1] GEMV step replays that streamed at least one wmx4 plane,
 * [2] tensors of the step (4 per layer and the LM head) with a wmx4 GEMV plane, [3] without. */
int vox_hip_batch_gemv_wmx4_stats(const vox_hip_batch_t *b, long long out4[4]);
/* The batched MFMA step's weight source (calls of <= 32 streams): on = 1 streams the wmx4 fragment plane of every tensor
 * that has one (the bf16 fragment copy of the others), on = 0 the bf16 fragment copies.  Both
 * give the same bits.  A batch created on a model with fragment planes (vox_hip_set_wmx4_batch)
 * starts with it on; otherwise it is off and cannot be turned on.  The two modes keep step
 * graphs of their own, so the mode may change between calls.  Returns 0; -1
 * (vox_hip_last_error) when the model has no fragment plane, or between
 * vox_hip_batch_begin_rows and vox_hip_batch_finish. */
int vox_hip_batch_set_wmx4(vox_hip_batch_t *b, int on);
/* Test entry: y[R][rows] = W x[r] for R in 1..8 rows through k_gemvr's STORE instance of the
 * bucket >= R (unused rows zero), from the raw rows (packed = 0), the wpack13 planes (1) or
 * the wmx4 plane built from W (2, as vox_hip_gemv_wpack).  Returns flags: bit 0 the wpack13
 * instance ran, bit 1 the per-row summation order is the single-row GEMV's, bit 2 the wmx4
 * instance ran (clear, and the raw rows streamed, when W is not MXFP4-valued); -1 on error. */
int vox_hip_gemv_rows(int rows, int K, const uint16_t *W, const float *x, int R, float *y, int packed);
/* Test entries for Q8 rows (W int8 [rows][K], scales [rows]): y[R][rows] = scale * (W x[r]) for R
 * in 1..8 rows through k_gemvr's Q8 STORE instance of the bucket >= R (unused rows zero), and
 * y[rows] for one row through the single-row Q8 GEMV, whose bits every row of the first has.
 * 0, or -1 (vox_hip_last_error) for a shape without an instance. */
int vox_hip_gemv_rows_q8(int rows, int K, const int8_t *W, const float *scales, const float *x, int R, float *y);
int vox_hip_gemv_q8(int rows, int K, const int8_t *W, const float *scales, const float *x, float *y);
/* Decoder state snapshot: [0]=kv logical length, [1]=next adapter row, [2]=prev token,
 * [3]=started, [4]=eos_seen, [5]=tokens generated. */
int vox_hip_stream_state(vox_hip_stream_t *s, int *out6);

/* ------------------------------------------------------------------------
 * Reference-boundary twins (host pointers in and out, synchronous).  These are what
 * voxtral_encoder.c / voxtral_decoder.c / voxtral_kernels.c call under USE_HIP in
 * place of the vox_metal_* functions.
 * ------------------------------------------------------------------------ */
/* voxtral_metal.h:38  C[M,N] = A[M,K] @ B[N,K]^T (B is a host bf16 weight pointer,
 * uploaded once and cached by pointer like voxtral_metal.m:165-201) */
void vox_hip_sgemm_bf16(int M, int N, int K, const float *A, const uint16_t *B_bf16, float *C);
/* voxtral_metal.h:262-265  C[M,N] = A[M,K] @ (scales[n] * B_q8[N,K])^T (vox_linear_q8 /
 * vox_matmul_t_q8 under USE_HIP, voxtral_kernels.c:316-377); B and scales are host
 * pointers, uploaded once and cached by pointer; bias is added by the caller. */
void vox_hip_sgemm_q8(int M, int N, int K, const float *A, const int8_t *B_q8, const float *scales,
                      float *C);
/* voxtral_metal.h:59 */
void vox_hip_fused_qkv_bf16(int M, int K, const float *input,
                            const uint16_t *wq_bf16, int Nq, const uint16_t *wk_bf16, int Nk,
                            const uint16_t *wv_bf16, int Nv, float *q, float *k, float *v);
/* voxtral_metal.h:86 */
void vox_hip_fused_ffn_bf16(int M, int dim, int hidden, const float *input,
                            const uint16_t *w1_bf16, const uint16_t *w3_bf16,
                            const uint16_t *w2_bf16, float *output);
/* voxtral_metal.h:136  (same semantics as vox_causal_attention, voxtral_kernels.c:541-611) */
void vox_hip_encoder_attention(float *out, const float *Q, const float *K, const float *V,
                               int seq_q, int seq_k, int n_heads, int n_kv_heads,
                               int head_dim, float scale, int window_size, int q_offset);
/* voxtral_metal.h:245  32 encoder layers + final norm in place on host x [new_len, enc_dim];
 * K/V appended to the stream's rolling cache at logical positions
 * logical_start..logical_start+new_len-1.  rope_freqs [new_len, head_dim/2, 2] from the
 * caller (vox_compute_rope_freqs).  Returns 0 / <0. */
int vox_hip_encoder_full_step(vox_hip_stream_t *s, float *x, int new_len,
                              const float *rope_freqs, int logical_start);
/* voxtral_metal.h:254  26 decoder layers on seq_len rows, KV written at logical
 * positions logical_start.. ; x [seq_len, dec_dim] updated in place. */
int vox_hip_decoder_prefill_step(vox_hip_stream_t *s, float *x, int seq_len,
                                 const float *rope_freqs, int logical_start);
/* voxtral_metal.h:161/164  upload the step input / release it */
void vox_hip_decoder_start(vox_hip_stream_t *s, const float *x, int dim);
void vox_hip_decoder_end(vox_hip_stream_t *s);
/* voxtral_metal.h:219  one token through all layers + final norm + LM head + argmax.
 * KV written at logical position logical_pos; returns the argmax id (first max wins,
 * voxtral_decoder.c:771-779) and fills logits [vocab] if non-NULL. */
int vox_hip_decoder_full_step(vox_hip_stream_t *s, const float *rope_freqs, int logical_pos,
                              float *logits);

/* ------------------------------------------------------------------------
 * Timing hooks for the benchmark (HIP events on the stream's own queue).
 * ------------------------------------------------------------------------ */
/* Average device time (ms) of the last decode call's dominant per-layer GEMV launches and
 * the bytes they streamed; filled only when profiling was enabled.  out8: [0] ms, [1] bytes,
 * [2] launches, [3] ms per launch, [5] bytes per launch, [6] encoder-GEMM stage ranges an
 * owner recomputed because a partial tile did not arrive in time (since creation). */
int vox_hip_stream_set_profiling(vox_hip_stream_t *s, int enable);
int vox_hip_stream_profile(vox_hip_stream_t *s, double *out8);
/* Synchronise the stream's HIP queue. */
int vox_hip_stream_sync(vox_hip_stream_t *s);

/* Device buffers for callers that keep their inputs resident in HBM (benchmark, tests). */
void *vox_hip_device_upload(const void *host, size_t bytes);
int vox_hip_device_free(void *dev);

#ifdef __cplusplus
}
#endif
#endif /* VOXTRAL_HIP_H */
