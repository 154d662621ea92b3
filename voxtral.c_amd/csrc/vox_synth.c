/*
 * vox_synth.c -- deterministic synthetic weights and inputs.
 *
 * The real Voxtral-Mini-4B-Realtime checkpoint is not available offline, so tests and
 * the benchmark use seeded random weights of the exact architecture (same tensor names,
 * shapes and dtype => same bytes and FLOPs).  Values are a counter-based hash
 * (splitmix64) of (seed, element index), so any slice can be generated independently
 * and in parallel; they are uniform with the requested standard deviation.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "vox_kv8.h"
#include "vox_wmx4.h"
#include "vox_wpack.h"

static inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static inline float unif(uint64_t seed, uint64_t i) {
    uint64_t h = splitmix64(seed ^ splitmix64(i));
    return (float)((h >> 40) * (1.0 / 16777216.0)) * 2.0f - 1.0f; /* [-1, 1) */
}

/* bf16 bits of offset + std * sqrt(3) * U[-1,1), round-to-nearest-even */
void vox_synth_bf16(uint16_t *out, size_t n, uint64_t seed, float std, float offset) {
    const float a = std * 1.7320508075688772f;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)n; i++) {
        float v = offset + a * unif(seed, (uint64_t)i);
        uint32_t u;
        memcpy(&u, &v, 4);
        u += 0x7fffu + ((u >> 16) & 1u);
        out[i] = (uint16_t)(u >> 16);
    }
}

void vox_synth_f32(float *out, size_t n, uint64_t seed, float lo, float hi) {
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)n; i++) {
        float u = 0.5f * (unif(seed, (uint64_t)i) + 1.0f);
        out[i] = lo + (hi - lo) * u;
    }
}

/* bf16 -> f32 (exact) */
void vox_bf16_to_f32(float *out, const uint16_t *in, size_t n) {
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)n; i++) {
        uint32_t u = ((uint32_t)in[i]) << 16;
        memcpy(&out[i], &u, 4);
    }
}

/* Per-row symmetric int8 quantisation of a bf16 [rows, cols] matrix, restating the
 * reference's quantize.py:35-46 (quantize_q8_row) and :96-125: amax = max|row| in f32;
 * scale = f32(amax / 127.0 in double); q = round-half-even(row / scale) in f32, clipped to
 * [-128, 127]; an all-zero row gets scale 0 and zeros.  Output layout as quantize.py
 * writes it (safetensors.c:393-408): scales [rows] f32, then q [rows, cols] int8. */
void vox_quantize_q8_bf16(const uint16_t *in, long long rows, long long cols, float *scales,
                          int8_t *q) {
#pragma omp parallel for schedule(dynamic, 16)
    for (long long r = 0; r < rows; r++) {
        const uint16_t *src = in + r * cols;
        int8_t *dst = q + r * cols;
        float amax = 0.0f;
        for (long long c = 0; c < cols; c++) {
            uint32_t u = ((uint32_t)src[c]) << 16;
            float v;
            memcpy(&v, &u, 4);
            v = fabsf(v);
            if (v > amax) amax = v;
        }
        if (amax == 0.0f) {
            scales[r] = 0.0f;
            memset(dst, 0, (size_t)cols);
            continue;
        }
        const float s = (float)((double)amax / 127.0);
        scales[r] = s;
        for (long long c = 0; c < cols; c++) {
            uint32_t u = ((uint32_t)src[c]) << 16;
            float v;
            memcpy(&v, &u, 4);
            float t = rintf(v / s);
            t = t < -128.0f ? -128.0f : (t > 127.0f ? 127.0f : t);
            dst[c] = (int8_t)t;
        }
    }
}

/* (float)q * scale per row: safetensors_get_f32 of a Q8 tensor (safetensors.c:393-408) */
void vox_dequant_q8(float *out, const int8_t *q, const float *scales, long long rows, long long cols) {
#pragma omp parallel for schedule(static)
    for (long long r = 0; r < rows; r++)
        for (long long c = 0; c < cols; c++) out[r * cols + c] = (float)q[r * cols + c] * scales[r];
}

/* wpack13 (vox_wpack.h): the pure pack / unpack functions the engine's loader uses, exported
 * for the CPU tests. */
int vox_wpack13_scan(const uint16_t *w, size_t n, int *emin, int *emax, int *D) {
    return vox_wpack13_scan_(w, n, emin, emax, D);
}
void vox_wpack13_pack(const uint16_t *w, long long rows, long long K, int D, uint32_t *main, uint8_t *side) {
    vox_wpack13_pack_(w, rows, K, D, main, side);
}
void vox_wpack13_unpack(const uint32_t *main, const uint8_t *side, long long rows, long long K, int D, uint16_t *w) {
    vox_wpack13_unpack_(main, side, rows, K, D, w);
}
int vox_wpack13_side_words_of(long long K, int rb) { return vox_wpack13_side_words(K, rb); }
void vox_wpack13_side_layout(const uint8_t *side, long long rows, long long K, int rb, int swiglu, uint32_t *out) {
    vox_wpack13_side_layout_(side, rows, K, rb, swiglu, out);
}

/* wmx4 (vox_wmx4.h): the rounding, scan, pack / unpack and plane layout the engine's loader
 * uses, exported for vox_weights.quantize_mxfp4 and the CPU tests. */
void vox_wmx4_round(const uint16_t *in, long long rows, long long K, uint16_t *out) { vox_wmx4_round_(in, rows, K, out); }
int vox_wmx4_scan(const uint16_t *w, long long rows, long long K) { return vox_wmx4_scan_(w, rows, K); }
void vox_wmx4_pack(const uint16_t *w, long long rows, long long K, uint32_t *nib, uint8_t *scl) {
    vox_wmx4_pack_(w, rows, K, nib, scl);
}
void vox_wmx4_unpack(const uint32_t *nib, const uint8_t *scl, long long rows, long long K, uint16_t *w) {
    vox_wmx4_unpack_(nib, scl, rows, K, w);
}
long long vox_wmx4_plane_words_of(long long rows, long long K, int rb) { return vox_wmx4_plane_words(rows, K, rb); }
void vox_wmx4_plane_layout(const uint32_t *nib, const uint8_t *scl, long long rows, long long K, int rb, int swiglu,
                           uint32_t *out) {
    vox_wmx4_plane_layout_(nib, scl, rows, K, rb, swiglu, out);
}
long long vox_wmx4_frag_words_of(long long N, long long K) { return vox_wmx4_frag_words(N, K); }
void vox_wmx4_frag_layout(const uint32_t *nib, const uint8_t *scl, long long N, long long K, uint32_t *out) {
    vox_wmx4_frag_layout_(nib, scl, N, K, out);
}

/* kv8 (vox_kv8.h): the FP8 E4M3 decoder KV ring element's rule, for tests and tools; the _n
 * forms run it over arrays (codes and / or back may be null) */
uint8_t vox_kv8_encode(float x) { return vox_kv8_encode_(x); }
float vox_kv8_decode(uint8_t c) { return vox_kv8_decode_(c); }
float vox_kv8_round(float x) { return vox_kv8_round_(x); }
void vox_kv8_encode_n(const float *x, long long n, uint8_t *codes, float *back) {
    for (long long i = 0; i < n; i++) {
        const uint8_t c = vox_kv8_encode_(x[i]);
        if (codes) codes[i] = c;
        if (back) back[i] = vox_kv8_decode_(c);
    }
}
void vox_kv8_decode_n(const uint8_t *codes, long long n, float *out) {
    for (long long i = 0; i < n; i++) out[i] = vox_kv8_decode_(codes[i]);
}
