/*
 * vox_wmx4.h -- wmx4: MXFP4 storage of a bf16 weight tensor that is already MXFP4-valued
 * (plain C, no HIP), and the rounding that makes a tensor so.
 *
 * A block is 32 consecutive k of one row.  Its weights are e2m1 values
 *   code & 7:  0 -> 0, 1 -> 0.5, 2 -> 1, 3 -> 1.5, 4 -> 2, 5 -> 3, 6 -> 4, 7 -> 6,   code & 8: sign
 * times the block's scale 2^e, e = floor(log2(amax)) - 2 with amax the block's largest
 * magnitude (so amax / 2^e is in [4, 8)), stored as the e8m0 byte e + 127; an all-zero block
 * stores 127.  Every such weight is exactly a bf16, so a tensor rounded to the format is an
 * ordinary bf16 tensor and the planes below decode to it without loss.
 *
 * Rounding (vox_wmx4_round): v / 2^e to the nearest e2m1 value, ties to the even code (the
 * even mantissa), saturating at +-6 (amax in (6, 8) 2^e); the sign of a zero is kept, and so
 * is the sign of a weight that rounds to zero.  Subnormal inputs count as signed zeros, Inf
 * and NaN stay as they are and do not enter amax (the scan then refuses the tensor), and e is
 * held at VOX_WMX4_MIN_E or above so that every output is a normal bf16 or zero.  The block's
 * amax rounds to 4 or 6 times 2^e, so a second rounding finds the same e: idempotent.
 *
 * Exponent window (vox_wmx4_scan): |e| <= VOX_WMX4_MAX_E = 64.  The kernel forms a weight
 * as e2m1 * float(byte << 23); inside the window the scale is a normal f32 in [2^-64, 2^64]
 * and every nonzero weight a normal f32 in [2^-65, 1.5 * 2^66], the very f32 that the bf16
 * weight widens to, so each product w * x is the bf16 instance's product for every x (normal,
 * subnormal or zero): what an RMSNorm output, an attention output or a SwiGLU product
 * reaches (|x| < 2^40 by a wide margin) stays finite against it as it does against the bf16
 * weight.  A real checkpoint's blocks sit near 2^-10..2^0; the window only has to exclude the
 * ends of the e8m0 range (byte 0 is no normal f32, byte 255 is NaN).
 *
 * Compact form (vox_wmx4_pack_ / unpack_): nibbles [rows][K / 8] dwords, weight k of a chunk
 * of 8 in bits 4 (k % 8) .. 4 (k % 8) + 3 (the low nibble of a byte is the even k), and
 * scales [rows][K / 32] bytes.
 *
 * Device plane, laid out for the GEMV kernel's geometry: one record of RW = RB + ceil(RB / 4)
 * dwords per (row group g of RB rows, chunk c of 8 k) at dword (g * K / 8 + c) * RW: dwords
 * 0 .. RB - 1 are the nibble dwords of chunk c of the rows gemv_row(g, 0 .. RB - 1), and byte
 * i of the dwords that follow is the scale byte of row i's block c / 4.  The thread that owns
 * chunk c fetches a group's weights and scales with one record load per K round.  Repeating
 * the scale per chunk costs 8 bits per 8 weights: 5 stored bits per weight at RB = 4 and 8
 * (6 at RB = 2, where half of the scale dword is padding).
 *
 * Fragment plane, laid out for the batched step's MFMA kernels (k_skl, k_skl2, k_sklx, k_skf):
 * the A operand of a [N, K] tensor in device row order, N % 16 == 0, K % 64 == 0.  One record
 * of VOX_WMX4_FRAG_REC = 144 dwords (576 B) per (16-row group g, 64-k block b) at dword
 * (g * K / 64 + b) * 144.  Lane l = 16 q + j of the wave that streams the group owns row
 * 16 g + j, k 64 b + 16 q .. 64 b + 16 q + 15 (the two 8-k halves of the bf16 fragment copy's
 * lane, frag_off in vox_hip_dev.h):
 *   dwords 2 l, 2 l + 1:  the row's nibble dwords of chunks 8 b + 2 q and 8 b + 2 q + 1, in the
 *                         compact form's nibble order (half t of the lane is dword 2 l + t);
 *   byte l of dwords 128 .. 143 (byte l & 3 of dword 128 + l / 4, little end first): the e8m0
 *                         byte of the row's block 2 b + (q >> 1), which holds both halves.
 * A lane fetches its block with one 8-B load at byte 8 l and one 1-B load at byte 512 + l, both
 * contiguous across the wave; the record does not depend on how many blocks a split takes.
 * Repeating each scale for the two lanes that share it costs 64 B per 2048 weights: 4.5 stored
 * bits per weight (576 B against the bf16 fragment's 2048).
 */
#ifndef VOX_WMX4_H
#define VOX_WMX4_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define VOX_WMX4_BLOCK 32
#define VOX_WMX4_MAX_E 64    /* |e| beyond which a tensor is not streamed as wmx4 */
#define VOX_WMX4_MIN_E (-125) /* the rounding's floor for e: 0.5 * 2^e stays a normal bf16 */

/* bf16 classes */
static inline int vox_wmx4_is_nonfinite(uint16_t b) { return ((b >> 7) & 0xff) == 0xff; }
static inline int vox_wmx4_is_subnormal(uint16_t b) { return ((b >> 7) & 0xff) == 0 && (b & 0x7f); }

/* The block's rule exponent from its finite normal weights; *zero is set when it has none. */
static inline int vox_wmx4_block_e(const uint16_t *w, int n, int *zero) {
    int amax = 0;
    for (int k = 0; k < n; k++) {
        const int a = w[k] & 0x7fff;
        if ((a >> 7) == 0xff || (a >> 7) == 0) continue;
        if (a > amax) amax = a;
    }
    *zero = amax == 0;
    if (!amax) return 0;
    const int e = (amax >> 7) - 127 - 2;
    return e < VOX_WMX4_MIN_E ? VOX_WMX4_MIN_E : e;
}

/* e2m1 code (sign in bit 3) of a finite bf16 under scale 2^e, round to nearest, ties to the
 * even code, saturating; |w| < 8 * 2^e is the caller's (the rule exponent gives it) */
static inline uint32_t vox_wmx4_code(uint16_t b, int e) {
    const uint32_t s = (uint32_t)(b >> 15) << 3;
    const int E = (b >> 7) & 0xff;
    if (E == 0) return s;
    /* |w| / 2^e = (128 + m) * 2^(E - 134 - e); in units of 2^-11 that is (128 + m) << sh */
    const int sh = E - 123 - e;
    if (sh < 0) return s; /* below 256 * 2^-12 < 0.25: rounds to zero */
    const uint32_t q = sh > 6 ? 0xffffu : (uint32_t)(128 + (b & 0x7f)) << sh;
    /* midpoints between neighbouring codes: 0.25 0.75 1.25 1.75 2.5 3.5 5 */
    static const uint32_t mid[7] = {512, 1536, 2560, 3584, 5120, 7168, 10240};
    uint32_t c = 0;
    while (c < 7 && (q > mid[c] || (q == mid[c] && (c & 1)))) c++;
    return s | c;
}
/* the bf16 that a code stands for under scale 2^e (e >= VOX_WMX4_MIN_E) */
static inline uint16_t vox_wmx4_decode(uint32_t code, int e) {
    static const int8_t de[8] = {0, -1, 0, 0, 1, 1, 2, 2};
    const uint32_t c = code & 7, s = (code >> 3) & 1;
    if (c == 0) return (uint16_t)(s << 15);
    return (uint16_t)(s << 15 | (uint32_t)(e + de[c] + 127) << 7 | ((c & 1) && c > 1 ? 0x40u : 0u));
}

static inline void vox_wmx4_round_rows(const uint16_t *in, long long r0, long long r1, long long K, uint16_t *out) {
    for (long long r = r0; r < r1; r++)
        for (long long k0 = 0; k0 < K; k0 += VOX_WMX4_BLOCK) {
            const int n = (int)(K - k0 < VOX_WMX4_BLOCK ? K - k0 : VOX_WMX4_BLOCK);
            const uint16_t *w = in + r * K + k0;
            uint16_t *o = out + r * K + k0;
            int zero;
            const int e = vox_wmx4_block_e(w, n, &zero);
            for (int k = 0; k < n; k++) {
                if (vox_wmx4_is_nonfinite(w[k])) o[k] = w[k];
                else if (zero || vox_wmx4_is_subnormal(w[k])) o[k] = (uint16_t)(w[k] & 0x8000);
                else o[k] = vox_wmx4_decode(vox_wmx4_code(w[k], e), e);
            }
        }
}
/* bf16 [rows, K] -> the nearest MXFP4-valued bf16 tensor (a last block of K % 32 weights is
 * rounded as a block of its own; in == out is allowed) */
static inline void vox_wmx4_round_(const uint16_t *in, long long rows, long long K, uint16_t *out) {
#pragma omp parallel for schedule(static) num_threads(16)
    for (long long r = 0; r < rows; r++) vox_wmx4_round_rows(in, r, r + 1, K, out);
}

/* 1 when one block (32 weights) is representable under its own rule exponent, inside the window */
static inline int vox_wmx4_block_ok(const uint16_t *w) {
    for (int k = 0; k < VOX_WMX4_BLOCK; k++)
        if (vox_wmx4_is_nonfinite(w[k]) || vox_wmx4_is_subnormal(w[k])) return 0;
    int zero;
    const int e = vox_wmx4_block_e(w, VOX_WMX4_BLOCK, &zero);
    if (zero) return 1;
    if (e < -VOX_WMX4_MAX_E || e > VOX_WMX4_MAX_E) return 0;
    for (int k = 0; k < VOX_WMX4_BLOCK; k++)
        if (vox_wmx4_decode(vox_wmx4_code(w[k], e), e) != w[k]) return 0;
    return 1;
}
/* rows r0..r1: stops at the first block that fails, so an ordinary bf16 tensor costs one block */
static inline int vox_wmx4_scan_rows(const uint16_t *w, long long r0, long long r1, long long K) {
    if (K <= 0 || K % VOX_WMX4_BLOCK) return 0;
    for (long long r = r0; r < r1; r++)
        for (long long k0 = 0; k0 < K; k0 += VOX_WMX4_BLOCK)
            if (!vox_wmx4_block_ok(w + r * K + k0)) return 0;
    return 1;
}
static inline int vox_wmx4_scan_(const uint16_t *w, long long rows, long long K) {
    return vox_wmx4_scan_rows(w, 0, rows, K);
}

/* rows r0..r1 of a tensor that passes the scan -> compact nibbles and scale bytes */
static inline void vox_wmx4_pack_rows(const uint16_t *w, long long r0, long long r1, long long K, uint32_t *nib,
                                      uint8_t *scl) {
    const long long kc = K / 8, kb = K / VOX_WMX4_BLOCK;
    for (long long r = r0; r < r1; r++)
        for (long long b = 0; b < kb; b++) {
            const uint16_t *p = w + r * K + b * VOX_WMX4_BLOCK;
            int zero;
            const int e = vox_wmx4_block_e(p, VOX_WMX4_BLOCK, &zero);
            scl[r * kb + b] = (uint8_t)(e + 127);
            for (int c = 0; c < 4; c++) {
                uint32_t d = 0;
                for (int k = 0; k < 8; k++) d |= vox_wmx4_code(p[c * 8 + k], e) << (4 * k);
                nib[r * kc + b * 4 + c] = d;
            }
        }
}
static inline void vox_wmx4_pack_(const uint16_t *w, long long rows, long long K, uint32_t *nib, uint8_t *scl) {
#pragma omp parallel for schedule(static) num_threads(16)
    for (long long r = 0; r < rows; r++) vox_wmx4_pack_rows(w, r, r + 1, K, nib, scl);
}
static inline void vox_wmx4_unpack_(const uint32_t *nib, const uint8_t *scl, long long rows, long long K, uint16_t *w) {
    const long long kc = K / 8, kb = K / VOX_WMX4_BLOCK;
#pragma omp parallel for schedule(static) num_threads(16)
    for (long long r = 0; r < rows; r++)
        for (long long c = 0; c < kc; c++)
            for (int k = 0; k < 8; k++)
                w[r * K + c * 8 + k] = vox_wmx4_decode(nib[r * kc + c] >> (4 * k), (int)scl[r * kb + c / 4] - 127);
}

/* the GEMV kernel's row of slot i in group g (k_gemv's gemv_rows; vox_wpack13_row) */
static inline long long vox_wmx4_row(long long g, int i, int rb, int swiglu) {
    if (!swiglu) return g * rb + i;
    const long long u = g * (rb / 2) + (i >> 1);
    return ((u >> 4) << 5) + (u & 15) + ((i & 1) << 4);
}
static inline int vox_wmx4_rec_words(int rb) { return rb + (rb + 3) / 4; }
/* dwords of the device plane of a [rows, K] tensor in groups of rb rows */
static inline long long vox_wmx4_plane_words(long long rows, long long K, int rb) {
    return rows / rb * (K / 8) * vox_wmx4_rec_words(rb);
}
/* compact form -> groups g0..g1 of the device plane */
static inline void vox_wmx4_plane_groups(const uint32_t *nib, const uint8_t *scl, long long g0, long long g1,
                                         long long K, int rb, int swiglu, uint32_t *out) {
    const long long kc = K / 8, kb = K / VOX_WMX4_BLOCK;
    const int rw = vox_wmx4_rec_words(rb);
    for (long long g = g0; g < g1; g++)
        for (long long c = 0; c < kc; c++) {
            uint32_t *rec = out + (g * kc + c) * rw;
            memset(rec, 0, (size_t)rw * 4);
            for (int i = 0; i < rb; i++) {
                const long long r = vox_wmx4_row(g, i, rb, swiglu);
                rec[i] = nib[r * kc + c];
                rec[rb + (i >> 2)] |= (uint32_t)scl[r * kb + c / 4] << (8 * (i & 3));
            }
        }
}
static inline void vox_wmx4_plane_layout_(const uint32_t *nib, const uint8_t *scl, long long rows, long long K, int rb,
                                          int swiglu, uint32_t *out) {
#pragma omp parallel for schedule(static) num_threads(16)
    for (long long g = 0; g < rows / rb; g++) vox_wmx4_plane_groups(nib, scl, g, g + 1, K, rb, swiglu, out);
}

/* ---- fragment plane (the batched step's A operand; layout in the header comment) ---- */
#define VOX_WMX4_FRAG_REC 144 /* dwords per (16-row group, 64-k block): 128 of nibbles, 16 of scale bytes */
/* dwords of the fragment plane of a [N, K] tensor; 0 for a shape it does not take */
static inline long long vox_wmx4_frag_words(long long N, long long K) {
    if (N <= 0 || K <= 0 || N % 16 || K % 64) return 0;
    return N / 16 * (K / 64) * VOX_WMX4_FRAG_REC;
}
/* compact form -> 16-row groups g0..g1 of the fragment plane */
static inline void vox_wmx4_frag_groups(const uint32_t *nib, const uint8_t *scl, long long g0, long long g1, long long K,
                                        uint32_t *out) {
    const long long kc = K / 8, kb = K / VOX_WMX4_BLOCK, nb = K / 64;
    for (long long g = g0; g < g1; g++)
        for (long long b = 0; b < nb; b++) {
            uint32_t *rec = out + (g * nb + b) * VOX_WMX4_FRAG_REC;
            memset(rec + 128, 0, 64);
            for (int l = 0; l < 64; l++) {
                const int q = l >> 4, j = l & 15;
                const long long r = g * 16 + j, c = b * 8 + 2 * q;
                rec[2 * l] = nib[r * kc + c];
                rec[2 * l + 1] = nib[r * kc + c + 1];
                rec[128 + (l >> 2)] |= (uint32_t)scl[r * kb + 2 * b + (q >> 1)] << (8 * (l & 3));
            }
        }
}
static inline void vox_wmx4_frag_layout_(const uint32_t *nib, const uint8_t *scl, long long N, long long K, uint32_t *out) {
    if (!vox_wmx4_frag_words(N, K)) return;
#pragma omp parallel for schedule(static) num_threads(16)
    for (long long g = 0; g < N / 16; g++) vox_wmx4_frag_groups(nib, scl, g, g + 1, K, out);
}
#endif
