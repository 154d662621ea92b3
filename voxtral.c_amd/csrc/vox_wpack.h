/*
 * vox_wpack.h -- wpack13: lossless 13-bit storage of a bf16 weight tensor (plain C, no HIP).
 *
 * Within one tensor the bf16 exponents that occur span a few tens of binades.  When the
 * nonzero weights span at most 30 binades, every weight w equals h * 2^D for one integer D
 * per tensor and an IEEE-half normal h (or +-0): sign, 5 exponent bits and bf16's 7
 * mantissa bits, 13 bits.  The GEMV multiplies x by 2^D once and feeds h to the FMA as a
 * half operand, so every product is the same real number as w * x.
 *
 * code(w) = s << 12 | e5 << 7 | m7, with e5 = E - 112 - D in 1..30 (E: bf16 exponent
 * field), and code(+-0) = s << 12.  code << 3 is the half's bit pattern.
 *
 * Main plane, row-major, 12 bytes (3 dwords) per chunk of 8 consecutive k of one row:
 *   dword p (p = 0..2) = code[2p] << 3 | code[2p+1] << 19 | L_p | U_p << 16
 * where the spare low 3 bits of the two halves carry weights 6 and 7:
 *   L_p = (code[6] >> 3p) & 7,  U_p = (code[7] >> 3p) & 7      (their low 9 bits)
 * Side byte of the chunk: code[6] >> 9 | (code[7] >> 9) << 4     (their top 4 bits)
 *
 * Side plane, laid out for the GEMV kernel's geometry: one record of SW dwords per (row
 * group g, thread t of the 256), SW = ceil(KQ * RB / 4), at dword (g * 256 + t) * SW.
 * Slot s = j * RB + i of a record is the side byte of row gemv_row(g, i), chunk
 * (j * 4 + t / 64) * 64 + t % 64 (chunk 0 when that is past the row: the kernel re-loads
 * chunk 0 there and meets x = 0).  Dword s / 4 holds slot s with q = s % 4 as
 *   low nibble at bits 12 - 4q .. 15 - 4q,  high nibble at bits 28 - 4q .. 31 - 4q
 * so that (dword << 4q) & 0xf000f000 lands both nibbles on top of the two halves.
 */
#ifndef VOX_WPACK_H
#define VOX_WPACK_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define VOX_WPACK_MAX_SPAN 29 /* Emax - Emin of a packable tensor */
#define VOX_WPACK_MAX_D 40    /* |D| beyond which the x prescale is not covered */

/* Exponent window of a range of weights, folded into *lo / *hi (bf16 exponent fields over
 * the nonzero weights; start them at 256 / -1) and *bad (Inf / NaN or a nonzero subnormal). */
static inline void vox_wpack13_scan_range(const uint16_t *w, size_t n, int *lo, int *hi, int *bad) {
    int l = *lo, h = *hi, b = *bad;
    for (size_t i = 0; i < n; i++) {
        const int e = (w[i] >> 7) & 0xff, m = w[i] & 0x7f;
        if (e == 0xff || (e == 0 && m)) b = 1;
        if (e == 0) continue;
        if (e < l) l = e;
        if (e > h) h = e;
    }
    *lo = l;
    *hi = h;
    *bad = b;
}
/* The tensor's D from its window: w = h * 2^D with h a half normal needs D in
 * [hi - 142, lo - 113]; the value nearest 0 is taken.  Returns 1 when packable. */
static inline int vox_wpack13_choose(int lo, int hi, int bad, int *D) {
    *D = 0;
    if (bad || hi - lo > VOX_WPACK_MAX_SPAN) return 0;
    if (hi < 0) return 1; /* all zero */
    const int dlo = hi - 142, dhi = lo - 113;
    const int d = dlo > 0 ? dlo : (dhi < 0 ? dhi : 0);
    *D = d;
    return d >= -VOX_WPACK_MAX_D && d <= VOX_WPACK_MAX_D;
}
/* Whole tensor: returns 1 when packable and sets *D; emin / emax are 0 / 0 when all zero. */
static inline int vox_wpack13_scan_(const uint16_t *w, size_t n, int *emin, int *emax, int *D) {
    int lo = 256, hi = -1, bad = 0;
    vox_wpack13_scan_range(w, n, &lo, &hi, &bad);
    *emin = hi < 0 ? 0 : lo;
    *emax = hi < 0 ? 0 : hi;
    return vox_wpack13_choose(lo, hi, bad, D);
}

static inline uint32_t vox_wpack13_code(uint16_t b, int D) {
    const uint32_t s = b >> 15, e = (b >> 7) & 0xff, m = b & 0x7f;
    if (e == 0) return s << 12;
    return s << 12 | (uint32_t)((int)e - 112 - D) << 7 | m;
}
static inline uint16_t vox_wpack13_decode(uint32_t code, int D) {
    const uint32_t s = code >> 12 & 1, e5 = code >> 7 & 0x1f, m = code & 0x7f;
    if (e5 == 0) return (uint16_t)(s << 15);
    return (uint16_t)(s << 15 | (uint32_t)((int)e5 + 112 + D) << 7 | m);
}

/* 8 bf16 -> 3 dwords + 1 byte */
static inline void vox_wpack13_pack8(const uint16_t *w, int D, uint32_t *main3, uint8_t *side) {
    uint32_t c[8];
    for (int k = 0; k < 8; k++) c[k] = vox_wpack13_code(w[k], D);
    for (int p = 0; p < 3; p++)
        main3[p] = c[2 * p] << 3 | c[2 * p + 1] << 19 | ((c[6] >> (3 * p)) & 7) | ((c[7] >> (3 * p)) & 7) << 16;
    *side = (uint8_t)(c[6] >> 9 | (c[7] >> 9) << 4);
}
static inline void vox_wpack13_unpack8(const uint32_t *main3, uint8_t side, int D, uint16_t *w) {
    uint32_t c6 = (uint32_t)(side & 15) << 9, c7 = (uint32_t)(side >> 4) << 9;
    for (int p = 0; p < 3; p++) {
        w[2 * p] = vox_wpack13_decode(main3[p] >> 3 & 0x1fff, D);
        w[2 * p + 1] = vox_wpack13_decode(main3[p] >> 19, D);
        c6 |= (main3[p] & 7) << (3 * p);
        c7 |= (main3[p] >> 16 & 7) << (3 * p);
    }
    w[6] = vox_wpack13_decode(c6, D);
    w[7] = vox_wpack13_decode(c7, D);
}

/* rows r0..r1 of a matrix [rows, K] (K % 8 == 0): main [rows][K / 8][3] dwords, side
 * [rows][K / 8] bytes */
static inline void vox_wpack13_pack_rows(const uint16_t *w, long long r0, long long r1, long long K, int D,
                                         uint32_t *main, uint8_t *side) {
    const long long kc = K / 8;
    for (long long r = r0; r < r1; r++)
        for (long long c = 0; c < kc; c++)
            vox_wpack13_pack8(w + r * K + c * 8, D, main + (r * kc + c) * 3, side + r * kc + c);
}
static inline void vox_wpack13_pack_(const uint16_t *w, long long rows, long long K, int D, uint32_t *main,
                                     uint8_t *side) {
#pragma omp parallel for schedule(static) num_threads(16)
    for (long long r = 0; r < rows; r++) vox_wpack13_pack_rows(w, r, r + 1, K, D, main, side);
}
static inline void vox_wpack13_unpack_(const uint32_t *main, const uint8_t *side, long long rows, long long K, int D,
                                       uint16_t *w) {
    const long long kc = K / 8;
#pragma omp parallel for schedule(static) num_threads(16)
    for (long long r = 0; r < rows; r++)
        for (long long c = 0; c < kc; c++)
            vox_wpack13_unpack8(main + (r * kc + c) * 3, side[r * kc + c], D, w + r * K + c * 8);
}

/* the GEMV kernel's row of slot i in group g (k_gemv's gemv_rows): SwiGLU pairs the w1 and
 * w3 rows of a hidden unit out of the 16-row interleave */
static inline long long vox_wpack13_row(long long g, int i, int rb, int swiglu) {
    if (!swiglu) return g * rb + i;
    const long long u = g * (rb / 2) + (i >> 1);
    return ((u >> 4) << 5) + (u & 15) + ((i & 1) << 4);
}
static inline int vox_wpack13_kq(long long K) { return (int)((K / 8 + 255) / 256); }
static inline int vox_wpack13_side_words(long long K, int rb) { return (vox_wpack13_kq(K) * rb + 3) / 4; }

/* side bytes [rows][K / 8] -> groups g0..g1 of the kernel's side plane ((rows / rb) * 256 * SW
 * dwords in all) */
static inline void vox_wpack13_side_groups(const uint8_t *side, long long g0, long long g1, long long K, int rb,
                                           int swiglu, uint32_t *out) {
    const long long kc = K / 8;
    const int kq = vox_wpack13_kq(K), sw = vox_wpack13_side_words(K, rb);
    for (long long g = g0; g < g1; g++)
        for (int t = 0; t < 256; t++) {
            uint32_t *rec = out + (g * 256 + t) * sw;
            memset(rec, 0, (size_t)sw * 4);
            for (int j = 0; j < kq; j++)
                for (int i = 0; i < rb; i++) {
                    const int s = j * rb + i, q = s & 3;
                    long long c = (long long)(j * 4 + t / 64) * 64 + t % 64;
                    if (c >= kc) c = 0;
                    const uint32_t b = side[vox_wpack13_row(g, i, rb, swiglu) * kc + c];
                    rec[s >> 2] |= (b & 15) << (12 - 4 * q) | (b >> 4) << (28 - 4 * q);
                }
        }
}
static inline void vox_wpack13_side_layout_(const uint8_t *side, long long rows, long long K, int rb, int swiglu,
                                            uint32_t *out) {
#pragma omp parallel for schedule(static) num_threads(16)
    for (long long g = 0; g < rows / rb; g++) vox_wpack13_side_groups(side, g, g + 1, K, rb, swiglu, out);
}
#endif
