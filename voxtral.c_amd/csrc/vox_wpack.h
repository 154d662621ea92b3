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
 * (j * 4 + t / 64) * 64 + t % 64 (chunk 0 when that is past the row: the kernel meets x = 0
 * there; see the compact plane below).  Dword s / 4 holds slot s with q = s % 4 as
 *   low nibble at bits 12 - 4q .. 15 - 4q,  high nibble at bits 28 - 4q .. 31 - 4q
 * so that (dword << 4q) & 0xf000f000 lands both nibbles on top of the two halves.
 *
 * Fragment plane, laid out for the batched step's MFMA kernels (k_skl, k_skl2, k_sklx, k_skf):
 * the A operand of a [N, K] tensor in device row order, N % 16 == 0, K % 64 == 0, in the same
 * codes and D.  One record of VOX_WPACK13_FRAG_REC = 416 dwords (1664 B) per (16-row group g,
 * 64-k block b) at dword (g * K / 64 + b) * 416.  Lane l = 16 q + j of the wave that streams the
 * group owns row 16 g + j, k 64 b + 16 q + i, i = 0..15 (the 16 weights of the bf16 fragment
 * copy's lane, frag_off in vox_hip_dev.h).  With low(i) = code(i) & 0xfff (exponent and
 * mantissa) and s(i) = code(i) >> 12, the lane's 26 bytes are
 *   dwords 4 l .. 4 l + 3 (p = 0..3) and 256 + 2 l, 256 + 2 l + 1 (p = 4, 5):
 *       low(2p) | n(p, 0) << 12 | low(2p + 1) << 16 | n(p, 1) << 28
 *     where the spare nibbles carry weights 12..15, nibble by nibble:
 *       n(p, h) = (low(12 + h) >> 4 p) & 15 for p = 0..2,  (low(14 + h) >> 4 (p - 3)) & 15 for p = 3..5
 *   the 16-bit word at byte 1536 + 2 l:  s(2p) << p | s(2p + 1) << (8 + p), p = 0..7.
 * A lane fetches its block with a 16-B load at byte 16 l, an 8-B load at 1024 + 8 l and a 2-B
 * load at 1536 + 2 l, each contiguous across the wave; the record does not depend on how many
 * blocks a split takes.  The kernel turns a dword pair into the bf16 copy's two weights with
 * packed 16-bit arithmetic: bits = s << 15 | (low + ((112 + D) << 7)), or s << 15 when low is 0
 * (exact: a packable tensor has no nonzero subnormal).  13 stored bits per weight.
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
/* ---- compact side plane ----
 * A row of K / 8 chunks that spans more than one K round of 256 chunks and ends inside its last
 * round (K = 3072: 384 chunks, 1.5 rounds) leaves the lanes past the row end without a chunk in
 * that round; the record above still gives each of them RB slots (of chunk 0).  The compact plane
 * holds no slot without a chunk.  A group's record has two sections:
 *   A: SWA = (KQ - 1) * RB / 4 dwords per thread t of the 256 at dword t * SWA: slots s = j * RB + i
 *      of the whole rounds j < KQ - 1, as above;
 *   B: SWB = ceil(RB / 4) dwords per thread t < NR = K / 8 - (KQ - 1) * 256 (the lanes with a chunk
 *      in the last round) at dword 256 * SWA + t * SWB: slot i of chunk (KQ - 1) * 256 + t.
 * Groups follow each other at 256 * SWA + NR * SWB dwords; a dword holds its four slots as above.
 * A thread's registers are the padded record's: section A, then section B (zeros without a
 * chunk).  It takes (KQ - 1) * RB % 4 == 0, so that the last round's slots start a dword; every
 * other shape -- one round, whole rounds, or a last round that shares a dword -- keeps the padded
 * plane, byte for byte. */
static inline int vox_wpack13_side_is_compact(long long K, int rb) {
    const int kq = vox_wpack13_kq(K);
    return kq > 1 && (K / 8) % 256 != 0 && ((kq - 1) * rb) % 4 == 0;
}
/* dwords of one group's record in the compact plane (the padded 256 * SW where it does not apply) */
static inline long long vox_wpack13_side_compact_group_words(long long K, int rb) {
    const int kq = vox_wpack13_kq(K);
    if (!vox_wpack13_side_is_compact(K, rb)) return 256LL * vox_wpack13_side_words(K, rb);
    return 256LL * ((kq - 1) * rb / 4) + (K / 8 - (kq - 1) * 256LL) * ((rb + 3) / 4);
}
/* side bytes [rows][K / 8] -> groups g0..g1 of the compact side plane ((rows / rb) *
 * vox_wpack13_side_compact_group_words dwords in all) */
static inline void vox_wpack13_side_compact_groups(const uint8_t *side, long long g0, long long g1, long long K, int rb,
                                                   int swiglu, uint32_t *out) {
    if (!vox_wpack13_side_is_compact(K, rb)) {
        vox_wpack13_side_groups(side, g0, g1, K, rb, swiglu, out);
        return;
    }
    const long long kc = K / 8, gw = vox_wpack13_side_compact_group_words(K, rb);
    const int kq = vox_wpack13_kq(K), swa = (kq - 1) * rb / 4, swb = (rb + 3) / 4;
    const int nr = (int)(kc - (kq - 1) * 256LL);
    for (long long g = g0; g < g1; g++) {
        uint32_t *rec = out + g * gw;
        memset(rec, 0, (size_t)gw * 4);
        for (int t = 0; t < 256; t++)
            for (int j = 0; j < (t < nr ? kq : kq - 1); j++)
                for (int i = 0; i < rb; i++) {
                    const int last = j == kq - 1, s = last ? i : j * rb + i, q = s & 3;
                    const long long c = (long long)(j * 4 + t / 64) * 64 + t % 64;
                    const uint32_t b = side[vox_wpack13_row(g, i, rb, swiglu) * kc + c];
                    uint32_t *d = last ? rec + 256 * swa + t * swb : rec + t * swa;
                    d[s >> 2] |= (b & 15) << (12 - 4 * q) | (b >> 4) << (28 - 4 * q);
                }
    }
}
static inline void vox_wpack13_side_compact_layout_(const uint8_t *side, long long rows, long long K, int rb, int swiglu,
                                                    uint32_t *out) {
#pragma omp parallel for schedule(static) num_threads(16)
    for (long long g = 0; g < rows / rb; g++) vox_wpack13_side_compact_groups(side, g, g + 1, K, rb, swiglu, out);
}
/* ---- fragment plane (the batched step's A operand; layout in the header comment) ---- */
#define VOX_WPACK13_FRAG_REC 416 /* dwords per (16-row group, 64-k block): 256 + 128 of fields, 32 of sign words */
/* dwords of the fragment plane of a [N, K] tensor; 0 for a shape it does not take */
static inline long long vox_wpack13_frag_words(long long N, long long K) {
    if (N <= 0 || K <= 0 || N % 16 || K % 64) return 0;
    return N / 16 * (K / 64) * VOX_WPACK13_FRAG_REC;
}
/* bf16 [N, K] of a packable tensor with its D -> 16-row groups g0..g1 of the fragment plane */
static inline void vox_wpack13_frag_groups(const uint16_t *w, long long g0, long long g1, long long K, int D,
                                           uint32_t *out) {
    const long long nb = K / 64;
    for (long long g = g0; g < g1; g++)
        for (long long b = 0; b < nb; b++) {
            uint32_t *rec = out + (g * nb + b) * VOX_WPACK13_FRAG_REC;
            uint16_t *sg = (uint16_t *)(rec + 384);
            for (int l = 0; l < 64; l++) {
                const uint16_t *p = w + (g * 16 + (l & 15)) * K + b * 64 + (l >> 4) * 16;
                uint32_t low[16], s = 0;
                for (int i = 0; i < 16; i++) {
                    const uint32_t c = vox_wpack13_code(p[i], D);
                    low[i] = c & 0xfff;
                    s |= (c >> 12) << ((i >> 1) + 8 * (i & 1));
                }
                for (int q = 0; q < 6; q++) {
                    const int t = 12 + 2 * (q / 3), sh = 4 * (q % 3);
                    const uint32_t d = low[2 * q] | ((low[t] >> sh) & 15) << 12 | low[2 * q + 1] << 16 |
                                       ((low[t + 1] >> sh) & 15) << 28;
                    rec[q < 4 ? 4 * l + q : 256 + 2 * l + q - 4] = d;
                }
                sg[l] = (uint16_t)s;
            }
        }
}
static inline void vox_wpack13_frag_layout_(const uint16_t *w, long long N, long long K, int D, uint32_t *out) {
    if (!vox_wpack13_frag_words(N, K)) return;
#pragma omp parallel for schedule(static) num_threads(16)
    for (long long g = 0; g < N / 16; g++) vox_wpack13_frag_groups(w, g, g + 1, K, D, out);
}
#endif
