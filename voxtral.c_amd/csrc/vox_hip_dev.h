// vox_hip_dev.h -- device helpers shared by the kernel files (bf16 conversion, DPP
// reductions, activations, the f32 -> 3 x bf16 split, 8/16-weight dot products).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vox_hip_internal.h"

namespace vox {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// streamed-once weights: non-temporal 16-B load (MI355X_MICROARCH.md row nt-weights)
__device__ __forceinline__ uint4 ldnt(const uint4* p) {
    u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ float bf2f(uint32_t bits16) { return __uint_as_float(bits16 << 16); }
__device__ __forceinline__ float bflo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bfhi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// round-to-nearest-even f32 -> bf16 bits: the native conversion (hipcc emits
// v_cvt_pk_bf16_f32 on gfx950, two values per instruction)
__device__ __forceinline__ uint32_t f2bf(float f) {
    const __bf16 b = (__bf16)f;
    return __builtin_bit_cast(unsigned short, b);
}

// Cross-lane reductions: DPP inside each 16-lane row (quad_perm xor1 / xor2, row half
// mirror, row mirror -- VALU ops with no LDS round trip), then two ds_bpermute steps
// across rows.  The pairing pattern is fixed, so results are deterministic.
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// v uniform within each row of 16 lanes: the 4 rows combined through scalar reads of lanes
// 0 / 16 / 32 / 48 (no ds_bpermute round trip); (r0 + r1) + (r2 + r3), the order of the
// xor-16-then-32 shuffle reduction, so the sums are the same bits
__device__ __forceinline__ float rows4_sum(float v) {
    const int iv = __float_as_int(v);
    const float a = __int_as_float(__builtin_amdgcn_readlane(iv, 0)), b = __int_as_float(__builtin_amdgcn_readlane(iv, 16));
    const float c = __int_as_float(__builtin_amdgcn_readlane(iv, 32)), d = __int_as_float(__builtin_amdgcn_readlane(iv, 48));
    return (a + b) + (c + d);
}
__device__ __forceinline__ float rows4_max(float v) {
    const int iv = __float_as_int(v);
    const float a = __int_as_float(__builtin_amdgcn_readlane(iv, 0)), b = __int_as_float(__builtin_amdgcn_readlane(iv, 16));
    const float c = __int_as_float(__builtin_amdgcn_readlane(iv, 32)), d = __int_as_float(__builtin_amdgcn_readlane(iv, 48));
    return fmaxf(fmaxf(a, b), fmaxf(c, d));
}
__device__ __forceinline__ float row_sum16(float v) {
    v += dpp<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp<0x141>(v);  // row_half_mirror
    v += dpp<0x140>(v);  // row_mirror
    return v;
}
__device__ __forceinline__ float row_max16(float v) {
    v = fmaxf(v, dpp<0xB1>(v));
    v = fmaxf(v, dpp<0x4E>(v));
    v = fmaxf(v, dpp<0x141>(v));
    v = fmaxf(v, dpp<0x140>(v));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    v = row_sum16(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
// All-DPP wave64 sum (no LDS round trip): the total lands in lane 63 only.
// row_bcast:15 adds row r-1's lane 15 into rows 1 and 3, row_bcast:31 adds lane 31 into rows 2 and 3.
__device__ __forceinline__ float wave_sum63(float v) {
    v = row_sum16(v);
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xA, 0xF, false));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xC, 0xF, false));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    v = row_max16(v);
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}

__device__ __forceinline__ float gelu_tanh(float v) {  // voxtral_kernels.c:505-513
    float x3 = v * v * v;
    float inner = 0.7978845608028654f * (v + 0.044715f * x3);
    return 0.5f * v * (1.0f + tanhf(inner));
}
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }
__device__ __forceinline__ float silu(float v) { return v / (1.0f + expf(-v)); }  // :498-503

// f32 -> three bf16 terms hi + mid + lo (= the exact f32 value; see k_gemm)
__device__ __forceinline__ void split3(float v, uint16_t& h, uint16_t& m, uint16_t& l) {
    const uint32_t b0 = f2bf(v);
    const float r1 = v - __uint_as_float(b0 << 16);
    const uint32_t b1 = f2bf(r1);
    const float r2 = r1 - __uint_as_float(b1 << 16);
    h = (uint16_t)b0;
    m = (uint16_t)b1;
    l = (uint16_t)f2bf(r2);
}

// element (row j, col k) of a fragment-major plane [16][K] (k_skl / k_skf B operand)
__device__ __forceinline__ size_t frag_off(int j, int k) {  // element (row j, col k) in a plane
    const int b = k >> 6, r = k & 63;
    return ((size_t)(b * 2 + ((r >> 3) & 1)) * 64 + (r >> 4) * 16 + j) * 8 + (r & 7);
}

// element (row j, column n) of a split-K result: the S partial slabs summed in order.  Rows
// come in blocks of 16 (k_skl's B operand): row j's slabs are those of row block j / 16,
// laid out [row block][S][16][N].
__device__ __forceinline__ float psum(const float* __restrict__ part, int S, int N, int j, int n) {
    part += (size_t)(j >> 4) * S * SK_ROWS * N;
    j &= 15;
    float v = part[(size_t)j * N + n];
    // unrolled: four slab loads in flight before their (in-order) adds
#pragma unroll 4
    for (int s = 1; s < S; s++) v += part[((size_t)s * SK_ROWS + j) * N + n];
    return v;
}
// the pair (n, n + 1) of psum (n even), every slab load of a chunk of 8 in flight before
// its adds (same order of additions: slab 0, 1, 2, ...)
__device__ __forceinline__ float2 psum2(const float* __restrict__ part, int S, int N, int j, int n) {
    part += (size_t)(j >> 4) * S * SK_ROWS * N + (size_t)(j & 15) * N + n;
    const size_t stride = (size_t)SK_ROWS * N;
    float2 v = *reinterpret_cast<const float2*>(part);
    for (int s0 = 1; s0 < S; s0 += 8) {
        float2 t[8];
#pragma unroll
        for (int c = 0; c < 8; c++)
            t[c] = s0 + c < S ? *reinterpret_cast<const float2*>(part + (s0 + c) * stride) : make_float2(0.f, 0.f);
#pragma unroll
        for (int c = 0; c < 8; c++)
            if (s0 + c < S) {
                v.x += t[c].x;
                v.y += t[c].y;
            }
    }
    return v;
}
// element (row j, col k) of the fragment-major planes of a row set: plane p of row block j / 16
__device__ __forceinline__ size_t frag_at(int j, int K, int p, int k) {
    return ((size_t)(j >> 4) * 3 + p) * SK_ROWS * K + frag_off(j & 15, k);
}

// dot of 8 bf16 weights (one uint4) with 8 f32 activations
__device__ __forceinline__ float dot8(uint4 w, float4 a, float4 b, float acc) {
    acc = fmaf(bflo(w.x), a.x, acc);
    acc = fmaf(bfhi(w.x), a.y, acc);
    acc = fmaf(bflo(w.y), a.z, acc);
    acc = fmaf(bfhi(w.y), a.w, acc);
    acc = fmaf(bflo(w.z), b.x, acc);
    acc = fmaf(bfhi(w.z), b.y, acc);
    acc = fmaf(bflo(w.w), b.z, acc);
    acc = fmaf(bfhi(w.w), b.w, acc);
    return acc;
}

// dot of 8 wpack13 weights (vox_wpack.h: three dwords of half pairs whose spare low bits,
// with the chunk's two side nibbles, hold the fourth pair) with 8 f32 activations already
// scaled by 2^D.  Same k order as dot8; the halves enter the f32 FMA as they are
// (v_fma_mix_f32), and half * (x * 2^D) is the real number w * x, so every FMA rounds as
// dot8's does.  sd: the side dword of this chunk's slot, q: the slot's index in it.
__device__ __forceinline__ float hlo(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
__device__ __forceinline__ float hhi(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
__device__ __forceinline__ float dot8h(uint4 w, uint32_t sd, int q, float4 a, float4 b, float acc) {
    const uint32_t HM = 0xfff8fff8u, SM = 0x00070007u;
    const uint32_t t = (w.x & SM) | ((w.y & SM) << 3) | ((w.z & SM) << 6);
    const uint32_t p3 = (t << 3) | ((sd << (4 * q)) & 0xf000f000u);
    const uint32_t p0 = w.x & HM, p1 = w.y & HM, p2 = w.z & HM;
    acc = fmaf(hlo(p0), a.x, acc);
    acc = fmaf(hhi(p0), a.y, acc);
    acc = fmaf(hlo(p1), a.z, acc);
    acc = fmaf(hhi(p1), a.w, acc);
    acc = fmaf(hlo(p2), b.x, acc);
    acc = fmaf(hhi(p2), b.y, acc);
    acc = fmaf(hlo(p3), b.z, acc);
    acc = fmaf(hhi(p3), b.w, acc);
    return acc;
}

// dot of 8 wmx4 weights (vox_wmx4.h: one dword of e2m1 nibbles, weight k in bits 4k .. 4k + 3,
// and the block's e8m0 scale byte) with 8 f32 activations.  v_cvt_scalef32_pk_f32_fp4 turns
// byte `sel` of the dword and the scale 2^(byte - 127), given as the f32 byte << 23, into the
// two f32 weights e2m1 * scale: exact, and the f32 that the bf16 weight widens to, so every
// FMA is dot8's, in dot8's order.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float dot8m4(uint32_t w, uint32_t scale_byte, float4 a, float4 b, float acc) {
    const float sc = __uint_as_float(scale_byte << 23);
    const f32x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 0);
    const f32x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 1);
    const f32x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 2);
    const f32x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 3);
    acc = fmaf(p0.x, a.x, acc);
    acc = fmaf(p0.y, a.y, acc);
    acc = fmaf(p1.x, a.z, acc);
    acc = fmaf(p1.y, a.w, acc);
    acc = fmaf(p2.x, b.x, acc);
    acc = fmaf(p2.y, b.y, acc);
    acc = fmaf(p3.x, b.z, acc);
    acc = fmaf(p3.y, b.w, acc);
    return acc;
}

// dot8m4 in two halves, for a kernel that feeds one decoded chunk to several input rows
// (k_gemvr): dec8m4 runs dot8m4's four converts once, dot8f runs dot8's FMAs in dot8's order
// on the eight f32 weights.  dot8f(dec8m4(w, s), a, b, acc) has dot8m4(w, s, a, b, acc)'s bits.
struct f32x8 {
    f32x2 p[4];
};
__device__ __forceinline__ f32x8 dec8m4(uint32_t w, uint32_t scale_byte) {
    const float sc = __uint_as_float(scale_byte << 23);
    f32x8 d;
    d.p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 0);
    d.p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 1);
    d.p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 2);
    d.p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 3);
    return d;
}
__device__ __forceinline__ float dot8f(const f32x8& d, float4 a, float4 b, float acc) {
    acc = fmaf(d.p[0].x, a.x, acc);
    acc = fmaf(d.p[0].y, a.y, acc);
    acc = fmaf(d.p[1].x, a.z, acc);
    acc = fmaf(d.p[1].y, a.w, acc);
    acc = fmaf(d.p[2].x, b.x, acc);
    acc = fmaf(d.p[2].y, b.y, acc);
    acc = fmaf(d.p[3].x, b.z, acc);
    acc = fmaf(d.p[3].y, b.w, acc);
    return acc;
}

// dot of 16 int8 weights (one uint4, Q8 rows) with 16 f32 activations: each byte is
// sign-extended and converted exactly (q8_matvec_fused, voxtral_kernels.c:277-318)
__device__ __forceinline__ float i8f(uint32_t w, int b) { return (float)((int32_t)(w << (24 - 8 * b)) >> 24); }
__device__ __forceinline__ float dot16q(uint4 w, const float4 (&x)[4], float acc) {
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        acc = fmaf(i8f(d[k], 0), x[k].x, acc);
        acc = fmaf(i8f(d[k], 1), x[k].y, acc);
        acc = fmaf(i8f(d[k], 2), x[k].z, acc);
        acc = fmaf(i8f(d[k], 3), x[k].w, acc);
    }
    return acc;
}

// 8 int8 (two dwords, k ascending) as the 8 bf16 of an MFMA operand: every int8 is a bf16, so
// the f32 conversion's high half is the value itself (k_skf / k_skl / k_gemmf, WF_Q8)
__device__ __forceinline__ bf16x8 i8x8_bf16(uint32_t lo, uint32_t hi) {
    uint32_t h[8];
#pragma unroll
    for (int b = 0; b < 4; b++) {
        h[b] = __float_as_uint(i8f(lo, b)) >> 16;
        h[4 + b] = __float_as_uint(i8f(hi, b)) >> 16;
    }
    return __builtin_bit_cast(bf16x8, make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)));
}

// ============================================================================
// Decoder KV element type.  f32 by default (the CPU reference's cache); the opt-in 16-bit
// mode (VOX_DECODER_KV_FP16, voxtral.c:189-190, voxtral_decoder.c:180-243) stores IEEE half:
// stores round to nearest even, loads widen to f32, all arithmetic stays f32.  Kernels that
// read the ring are templated on the element type; the two single-store epilogues (decode
// QKV GEMV, batched RoPE + append) take it as a uniform runtime value (KV_F32 / KV_F16 / KV_FP8).
// ============================================================================
typedef _Float16 kvh_t;
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
// The opt-in one-byte mode (VOX_HIP_KV_FP8, KV_FP8): OCP FP8 E4M3 without a scale, by the
// rule of vox_kv8.h.  Loads widen with v_cvt_pk_f32_fp8 (exact); the store clamps to +-448 in
// f32 first (the conversion by itself gives NaN past the largest finite value, the rule
// saturates) and then rounds with v_cvt_pk_fp8_f32 (nearest, ties to even, subnormals kept);
// NaN is written as 0x7f with the sign whatever the instruction makes of it.
__device__ __forceinline__ float kv8_clamp(float v) { return v > 448.f ? 448.f : v < -448.f ? -448.f : v; }
__device__ __forceinline__ unsigned kv8_fix_nan(float v, unsigned code) {
    return v != v ? (0x7fu | ((__float_as_uint(v) >> 24) & 0x80u)) : code;
}
// the pair (a, b) as two codes, a in bits 0..7
__device__ __forceinline__ unsigned kv8_enc2(float a, float b) {
    const unsigned w = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(a), kv8_clamp(b), 0, false);
    return kv8_fix_nan(a, w & 0xffu) | (kv8_fix_nan(b, (w >> 8) & 0xffu) << 8);
}
struct kv8_t {
    uint8_t b;
    kv8_t() = default;
    __device__ __forceinline__ explicit kv8_t(float v) : b((uint8_t)(kv8_enc2(v, v) & 0xffu)) {}
    __device__ __forceinline__ explicit operator float() const {
        return __builtin_amdgcn_cvt_pk_f32_fp8((int)b, false)[0];
    }
};
static_assert(sizeof(kv8_t) == 1, "kv8_t: one byte per ring element");
// ring element type of the launchers' kvt argument
template <class T> __device__ __forceinline__ float4 kv_ld4(const T* p) {
    if constexpr (sizeof(T) == 4) {
        return *reinterpret_cast<const float4*>(p);
    } else if constexpr (sizeof(T) == 2) {
        const h16x4 h = *reinterpret_cast<const h16x4*>(p);
        return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
    } else {
        const int w = *reinterpret_cast<const int*>(p);
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
        return make_float4(lo[0], lo[1], hi[0], hi[1]);
    }
}
template <class T> __device__ __forceinline__ float2 kv_ld2(const T* p) {
    if constexpr (sizeof(T) == 4) {
        return *reinterpret_cast<const float2*>(p);
    } else if constexpr (sizeof(T) == 2) {
        const h16x2 h = *reinterpret_cast<const h16x2*>(p);
        return make_float2((float)h[0], (float)h[1]);
    } else {
        const auto v = __builtin_amdgcn_cvt_pk_f32_fp8((int)*reinterpret_cast<const uint16_t*>(p), false);
        return make_float2(v[0], v[1]);
    }
}
template <class T> __device__ __forceinline__ float kv_round(float v) { return (float)(T)v; }
template <class T> __device__ __forceinline__ void kv_st2(T* p, float a, float b) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float2*>(p) = make_float2(a, b);
    } else if constexpr (sizeof(T) == 2) {
        *reinterpret_cast<h16x2*>(p) = h16x2{(T)a, (T)b};
    } else {
        *reinterpret_cast<uint16_t*>(p) = (uint16_t)kv8_enc2(a, b);
    }
}
// A value as the f32 it rounds to, before a half store.  Without it the compiler folds a roped
// key's last fma and the conversion into v_fma_mixlo_f16, which rounds the exact fma once: at an
// f32 value that lies halfway between two halves the stored half is then not the nearest-even
// rounding of the f32 ring's element.  The encoder's half instances store kv_f32(...) values, so
// their rings hold half(f32 element) bit for bit; the decoder's instances are as they were.
__device__ __forceinline__ float kv_f32(float v) {
    asm volatile("" : "+v"(v));
    return v;
}
// element e of a ring (f32, half or fp8 by the element type) written as the pair (a, b) at e, e + 1
__device__ __forceinline__ void kv_st2_rt(float* base, size_t e, float a, float b, int kvt) {
    if (kvt == KV_FP8) kv_st2(reinterpret_cast<kv8_t*>(base) + e, a, b);
    else if (kvt == KV_F16) kv_st2(reinterpret_cast<kvh_t*>(base) + e, a, b);
    else kv_st2(base + e, a, b);
}

// stream_fill_alts (voxtral.c:955-1010) partials for one logit: running max / sum of
// exp for the softmax, and an ascending-id-stable top-4 of ids >= TOKEN_TEXT_MIN (rows
// arrive in ascending order, so a strict '>' keeps the lower id first on ties).
__device__ __forceinline__ void alt_row(float v, int r, float& am, float& as, float (&tv)[4], int (&ti)[4]) {
    if (v > am) {
        as = as * expf(am - v) + 1.0f;
        am = v;
    } else {
        as += expf(v - am);
    }
    if (r >= ALT_TEXT_MIN && v > tv[3]) {
        // v replaces the smallest and rises past every strictly smaller entry; the entries
        // above it are sorted, so no later pair swaps.  Static indices only: a run-time index
        // into tv / ti put both arrays in scratch (48 B per lane).
        tv[3] = v;
        ti[3] = r;
#pragma unroll
        for (int k = 3; k > 0; k--) {
            const bool up = tv[k] > tv[k - 1];
            const float fv = tv[k];
            const int fi = ti[k];
            tv[k] = up ? tv[k - 1] : fv;
            ti[k] = up ? ti[k - 1] : fi;
            tv[k - 1] = up ? fv : tv[k - 1];
            ti[k - 1] = up ? fi : ti[k - 1];
        }
    }
}

}  // namespace vox
