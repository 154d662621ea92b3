// vox_hip_gemv.h -- the two weight-streaming GEMV kernel templates, k_gemv and k_gemvr, and nothing else.
// Each weight format's instances are made by its own vox_hip_gemv_<format>.hip (vox_hip_gemv_pick.h).
#pragma once
#include "vox_hip_internal.h"
#include "vox_hip_dev.h"

namespace vox {

// ============================================================================
// M=1 weight-streaming GEMV with fused prologue / epilogue (decoder step).
//
// A block (4 waves) owns groups of RB rows and streams them with K split across its
// waves: wave w reads the 1-KiB chunk blocks j*4+w of every row, so each wave keeps only
// its quarter of x in registers (loaded once per block, normalised there when PRO_NORM),
// never stages x through LDS, and a launch needs no more blocks than CUs x 4 to stay
// balanced (grid-stride over groups).  Weights: 16-B non-temporal loads straight to
// VGPRs (cdna_hip_programming.md "GEMV / M <= 16" row).  Partial sums meet in LDS; wave
// 0 applies the epilogue.  Summation order is fixed (deterministic).
// ============================================================================
template <int EPI, int RB>
__device__ __forceinline__ void gemv_rows(int g, int (&rows)[RB]) {
#pragma unroll
    for (int i = 0; i < RB; i++) {
        if (EPI == EPI_SWIGLU) {
            // pair i = (w1 row, w3 row) of hidden unit u = g*RB/2 + i/2 (16-row interleave)
            const int u = g * (RB / 2) + (i >> 1);
            rows[i] = ((u >> 4) << 5) + (u & 15) + ((i & 1) << 4);
        } else {
            rows[i] = g * RB + i;
        }
    }
}

// Weight rows come in through a buffer descriptor: the row offset is wave-uniform (an SGPR
// soffset) and each lane keeps one 32-bit chunk offset per K round (voff), instead of a
// 64-bit address per (row, round) -- the register count sets how many blocks stay resident.
// Non-temporal (aux = 2: nt): every weight byte is read once per step.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
template <int RB, int KQ, bool WP = false>
__device__ __forceinline__ void gemv_load(__amdgpu_buffer_rsrc_t W, int rowbytes, const int (&rows)[RB],
                                          const int (&voff)[KQ], uint4 (&wv)[KQ][RB]) {
#pragma unroll
    for (int j = 0; j < KQ; j++)
#pragma unroll
        for (int i = 0; i < RB; i++) {
            if constexpr (WP) {  // wpack13: 12-B chunks
                const u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(W, voff[j], rows[i] * rowbytes, 2);
                wv[j][i] = make_uint4(v.x, v.y, v.z, 0u);
                continue;
            }
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(W, voff[j], rows[i] * rowbytes, 2);
            wv[j][i] = make_uint4(v.x, v.y, v.z, v.w);
        }
}

// Q8 rows (WQ8): 16-B chunks of 16 int8, so a lane holds 16 x values per chunk, and the
// group's RB row scales are fetched with its weights (applied before the epilogue:
// y = scale * sum + bias, voxtral_kernels.c:316).
#ifdef VOX_GEMV_STAMPS
// diagnostic build only (tools/kbench_stamps): per block s_memrealtime at entry, when the
// first group's weights have been consumed, and at exit (one pointer per format object, set
// together by gemv_set_stamps)
static __device__ unsigned long long* g_gemv_stamps;
#define GEMV_STAMP(k) \
    do { if (g_gemv_stamps && tid == 0) g_gemv_stamps[(size_t)blockIdx.x * 4 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define GEMV_STAMP(k) do {} while (0)
#endif

// wpack13 rows (WF_P13, vox_wpack.h): 12-B chunks of 8 weights as IEEE halves plus one side
// dword record per (group, thread), fetched with the group's weights by one load; x is
// scaled by 2^D once per block after the prologue.  ldexpf is exact for 0 and for |x| in
// [2^(-126-D), 2^(127-D)); |D| <= 40 (VOX_WPACK_MAX_D) puts those bounds at 2^-86 and 2^87
// or beyond, past anything an RMSNorm output, an attention output or a SwiGLU product of
// this model reaches.  Every output is then bit-identical to the bf16 instance's.
template <int SW>
__device__ __forceinline__ void gemv_load_side(__amdgpu_buffer_rsrc_t S, int voff, int soff, uint32_t (&sd)[SW]) {
    if constexpr (SW == 1) {
        sd[0] = __builtin_amdgcn_raw_buffer_load_b32(S, voff, soff, 2);
    } else if constexpr (SW == 2) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(S, voff, soff, 2);
        sd[0] = v.x; sd[1] = v.y;
    } else if constexpr (SW == 3) {
        const u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(S, voff, soff, 2);
        sd[0] = v.x; sd[1] = v.y; sd[2] = v.z;
    } else {
        static_assert(SW % 4 != 3, "side record size");
#pragma unroll
        for (int o = 0; o + 4 <= SW; o += 4) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(S, voff + o * 4, soff, 2);
            sd[o] = v.x; sd[o + 1] = v.y; sd[o + 2] = v.z; sd[o + 3] = v.w;
        }
        if constexpr (SW % 4 == 1) sd[SW - 1] = __builtin_amdgcn_raw_buffer_load_b32(S, voff + (SW - 1) * 4, soff, 2);
        if constexpr (SW % 4 == 2) {
            const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(S, voff + (SW - 2) * 4, soff, 2);
            sd[SW - 2] = v.x; sd[SW - 1] = v.y;
        }
    }
}

// wmx4 plane (WF_MX4, vox_wmx4.h): one record of RW = RB + ceil(RB / 4) dwords per (group,
// chunk): the RB rows' nibble dwords of that chunk and their blocks' e8m0 scale bytes, so the
// thread that owns a chunk fetches a group's weights with one record load per K round (the
// wave's 64 records are contiguous).  dot8m4 rebuilds each weight as the exact f32 of the bf16
// weight and runs dot8's FMAs: every output is bit-identical to the bf16 instance's.
template <int RW, int KQ>
__device__ __forceinline__ void gemv_load_mx4(__amdgpu_buffer_rsrc_t W, int soff, const int (&voff)[KQ],
                                              uint32_t (&mr)[KQ][RW]) {
#pragma unroll
    for (int j = 0; j < KQ; j++) gemv_load_side<RW>(W, voff[j], soff, mr[j]);
}

template <int PRO, int EPI, int RB, int KQ, int WF>
__global__ __launch_bounds__(256) void k_gemv(GemvArgs a) {
    constexpr bool WQ8 = WF == WF_Q8, WP = WF == WF_P13, WM = WF == WF_MX4;
    constexpr int XPC = WQ8 ? 4 : 2;  // float4 of x per 16-B chunk
    constexpr int SW = WP ? (KQ * RB + 3) / 4 : 1;  // side dwords per (group, thread)
    constexpr int RW = RB + (RB + 3) / 4;           // wmx4 record dwords per (group, chunk)
    __shared__ float red[2][4][RB];
    __shared__ float sred[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, KC = WQ8 ? K >> 4 : K >> 3;
    const int ngroups = a.rows / RB;
    // Groups: block b takes b, b + G, b + 2G, ... (static; run-time claims measured 3-4x
    // slower)
    const int G = gridDim.x;
    int g = blockIdx.x;
    int rows[RB];
    uint4 wv[WM ? 1 : KQ][RB];
    uint32_t mr[WM ? KQ : 1][RW];
    float wsc[RB];
    GEMV_STAMP(0);
    bool first_group = true;
    // wmx4: "rowbytes" is a group's bytes (KC records), the plane ngroups of them
    const int rowbytes = WM ? KC * (RW * 4) : WP ? KC * 12 : K * (WQ8 ? 1 : 2);
    void* const wbase = const_cast<void*>(WM ? a.wm_plane : WP ? a.wp_main : a.W);
    const __amdgpu_buffer_rsrc_t wrs =
        __builtin_amdgcn_make_buffer_rsrc(wbase, 0, (WM ? ngroups : a.rows) * rowbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wnone = __builtin_amdgcn_make_buffer_rsrc(wbase, 0, 0, 0x00020000);
    void* const sbase = const_cast<void*>(WP ? a.wp_side : a.W);
    const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(sbase, 0, ngroups * (256 * SW * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t snone = __builtin_amdgcn_make_buffer_rsrc(sbase, 0, 0, 0x00020000);
    uint32_t sd[SW];
    // chunk offsets per K round; chunks past K (K not a multiple of 16 B * 256) re-load
    // chunk 0 and meet x = 0: every load is unconditional, so hipcc issues them all before
    // the first wait (a guarded load makes it wait vmcnt(0) at each branch join)
    int voff[KQ];
#pragma unroll
    for (int j = 0; j < KQ; j++) {
        const int c0 = (j * 4 + wave) * 64 + lane;
        voff[j] = (c0 < KC ? c0 : 0) * (WM ? RW * 4 : WP ? 12 : 16);
    }
    // first group's weights are independent of x: issue them before the prologue
    gemv_rows<EPI, RB>(g, rows);
    if (WP) gemv_load_side<SW>(srs, tid * (SW * 4), g * (256 * SW * 4), sd);  // first: every chunk needs it
    if constexpr (WM) gemv_load_mx4<RW, KQ>(wrs, g * rowbytes, voff, mr);
    else gemv_load<RB, KQ, WP>(wrs, rowbytes, rows, voff, wv);
    if ((EPI == EPI_LOGITS || EPI == EPI_LOGITS_ALT) && WQ8 && wave == 0) {
#pragma unroll
        for (int i = 0; i < RB; i++) wsc[i] = a.wscale[rows[i]];
    }

    float4 xr[KQ][XPC];
    // bf16: the RMSNorm weights (and ada) go out with x -- independent of the row sum, so the
    // prologue waits for one L2 round trip instead of two (C2 +0.7 %, W1|W3 21.0 -> 20.8 us);
    // Q8 (16 x values per chunk) keeps them after the sum: the early registers cost it 0.5 %
    // (profiles/r5_gemv_prologue_ab.txt)
    constexpr bool EARLY = PRO != PRO_NONE && !WQ8;
    constexpr int NXP = EARLY ? XPC : 1;
    float4 nwr[KQ][NXP], adr[KQ][NXP];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < KQ; j++) {
        const int c = (j * 4 + wave) * 64 + lane;
        const float4* xp = reinterpret_cast<const float4*>(a.x) + XPC * (c < KC ? c : 0);
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int h = 0; h < XPC; h++) {
            const float4 xv = xp[h];
            xr[j][h] = c < KC ? xv : z;
        }
        if (EARLY) {
            const int cc = c < KC ? c : 0;
            const float4* wp = reinterpret_cast<const float4*>(a.norm_w) + XPC * cc;
            const float4* ap = reinterpret_cast<const float4*>(PRO == PRO_NORM_ADA ? a.ada : a.norm_w) + XPC * cc;
#pragma unroll
            for (int h = 0; h < NXP; h++) {
                nwr[j][h] = wp[h];
                if (PRO == PRO_NORM_ADA) adr[j][h] = ap[h];
            }
        }
        if (PRO != PRO_NONE) {
#pragma unroll
            for (int h = 0; h < XPC; h++) {
                const float4 v = xr[j][h];
                ss = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, ss))));
            }
        }
    }
    if (PRO != PRO_NONE) {
        // RMSNorm prologue (voxtral_kernels.c:475-492; ada: voxtral_decoder.c:742-745)
        ss = wave_sum(ss);
        if (lane == 0) sred[wave] = ss;
        __syncthreads();
        const float tot = sred[0] + sred[1] + sred[2] + sred[3];
        const float inv = 1.0f / sqrtf(tot / (float)K + a.eps);
#pragma unroll
        for (int j = 0; j < KQ; j++) {
            const int c0 = (j * 4 + wave) * 64 + lane;
            const int c = c0 < KC ? c0 : 0;
            const float4* wp = reinterpret_cast<const float4*>(a.norm_w) + XPC * c;
            const float4* ap = reinterpret_cast<const float4*>(PRO == PRO_NORM_ADA ? a.ada : a.norm_w) + XPC * c;
#pragma unroll
            for (int h = 0; h < XPC; h++) {
                float4 v = xr[j][h];
                const float4 nw = EARLY ? nwr[j][h % NXP] : wp[h];
                v.x = v.x * inv * nw.x; v.y = v.y * inv * nw.y;
                v.z = v.z * inv * nw.z; v.w = v.w * inv * nw.w;
                if (PRO == PRO_NORM_ADA) {
                    const float4 ad = EARLY ? adr[j][h % NXP] : ap[h];
                    v.x *= (1.0f + ad.x); v.y *= (1.0f + ad.y);
                    v.z *= (1.0f + ad.z); v.w *= (1.0f + ad.w);
                }
                xr[j][h] = v;
            }
        }
    }

    if (WP) {
#pragma unroll
        for (int j = 0; j < KQ; j++)
#pragma unroll
            for (int h = 0; h < XPC; h++) {
                float4 v = xr[j][h];
                v.x = ldexpf(v.x, a.wp_d); v.y = ldexpf(v.y, a.wp_d);
                v.z = ldexpf(v.z, a.wp_d); v.w = ldexpf(v.w, a.wp_d);
                xr[j][h] = v;
            }
    }

    constexpr bool QKVE = (EPI == EPI_QKV || EPI == EPI_QKV_BIAS);
    int lp = 0;
    if (QKVE) lp = a.state ? a.state[0] : a.pos;
    float best = -INFINITY;
    int besti = 0x7fffffff;
    // EPI_LOGITS_ALT: online softmax partial (max, sum exp) and the 4 largest text logits
    float am = -INFINITY, as = 0.f, tv[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int ti[4] = {-1, -1, -1, -1};
    // Epilogue ownership: lane l of wave 0 finishes row l (STORE / RESID) or row pair
    // (2l, 2l+1) (QKV rope pairs, SWIGLU w1/w3 pairs), so the epilogue's reads (residual,
    // bias, rope, Q8 scales) go out in parallel at the top of the iteration instead of one
    // dependent round trip per row after the reduction.  The LM head keeps one lane (its
    // running argmax is sequential over ascending rows).
    constexpr bool LOGIT = (EPI == EPI_LOGITS || EPI == EPI_LOGITS_ALT);
    constexpr bool PAIRED = (QKVE || EPI == EPI_SWIGLU);
    constexpr int NL = LOGIT ? 1 : (PAIRED ? RB / 2 : RB);
    const bool owner = wave == 0 && lane < NL;
    const int i0 = PAIRED ? 2 * lane : lane;
    int buf = 0;
    for (;;) {
        const int gcur = g;
        // epilogue inputs of this group (independent of the dot products)
        int er0 = 0, er1 = 0;
        float ein0 = 0.f, ein1 = 0.f, esc0 = 1.f, esc1 = 1.f, eb0 = 0.f, eb1 = 0.f;
        if (!LOGIT && owner) {
            int rr[RB];
            gemv_rows<EPI, RB>(gcur, rr);
#pragma unroll
            for (int i = 0; i < RB; i++) {
                if (i == i0) er0 = rr[i];
                if (i == i0 + 1) er1 = rr[i];
            }
            if (WQ8) {
                esc0 = a.wscale[er0];
                if (PAIRED) esc1 = a.wscale[er1];
            }
            if (EPI == EPI_RESID) ein0 = a.y[er0] + (a.bias ? a.bias[er0] : 0.f);
            if (EPI == EPI_STORE) ein0 = a.bias ? a.bias[er0] : 0.f;
            if (EPI == EPI_QKV_BIAS) {
                eb0 = a.bias[er0];
                eb1 = a.bias[er1];
            }
            if (QKVE && er0 < a.qd + a.kvd) {
                const int col = er0 < a.qd ? er0 : er0 - a.qd;
                const float* rp = a.rope + (size_t)lp * a.hd + ((col % a.hd) & ~1);
                ein0 = rp[0];
                ein1 = rp[1];
            }
        }
        float acc[RB];
#pragma unroll
        for (int i = 0; i < RB; i++) acc[i] = 0.f;
#pragma unroll
        for (int j = 0; j < KQ; j++)
#pragma unroll
            for (int i = 0; i < RB; i++) {
                if constexpr (WM) acc[i] = dot8m4(mr[j][i], (mr[j][RB + (i >> 2)] >> (8 * (i & 3))) & 0xffu, xr[j][0], xr[j][1], acc[i]);
                else if (WQ8) acc[i] = dot16q(wv[j][i], reinterpret_cast<const float4(&)[4]>(xr[j]), acc[i]);
                else if (WP) acc[i] = dot8h(wv[j][i], sd[(j * RB + i) >> 2], (j * RB + i) & 3, xr[j][0], xr[j][1], acc[i]);
                else acc[i] = dot8(wv[j][i], xr[j][0], xr[j][XPC - 1], acc[i]);
            }
        if (first_group) {
            GEMV_STAMP(1);
            first_group = false;
        }
        int rcur[RB];
        float scur[RB];
        if (LOGIT) {
#pragma unroll
            for (int i = 0; i < RB; i++) {
                rcur[i] = rows[i];
                scur[i] = WQ8 ? wsc[i] : 1.0f;
            }
        }
        g += G;
        // The next group's loads go out before this group's reduction, unconditionally: a
        // load under `if (more)` keeps the old weight registers alive across the branch and
        // doubles the weight register set (fewer resident blocks).  Past the last group they
        // go through a zero-length descriptor: the range check returns zeros, no traffic.
        {
            const bool more = g < ngroups;
            gemv_rows<EPI, RB>(more ? g : 0, rows);
            if (WP) gemv_load_side<SW>(more ? srs : snone, tid * (SW * 4), (more ? g : 0) * (256 * SW * 4), sd);
            if constexpr (WM) gemv_load_mx4<RW, KQ>(more ? wrs : wnone, (more ? g : 0) * rowbytes, voff, mr);
            else gemv_load<RB, KQ, WP>(more ? wrs : wnone, rowbytes, rows, voff, wv);
            if (LOGIT && WQ8 && wave == 0) {
#pragma unroll
                for (int i = 0; i < RB; i++) wsc[i] = a.wscale[rows[i]];
            }
        }
#pragma unroll
        for (int i = 0; i < RB; i++) acc[i] = wave_sum(acc[i]);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < RB; i++) red[buf][wave][i] = acc[i];
        }
        __syncthreads();
        if (!LOGIT && owner) {
            float v0 = ((red[buf][0][i0] + red[buf][1][i0]) + red[buf][2][i0]) + red[buf][3][i0];
            float v1 = 0.f;
            if (PAIRED) v1 = ((red[buf][0][i0 + 1] + red[buf][1][i0 + 1]) + red[buf][2][i0 + 1]) + red[buf][3][i0 + 1];
            if (WQ8) {
                v0 *= esc0;
                v1 *= esc1;
            }
            if (EPI == EPI_QKV_BIAS) {
                v0 += eb0;
                v1 += eb1;
            }
            if (EPI == EPI_STORE || EPI == EPI_RESID) {
                a.y[er0] = ein0 + v0;  // RESID: residual + bias were read at the top
            } else if (EPI == EPI_SWIGLU) {
                a.y[gcur * (RB / 2) + lane] = silu(v0) * v1;
            } else if (QKVE) {
                if (er0 < a.qd + a.kvd) {
                    const float o0 = v0 * ein0 - v1 * ein1, o1 = v0 * ein1 + v1 * ein0;
                    if (er0 < a.qd) {
                        a.y[er0] = o0;
                        a.y[er1] = o1;
                    } else {
                        // (o0 / o1 are f32 values here: shared with the q store above and passed through
                        // the runtime kvt switch, no k_gemv instance folds them into v_fma_mixlo_f16 -- see
                        // kv_f32; this kernel is the decoder's too, so it carries no barrier of its own,
                        // and tests/test_gpu_enc_kv16.py holds the encoder's one-row path to the exact rule)
                        kv_st2_rt(a.Kc, (size_t)(lp % a.cap) * a.kvd + (er0 - a.qd), o0, o1, a.kvt);
                    }
                } else {
                    kv_st2_rt(a.Vc, (size_t)(lp % a.cap) * a.kvd + (er0 - a.qd - a.kvd), v0, v1, a.kvt);
                }
            }
        }
        if (LOGIT && wave == 0 && lane == 0) {
            float v[RB];
#pragma unroll
            for (int i = 0; i < RB; i++) {
                v[i] = ((red[buf][0][i] + red[buf][1][i]) + red[buf][2][i]) + red[buf][3][i];
                if (WQ8) v[i] *= scur[i];
            }
#pragma unroll
            for (int i = 0; i < RB; i++) {
                a.y[rcur[i]] = v[i];
                // first max wins (voxtral_decoder.c:771-779): rows ascend within a block
                if (v[i] > best) { best = v[i]; besti = rcur[i]; }
                if (EPI == EPI_LOGITS_ALT) alt_row(v[i], rcur[i], am, as, tv, ti);
            }
        }
        buf ^= 1;
        if (g >= ngroups) break;
    }
    GEMV_STAMP(2);
    if ((EPI == EPI_LOGITS || EPI == EPI_LOGITS_ALT) && wave == 0 && lane == 0) {
        a.part_val[blockIdx.x] = best;
        a.part_idx[blockIdx.x] = besti;
        if (EPI == EPI_LOGITS_ALT) {
            float* pa = a.part_alt + (size_t)blockIdx.x * ALT_PART;
            pa[0] = am;
            pa[1] = as;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                pa[2 + k] = tv[k];
                pa[6 + k] = __int_as_float(ti[k]);
            }
        }
    }
}

// ============================================================================
// R-row weight-streaming GEMV (R = 1, 2, 4, 8: the slot buckets of a small batched decode
// step): y[r] = W x[r].  k_gemv's block, row groups, grid, chunk mapping, non-temporal buffer
// loads, early next-group loads and zero-length descriptor, so the P13 instance streams the
// model's own wpack13 planes and the MX4 instance its wmx4 GEMV plane (one record load per K
// round, k_gemv<WF_MX4>'s fetch; each (round, row) nibble dword is decoded to eight f32 once
// and feeds the R chains); every weight register feeds R FMA chains.  The x rows of a pass
// live in registers (R * KQ * 8 floats per thread).  More than 160 floats (R * KQ > 20: W2 of
// the full model at 8 rows would take 320) do not fit beside the weights: such an instance
// runs two passes of R / 2 rows over the block's groups and reads its weights twice
// (DESIGN.md 18.3).  The Q8 instance (WF_Q8) streams int8 rows as k_gemv<WF_Q8>
// does: 16 weights per chunk, so R * KQ * 16 floats of x, the same 160-float bound per pass
// (up to four passes), dot16q per (chunk, row) and the row's f32 scale times the reduced sum
// in the epilogue owner, before the epilogue.
//
// Each row's arithmetic is k_gemv's, in k_gemv's order, in registers of its own: chunks in j
// order, the wave sum, the four waves added ((0 + 1) + 2) + 3, and the RMSNorm prologue per
// row.  So the bits of y[r] depend on W and x[r] alone -- not on R, on r or on the other
// rows -- and equal k_gemv's for every shape.
//
// Epilogues per row r: STORE / RESID on row r of y (stride ldy), SWIGLU into row r of the
// hidden buffer, QKV with RoPE at slots[r].pos, q into row r of y and K/V into the slot's own
// rings (a slot that is not live appends nothing; its q row is never read).
// ============================================================================
// Q8 instance: rows per pass.  A pass holds RP * KQ * 16 floats of x per lane, at most the 160
// the bf16 instances hold; wider instances run R / RP passes
constexpr int gemvr_rp_q8(int R, int KQ) {
    int rp = R;
    while (rp > 1 && rp * KQ * 16 > 160) rp /= 2;
    return rp;
}

template <int PRO, int EPI, int RB, int KQ, int WF, int R>
__global__ __launch_bounds__(256) void k_gemvr(GemvRArgs ra) {
    constexpr bool WQ8 = WF == WF_Q8, WP = WF == WF_P13, WM = WF == WF_MX4;
    constexpr int XPC = WQ8 ? 4 : 2;  // float4 of x per 16-B chunk
    constexpr int SW = WP ? (KQ * RB + 3) / 4 : 1;  // side dwords per (group, thread)
    constexpr int RW = RB + (RB + 3) / 4;           // wmx4 record dwords per (group, chunk)
    constexpr int RP = WQ8 ? gemvr_rp_q8(R, KQ) : R * KQ > 20 ? R / 2 : R;  // rows per pass
    constexpr bool QKVE = EPI == EPI_QKV;
    constexpr bool PAIRED = QKVE || EPI == EPI_SWIGLU;
    constexpr int NL = PAIRED ? RB / 2 : RB;        // epilogue lanes per row
    static_assert(RP * NL <= 64, "the epilogue owners are lanes of wave 0");
    __shared__ float red[2][4][RP][RB];
    __shared__ float sred[4][RP];
    const GemvArgs& a = ra.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, KC = WQ8 ? K >> 4 : K >> 3;
    const int ngroups = a.rows / RB;
    const int G = gridDim.x;
    // wmx4: "rowbytes" is a group's bytes (KC records), the plane ngroups of them (k_gemv)
    const int rowbytes = WM ? KC * (RW * 4) : WP ? KC * 12 : K * (WQ8 ? 1 : 2);
    void* const wbase = const_cast<void*>(WM ? a.wm_plane : WP ? a.wp_main : a.W);
    const __amdgpu_buffer_rsrc_t wrs =
        __builtin_amdgcn_make_buffer_rsrc(wbase, 0, (WM ? ngroups : a.rows) * rowbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wnone = __builtin_amdgcn_make_buffer_rsrc(wbase, 0, 0, 0x00020000);
    void* const sbase = const_cast<void*>(WP ? a.wp_side : a.W);
    const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(sbase, 0, ngroups * (256 * SW * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t snone = __builtin_amdgcn_make_buffer_rsrc(sbase, 0, 0, 0x00020000);
    // chunk offsets per K round, as k_gemv: chunks past K re-load chunk 0 and meet x = 0
    int voff[KQ];
#pragma unroll
    for (int j = 0; j < KQ; j++) {
        const int c0 = (j * 4 + wave) * 64 + lane;
        voff[j] = (c0 < KC ? c0 : 0) * (WM ? RW * 4 : WP ? 12 : 16);
    }
    // epilogue ownership: thread orow * NL + ol of wave 0 finishes row (or row pair) ol of the
    // group for input row orow of the pass
    const bool owner = tid < RP * NL;
    const int orow = owner ? tid / NL : 0, ol = tid % NL;
    const int i0 = PAIRED ? 2 * ol : ol;
    int buf = 0;
#pragma unroll 1
    for (int r0 = 0; r0 < R; r0 += RP) {
        int g = blockIdx.x;
        int rows[RB];
        uint4 wv[WM ? 1 : KQ][RB];
        uint32_t mr[WM ? KQ : 1][RW];
        uint32_t sd[SW];
        // first group's weights are independent of x: issue them before the prologue
        gemv_rows<EPI, RB>(g, rows);
        if (WP) gemv_load_side<SW>(srs, tid * (SW * 4), g * (256 * SW * 4), sd);
        if constexpr (WM) gemv_load_mx4<RW, KQ>(wrs, g * rowbytes, voff, mr);
        else gemv_load<RB, KQ, WP>(wrs, rowbytes, rows, voff, wv);

        float4 xr[RP][KQ][XPC];
        // Q8 (16 x values per chunk) fetches the norm and ada rows after the row sums, as
        // k_gemv<WF_Q8> does: they are not held across the sum's barrier
        constexpr bool EARLY = !WQ8;
        float4 nwr[KQ][EARLY ? XPC : 1], adr[KQ][EARLY ? XPC : 1];
        float ss[RP];
#pragma unroll
        for (int r = 0; r < RP; r++) ss[r] = 0.f;
#pragma unroll
        for (int j = 0; j < KQ; j++) {
            const int c = (j * 4 + wave) * 64 + lane;
            const int cc = c < KC ? c : 0;
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int r = 0; r < RP; r++) {
                const float4* xp = reinterpret_cast<const float4*>(a.x + (size_t)(r0 + r) * ra.ldx) + XPC * cc;
#pragma unroll
                for (int h = 0; h < XPC; h++) {
                    const float4 xv = xp[h];
                    xr[r][j][h] = c < KC ? xv : z;
                }
            }
            if (PRO != PRO_NONE) {
                // the norm weights (and the ada row) are shared by the rows
                const float4* wp = reinterpret_cast<const float4*>(a.norm_w) + XPC * cc;
                const float4* ap = reinterpret_cast<const float4*>(PRO == PRO_NORM_ADA ? a.ada : a.norm_w) + XPC * cc;
                if constexpr (EARLY) {
#pragma unroll
                    for (int h = 0; h < XPC; h++) {
                        nwr[j][h] = wp[h];
                        if (PRO == PRO_NORM_ADA) adr[j][h] = ap[h];
                    }
                }
#pragma unroll
                for (int r = 0; r < RP; r++)
#pragma unroll
                    for (int h = 0; h < XPC; h++) {
                        const float4 v = xr[r][j][h];
                        ss[r] = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, ss[r]))));
                    }
            }
        }
        if (PRO != PRO_NONE) {
            // RMSNorm prologue, per row (k_gemv's arithmetic)
#pragma unroll
            for (int r = 0; r < RP; r++) {
                ss[r] = wave_sum(ss[r]);
                if (lane == 0) sred[wave][r] = ss[r];
            }
            __syncthreads();
            if constexpr (WQ8) {
                // one fetch of each norm / ada float4 for the RP rows; per element the
                // arithmetic below is the other branch's
                float inv[RP];
#pragma unroll
                for (int r = 0; r < RP; r++) {
                    const float tot = sred[0][r] + sred[1][r] + sred[2][r] + sred[3][r];
                    inv[r] = 1.0f / sqrtf(tot / (float)K + a.eps);
                }
#pragma unroll
                for (int j = 0; j < KQ; j++) {
                    const int c0 = (j * 4 + wave) * 64 + lane;
                    const int cc = c0 < KC ? c0 : 0;
                    const float4* wp = reinterpret_cast<const float4*>(a.norm_w) + XPC * cc;
                    const float4* ap = reinterpret_cast<const float4*>(PRO == PRO_NORM_ADA ? a.ada : a.norm_w) + XPC * cc;
#pragma unroll
                    for (int h = 0; h < XPC; h++) {
                        const float4 nw = wp[h];
                        float4 ad = nw;
                        if (PRO == PRO_NORM_ADA) ad = ap[h];
#pragma unroll
                        for (int r = 0; r < RP; r++) {
                            float4 v = xr[r][j][h];
                            v.x = v.x * inv[r] * nw.x; v.y = v.y * inv[r] * nw.y;
                            v.z = v.z * inv[r] * nw.z; v.w = v.w * inv[r] * nw.w;
                            if (PRO == PRO_NORM_ADA) {
                                v.x *= (1.0f + ad.x); v.y *= (1.0f + ad.y);
                                v.z *= (1.0f + ad.z); v.w *= (1.0f + ad.w);
                            }
                            xr[r][j][h] = v;
                        }
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < RP; r++) {
                    const float tot = sred[0][r] + sred[1][r] + sred[2][r] + sred[3][r];
                    const float inv = 1.0f / sqrtf(tot / (float)K + a.eps);
#pragma unroll
                    for (int j = 0; j < KQ; j++)
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            float4 v = xr[r][j][h];
                            const float4 nw = nwr[j][h];
                            v.x = v.x * inv * nw.x; v.y = v.y * inv * nw.y;
                            v.z = v.z * inv * nw.z; v.w = v.w * inv * nw.w;
                            if (PRO == PRO_NORM_ADA) {
                                const float4 ad = adr[j][h];
                                v.x *= (1.0f + ad.x); v.y *= (1.0f + ad.y);
                                v.z *= (1.0f + ad.z); v.w *= (1.0f + ad.w);
                            }
                            xr[r][j][h] = v;
                        }
                }
            }
        }
        if (WP) {
#pragma unroll
            for (int r = 0; r < RP; r++)
#pragma unroll
                for (int j = 0; j < KQ; j++)
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        float4 v = xr[r][j][h];
                        v.x = ldexpf(v.x, a.wp_d); v.y = ldexpf(v.y, a.wp_d);
                        v.z = ldexpf(v.z, a.wp_d); v.w = ldexpf(v.w, a.wp_d);
                        xr[r][j][h] = v;
                    }
        }

        // the owner's row of this pass: output row, and for QKV the slot's position and rings
        float* const yrow = a.y + (size_t)(r0 + orow) * ra.ldy;
        int lp = 0, live = 0;
        float *Kc = nullptr, *Vc = nullptr;
        if (QKVE && owner) {
            const BatchSlot* sl = ra.slots + (r0 + orow);
            live = sl->live;
            lp = live ? sl->pos : 0;
            Kc = reinterpret_cast<float*>(sl->Kc + ra.ring_off);
            Vc = reinterpret_cast<float*>(sl->Vc + ra.ring_off);
        }
        for (;;) {
            const int gcur = g;
            // epilogue inputs of this group (independent of the dot products)
            int er0 = 0, er1 = 0;
            float ein0 = 0.f, ein1 = 0.f, esc0 = 1.f, esc1 = 1.f;
            if (owner) {
                int rr[RB];
                gemv_rows<EPI, RB>(gcur, rr);
#pragma unroll
                for (int i = 0; i < RB; i++) {
                    if (i == i0) er0 = rr[i];
                    if (i == i0 + 1) er1 = rr[i];
                }
                if (WQ8) {
                    esc0 = a.wscale[er0];
                    if (PAIRED) esc1 = a.wscale[er1];
                }
                if (EPI == EPI_RESID) ein0 = yrow[er0];
                if (QKVE && er0 < a.qd + a.kvd) {
                    const int col = er0 < a.qd ? er0 : er0 - a.qd;
                    const float* rp = a.rope + (size_t)lp * a.hd + ((col % a.hd) & ~1);
                    ein0 = rp[0];
                    ein1 = rp[1];
                }
            }
            float acc[RP][RB];
#pragma unroll
            for (int r = 0; r < RP; r++)
#pragma unroll
                for (int i = 0; i < RB; i++) acc[r][i] = 0.f;
#pragma unroll
            for (int j = 0; j < KQ; j++)
#pragma unroll
                for (int i = 0; i < RB; i++) {
                    if constexpr (WM) {
                        // one decode per (round, row) of the group, then dot8's FMAs per input row
                        const f32x8 wd = dec8m4(mr[j][i], (mr[j][RB + (i >> 2)] >> (8 * (i & 3))) & 0xffu);
#pragma unroll
                        for (int r = 0; r < RP; r++) acc[r][i] = dot8f(wd, xr[r][j][0], xr[r][j][1], acc[r][i]);
                    } else if constexpr (WQ8) {
#pragma unroll
                        for (int r = 0; r < RP; r++)
                            acc[r][i] = dot16q(wv[j][i], reinterpret_cast<const float4(&)[4]>(xr[r][j]), acc[r][i]);
                    } else {
#pragma unroll
                        for (int r = 0; r < RP; r++) {
                            if (WP) acc[r][i] = dot8h(wv[j][i], sd[(j * RB + i) >> 2], (j * RB + i) & 3, xr[r][j][0], xr[r][j][1], acc[r][i]);
                            else acc[r][i] = dot8(wv[j][i], xr[r][j][0], xr[r][j][1], acc[r][i]);
                        }
                    }
                }
            g += G;
            // the next group's loads before this group's reduction, unconditionally; past the
            // last group through the zero-length descriptor (k_gemv)
            {
                const bool more = g < ngroups;
                gemv_rows<EPI, RB>(more ? g : 0, rows);
                if (WP) gemv_load_side<SW>(more ? srs : snone, tid * (SW * 4), (more ? g : 0) * (256 * SW * 4), sd);
                if constexpr (WM) gemv_load_mx4<RW, KQ>(more ? wrs : wnone, (more ? g : 0) * rowbytes, voff, mr);
                else gemv_load<RB, KQ, WP>(more ? wrs : wnone, rowbytes, rows, voff, wv);
            }
#pragma unroll
            for (int r = 0; r < RP; r++)
#pragma unroll
                for (int i = 0; i < RB; i++) acc[r][i] = wave_sum(acc[r][i]);
            if (lane == 0) {
#pragma unroll
                for (int r = 0; r < RP; r++)
#pragma unroll
                    for (int i = 0; i < RB; i++) red[buf][wave][r][i] = acc[r][i];
            }
            __syncthreads();
            if (owner) {
                float v0 = ((red[buf][0][orow][i0] + red[buf][1][orow][i0]) + red[buf][2][orow][i0]) + red[buf][3][orow][i0];
                float v1 = 0.f;
                if (PAIRED)
                    v1 = ((red[buf][0][orow][i0 + 1] + red[buf][1][orow][i0 + 1]) + red[buf][2][orow][i0 + 1]) +
                         red[buf][3][orow][i0 + 1];
                if (WQ8) {  // y = scale * sum before anything else (k_gemv)
                    v0 *= esc0;
                    v1 *= esc1;
                }
                if (EPI == EPI_STORE || EPI == EPI_RESID) {
                    yrow[er0] = ein0 + v0;
                } else if (EPI == EPI_SWIGLU) {
                    yrow[gcur * (RB / 2) + ol] = silu(v0) * v1;
                } else if (QKVE) {
                    if (er0 < a.qd + a.kvd) {
                        const float o0 = v0 * ein0 - v1 * ein1, o1 = v0 * ein1 + v1 * ein0;
                        if (er0 < a.qd) {
                            yrow[er0] = o0;
                            yrow[er1] = o1;
                        } else if (live) {
                            kv_st2_rt(Kc, (size_t)(lp % a.cap) * a.kvd + (er0 - a.qd), o0, o1, a.kvt);
                        }
                    } else if (live) {
                        kv_st2_rt(Vc, (size_t)(lp % a.cap) * a.kvd + (er0 - a.qd - a.kvd), v0, v1, a.kvt);
                    }
                }
            }
            buf ^= 1;
            if (g >= ngroups) break;
        }
    }
}

}  // namespace vox
