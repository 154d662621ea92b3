// vox_hip_enc_attn_mf16.hip -- the M > 1 causal / windowed attention over the encoder's IEEE-half
// K/V rings on the f16 matrix pipe (k_attn_rows_mf16; opt-in:
// vox_hip_set_enc_attn_mf16 / VOX_HIP_ENC_ATTN_MF16=1).  A half ring element is already an operand
// of v_mfma_f32_16x16x32_f16, so K and V enter as loaded: no widening, no split.  Queries and
// softmax weights enter as three f16 planes of the row-scaled value (hi + mid + lo, within 2^-25
// absolute of a value scaled into [2^14, 2^15)); every f16 x f16 product is exact in the f32
// accumulator.  Nothing is rounded to half that k_attn_mf<64, half> keeps in f32 beyond 2^-39 of a
// row's largest magnitude (2^-28 if the instruction flushed subnormal f16 inputs).
//
// Semantics, grid, partial layout and epilogues are k_attn_mf's at head_dim 64; the split of the
// key range into 32-key tiles over 4 waves, the next tile in registers, the split spans rounded to
// whole tiles, the mask, the rows past the range's last key reading that key's row and the wave
// merge are k_attn_rows_mf8's (vox_hip_enc_attn_mf8.hip).  No LDS in the loop.
//
// Q.K (per 16 keys, two 32-deep chunks x three planes): S^T = K Q^T.  A = K, lane (c = l % 16,
// g = l / 16) holds the 16 contiguous halfs [16 g, 16 g + 16) of key row c (two 16-B loads; chunk
// ch = the ch-th of them, so k-index 8 g + i of chunk ch is dim 16 g + 8 ch + i); B = Q^T, the lane
// holds the same dims of query c as hi / mid / lo f16 of q * 2^(14 - e), e = floor(log2(max |q|))
// of the query's 64 dims (a reduction over its four g lanes), made once per block (12 registers).
// The score is acc * scale * 2^(e - 14) in f32.  The accumulator leaves lane (query c, g) with the
// scores of keys 4 g + i of each 16-key half: the A operand of P.V with k-index 8 g + i meaning
// key mf8_key(g, i), so P never changes lanes.
//
// P.V (per 32 keys, four 16-dim column tiles x three planes): A = planes of p * 2^15 (p <= 1), B =
// V, column c of tile t = dim 4 c + t.  The lane loads the 4 halfs [4 c, 4 c + 4) of each of its
// eight key rows (one 8-B load per row; 16 lanes cover a 128-B row) and transposes in registers:
// one v_perm_b32 per (row pair, dim) packs the two rows' halfs of that dim.  o carries the 2^15,
// taken off once, exactly, where the waves merge; l sums the unscaled f32 weights.
#include "vox_hip_internal.h"
#include "vox_hip_dev.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace vox {

constexpr int MF16R_TILE = 32;  // keys per tile

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

// the kernel's matrix instruction: D = A B + C over 32 f16 of depth, f32 accumulator
__device__ __forceinline__ f32x4 mf16_mma(h16x8 a, h16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// 2^n as f32, -126 <= n <= 127
__device__ __forceinline__ float mf16_pow2(int n) { return __uint_as_float((uint32_t)(n + 127) << 23); }

// eight f32 (|v| < 65504) as three f16x8 planes: hi = f16(v), mid = f16(v - hi), lo = f16(v - hi -
// mid), the differences exact in f32
__device__ __forceinline__ void mf16_split8(const float (&v)[8], h16x8& ph, h16x8& pm, h16x8& pl) {
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const _Float16 h = (_Float16)v[e];
        const float r1 = v[e] - (float)h;
        const _Float16 m = (_Float16)r1;
        ph[e] = h;
        pm[e] = m;
        pl[e] = (_Float16)(r1 - (float)m);
    }
}

// the halfs one lane holds of a 32-key tile: 16 K halfs of its key row in each 16-key half (two
// chunks of 8), and 4 V halfs of each of its eight key rows
struct Mf16RowsTile {
    uint4 k[2][2];
    uint2 v[8];
};

// waves_per_eu(3): two tiles in flight are 64 registers; left alone the compiler takes 160 VGPRs +
// 16 AGPRs (two waves per SIMD), asked for three it fits 161 without a spill, the occupancy of
// k_attn_mf and k_attn_rows_mf8 (677 rows 26.3 -> 23.8 us, 1500 rows 88.4 -> 78.8 us)
template <int BAT>
__attribute__((amdgpu_waves_per_eu(3)))
__global__ __launch_bounds__(256) void k_attn_rows_mf16(const float* __restrict__ Q, int ldq, const uint16_t* __restrict__ Kc,
                                                        const uint16_t* __restrict__ Vc, int cap, float* __restrict__ O,
                                                        int ldo, int M, int H, int KVH, int q_pos0, int k_first,
                                                        int window, float scale, int ns, float* __restrict__ part,
                                                        const EncRows er, uint16_t* __restrict__ xs) {
    constexpr int HD = 64, NB = 4;
    __shared__ float sm[4][16], sl[4][16];
    __shared__ __attribute__((aligned(16))) float so[4][16][HD + 4];
    const int zsplit = BAT ? (int)blockIdx.z % ns : (int)blockIdx.z;
    // query blocks in reverse order (k_attn_mf): the longest blocks are dispatched first
    const int qbi = (int)gridDim.y - 1 - (int)blockIdx.y;
    int rbase = 0, Mr = M;  // first stacked row of this stream, its row count
    if (BAT) {
        const int zb = (int)blockIdx.z / ns;
        rbase = er.off[zb];
        Mr = er.nr[zb];
        q_pos0 = er.pos0[zb];
        Kc = reinterpret_cast<const uint16_t*>(er.Kc[zb]);
        Vc = reinterpret_cast<const uint16_t*>(er.Vc[zb]);
        if (qbi * 16 >= Mr) return;  // uniform per block
    }
    const int h = blockIdx.x, q0 = qbi * 16;
    const int kvh = h / (H / KVH), kvd = KVH * HD;  // kvd: halfs per ring slot
    const int nq = min(16, Mr - q0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;

    // B operand of Q.K: query c (zero past the block's rows), dims 16 g + 8 ch + i, three planes of
    // q * 2^(14 - e); qdown = scale * 2^(e - 14) brings a score back
    h16x8 qp3[2][3];
    float qdown;
    {
        const float* qr = Q + (size_t)(rbase + q0 + c) * ldq + h * HD + 16 * g;
        float qv[2][8];
        uint32_t mag = 0;  // the largest |q| of the row as bits: ordered like the values
#pragma unroll
        for (int ch = 0; ch < 2; ch++) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (c < nq) {
                a = *reinterpret_cast<const float4*>(qr + 8 * ch);
                b = *reinterpret_cast<const float4*>(qr + 8 * ch + 4);
            }
            const float t[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 8; i++) {
                qv[ch][i] = t[i];
                mag = max(mag, __float_as_uint(t[i]) & 0x7fffffffu);
            }
        }
        mag = max(mag, (uint32_t)__shfl_xor((int)mag, 16, 64));
        mag = max(mag, (uint32_t)__shfl_xor((int)mag, 32, 64));
        // e of a zero row is 0; a row below 2^-100 keeps e = -100 (its planes are then smaller than
        // 2^14, never larger), so that both powers stay normal f32
        const int e = mag == 0 ? 0 : max((int)(mag >> 23) - 127, -100);
        const float up = mf16_pow2(14 - e);
        qdown = scale * mf16_pow2(e - 14);
#pragma unroll
        for (int ch = 0; ch < 2; ch++) {
#pragma unroll
            for (int i = 0; i < 8; i++) qv[ch][i] *= up;
            mf16_split8(qv[ch], qp3[ch][0], qp3[ch][1], qp3[ch][2]);
        }
    }
    const int qfirst = q_pos0 + q0, qlast = q_pos0 + q0 + nq - 1;
    int kstart = max(qfirst - window + 1, k_first);
    int kend = qlast;
    if (ns > 1) {
        const int span = ((kend - kstart + 1 + ns - 1) / ns + MF16R_TILE - 1) / MF16R_TILE * MF16R_TILE;
        kstart += zsplit * span;
        kend = min(kend, kstart + span - 1);
    }
    const int qp = q_pos0 + q0 + c;  // the query of this lane's S^T column

    // the halfs of the tile at key kt (kt <= kend): the slot modulo once per tile, the wrap per key
    // row (cap >= the tile); rows past kend read row kend
    auto load = [&](int kt, Mf16RowsTile& T) {
        const int slot0 = kt % cap, last = kend - kt;
        auto row = [&](int key) {
            int s = slot0 + min(key, last);
            s = s >= cap ? s - cap : s;
            return (size_t)s * kvd + kvh * HD;
        };
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint4* kr = reinterpret_cast<const uint4*>(Kc + row(16 * j + c) + 16 * g);
            T.k[j][0] = kr[0];
            T.k[j][1] = kr[1];
        }
#pragma unroll
        for (int i = 0; i < 8; i++) T.v[i] = *reinterpret_cast<const uint2*>(Vc + row(mf8_key(g, i)) + 4 * c);
    };

    // running state: m and l of query c (l a per-lane share, summed over g at the end); o rows =
    // queries 4 g + i, column tile t = dim 4 c + t, scaled by 2^15
    float m = -1e30f, l = 0.f;
    f32x4 o[NB];
#pragma unroll
    for (int t = 0; t < NB; t++) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    Mf16RowsTile cur, nxt;
    int kt = kstart + wave * MF16R_TILE;
    if (kt <= kend) load(kt, cur);
    for (; kt <= kend; kt += 4 * MF16R_TILE) {
        const bool more = kt + 4 * MF16R_TILE <= kend;
        if (more) load(kt + 4 * MF16R_TILE, nxt);
        // ---- scores of the two 16-key halves: lane (query c, g) element i = key 16 j + 4 g + i ----
        f32x4 s[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ch = 0; ch < 2; ch++) {
                const h16x8 ka = __builtin_bit_cast(h16x8, cur.k[j][ch]);
#pragma unroll
                for (int p = 0; p < 3; p++) s[j] = mf16_mma(ka, qp3[ch][p], s[j]);
            }
        }
        // ---- softmax step (k_attn_mf's mask); the tile's max meets across g ----
        float sc[8], mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int kp = kt + mf8_key(g, i);
            const bool valid = c < nq && kp <= kend && kp <= qp && kp >= qp - window + 1 && kp >= k_first;
            sc[i] = valid ? s[i >> 2][i & 3] * qdown : -INFINITY;
            mx = fmaxf(mx, sc[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mnew = fmaxf(m, mx);
        const float alpha = expf(m - mnew);
        m = mnew;
        float pv[8], ps = 0.f;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            pv[i] = (sc[i] == -INFINITY) ? 0.f : expf(sc[i] - mnew);
            ps += pv[i];
            pv[i] *= 32768.f;
        }
        l = fmaf(l, alpha, ps);
        h16x8 pp[3];
        mf16_split8(pv, pp[0], pp[1], pp[2]);
        // output rows 4 g + i are queries 4 g + i: their rescale factor sits on lane 4 g + i
        float fq[4];
#pragma unroll
        for (int i = 0; i < 4; i++) fq[i] = __shfl(alpha, 4 * g + i, 64);
        // ---- P.V: the halfs of dim 4 c + t of rows (2 q, 2 q + 1) packed by one perm ----
#pragma unroll
        for (int t = 0; t < NB; t++) {
            uint32_t b[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t r0 = (t & 2) ? cur.v[2 * q].y : cur.v[2 * q].x;
                const uint32_t r1 = (t & 2) ? cur.v[2 * q + 1].y : cur.v[2 * q + 1].x;
                b[q] = __builtin_amdgcn_perm(r1, r0, (t & 1) ? 0x07060302u : 0x05040100u);
            }
            const h16x8 vb = __builtin_bit_cast(h16x8, make_uint4(b[0], b[1], b[2], b[3]));
#pragma unroll
            for (int i = 0; i < 4; i++) o[t][i] *= fq[i];
#pragma unroll
            for (int p = 0; p < 3; p++) o[t] = mf16_mma(pp[p], vb, o[t]);
        }
        if (more) cur = nxt;
    }

    // ---- merge the waves and write the block's rows: k_attn_mf's merge and epilogues ----
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (g == 0) {
        sm[wave][c] = m;
        sl[wave][c] = l;
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int t = 0; t < NB; t++) so[wave][4 * g + i][NB * c + t] = o[t][i] * (1.0f / 32768.f);
    __syncthreads();
    const int r = tid >> 4, d0 = (tid & 15) * NB;  // query r, dims [d0, d0 + NB)
    if (r >= nq) return;
    float mxw = -1e30f;
#pragma unroll
    for (int wv = 0; wv < 4; wv++) mxw = fmaxf(mxw, sm[wv][r]);
    float f[4], den = 0.f;
#pragma unroll
    for (int wv = 0; wv < 4; wv++) {
        f[wv] = expf(sm[wv][r] - mxw);
        den = fmaf(f[wv], sl[wv][r], den);
    }
    float num[NB];
#pragma unroll
    for (int e = 0; e < NB; e++) {
        num[e] = 0.f;
#pragma unroll
        for (int wv = 0; wv < 4; wv++) num[e] = fmaf(f[wv], so[wv][r][d0 + e], num[e]);
    }
    if (ns > 1) {
        float* pp = part + ((size_t)(h * M + rbase + q0 + r) * ns + zsplit) * (HD + 2);
#pragma unroll
        for (int e = 0; e < NB; e++) pp[d0 + e] = num[e];
        if ((tid & 15) == 0) {
            pp[HD] = mxw;
            pp[HD + 1] = den;
        }
    } else if (xs) {
        // the output row straight into the fragment-major planes of the wo input (H * HD columns)
        const float inv = den > 0.f ? 1.0f / den : 0.f;
        const int row = rbase + q0 + r, K = H * HD, k = h * HD + d0;
        uint16_t hh[4], mm[4], ll[4];
#pragma unroll
        for (int e = 0; e < 4; e++) split3(num[e] * inv, hh[e], mm[e], ll[e]);
        *reinterpret_cast<uint2*>(xs + frag_at(row, K, 0, k)) = make_uint2(hh[0] | ((uint32_t)hh[1] << 16), hh[2] | ((uint32_t)hh[3] << 16));
        *reinterpret_cast<uint2*>(xs + frag_at(row, K, 1, k)) = make_uint2(mm[0] | ((uint32_t)mm[1] << 16), mm[2] | ((uint32_t)mm[3] << 16));
        *reinterpret_cast<uint2*>(xs + frag_at(row, K, 2, k)) = make_uint2(ll[0] | ((uint32_t)ll[1] << 16), ll[2] | ((uint32_t)ll[3] << 16));
    } else {
        const float inv = den > 0.f ? 1.0f / den : 0.f;
        float* op = O + (size_t)(rbase + q0 + r) * ldo + h * HD + d0;
#pragma unroll
        for (int e = 0; e < NB; e++) op[e] = num[e] * inv;
    }
}

// One wave, mf16_mma on caller-supplied f16 bits: product i of a 16-product round sits alone at
// depth 0 of A's row i and B's column i, so D's diagonal holds a[i] * b[i] (lane (i, i / 4),
// element i % 4) and nothing else is added to it.
__global__ __launch_bounds__(64) void k_mf16_probe(float* __restrict__ out, const uint16_t* __restrict__ a,
                                                   const uint16_t* __restrict__ b, int n) {
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    for (int base = 0; base < n; base += 16) {
        const bool mine = g == 0 && base + c < n;
        uint4 ua = make_uint4(mine ? a[base + c] : 0u, 0u, 0u, 0u), ub = make_uint4(mine ? b[base + c] : 0u, 0u, 0u, 0u);
        const f32x4 d = mf16_mma(__builtin_bit_cast(h16x8, ua), __builtin_bit_cast(h16x8, ub), f32x4{0.f, 0.f, 0.f, 0.f});
        if (g == c / 4 && base + c < n) out[base + c] = d[c & 3];
    }
}

// ============================================================================
// Host side: the process-wide switch, the launch count, the launchers
// ============================================================================
static int g_enc_attn_mf16 = -1;
static long long g_enc_attn_mf16_n;
int enc_attn_mf16_mode() {
    if (g_enc_attn_mf16 < 0) {
        const char* e = getenv("VOX_HIP_ENC_ATTN_MF16");
        g_enc_attn_mf16 = e && atoi(e) == 1 ? 1 : 0;
    }
    return g_enc_attn_mf16;
}
void enc_attn_mf16_set(int on) { g_enc_attn_mf16 = on ? 1 : 0; }
long long enc_attn_mf16_count() { return g_enc_attn_mf16_n; }

bool attn_rows_mf16_ok(int hd, int kvt, int cap) { return hd == 64 && kvt == KV_F16 && cap >= MF16R_TILE; }

hipError_t launch_attn_rows_mf16(bool bat, dim3 grid, const float* Q, int ldq, const float* Kc, const float* Vc, int cap,
                                 float* O, int ldo, int M, int H, int KVH, int q_pos0, int k_first, int window, float scale,
                                 int ns, float* part, const EncRows& er, uint16_t* xs, hipStream_t st) {
    if (cap < MF16R_TILE || KVH < 1 || H % KVH || ns < 1 || (ns > 1 && !part) || k_first < 0 || window < 1 ||
        (int)grid.x != H || (bat ? er.B < 1 || (int)grid.z != ns * er.B : (!Kc || !Vc || q_pos0 < 0 || (int)grid.z != ns)))
        return hipErrorInvalidValue;
    const uint16_t* kc = reinterpret_cast<const uint16_t*>(Kc);
    const uint16_t* vc = reinterpret_cast<const uint16_t*>(Vc);
    if (bat)
        hipLaunchKernelGGL(k_attn_rows_mf16<1>, grid, dim3(256), 0, st, Q, ldq, kc, vc, cap, O, ldo, M, H, KVH, q_pos0, k_first,
                           window, scale, ns, part, er, xs);
    else
        hipLaunchKernelGGL(k_attn_rows_mf16<0>, grid, dim3(256), 0, st, Q, ldq, kc, vc, cap, O, ldo, M, H, KVH, q_pos0, k_first,
                           window, scale, ns, part, er, xs);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) g_enc_attn_mf16_n++;
    return e;
}

hipError_t launch_mf16_probe(float* out, const uint16_t* a, const uint16_t* b, int n, hipStream_t st) {
    if (!out || !a || !b || n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mf16_probe, dim3(1), dim3(64), 0, st, out, a, b, n);
    return hipGetLastError();
}

}  // namespace vox
