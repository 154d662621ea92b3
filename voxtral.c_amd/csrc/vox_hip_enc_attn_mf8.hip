// vox_hip_enc_attn_mf8.hip -- the M > 1 causal / windowed attention over the encoder's FP8 (E4M3)
// K/V rings on the bf16 matrix pipe (k_attn_rows_mf8; opt-in:
// vox_hip_set_enc_attn_mf8 / VOX_HIP_ENC_ATTN_MF8=1).  The twin of k_attn_decode_mf8 for query
// rows: every E4M3 code is a bf16 value and an f32 is the exact sum of three bf16 planes (split3),
// so v_mfma_f32_16x16x32_bf16 over (K as bf16) x (Q planes) and (P planes) x (V as bf16) forms
// exact products and adds them in f32.  Nothing is rounded that k_attn_mf<64, kv8_t> does not
// round; only the order of the sums differs.
//
// Semantics, grid, partial layout and epilogues are k_attn_mf's at head_dim 64: block = (head, 16
// queries, key split) of 4 waves; query i sits at q_pos0 + i and sees keys
// max(k_first, qp - window + 1) .. qp at ring slot p % cap.  The block's key range is cut into
// 32-key tiles from its first key; wave w takes tiles w, w + 4, ..., the next tile's codes in
// registers while the current one is multiplied.  With ns > 1 the split span is rounded up to whole
// tiles, so only a range's last tile is ragged; a split (or wave) left without keys contributes
// (-1e30, 0, 0).  Rows of a tile past the range's last key read that key's row (a key of the
// call) and are masked: no ring slot outside the call's key range is read.
//
// Q.K (per 16 keys, two 32-deep chunks x three planes): S^T = K Q^T.  A = K, lane (c = l % 16,
// g = l / 16) holds the 16 contiguous codes [16 g, 16 g + 16) of key row c (one 16-B load; chunk
// ch = its bytes 8 ch .. 8 ch + 7, so k-index 8 g + i of chunk ch is dim 16 g + 8 ch + i); B = Q^T,
// the lane holds the same dims of query c as hi / mid / lo bf16, split once (24 registers).  The
// accumulator leaves lane (query c, g) with the scores of keys 4 g + i of each 16-key half:
// exactly the A operand of P.V with k-index 8 g + i meaning key mf8_key(g, i), so P never changes
// lanes.
//
// P.V (per 32 keys, four 16-dim column tiles x three planes): A = P planes, B = V, column c of
// tile t = dim 4 c + t.  The lane loads the 4 codes [4 c, 4 c + 4) of each of its eight key rows
// (one 4-B load per row; 16 lanes cover a 64-B row) and transposes in registers: one v_perm_b32
// interleaves two rows' bytes into (key, key + 1) pairs of two dims, the packed convert's word
// select picks the dim.  o's rows are queries 4 g + i, dims 4 c + t: k_attn_mf's accumulator, so
// the wave merge in LDS and the three epilogues are k_attn_mf's.  No LDS in the loop.
#include "vox_hip_internal.h"
#include "vox_hip_dev.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace vox {

constexpr int MF8R_TILE = 32;  // keys per tile

// the codes one lane holds of a 32-key tile: 16 K bytes of its key row in each 16-key half, and
// 4 V bytes of each of its eight key rows
struct Mf8RowsTile {
    uint4 k[2];
    uint32_t v[8];
};

template <int BAT>
__global__ __launch_bounds__(256) void k_attn_rows_mf8(const float* __restrict__ Q, int ldq, const uint8_t* __restrict__ Kc,
                                                       const uint8_t* __restrict__ Vc, int cap, float* __restrict__ O,
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
        Kc = reinterpret_cast<const uint8_t*>(er.Kc[zb]);
        Vc = reinterpret_cast<const uint8_t*>(er.Vc[zb]);
        if (qbi * 16 >= Mr) return;  // uniform per block
    }
    const int h = blockIdx.x, q0 = qbi * 16;
    const int kvh = h / (H / KVH), kvd = KVH * HD;  // kvd: bytes per ring slot
    const int nq = min(16, Mr - q0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;

    // B operand of Q.K: query c (zero past the block's rows), dims 16 g + 8 ch + i, three planes
    bf16x8 qp3[2][3];
    {
        const float* qr = Q + (size_t)(rbase + q0 + c) * ldq + h * HD + 16 * g;
#pragma unroll
        for (int ch = 0; ch < 2; ch++) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (c < nq) {
                a = *reinterpret_cast<const float4*>(qr + 8 * ch);
                b = *reinterpret_cast<const float4*>(qr + 8 * ch + 4);
            }
            const float qv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            mf8_split8(qv, qp3[ch][0], qp3[ch][1], qp3[ch][2]);
        }
    }
    const int qfirst = q_pos0 + q0, qlast = q_pos0 + q0 + nq - 1;
    int kstart = max(qfirst - window + 1, k_first);
    int kend = qlast;
    if (ns > 1) {
        const int span = ((kend - kstart + 1 + ns - 1) / ns + MF8R_TILE - 1) / MF8R_TILE * MF8R_TILE;
        kstart += zsplit * span;
        kend = min(kend, kstart + span - 1);
    }
    const int qp = q_pos0 + q0 + c;  // the query of this lane's S^T column

    // the codes of the tile at key kt (kt <= kend): the slot modulo once per tile, the wrap per key
    // row (cap >= the tile); rows past kend read row kend
    auto load = [&](int kt, Mf8RowsTile& T) {
        const int slot0 = kt % cap, last = kend - kt;
        auto row = [&](int key) {
            int s = slot0 + min(key, last);
            s = s >= cap ? s - cap : s;
            return (size_t)s * kvd + kvh * HD;
        };
#pragma unroll
        for (int j = 0; j < 2; j++) T.k[j] = *reinterpret_cast<const uint4*>(Kc + row(16 * j + c) + 16 * g);
#pragma unroll
        for (int i = 0; i < 8; i++) T.v[i] = *reinterpret_cast<const uint32_t*>(Vc + row(mf8_key(g, i)) + 4 * c);
    };

    // running state: m and l of query c (l a per-lane share, summed over g at the end); o rows =
    // queries 4 g + i, column tile t = dim 4 c + t
    float m = -1e30f, l = 0.f;
    f32x4 o[NB];
#pragma unroll
    for (int t = 0; t < NB; t++) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    Mf8RowsTile cur, nxt;
    int kt = kstart + wave * MF8R_TILE;
    if (kt <= kend) load(kt, cur);
    for (; kt <= kend; kt += 4 * MF8R_TILE) {
        const bool more = kt + 4 * MF8R_TILE <= kend;
        if (more) load(kt + 4 * MF8R_TILE, nxt);
        // ---- scores of the two 16-key halves: lane (query c, g) element i = key 16 j + 4 g + i ----
        f32x4 s[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            const bf16x8 ka[2] = {mf8_cvt8(cur.k[j].x, cur.k[j].y), mf8_cvt8(cur.k[j].z, cur.k[j].w)};
#pragma unroll
            for (int ch = 0; ch < 2; ch++)
#pragma unroll
                for (int p = 0; p < 3; p++) s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[ch], qp3[ch][p], s[j], 0, 0, 0);
        }
        // ---- softmax step (k_attn_mf's mask); the tile's max meets across g ----
        float sc[8], mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int kp = kt + mf8_key(g, i);
            const bool valid = c < nq && kp <= kend && kp <= qp && kp >= qp - window + 1 && kp >= k_first;
            sc[i] = valid ? s[i >> 2][i & 3] * scale : -INFINITY;
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
        }
        l = fmaf(l, alpha, ps);
        bf16x8 pp[3];
        mf8_split8(pv, pp[0], pp[1], pp[2]);
        // output rows 4 g + i are queries 4 g + i: their rescale factor sits on lane 4 g + i
        float fq[4];
#pragma unroll
        for (int i = 0; i < 4; i++) fq[i] = __shfl(alpha, 4 * g + i, 64);
        // ---- P.V: rows (2 q, 2 q + 1) interleaved per dim pair, then converted per dim ----
        uint32_t w[4][2];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            w[q][0] = __builtin_amdgcn_perm(cur.v[2 * q + 1], cur.v[2 * q], 0x05010400u);
            w[q][1] = __builtin_amdgcn_perm(cur.v[2 * q + 1], cur.v[2 * q], 0x07030602u);
        }
#pragma unroll
        for (int t = 0; t < NB; t++) {
            uint32_t b[4];
#pragma unroll
            for (int q = 0; q < 4; q++) b[q] = (t & 1) ? mf8_cvt2<true>(w[q][t >> 1]) : mf8_cvt2<false>(w[q][t >> 1]);
            const bf16x8 vb = __builtin_bit_cast(bf16x8, make_uint4(b[0], b[1], b[2], b[3]));
#pragma unroll
            for (int i = 0; i < 4; i++) o[t][i] *= fq[i];
#pragma unroll
            for (int p = 0; p < 3; p++) o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pp[p], vb, o[t], 0, 0, 0);
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
        for (int t = 0; t < NB; t++) so[wave][4 * g + i][NB * c + t] = o[t][i];
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

// ============================================================================
// Host side: the process-wide switch, the launch count, the launcher
// ============================================================================
static int g_enc_attn_mf8 = -1;
static long long g_enc_attn_mf8_n;
int enc_attn_mf8_mode() {
    if (g_enc_attn_mf8 < 0) {
        const char* e = getenv("VOX_HIP_ENC_ATTN_MF8");
        g_enc_attn_mf8 = e && atoi(e) == 1 ? 1 : 0;
    }
    return g_enc_attn_mf8;
}
void enc_attn_mf8_set(int on) { g_enc_attn_mf8 = on ? 1 : 0; }
long long enc_attn_mf8_count() { return g_enc_attn_mf8_n; }

bool attn_rows_mf8_ok(int hd, int kvt, int cap) { return hd == 64 && kvt == KV_FP8 && cap >= MF8R_TILE; }

hipError_t launch_attn_rows_mf8(bool bat, dim3 grid, const float* Q, int ldq, const float* Kc, const float* Vc, int cap,
                                float* O, int ldo, int M, int H, int KVH, int q_pos0, int k_first, int window, float scale,
                                int ns, float* part, const EncRows& er, uint16_t* xs, hipStream_t st) {
    if (cap < MF8R_TILE || KVH < 1 || H % KVH || ns < 1 || (ns > 1 && !part) || k_first < 0 || window < 1 ||
        (int)grid.x != H || (bat ? er.B < 1 || (int)grid.z != ns * er.B : (!Kc || !Vc || q_pos0 < 0 || (int)grid.z != ns)))
        return hipErrorInvalidValue;
    const uint8_t* kc = reinterpret_cast<const uint8_t*>(Kc);
    const uint8_t* vc = reinterpret_cast<const uint8_t*>(Vc);
    if (bat)
        hipLaunchKernelGGL(k_attn_rows_mf8<1>, grid, dim3(256), 0, st, Q, ldq, kc, vc, cap, O, ldo, M, H, KVH, q_pos0, k_first,
                           window, scale, ns, part, er, xs);
    else
        hipLaunchKernelGGL(k_attn_rows_mf8<0>, grid, dim3(256), 0, st, Q, ldq, kc, vc, cap, O, ldo, M, H, KVH, q_pos0, k_first,
                           window, scale, ns, part, er, xs);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) g_enc_attn_mf8_n++;
    return e;
}

}  // namespace vox
