// vox_hip_attn_mf8.hip -- decode attention over FP8 (E4M3) KV rings on the matrix pipe
// (k_attn_decode_mf8; opt-in: vox_hip_set_attn_mf8 / VOX_HIP_ATTN_MF8=1).
//
// Every E4M3 code is a bf16 value (3 mantissa bits, exponents inside bf16's, subnormals
// included) and an f32 is the exact sum of three bf16 planes (split3), so
// v_mfma_f32_16x16x32_bf16 over (K as bf16) x (Q planes) and (P planes) x (V as bf16) forms exact
// products and adds them in f32: nothing is rounded that k_attn_decode<.., kv8_t> does not round,
// only the order of the sums differs.
//
// Work split: one block of MF8_WAVES waves per (stream, kv head, range of `rk` keys); each wave
// streams its contiguous share of the range in 32-key tiles with a running (m, l, o) per head, the
// next tile's K / V loads in flight while the current one is multiplied; the waves merge once in
// LDS, the blocks of a (stream, kv head) through (o, m, l) partials and a last arriver, in
// k_attn_decode's partial layout.
//
// Q.K (per 16 keys, four 32-deep chunks x three planes): A = K, lane (key = l % 16, g = l / 16)
// holds the 32 contiguous codes [32 g, 32 g + 32) of its key row (two 16-B loads; chunk c = its
// bytes 8 c .. 8 c + 7, so k-index 8 g + i of chunk c is dim 32 g + 8 c + i); B = Q^T, lane
// (head = l % 16, g) holds the same dims of its head's query as hi / mid / lo bf16, zero for
// heads past the group.  The accumulator leaves lane (head = l % 16, g) with the scores of keys
// 4 g + i of each 16-key half: exactly the A operand of P.V with k-index 8 g + i meaning key
// 4 g + i (i < 4) or 16 + 4 g + i - 4 of the tile, so P never changes lanes.
//
// P.V (per 32 keys, eight 16-dim column tiles x three planes): A = P planes, B = V, lane
// (c = l % 16, g), column tile t = dim 8 c + t.  The lane loads the 8 codes [8 c, 8 c + 8) of its
// eight key rows straight from the ring (one 8-B load per row; 16 lanes cover a 128-B row) and
// transposes in registers: one v_perm_b32 interleaves two rows' bytes into (key, key + 1) pairs
// of two dims, the packed convert's word select picks the dim.  No LDS stage.
#include "vox_hip_internal.h"
#include "vox_hip_dev.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <type_traits>
#include <stdlib.h>

namespace vox {

constexpr int MF8_WAVES = 4;   // waves per block
constexpr int MF8_TILE = 32;   // keys per tile
// keys per block (a multiple of MF8_WAVES * MF8_TILE; tools/kbench sweeps it): the partials of a
// head stay within attn_maxch(window) = window / 64
VOX_KB_KNOB(g_attn_mf8_range, 256);

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// the codes one lane holds of a 32-key tile: its key row's 32 K bytes in each 16-key half, and
// 8 V bytes of each of its eight key rows
struct Mf8Tile {
    uint4 k[2][2];
    uint2 v[8];
};
template <int FUSE, class AP>
__global__ __launch_bounds__(MF8_WAVES * 64) void k_attn_decode_mf8(const AP P, int cap, int pos_host, int window,
                                                                    float scale, int H, int KVH, int maxs, int rk,
                                                                    const AttnFuse F) {
    constexpr int HD = 128, NWV = MF8_WAVES, NT = NWV * 64;
    constexpr bool ATTN_ROWS = std::is_base_of<AttnSlots, AP>::value;  // fused output also as f32 rows (out != null)
    constexpr bool RAGGED = std::is_base_of<AttnPtrsRag, AP>::value || std::is_base_of<AttnSlotsRag, AP>::value;
    const int zb = blockIdx.z;
    const BatchSlot* __restrict__ sl = P.slots ? P.slots + zb : nullptr;
    if (sl && !sl->live) return;  // a stopped slot's blocks leave at once (uniform per block)
    size_t ring_off = P.ring_off;
    if constexpr (RAGGED) {
        cap = P.caps[zb];
        ring_off = (size_t)P.layer * cap * KVH * HD;
    }
    if (cap < MF8_TILE) return;  // the per-row wrap below is one subtraction: a ring holds at least a tile
    const uint8_t* __restrict__ Kc = reinterpret_cast<const uint8_t*>(sl ? sl->Kc + ring_off : attn_k(P, zb));
    const uint8_t* __restrict__ Vc = reinterpret_cast<const uint8_t*>(sl ? sl->Vc + ring_off : attn_v(P, zb));
    const int* __restrict__ state = sl ? nullptr : attn_state(P, zb);
    float* __restrict__ part = attn_part(P, zb);
    float* __restrict__ out = attn_out(P, zb);
    __shared__ __attribute__((aligned(16))) float sQ[4][HD];
    __shared__ float sM[NWV][4], sL[NWV][4];
    __shared__ __attribute__((aligned(16))) float sO[NWV][4][HD];
    __shared__ __attribute__((aligned(16))) float sRow[4][HD];
    __shared__ __attribute__((aligned(16))) uint8_t sKn[FUSE ? HD : 16], sVn[FUSE ? HD : 16];  // the new key's codes
    const int hpk = H / KVH, nh = hpk;  // heads of the group (<= 4)
    const int kvh = (int)blockIdx.x % KVH, sb = (int)blockIdx.x / KVH;  // the kv heads of a key range are neighbours
    const int h0 = kvh * hpk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g = lane >> 4;
    const int kvd = KVH * HD;  // bytes per ring slot

    const int lp = sl ? sl->pos : state ? state[0] : pos_host;
    const int L = min(lp + 1, window);
    const int first = lp - L + 1;
    const int S = (L + rk - 1) / rk;  // key ranges of this context
    if (sb >= S) return;              // uniform per block
    const int rkw = rk / NWV;         // keys per wave (a multiple of the tile)
    const int kbeg = first + sb * rk + wave * rkw;
    const int kend = min(kbeg + rkw, lp + 1);
    const int nt = kend > kbeg ? (kend - kbeg + MF8_TILE - 1) / MF8_TILE : 0;  // 0: a wave with no keys

    // the codes of the tile at key kt: rows past the wave's keys read the tile's first row (a key of
    // the context) and are masked below; the slot modulo once per tile, the wrap per key row
    auto load = [&](int kt, Mf8Tile& T) {
        const int slot0 = kt % cap;
        auto row = [&](int key) {
            int s = slot0 + (kt + key < kend ? key : 0);
            s = s >= cap ? s - cap : s;
            return (size_t)s * kvd + kvh * HD;
        };
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint4* kr = reinterpret_cast<const uint4*>(Kc + row(16 * j + c16) + 32 * g);
            T.k[j][0] = kr[0];
            T.k[j][1] = kr[1];
        }
#pragma unroll
        for (int i = 0; i < 8; i++) T.v[i] = *reinterpret_cast<const uint2*>(Vc + row(mf8_key(g, i)) + 8 * c16);
    };
    Mf8Tile cur, nxt;
    if (nt > 0) load(kbeg, cur);  // in flight across the query staging

    const bool holds_new = sb == S - 1;  // the range whose keys end at the new position lp
    if (FUSE) {
        // RoPE of the group's queries and, in the range holding lp, of the new key plus the KV append
        // (k_attn_decode's fused prologue, voxtral_decoder.c:709-722), from the QKV slabs of stream zb;
        // the new key's codes also stay in LDS for the tile that holds lp
        const int qd = H * HD;
        const float* rp = F.rope + (size_t)lp * HD;
        const size_t slot = (size_t)(lp % cap) * kvd + kvh * HD;
        const int nq = nh * HD / 2, nj = nq + (holds_new ? HD / 2 + HD : 0);
        for (int j = tid; j < nj; j += NT) {
            if (j < nq) {
                const int h = j / (HD / 2), d = j % (HD / 2);
                const int col = (h0 + h) * HD + 2 * d;
                const float2 xx = psum2(F.qkv, F.S, F.N, zb, col);
                const float x0 = xx.x, x1 = xx.y;
                const float c = rp[2 * d], sn = rp[2 * d + 1];
                sQ[h][2 * d] = x0 * c - x1 * sn;
                sQ[h][2 * d + 1] = x0 * sn + x1 * c;
            } else if (j < nq + HD / 2) {
                const int d = j - nq, col = qd + kvh * HD + 2 * d;
                const float2 xx = psum2(F.qkv, F.S, F.N, zb, col);
                const float x0 = xx.x, x1 = xx.y;
                const float c = rp[2 * d], sn = rp[2 * d + 1];
                const uint16_t code2 = (uint16_t)kv8_enc2(x0 * c - x1 * sn, x0 * sn + x1 * c);
                *reinterpret_cast<uint16_t*>(&sKn[2 * d]) = code2;
                *reinterpret_cast<uint16_t*>(const_cast<uint8_t*>(Kc) + slot + 2 * d) = code2;
            } else {
                const int e = j - nq - HD / 2;
                const uint8_t code = kv8_t(psum(F.qkv, F.S, F.N, zb, qd + kvd + kvh * HD + e)).b;
                sVn[e] = code;
                const_cast<uint8_t*>(Vc)[slot + e] = code;
            }
        }
    } else {
        const float* __restrict__ q = attn_q(P, zb);
        for (int e = tid; e < nh * HD; e += NT) sQ[e / HD][e % HD] = q[(size_t)h0 * HD + e];
    }
    __syncthreads();

    // B operand of Q.K: the lane's head (c16, zero past the group), dims 32 g + 8 c + i, three planes,
    // held for the whole loop
    bf16x8 qp[4][3];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        float qv[8];
#pragma unroll
        for (int i = 0; i < 8; i++) qv[i] = c16 < nh ? sQ[c16 & 3][32 * g + 8 * c + i] : 0.f;
        mf8_split8(qv, qp[c][0], qp[c][1], qp[c][2]);
    }

    // running state: m and l of head c16 (l a per-lane share, summed over g at the end); o rows =
    // heads (lanes g = 0, element i = head i), column tile t = dim 8 c16 + t
    float m = -1e30f, lsum = 0.f;
    f32x4 o[8];
#pragma unroll
    for (int t = 0; t < 8; t++) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ti = 0; ti < nt; ti++) {
        const int kt = kbeg + ti * MF8_TILE;
        if (ti + 1 < nt) load(kt + MF8_TILE, nxt);
        if (FUSE && holds_new && lp >= kt && lp < kt + MF8_TILE) {
            // this tile holds the new key (wave-uniform test): its codes from LDS, not from the ring
            const int kl = lp - kt;
            if (c16 == (kl & 15)) {
                const uint4* kr = reinterpret_cast<const uint4*>(&sKn[32 * g]);
#pragma unroll
                for (int j = 0; j < 2; j++)
                    if (j == (kl >> 4)) {
                        cur.k[j][0] = kr[0];
                        cur.k[j][1] = kr[1];
                    }
            }
#pragma unroll
            for (int i = 0; i < 8; i++)
                if (mf8_key(g, i) == kl) cur.v[i] = *reinterpret_cast<const uint2*>(&sVn[8 * c16]);
        }
        // ---- scores of the two 16-key halves: lane (head c16, g) element i = key 16 j + 4 g + i ----
        f32x4 s[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            const uint32_t kw[8] = {cur.k[j][0].x, cur.k[j][0].y, cur.k[j][0].z, cur.k[j][0].w,
                                    cur.k[j][1].x, cur.k[j][1].y, cur.k[j][1].z, cur.k[j][1].w};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const bf16x8 ka = mf8_cvt8(kw[2 * c], kw[2 * c + 1]);
#pragma unroll
                for (int p = 0; p < 3; p++) s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qp[c][p], s[j], 0, 0, 0);
            }
        }
        // ---- softmax step: keys past the wave's share are -inf; the tile's max meets across g ----
        float sc[8], mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            sc[i] = (kt + mf8_key(g, i) < kend) ? s[i >> 2][i & 3] * scale : -INFINITY;
            mx = fmaxf(mx, sc[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);  // finite: the tile has a key
        const float fac = expf(m - mn);
        m = mn;
        float pv[8], ps = 0.f;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            pv[i] = c16 < nh ? expf(sc[i] - mn) : 0.f;  // rows past the group stay zero
            ps += pv[i];
        }
        lsum = fmaf(lsum, fac, ps);
        bf16x8 pp[3];
        mf8_split8(pv, pp[0], pp[1], pp[2]);
        // o's rows are heads: head i's factor from lane i
        float fh[4];
#pragma unroll
        for (int i = 0; i < 4; i++) fh[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fac), i));
        // ---- P.V: rows (2 q, 2 q + 1) interleaved per dim pair u, then converted per dim ----
        uint32_t w[4][4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            w[q][0] = __builtin_amdgcn_perm(cur.v[2 * q + 1].x, cur.v[2 * q].x, 0x05010400u);
            w[q][1] = __builtin_amdgcn_perm(cur.v[2 * q + 1].x, cur.v[2 * q].x, 0x07030602u);
            w[q][2] = __builtin_amdgcn_perm(cur.v[2 * q + 1].y, cur.v[2 * q].y, 0x05010400u);
            w[q][3] = __builtin_amdgcn_perm(cur.v[2 * q + 1].y, cur.v[2 * q].y, 0x07030602u);
        }
#pragma unroll
        for (int t = 0; t < 8; t++) {
            uint32_t b[4];
#pragma unroll
            for (int q = 0; q < 4; q++) b[q] = (t & 1) ? mf8_cvt2<true>(w[q][t >> 1]) : mf8_cvt2<false>(w[q][t >> 1]);
            const bf16x8 vb = __builtin_bit_cast(bf16x8, make_uint4(b[0], b[1], b[2], b[3]));
#pragma unroll
            for (int i = 0; i < 4; i++) o[t][i] *= fh[i];
#pragma unroll
            for (int p = 0; p < 3; p++) o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pp[p], vb, o[t], 0, 0, 0);
        }
        if (ti + 1 < nt) cur = nxt;
    }

    // ---- merge the waves (in LDS), as k_attn_decode does ----
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    if (lane < nh) {
        sM[wave][lane] = m;
        sL[wave][lane] = lsum;
    }
    if (g == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (i < nh) {
                *reinterpret_cast<float4*>(&sO[wave][i][8 * c16]) = make_float4(o[0][i], o[1][i], o[2][i], o[3][i]);
                *reinterpret_cast<float4*>(&sO[wave][i][8 * c16 + 4]) = make_float4(o[4][i], o[5][i], o[6][i], o[7][i]);
            }
    }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t Pr = __builtin_amdgcn_make_buffer_rsrc(part, 0, 0x7fffffff, 0x00020000);
    for (int e = tid; e < nh * HD; e += NT) {
        const int h = e / HD, d = e % HD;
        float M = -1e30f;
#pragma unroll
        for (int w = 0; w < NWV; w++) M = fmaxf(M, sM[w][h]);
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; w++) {
            const float f = expf(sM[w][h] - M);
            den = fmaf(f, sL[w][h], den);
            num = fmaf(f, sO[w][h][d], num);
        }
        if (S == 1) {
            sRow[h][d] = den > 0.f ? num * (1.0f / den) : 0.f;
        } else {
            // partials go out write-through (sc1): the merging block may sit behind another L2
            const int po = (int)(((size_t)(h0 + h) * maxs + sb) * (HD + 2)) * 4;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(num), Pr, po + d * 4, 0, 16);
            if (d == 0) {
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(M), Pr, po + HD * 4, 0, 16);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(den), Pr, po + (HD + 1) * 4, 0, 16);
            }
        }
    }
    int* cnt = reinterpret_cast<int*>(part + (size_t)H * maxs * (HD + 2)) + kvh;
    if (S > 1) {
        // the last of the S blocks of this (stream, kv head) to arrive merges their partials: stores
        // drained, one arrival count per kv head past the partials, reset by the merging block
        __shared__ int sLast;
        __shared__ float sCf[4][ATT_MAX_PARTS];
        __shared__ float sCden[4];
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        if (tid == 0) sLast = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == S - 1;
        __syncthreads();
        if (!sLast) return;
        for (int h = wave; h < nh; h += NWV) {
            float mk[2], lk[2], mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int k = lane + 64 * j;
                const int po = (int)(((size_t)(h0 + h) * maxs + k) * (HD + 2) + HD) * 4;
                mk[j] = k < S ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(Pr, po, 0, 16)) : -INFINITY;
                lk[j] = k < S ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(Pr, po + 4, 0, 16)) : 0.f;
                mx = fmaxf(mx, mk[j]);
            }
            mx = wave_max(mx);
            float den = 0.f;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int k = lane + 64 * j;
                if (k < S) {
                    const float f = expf(mk[j] - mx);
                    sCf[h][k] = f;
                    den = fmaf(f, lk[j], den);
                }
            }
            den = wave_sum(den);
            if (lane == 0) sCden[h] = den;
        }
        __syncthreads();
        for (int e = tid; e < nh * HD; e += NT) {
            const int h = e / HD, d = e % HD;
            auto pnum = [&](int k) {
                return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                    Pr, (int)(((size_t)(h0 + h) * maxs + k) * (HD + 2) + d) * 4, 0, 16));
            };
            float num = 0.f;
            int k = 0;
            for (; k + 8 <= S; k += 8) {  // 8 partial loads in flight per step, in range order
                float t[8];
#pragma unroll
                for (int j = 0; j < 8; j++) t[j] = pnum(k + j);
#pragma unroll
                for (int j = 0; j < 8; j++) num = fmaf(sCf[h][k + j], t[j], num);
            }
            for (; k < S; k++) num = fmaf(sCf[h][k], pnum(k), num);
            const float den = sCden[h];
            sRow[h][d] = den > 0.f ? num * (1.0f / den) : 0.f;
        }
    }
    __syncthreads();
    // ---- the group's attention rows: f32 rows (unfused; the wide step's row-major fallback) and, fused,
    // the wo input planes of stream zb, 8 consecutive dims per thread ----
    if (!FUSE || (ATTN_ROWS && out))
        for (int e = tid; e < nh * HD; e += NT) out[(size_t)h0 * HD + e] = sRow[e / HD][e % HD];
    if (FUSE) {
        for (int e = tid; e < nh * HD / 8; e += NT) {
            const int h = e / (HD / 8), d0 = (e % (HD / 8)) * 8;
            uint32_t hp[4], mp[4], lq[4];
#pragma unroll
            for (int i = 0; i < 8; i += 2) {
                uint16_t a0, b0, c0, a1, b1, c1;
                split3(sRow[h][d0 + i], a0, b0, c0);
                split3(sRow[h][d0 + i + 1], a1, b1, c1);
                hp[i / 2] = a0 | ((uint32_t)a1 << 16);
                mp[i / 2] = b0 | ((uint32_t)b1 << 16);
                lq[i / 2] = c0 | ((uint32_t)c1 << 16);
            }
            const int kq = (h0 + h) * HD + d0;
            *reinterpret_cast<uint4*>(F.xs + frag_at(zb, H * HD, 0, kq)) = make_uint4(hp[0], hp[1], hp[2], hp[3]);
            *reinterpret_cast<uint4*>(F.xs + frag_at(zb, H * HD, 1, kq)) = make_uint4(mp[0], mp[1], mp[2], mp[3]);
            *reinterpret_cast<uint4*>(F.xs + frag_at(zb, H * HD, 2, kq)) = make_uint4(lq[0], lq[1], lq[2], lq[3]);
        }
    }
    if (S > 1 && tid == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// all 256 codes through mf8_cvt2, the kernel's FP8 -> bf16 route (the convert test)
__global__ void k_attn_mf8_codes(uint16_t* __restrict__ bits) {
    const uint32_t c = threadIdx.x * 2, w = c | ((c + 1) << 8);
    const uint32_t lo = mf8_cvt2<false>(w), hi = mf8_cvt2<true>(w << 16);
    bits[c] = (uint16_t)lo;
    bits[c + 1] = (uint16_t)(hi >> 16);
}

// ============================================================================
// Host side: the process-wide switch, the launch counts per form, the launchers
// ============================================================================
static int g_attn_mf8 = -1;
static long long g_attn_mf8_n[ATTN_MF8_FORMS];
int attn_mf8_mode() {
    if (g_attn_mf8 < 0) {
        const char* e = getenv("VOX_HIP_ATTN_MF8");
        g_attn_mf8 = e && atoi(e) == 1 ? 1 : 0;
    }
    return g_attn_mf8;
}
void attn_mf8_set(int on) { g_attn_mf8 = on ? 1 : 0; }
void attn_mf8_counts(long long* out) {
    for (int i = 0; i < ATTN_MF8_FORMS; i++) out[i] = g_attn_mf8_n[i];
}

template <int FUSE, class AP>
static hipError_t mf8_launch(const AP& p, const AttnFuse& f, int nb, int cap, int pos_host, int window, float scale, int H,
                             int KVH, int splits, hipStream_t st, int form) {
    const int maxs = attn_maxch(window), rk = g_attn_mf8_range;
    constexpr bool ragged = std::is_base_of_v<AttnPtrsRag, AP> || std::is_base_of_v<AttnSlotsRag, AP>;
    if (H % KVH || H / KVH > 4 || maxs > ATT_MAX_PARTS || splits < 2 || splits > attn_maxsplits(window) || nb < 1 ||
        rk % (MF8_WAVES * MF8_TILE) || (window + rk - 1) / rk > maxs || (!ragged && cap < MF8_TILE))
        return hipErrorInvalidValue;
    const int nsb = (splits * ATT_BLOCK_KEYS + rk - 1) / rk;  // key ranges provided per kv head
    hipLaunchKernelGGL((k_attn_decode_mf8<FUSE, AP>), dim3(nsb * KVH, 1, nb), dim3(MF8_WAVES * 64), 0, st, p, cap, pos_host,
                       window, scale, H, KVH, maxs, rk, f);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) g_attn_mf8_n[form]++;
    return e;
}

hipError_t launch_attn_mf8(const AttnPtrs& p, int nb, int cap, int pos_host, int window, float scale, int H, int KVH,
                           int splits, hipStream_t st, int form) {
    if (nb > VOX_MAX_BATCH || (form != ATTN_MF8_SINGLE && form != ATTN_MF8_BATCH)) return hipErrorInvalidValue;
    return mf8_launch<0>(p, AttnFuse{}, nb, cap, pos_host, window, scale, H, KVH, splits, st, form);
}
hipError_t launch_attn_mf8_fused(const AttnPtrs& p, const AttnFuse& f, int nb, int cap, int window, float scale, int H,
                                 int KVH, int splits, hipStream_t st) {
    return mf8_launch<1>(p, f, nb, cap, 0, window, scale, H, KVH, splits, st, ATTN_MF8_PTRS);
}
hipError_t launch_attn_mf8_fused(const AttnPtrsRag& p, const AttnFuse& f, int nb, int cap, int window, float scale, int H,
                                 int KVH, int splits, hipStream_t st) {
    return mf8_launch<1>(p, f, nb, cap, 0, window, scale, H, KVH, splits, st, ATTN_MF8_PTRS_RAG);
}
hipError_t launch_attn_mf8_fused(const AttnSlots& p, const AttnFuse& f, int nb, int cap, int window, float scale, int H,
                                 int KVH, int splits, hipStream_t st) {
    return mf8_launch<1>(p, f, nb, cap, 0, window, scale, H, KVH, splits, st, ATTN_MF8_SLOTS);
}
hipError_t launch_attn_mf8_fused(const AttnSlotsRag& p, const AttnFuse& f, int nb, int cap, int window, float scale, int H,
                                 int KVH, int splits, hipStream_t st) {
    return mf8_launch<1>(p, f, nb, cap, 0, window, scale, H, KVH, splits, st, ATTN_MF8_SLOTS_RAG);
}
hipError_t launch_attn_mf8_codes(uint16_t* bits, hipStream_t st) {
    hipLaunchKernelGGL(k_attn_mf8_codes, dim3(1), dim3(128), 0, st, bits);
    return hipGetLastError();
}

}  // namespace vox
