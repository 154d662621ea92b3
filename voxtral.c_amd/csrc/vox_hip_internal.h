// vox_hip_internal.h -- kernel launch interface shared by the engine and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vox {

enum { EPI_STORE = 0, EPI_RESID = 1, EPI_GELU = 2, EPI_GELU_ERF = 3, EPI_SWIGLU = 4, EPI_QKV = 5, EPI_LOGITS = 6,
       EPI_LOGITS_ALT = 7,
       EPI_PARTIAL = 8,      // split-K GEMM slice: raw f32 tile into a workspace, epilogue in k_splitk_reduce
       EPI_QKV_BIAS = 9 };   // EPI_QKV with the projection's bias added before RoPE (the encoder's)
constexpr int ALT_TEXT_MIN = 1000;   // TOKEN_TEXT_MIN (voxtral.c:399)
constexpr int ALT_PART = 10;         // per-block alt partial: m, s, 4 values, 4 ids
constexpr int ALT_REC = 8;           // per-step alt record: p_best, (id, p) x 3, pad
enum { PRO_NONE = 0, PRO_NORM = 1, PRO_NORM_ADA = 2 };
// k_gemv weight formats: bf16 rows, Q8 rows + row scales, wpack13 planes (vox_wpack.h), wmx4
// plane (vox_wmx4.h).  The skinny MFMA kernels (k_skf, k_skl, k_skl2, k_sklx) take WF_BF16 and
// WF_Q8 as fragment-major copies and WF_MX4 as the wmx4 fragment plane.
enum { WF_BF16 = 0, WF_Q8 = 1, WF_P13 = 2, WF_MX4 = 3 };

constexpr int GEMV_MAX_BLOCKS = 1024;  // 4 blocks of 256 threads per CU on 256 CUs

struct GemvArgs {
    const float* x;        // input vector [K] (device)
    int K;
    const void* W;         // bf16 [rows, K], or int8 [rows, K] when wscale is set
    const float* wscale;   // Q8 per-row scales (null: bf16 weights)
    // wpack13 copy of W (vox_wpack.h; null: stream W itself): main plane, the side plane
    // laid out for this launch's row groups, and the tensor's exponent offset D
    const void* wp_main = nullptr;
    const void* wp_side = nullptr;
    int wp_d = 0;
    // wmx4 copy of W (vox_wmx4.h; null: none), laid out for gemv_rowgroup_mx4(rows); streamed
    // in preference to the wpack13 planes
    const void* wm_plane = nullptr;
    int rows;              // output rows streamed (2*hidden for SWIGLU)
    const float* norm_w;   // PRO_NORM*: RMSNorm weight [K]
    const float* ada;      // PRO_NORM_ADA: ada_scale row [K]
    float eps;
    float* y;              // output
    const float* bias;     // optional bias (STORE / RESID)
    // EPI_QKV
    int qd, kvd, hd;
    const float* rope;     // rope table [pos][hd]
    const int* state;      // device state (state[0] = logical position) or null
    int pos;               // logical position when state == null
    float* Kc;             // decoder ring (elements of type kvt)
    float* Vc;
    int cap;
    int kvt = 0;           // KV_F32 / KV_F16 / KV_FP8
    // EPI_LOGITS(_ALT)
    float* part_val;
    int* part_idx;
    float* part_alt;       // EPI_LOGITS_ALT: [blocks][ALT_PART]
};

// decoder KV ring element types (vox_hip_model_set_kv_dtype); the element's size in bytes
enum { KV_F32 = 0, KV_F16 = 1, KV_FP8 = 2 };
static inline size_t kv_esize(int kvt) { return kvt == KV_FP8 ? 1 : kvt == KV_F16 ? 2 : 4; }
// Which rings exist, for every launcher's kvt argument (the element type that Kc / Vc point at):
// f32 rings at any head_dim; the decoder's 16-bit (VOX_DECODER_KV_FP16) and one-byte (VOX_HIP_KV_FP8,
// vox_kv8.h) rings at head_dim 128 only; the encoder's opt-in 16-bit rings
// and one-byte rings (vox_hip_model_set_enc_kv_dtype; FP8 by the same vox_kv8.h rule) at head_dim 64.
// The launchers pick their instance through kv_ring (vox_hip_kernels.hip): at head_dim 64 a narrow
// ring selects the encoder's instances (KvRing<.., 1>), at 128 the decoder's.
static inline bool kv_ring_ok(int kvt, int hd) {
    return kvt == KV_F32 || ((kvt == KV_F16 || kvt == KV_FP8) && (hd == 128 || hd == 64));
}

constexpr int VOX_MAX_BATCH = 32;    // streams per skinny batched decode step (two 16-row blocks of the MFMA B
                                     // operand), per batched encoder pass (EncRows) and per vox_hip_skinny_wmx4 call
constexpr int VOX_MAX_SLOTS = 128;   // slots of a batch object: buckets 64 and 128 take the k_gemmf step (batch_step_wide)

// One row of a batched decode step, in device memory (the batch's slot table).  The step
// graph's kernel arguments point at the table, never at a stream, so streams join and leave
// a batch without a graph capture: the host rewrites the table before a call, the step's
// last kernel (k_argmax_batch_final) advances it, and a slot whose `live` is 0 costs no
// attention, KV append, argmax or state change (its row still rides through the GEMMs).
struct BatchSlot {
    int* state;             // the stream's {kv logical pos, next adapter row, prev token, step}
    int* tokens;            // the stream's token ring (tokens_cap entries)
    const float* adapter;   // the stream's adapter rows
    char* Kc;               // layer-0 base of the stream's decoder K / V rings (bytes)
    char* Vc;
    float* alts;            // stream_fill_alts records (null: no alternatives for this slot)
    int adapter_rows;       // rows the slot may consume (the stream's adapter count at the call)
    int left;               // steps the slot may still take in this call
    int stop_tok;           // the slot stops after emitting this id (TOKEN_EOS, or -1)
    int live;               // the current step runs for this slot
    int pos;                // state[0] mirror: the attention starts without the state hop
    int produced;           // steps taken in this call (index into the batch's token log)
    const float* ada;       // the slot's ada table [dec_layers][dec_dim] (the model's, or its stream's delay's;
                            // read by the per-slot norm instances of a call with delays of its own)
};
static_assert(sizeof(BatchSlot) == 80, "BatchSlot layout");
// k_gemvr: k_gemv over R <= 8 input rows (a small batched decode step).  g describes row 0
// (x, y) and everything the rows share; biases are not taken.
constexpr int GEMVR_MAX_ROWS = 8;
struct GemvRArgs {
    GemvArgs g;
    int ldx, ldy;            // floats between consecutive rows of x / y
    // EPI_QKV: row r takes position, liveness and rings (layer-0 base + ring_off bytes) from
    // slots[r]; g.state / g.pos / g.Kc / g.Vc are not used
    const BatchSlot* slots;
    size_t ring_off;
};
constexpr int BATCH_TOKLOG = 64;    // per-slot token log entries (>= the steps between reads)

// per-stream operands of one decode-attention launch (blockIdx.z = stream of a batch)
struct AttnPtrs {
    const float* q[VOX_MAX_BATCH];
    const float* Kc[VOX_MAX_BATCH];
    const float* Vc[VOX_MAX_BATCH];
    const int* state[VOX_MAX_BATCH];
    float* part[VOX_MAX_BATCH];
    float* out[VOX_MAX_BATCH];
    // batched step: Kc / Vc / position / liveness from the slot table (layer base + ring_off)
    const BatchSlot* slots = nullptr;
    size_t ring_off = 0;
};
// The slot-table case of AttnPtrs in compact form (the wide batched step: up to VOX_MAX_SLOTS
// rows, where six pointer arrays would be ~6 KB of kernel arguments): row z reads q at
// q + z * q_ld (unused by the fused instances), keeps its partials at part + z * part_ld and
// takes ring, position and liveness from slots[z]
struct AttnSlots {
    const float* q;
    float* part;
    float* out;              // f32 rows (unused by the fused instances: they write F.xs)
    size_t q_ld, part_ld, out_ld;
    const BatchSlot* slots;
    size_t ring_off;
};
// The ragged forms of the two: a batched call in which some stream's decoder rings
// are shorter than window + slack (vox_hip_model_set_kv_grow).  Row z's ring holds caps[z] slots:
// that capacity is the slot modulo, and layer `layer` of the ring starts
// layer * caps[z] * KVH * hd * sizeof(element) bytes past the slot's Kc / Vc (ring_off and the
// launch's shared cap are not read).  caps is a table beside the slot table, [slot] ints, that
// only these instances read: BatchSlot, its upload and every plain instance stay as they are.
struct AttnPtrsRag : AttnPtrs {
    const int* caps = nullptr;
    int layer = 0;
};
struct AttnSlotsRag : AttnSlots {
    const int* caps;
    int layer;
};
// batched decode attention with the QKV epilogue folded in (k_attn_decode<.., FUSE = 1>):
// RoPE of q / k and the KV append read the QKV projection's split-K slabs, and the output
// goes straight into the wo input planes
struct AttnFuse {
    const float* qkv;      // [S][16][N] slabs, row z = stream z of the batch
    int S, N;              // slab count, row length (H*hd + 2*KVH*hd)
    const float* rope;     // [pos][hd] (cos, sin) table
    uint16_t* xs;          // [3][16][H*hd] fragment-major planes of the attention output
};

constexpr int ARGB = 64;                // argmax partial blocks per row

int gemv_grid(int rows);
int gemv_rowgroup(int rows);  // rows per k_gemv group (the wpack13 side plane is laid out for it)
int gemv_rowgroup_mx4(int rows);  // rows per group of the wmx4 instances (the wmx4 plane is laid out for it)
int gemv_grid_mx4(int rows);      // blocks of a wmx4 launch (the LM head's argmax partials)
bool gemv_ok_mx4(int rows, int K);  // shapes the wmx4 instances accept
bool gemv_ok(int rows, int K, int q8);  // shapes launch_gemv accepts (rows, K multiple of the chunk)
int attn_maxch(int window);      // decode-attention partials per head (64-key blocks)
int attn_maxsplits(int window);  // 256-key spans of a window (graph buckets)
hipError_t launch_rmsnorm_rows(const float* x, int ldx, float* y, int ldy, const float* w,
                               const float* ada, int M, int D, float eps, hipStream_t st);
// row r's ada row = slots[r].ada + ada_off (M <= VOX_MAX_SLOTS; a slot without a table: no ada)
hipError_t launch_rmsnorm_rows_slots(const float* x, int ldx, float* y, int ldy, const float* w, const BatchSlot* slots,
                                     size_t ada_off, int M, int D, float eps, hipStream_t st);
// ws: f32 workspace for split-K partials (ws_elems floats; nullptr = no split)
hipError_t launch_gemm(int epi, int nsplit, const float* A, int lda, const void* W,
                       const float* wscale, int K, int M, int N, const float* bias, float* C,
                       int ldc, hipStream_t st, float* ws = nullptr, size_t ws_elems = 0);
hipError_t launch_rope_kv(const float* qkv, int M, int qd, int kvd, int hd, const float* rope,
                          int pos0, float* q, float* Kc, float* Vc, int cap, hipStream_t st, int kvt = 0);
hipError_t launch_attn_rows_mf(int hd, const float* Q, int ldq, const float* Kc, const float* Vc,
                             int cap, float* O, int ldo, int M, int H, int KVH, int q_pos0,
                             int k_first, int window, float scale, hipStream_t st, float* ws = nullptr,
                             size_t ws_elems = 0, uint16_t* xs = nullptr, int kvt = 0, int* ns_out = nullptr);
// ns_out: the number of key-range splits the launch took (> 1: split grid + combine)
// xs: the output also (or only, through the combine kernel) as fragment-major planes
// the skinny encoder's QKV slabs (+ bias) -> RoPE'd q rows and the K/V ring slots (one pass)
hipError_t launch_slabs_rope_kv(const float* part, int S, int M, const float* bias, int qd, int kvd, int hd,
                                const float* rope, int pos0, float* q, float* Kc, float* Vc, int cap, hipStream_t st,
                                int kvt = 0);
hipError_t launch_gemv(int pro, int epi, const GemvArgs& a, hipStream_t st);
const void* gemv_kernel(int pro, int epi, const GemvArgs& a);
hipError_t launch_gemv_timed(int pro, int epi, const GemvArgs& a, hipEvent_t start, hipEvent_t stop,
                             hipStream_t st);
int gemv_occupancy(const void* fn);
// R = 1, 2, 4 or 8 rows; (pro, epi) in {NORM/QKV, NONE/RESID, NORM_ADA/SWIGLU, NORM/STORE (the
// LM head), NONE/STORE}.  gemvr_ok: the launch has an instance (K rounds <= 2 where the input
// is a dec_dim row or the group is 8 rows, <= 5 otherwise)
bool gemvr_ok(int pro, int epi, int rows, int K);
// the same for the wmx4 instances (g.wm_plane set: streamed in preference to the wpack13 planes,
// in groups of gemv_rowgroup_mx4(rows) = 4 or 8 rows)
bool gemvr_ok_mx4(int pro, int epi, int rows, int K);
// the same for the Q8 instances (g.wscale set: int8 rows of K bytes with one f32 scale per row,
// taken in preference to every plane; K rounds of 256 16-weight chunks, <= 3)
bool gemvr_ok_q8(int pro, int epi, int rows, int K);
hipError_t launch_gemvr(int pro, int epi, int R, const GemvRArgs& a, hipStream_t st);
const void* gemvr_kernel(int pro, int epi, int R, const GemvRArgs& a);
// part: H * attn_maxch(window) * (hd + 2) floats of partials, then KVH ints (zeroed before
// the first launch) that count the split blocks' arrivals
hipError_t launch_attn_decode(int hd, const float* q, const float* Kc, const float* Vc, int cap,
                              const int* state, int pos_host, int window, float scale, int H,
                              int KVH, float* part, float* out, int splits, hipStream_t st, int kvt = 0);
// the same over nb streams at once (device state positions; pointers per stream)
hipError_t launch_attn_decode_batch(int hd, const AttnPtrs& p, int nb, int cap, int window, float scale,
                                    int H, int KVH, int splits, hipStream_t st, int kvt = 0);
// the FP8 ring helpers over groups of 8 values (vox_hip_kv8_convert): x [8 groups] -> codes, back
hipError_t launch_kv8_convert(const float* x, int groups, uint8_t* codes, float* back, hipStream_t st);
constexpr int ATT_BLOCK_KEYS = 256;  // keys one decode-attention block covers
// the batched step's attention: RoPE + KV append from the QKV slabs, output as planes
// (one block per stream x kv head x 256-key split; splits > 1 adds the combine kernel)
hipError_t launch_attn_batch_fused(int hd, const AttnPtrs& p, const AttnFuse& f, int nb, int cap, int window,
                                   float scale, int H, int KVH, int splits, hipStream_t st, int kvt = 0);

// the same for the wide step: nb <= VOX_MAX_SLOTS slots, f.qkv the QKV projection's f32 rows
// (f.S = 1: [nb][N]), f.xs the wo input planes [row block][3][16][H * hd] that k_gemmf reads.
// splits == 1: one 1024-thread block per (slot, kv head); > 1: the 128-key split grid, the last
// block of a (slot, kv head) to arrive merging the partials
hipError_t launch_attn_batch_wide(int hd, const AttnSlots& p, const AttnFuse& f, int nb, int cap, int window,
                                  float scale, int H, int KVH, int splits, hipStream_t st, int kvt = 0);

// the two launches above over rings of per-slot capacity (p.caps, p.layer; no shared cap): the
// same grids, blocks and arithmetic, only the ring addresses differ
hipError_t launch_attn_batch_fused_rag(int hd, const AttnPtrsRag& p, const AttnFuse& f, int nb, int window, float scale,
                                       int H, int KVH, int splits, hipStream_t st, int kvt = 0);
hipError_t launch_attn_batch_wide_rag(int hd, const AttnSlotsRag& p, const AttnFuse& f, int nb, int window, float scale,
                                      int H, int KVH, int splits, hipStream_t st, int kvt = 0);

// a batched encoder pass: rows [off[b], off[b] + nr[b]) of the stacked rows belong to stream
// b, at logical positions pos0[b] + i, with its own K/V ring (layer base)
struct EncRows {
    int B;
    int off[VOX_MAX_BATCH], nr[VOX_MAX_BATCH], pos0[VOX_MAX_BATCH];
    float* Kc[VOX_MAX_BATCH];
    float* Vc[VOX_MAX_BATCH];
};
// RoPE + K/V append of every stacked row into its stream's ring (k_rope_kv per row block)
// kvt (here and in launch_attn_rows): the rings' element type, er.Kc / er.Vc point at such
// elements (kv_ring_ok)
hipError_t launch_rope_kv_rows(const float* qkv, int N, int qd, int kvd, int hd, const float* rope_table,
                               const EncRows& er, float* q, int cap, hipStream_t st, int kvt = 0);
// windowed attention of every stream's rows against its own ring, one launch (+ one combine):
// Q / O stacked [N, H*hd]
hipError_t launch_attn_rows(int hd, const float* Q, const EncRows& er, int N, int cap, float* O, int H, int KVH,
                            int window, float scale, float* ws, size_t ws_elems, hipStream_t st, uint16_t* xs = nullptr,
                            int kvt = 0);
constexpr int STEP_GRAPHS = 8;       // step graphs by attention split count 1, 2, 4, ..., 128
hipError_t launch_attn_batch_dbg(const AttnPtrs& p, const AttnFuse& f, int nb, int cap, int window, float scale, int H,
                                 int KVH, int splits, hipStream_t st);
hipError_t launch_attn_dbg(int dbg, const float* q, const float* Kc, const float* Vc, int cap,
                           const int* state, float* part, float* out, hipStream_t st);
hipError_t launch_embed_step(const float* adapter, const void* emb, const float* esc, const int* state,
                             int D, float* x, hipStream_t st);
hipError_t launch_embed_rows(const float* adapter, const void* emb, const float* esc, int row0, int n,
                             int first_tok, int rest_tok, int D, float* x, hipStream_t st);
hipError_t launch_argmax_final(const float* pv, const int* pi, int n, int* state, int* tokens,
                               int cap, const float* adapter, int adapter_rows,
                               const void* emb, const float* esc, int D, float* x,
                               const float* part_alt, float* alts, int V, hipStream_t st);
// batched step: x_i = adapter_i[state[1]] + tok_emb[state[2]] for every live slot, 0 otherwise
hipError_t launch_embed_batch(const BatchSlot* slots, int nb, const void* emb, const float* esc, int D, float* x,
                              hipStream_t st);
// batched step's end: per live slot the first-max argmax of its logits row, the token into the
// stream's ring and toklog[slot][produced % BATCH_TOKLOG], the stream state and the slot
// advanced (the slot stops at stop_tok, after `left` steps or at its last adapter row), the
// next input row (0 for a slot that stopped); slots with alts also get the step's
// stream_fill_alts record (palt: [nb][ARGB][ALT_PART] scratch).  nb <= VOX_MAX_SLOTS (as
// launch_embed_batch)
hipError_t launch_argmax_batch(const float* logits, int nb, int V, float* pval, int* pidx, float* palt,
                               BatchSlot* slots, int tokens_cap, int* toklog, const void* emb, const float* esc, int D,
                               float* x, hipStream_t st);
// Batched decode GEMMs for M <= 16 rows held as three bf16 planes xs[3][16][K] (hi/mid/lo =
// the exact f32 rows) in MFMA fragment order; weights packed by launch_frag_pack.
// tools/kbench sweep knobs: variables in a kbench build (-DVOX_KBENCH), compile-time constants
// (the product's own choice) in the library
#ifdef VOX_KBENCH
#define VOX_KB_KNOB(name, v) int name = v
#else
#define VOX_KB_KNOB(name, v) constexpr int name = v
#endif
constexpr int SK_ROWS = 16;
constexpr int SK_MAX_ROWS = 96;  // rows of one skinny launch: up to 6 row blocks of 16
                                 // (planes [rb][3][16][K], slabs [rb][S][16][N])
constexpr int PLANE_MAX_ROWS = 1024;  // rows of a planes buffer (one encoder pass, ENC_SUB)
hipError_t launch_frag_pack(const void* src, int N, int K, int q8, void* dst, hipStream_t st);
// RMSNorm (+ ada) of nb rows into planes; S > 0: x += the S split slabs of part first
hipError_t launch_rmsnorm_fplanes(float* x, int nb, int D, const float* w, const float* ada, float eps,
                                  uint16_t* xs, const float* part, int S, hipStream_t st, const float* bias = nullptr);
// the same without slabs, row j's ada row = slots[j].ada + ada_off (nb <= VOX_MAX_SLOTS, D <= 4096)
hipError_t launch_rmsnorm_fplanes_slots(float* x, int nb, int D, const float* w, const BatchSlot* slots, size_t ada_off,
                                        float eps, uint16_t* xs, hipStream_t st);
// x[j] += the S slabs of row j (+ bias); out[j] = the S slabs of row j (+ bias)
hipError_t launch_resid_slabs(float* x, int nb, int D, const float* part, int S, const float* bias, hipStream_t st);
hipError_t launch_slabs_rows(const float* part, int S, int nb, int N, const float* bias, float* out, int ldo,
                             hipStream_t st);
hipError_t launch_split_fplanes(const float* x, int nb, int K, uint16_t* xs, hipStream_t st);
// silu(W1 x) * (W3 x) from the split W1|W3 slabs (N = 2H rows) into planes
hipError_t launch_swiglu_fplanes(const float* part, int S, int H, int nb, uint16_t* xs, hipStream_t st);
// C[j][n] = sum_k x_j[k] W[n][k] (LM head: k_skf)
// mx4 (here and in the launchers below): Wf is the wmx4 fragment plane (vox_wmx4.h) of a bf16
// matrix instead of its fragment-major copy; same geometry, same bits
hipError_t launch_gemm_skf(const uint16_t* xs, int K, const void* Wf, const float* wscale, int N, int nb, float* C,
                           int ldc, hipStream_t st, int mx4 = 0);
// launch_gemm_skf for 17..32 rows (two 16-row blocks of planes, one weight read)
hipError_t launch_gemm_skf2(const uint16_t* xs, int K, const void* Wf, const float* wscale, int N, int nb, float* C,
                            int ldc, hipStream_t st, int mx4 = 0);
// split-K slabs part[s][16][N], s < skl_splits(K, N) (projections: k_skl; k_sklx and the
// encoder's skinny chain use skl_splits(K))
int skl_splits(int K, int N = 0);
// ssq: RMSNorm applied to the results (planes from launch_resid_xw_fplanes, nsl slices per row)
constexpr int SKL_MAX_SLICES = 12;  // D <= 3072
// pair: 17..32 rows through k_skl2 (both row blocks in one block; same bits) where its
// configuration exists (the batched step)
hipError_t launch_gemm_skl(const uint16_t* xs, int K, const void* Wf, const float* wscale, int N, int nb,
                           float* part, hipStream_t st, const float* ssq = nullptr, int nsl = 0, float eps = 0.f,
                           int pair = 0, int mx4 = 0);
hipError_t launch_gemm_skl_cfg(int nw, int ks, const uint16_t* xs, int K, const void* Wf, int N, int nb, float* part,
                               hipStream_t st);  // tools/kbench sweep
hipError_t launch_gemm_skl2_cfg(int nw, int ks, const uint16_t* xs, int K, const void* Wf, int N, int nb, float* part,
                                hipStream_t st);  // tools/kbench sweep: 17..32 rows, weights shared by both row blocks
// x += the S slabs (+ bias); planes of x * w (* (1 + ada)); the row's sums of squares per
// 256-column slice to ssq[row / 16][D / 256][row % 16] (the inverse RMS is applied by
// launch_gemm_skl)
hipError_t launch_resid_xw_fplanes(float* x, int nb, int D, const float* w, const float* ada, uint16_t* xs,
                                   const float* part, int S, const float* bias, float* ssq, hipStream_t st);
// the same with row j's ada row = slots[j].ada + ada_off (same products, same order)
hipError_t launch_resid_xw_fplanes_slots(float* x, int nb, int D, const float* w, const BatchSlot* slots, size_t ada_off,
                                         uint16_t* xs, const float* part, int S, const float* bias, float* ssq,
                                         hipStream_t st);
// k_sklx: k_skl with the neighbouring row kernels folded in (bf16 weights, or their wmx4
// fragment plane).  Inputs are
// always planes; SKX_PRO_SCALE planes hold x * w (* (1 + ada)) of an RMSNorm whose inverse RMS
// is applied to the MFMA results, computed from the row sums of squares that the producer left
// per column slice (ssq_in[rb][nsl][16], summed in slice order).  Epilogue: the slabs go out
// write-through and one ticket per (row block, column slice) counts them; the block that
// completes a slice sums its S slabs in split order (as psum) and finishes it: SKX_EPI_QKV =
// bias + RoPE + K/V ring append (k_slabs_rope_kv), SKX_EPI_RESID = x += slabs + bias, the
// slice's row sums of squares to ssq_out[rb][X][16] and (planes != null) the next
// projection's planes x * nw (* (1 + ada)), SKX_EPI_SWIGLU = silu(W1) * W3 into the next
// projection's planes (k_swiglu_fplanes).
enum { SKX_PRO_PLANES = 0, SKX_PRO_SCALE = 1 };
enum { SKX_EPI_QKV = 1, SKX_EPI_RESID = 2, SKX_EPI_SWIGLU = 3 };
struct SklFused {
    const float* ssq_in = nullptr;
    int nsl = 0;
    float eps = 0.f;
    float* part = nullptr;
    int* ticket = nullptr;  // zeroed once; every finishing block resets its own
    const float* bias = nullptr;
    float* x = nullptr;
    float* ssq_out = nullptr;
    uint16_t* planes = nullptr;
    const float* nw = nullptr;   // SKX_EPI_RESID planes: the next RMSNorm's weight (and ada)
    const float* ada = nullptr;
    const float* rope = nullptr;  // row of position pos0
    int qd = 0, kvd = 0, hd = 0, pos0 = 0, cap = 0;
    float* q = nullptr;
    float* Kc = nullptr;
    float* Vc = nullptr;
    int kvt = 0;                  // SKX_EPI_QKV: the encoder ring's element, KV_F32 / KV_F16 / KV_FP8
};
// column slices of a k_sklx launch (the ssq_out slices its consumer sums)
int sklx_slices(int N, int K);
constexpr int SKX_TICKETS = 4 * 1024;
// mx4: SKX_PRO_SCALE / SKX_EPI_SWIGLU only (the batched decode step's W1|W3)
hipError_t launch_gemm_sklx(int pro, int epi, const uint16_t* xs, int K, const void* Wf, int N, int nb,
                            const SklFused& f, hipStream_t st, int mx4 = 0);
// k_gemmf (vox_hip_gemmf.hip): stream-K MFMA GEMM, planes x fragment-major bf16 (or int8) weights;
// epi in {STORE, RESID, GELU, GELU_ERF, SWIGLU}; SWIGLU with xo writes the gate rows as
// planes [rb][3][16][N / 2].  ws: gemmf_ws_floats(gemmf_grid()) floats of partial tiles,
// flags: gemmf_grid() ints (zeroed once), epoch: > 0, new for every launch on the stream.
bool gemmf_ok(int M, int N, int K);
int gemmf_grid();
size_t gemmf_flag_ints();      // flags buffer: gemmf_grid() flags, then the recompute counter
int set_gemmf_wait(int ticks); // owner's wait per partial in 100 MHz ticks (< 0: always recompute); returns the old
size_t gemmf_ws_floats(int blocks);
// epoch_dev (null: none): a device word added to `epoch` by the kernel, so that a captured launch
// hands off under a new epoch at every replay (launch_gemmf_epoch_bump advances the word);
// rb: row blocks per tile with two planes (0: by shape; 4 or 8); wscale (null: Wf is the bf16
// fragment copy): the [N] row scales of Wf = the int8 fragment copy (k_frag_pack<1>), applied
// to the finished sums before the epilogue (the WF_Q8 instances; same tiles, grid and order)
hipError_t launch_gemmf(int epi, int np, const uint16_t* xs, int K, int M, const void* Wf, int N, const float* bias,
                        float* C, int ldc, uint16_t* xo, float* ws, size_t ws_floats, int* flags, int epoch,
                        hipStream_t st, const int* epoch_dev = nullptr, int rb = 0, const float* wscale = nullptr);
// *epoch_dev += by (back to 1 before the sum could overflow): the last kernel of a captured step
hipError_t launch_gemmf_epoch_bump(int* epoch_dev, int by, hipStream_t st);
// row blocks per tile of the wide step's projections with two planes (profiles/batch_wide_kbench.txt)
int gemmf_wide_rb(int M, int N, int K);
int gemm_planes_np();  // activation planes of the M > 1 GEMMs (2, or 3 with VOX_HIP_GEMM_PLANES=3)
int set_gemm_planes(int np);  // 2 or 3 (vox_hip_set_gemm_planes); -1 otherwise
hipError_t launch_im2col3(const float* src, int C, int T, int stride, int off, float* A,
                          hipStream_t st);
hipError_t launch_mel_tail(const float* melp, int n_new, int MB, float* tail, hipStream_t st);
// device log-mel (vox_hip_mel_*): nframes frames from samples[start0 + 160 f ..]; tables
// transposed: dcosT / dsinT [400][201], filtT [201][128]
hipError_t launch_mel_frames(const float* samples, long long start0, int nframes, const float* window,
                             const float* dcosT, const float* dsinT, const float* filtT, float log_min, float* mel,
                             hipStream_t st);
hipError_t launch_mel_reflect(float* buf, long long n, long long real_end, int len, hipStream_t st);

}  // namespace vox
