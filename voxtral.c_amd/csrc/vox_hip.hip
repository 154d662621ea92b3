// vox_hip.hip -- host side of the MI355X backend: implements include/voxtral_hip.h.
//
// Replaces voxtral_metal.m (SeungheonOh/voxtral.c) for the hot path.  Model weights are
// uploaded once into HBM and packed (Q|K|V merged, W1|W3 interleaved); each stream owns
// its rolling KV caches, conv-stem tails and adapter buffer in HBM; the decoder step is
// one hipGraph replay whose kernels read the step position from device memory, so a run
// of greedy steps never returns to the host (DESIGN.md "Decoder step").
#include "../../include/voxtral_hip.h"
#include "vox_hip_internal.h"
#include "vox_wmx4.h"
#include "vox_wpack.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <stddef.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

using namespace vox;

#define TOKEN_BOS 1
#define TOKEN_EOS 2
#define TOKEN_STREAMING_PAD 32

static thread_local std::string g_err;
static int g_inited = 0;
static size_t g_mem_used = 0;

static int set_err(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    fprintf(stderr, "voxtral_hip: %s\n", buf);
    return -1;
}

// a switch of the form "unset or anything but 0 means on"; the callers read theirs once per process
static int env_on(const char* name) {
    const char* e = getenv(name);
    return (e && atoi(e) == 0) ? 0 : 1;
}

#define CK(expr)                                                                          \
    do {                                                                                  \
        hipError_t e__ = (expr);                                                          \
        if (e__ != hipSuccess)                                                            \
            return set_err("%s failed at %s:%d: %s", #expr, __FILE__, __LINE__, hipGetErrorString(e__)); \
    } while (0)

template <class T>
static hipError_t dalloc(T** p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    hipError_t e = hipMalloc((void**)p, n * sizeof(T));
    if (e == hipSuccess) {
        g_mem_used += n * sizeof(T);
        // The streams are non-blocking, so nothing orders a null-stream memset before the
        // kernels a stream enqueues next: wait for the zeroing before handing the buffer out.
        e = hipMemsetAsync(*p, 0, n * sizeof(T), nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    return e;
}
// Host -> device copy that has landed when it returns (a pageable-source hipMemcpy may
// return once the data is staged, before the DMA that the stream kernels depend on).
static hipError_t h2d(void* dst, const void* src, size_t bytes) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, nullptr);
    return e == hipSuccess ? hipStreamSynchronize(nullptr) : e;
}
template <class T>
static void dfree(T*& p) {
    if (p) hipFree((void*)p);
    p = nullptr;
}

extern "C" const char* vox_hip_last_error(void) { return g_err.c_str(); }
extern "C" void vox_hip_clear_error(void) { g_err.clear(); }

extern "C" int vox_hip_init(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_err("no HIP device");
        return 0;
    }
    g_inited = 1;
    return 1;
}
extern "C" int vox_hip_available(void) { return g_inited; }
extern "C" void vox_hip_shutdown(void) { g_inited = 0; }
extern "C" size_t vox_hip_memory_used(void) { return g_mem_used; }
extern "C" int vox_hip_set_device(int device) {
    CK(hipSetDevice(device));
    return 0;
}

extern "C" void vox_hip_config_voxtral_4b(vox_hip_config_t* c) {
    // voxtral.h:26-50
    c->enc_dim = 1280; c->enc_layers = 32; c->enc_heads = 32; c->enc_kv_heads = 32;
    c->enc_head_dim = 64; c->enc_hidden = 5120; c->enc_window = 750;
    c->dec_dim = 3072; c->dec_layers = 26; c->dec_heads = 32; c->dec_kv_heads = 8;
    c->dec_head_dim = 128; c->dec_hidden = 9216; c->dec_window = 8192;
    c->vocab = 131072; c->mel_bins = 128; c->downsample = 4; c->ada_dim = 32;
    c->rope_theta = 1000000.0f; c->enc_eps = 1e-5f; c->dec_eps = 1e-5f; c->gelu_erf = 0;
}

// ---------------------------------------------------------------------------
// Host math that the reference runs on the CPU once per load (kept bit-identical)
// ---------------------------------------------------------------------------
static float host_gelu(float v, int erf_mode) {
    if (erf_mode) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
    float x3 = v * v * v;
    float inner = 0.7978845608028654f * (v + 0.044715f * x3);
    return 0.5f * v * (1.0f + tanhf(inner));
}

// vox_compute_rope_freqs (voxtral_kernels.c:617-629) for positions [p0, p0+n)
static void host_rope(float* out, int p0, int n, int dim, float theta) {
    int half = dim / 2;
    for (int s = 0; s < n; s++) {
        float p = (float)(p0 + s);
        for (int d = 0; d < half; d++) {
            float freq = 1.0f / powf(theta, (float)(2 * d) / (float)dim);
            float ang = p * freq;
            out[(size_t)s * dim + 2 * d] = cosf(ang);
            out[(size_t)s * dim + 2 * d + 1] = sinf(ang);
        }
    }
}

// ---------------------------------------------------------------------------
// Model
// ---------------------------------------------------------------------------
// Weight matrices are raw bytes: bf16 [rows, K], or int8 [rows, K] when the matching
// scale array (Q8 per-row scales, quantize.py) is non-null.
struct EncLayerD {
    uint8_t *wqkv, *wo, *w13, *w2;
    float *sqkv, *so, *s13, *s2;
    float *bqkv, *bo, *b2, *attn_norm, *ffn_norm;
};
// wpack13 copy of a bf16 matrix for the single-stream GEMV (vox_wpack.h): 13 bits per
// weight, decoded without loss.  main == null: the tensor stays raw.
struct WPackD {
    uint8_t *main, *side;
    int d;
};
// wmx4 plane of a bf16 matrix that is MXFP4-valued (vox_wmx4.h), for the single-stream GEMV:
// 5 bits per weight, decoded without loss.  null: none (the tensor streams as wpack13 or raw).
// frag: its wmx4 fragment plane for the batched MFMA step (vox_hip_set_wmx4_batch), 4.5 bits per
// weight; null: the step reads the tensor's bf16 fragment-major copy.
struct WMx4D {
    uint8_t* plane;
    uint8_t* frag;
};
struct DecLayerD {
    uint8_t *wqkv, *wo, *w13, *w2;
    float *sqkv, *so, *s13, *s2;
    float *attn_norm, *ffn_norm;
    WPackD pqkv, po, p13, p2;
    WMx4D mqkv, mo, m13, m2;
};
// the same matrices in MFMA fragment order for the batched step (k_skf; built on first use)
struct DecFragD {
    uint8_t *wqkv, *wo, *w13, *w2;
};
static int frag_copy(uint8_t** dst, const uint8_t* src, int N, int K, int q8);
struct vox_hip_model;
static int model_frag(vox_hip_model* m);

struct vox_hip_model {
    vox_hip_config_t c;
    int delay_tokens;
    uint16_t *conv0_w, *conv1_w;
    float *conv0_b, *conv1_b, *enc_norm, *dec_norm;
    std::vector<EncLayerD> enc;
    std::vector<DecLayerD> dec;
    uint8_t *ad0, *ad1, *tok_emb;
    float *ad0_s, *ad1_s, *tok_emb_s;  // Q8 scales (null: bf16)
    float* ada_scale;              // device [dec_layers][dec_dim]
    std::vector<float> ada_host;   // host copy
    std::vector<std::vector<float>> ada_down, ada_up;
    // ada tables of streams with a delay of their own (vox_hip_stream_set_delay), [delay]: built on
    // first use, then neither moved nor freed before the model (slot tables and graphs hold them)
    float* ada_tab[VOX_HIP_MAX_DELAY_TOKENS + 1];
    std::vector<float> ada_tab_host[VOX_HIP_MAX_DELAY_TOKENS + 1];
    float *rope_enc, *rope_dec;    // device tables [rope_positions][hd]
    int rope_positions;
    int rope_gen;                  // bumped when the tables are reallocated (graphs hold the pointer)
    std::vector<DecFragD> dfrag;   // fragment-major decoder matrices (empty until a batch or a bf16 prefill)
    std::vector<DecFragD> efrag;   // fragment-major encoder matrices (empty until a short chunk)
    uint8_t* lm_frag;              // fragment-major LM head (tied embeddings)
    int kvt;                       // decoder KV ring element of streams created from now on (KV_F32 / KV_F16 / KV_FP8)
    int ekvt;                      // encoder KV ring element of streams created from now on (KV_F32 / KV_F16 / KV_FP8)
    WPackD plm;                    // wpack13 copy of the LM head
    int wpack;                     // VOX_HIP_WPACK (default 1), read once at creation
    vox_hip_wpack_stats_t wstats;
    WMx4D mlm;                     // wmx4 plane of the LM head
    int wmx4;                      // vox_hip_wmx4() at creation (0 off, 1 detect, 2 round)
    vox_hip_wmx4_stats_t mstats;
    int wmx4_batch;                // vox_hip_wmx4_batch() at creation: fragment planes beside the GEMV planes
    long long fstats[4];           // fragment planes: tensors, plane bytes, their bf16 bytes, host microseconds
    int gemmf_q8;                  // vox_hip_gemmf_q8() at creation: k_gemmf streams the int8 fragment copies of Q8 tensors
    long long n_gemmf_q8;          // k_gemmf launches on int8 fragments (vox_hip_model_gemmf_q8_stats)
    int begun_calls;               // batched calls of this model between begin_rows and finish (their slots read ada_scale)
    int kv_grow;                   // first decoder ring capacity (slots) of streams created from now on; 0: the full ring
};

static int upload(void* dst, const void* src, size_t bytes) {
    if (!src) return set_err("null weight pointer");
    CK(h2d(dst, src, bytes));
    return 0;
}

// f32 tensor that holds bf16 values (the reference's load_f32 of a BF16 tensor) -> bf16
static int upload_f32_as_bf16(uint16_t* dst, const float* src, size_t n) {
    std::vector<uint16_t> tmp(n);
    for (size_t i = 0; i < n; i++) {
        uint32_t u;
        memcpy(&u, &src[i], 4);
        if (u & 0xffffu) return set_err("conv weight is not bf16-representable (element %zu)", i);
        tmp[i] = (uint16_t)(u >> 16);
    }
    return upload(dst, tmp.data(), n * 2);
}

// One device matrix (bf16, or int8 + per-row f32 scales) from a host pointer pair.
static int upload_mat(uint8_t** dst, float** dscale, const void* src, const float* scale, size_t rows,
                      size_t cols) {
    const size_t esz = scale ? 1 : 2;
    CK(dalloc(dst, rows * cols * esz));
    if (upload(*dst, src, rows * cols * esz)) return -1;
    *dscale = nullptr;
    if (scale) {
        CK(dalloc(dscale, rows));
        if (upload(*dscale, scale, rows * 4)) return -1;
    }
    return 0;
}

// merged Q|K|V rows (voxtral_metal.m merged_3 warmup); all three bf16 or all three Q8
static int upload_qkv(uint8_t** dst, float** dscale, const void* wq, const float* sq, const void* wk,
                      const float* sk, const void* wv, const float* sv, int nq, int nkv, int K) {
    if (!sq != !sk || !sq != !sv) return set_err("wq/wk/wv mix bf16 and Q8");
    const size_t esz = sq ? 1 : 2, rows = (size_t)nq + 2 * nkv;
    CK(dalloc(dst, rows * K * esz));
    if (upload(*dst, wq, (size_t)nq * K * esz) || upload(*dst + (size_t)nq * K * esz, wk, (size_t)nkv * K * esz) ||
        upload(*dst + (size_t)(nq + nkv) * K * esz, wv, (size_t)nkv * K * esz))
        return -1;
    *dscale = nullptr;
    if (sq) {
        CK(dalloc(dscale, rows));
        if (upload(*dscale, sq, (size_t)nq * 4) || upload(*dscale + nq, sk, (size_t)nkv * 4) ||
            upload(*dscale + nq + nkv, sv, (size_t)nkv * 4))
            return -1;
    }
    return 0;
}

// rows 32g..32g+15 <- w1 rows 16g..16g+15, rows 32g+16..32g+31 <- w3 rows 16g..
// (Q8: the row scales are interleaved the same way)
static int upload_w13(uint8_t** dst, float** dscale, const void* w1, const float* s1, const void* w3,
                      const float* s3, int hidden, int K) {
    if (!w1 || !w3) return set_err("null w1/w3");
    if (!s1 != !s3) return set_err("w1/w3 mix bf16 and Q8");
    if (hidden % 16) return set_err("hidden %d not a multiple of 16", hidden);
    const size_t esz = s1 ? 1 : 2;
    CK(dalloc(dst, (size_t)2 * hidden * K * esz));
    size_t grp = (size_t)16 * K * esz;
    CK(hipMemcpy2D(*dst, 2 * grp, w1, grp, grp, hidden / 16, hipMemcpyHostToDevice));
    CK(hipMemcpy2D(*dst + grp, 2 * grp, w3, grp, grp, hidden / 16, hipMemcpyHostToDevice));
    *dscale = nullptr;
    if (s1) {
        CK(dalloc(dscale, (size_t)2 * hidden));
        const size_t g4 = 16 * 4;
        CK(hipMemcpy2D(*dscale, 2 * g4, s1, g4, g4, hidden / 16, hipMemcpyHostToDevice));
        CK(hipMemcpy2D((char*)*dscale + g4, 2 * g4, s3, g4, g4, hidden / 16, hipMemcpyHostToDevice));
    }
    return 0;
}

// f(lo, hi) over [0, n) on up to 16 host threads
template <class F>
static void par_range(long long n, F f) {
    const long long nt = std::max(1LL, std::min<long long>({16, (long long)std::thread::hardware_concurrency(), n}));
    std::vector<std::thread> th;
    for (long long t = 1; t < nt; t++) th.emplace_back([=] { f(n * t / nt, n * (t + 1) / nt); });
    f(0, n / nt);
    for (auto& t : th) t.join();
}

// The wpack13 planes of a bf16 matrix whose rows are in device order (host copy), for
// k_gemv's row groups of this shape.  A tensor outside the format's window (vox_wpack.h),
// or of a shape launch_gemv does not take, stays raw: P->main stays null.
static int wpack_make(int enabled, vox_hip_wpack_stats_t& S, WPackD* P, const uint16_t* w, int rows, int K, int swiglu) {
    P->main = P->side = nullptr;
    P->d = 0;
    const size_t n = (size_t)rows * K;
    auto raw = [&] { S.raw_tensors++; S.raw_bytes += (long long)n * 2; return 0; };
    if (!w) return set_err("null weight pointer");
    if (!enabled || !gemv_ok(rows, K, 0)) return raw();
    const auto t0 = std::chrono::steady_clock::now();
    int lo = 256, hi = -1, bad = 0;
    std::mutex mu;
    par_range(rows, [&](long long r0, long long r1) {
        int l = 256, h = -1, b = 0;
        vox_wpack13_scan_range(w + r0 * K, (size_t)(r1 - r0) * K, &l, &h, &b);
        std::lock_guard<std::mutex> g(mu);
        lo = std::min(lo, l); hi = std::max(hi, h); bad |= b;
    });
    int d;
    if (!vox_wpack13_choose(lo, hi, bad, &d)) return raw();
    const int rb = gemv_rowgroup(rows), sw = vox_wpack13_side_words(K, rb);
    const size_t mainw = n / 8 * 3, sidew = (size_t)rows / rb * 256 * sw;
    std::vector<uint32_t> hm(mainw), hs(sidew);
    std::vector<uint8_t> hb(n / 8);
    par_range(rows, [&](long long r0, long long r1) { vox_wpack13_pack_rows(w, r0, r1, K, d, hm.data(), hb.data()); });
    par_range(rows / rb, [&](long long g0, long long g1) { vox_wpack13_side_groups(hb.data(), g0, g1, K, rb, swiglu, hs.data()); });
    CK(dalloc(&P->main, mainw * 4));
    CK(dalloc(&P->side, sidew * 4));
    if (upload(P->main, hm.data(), mainw * 4) || upload(P->side, hs.data(), sidew * 4)) return -1;
    P->d = d;
    S.packed_tensors++;
    S.packed_bytes += (long long)(mainw + sidew) * 4;
    S.packed_raw_bytes += (long long)n * 2;
    S.pack_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}
static void wpack_args(GemvArgs& a, const WPackD& P) {
    a.wp_main = P.main;
    a.wp_side = P.side;
    a.wp_d = P.d;
}

// wmx4 mode of models created from now on (include/voxtral_hip.h); VOX_HIP_WMX4 gives the
// initial value
static int g_wmx4 = -1;
static int wmx4_mode() {
    if (g_wmx4 < 0) {
        const char* e = getenv("VOX_HIP_WMX4");
        const int v = e ? atoi(e) : 0;
        g_wmx4 = v == 1 || v == 2 ? v : 0;
    }
    return g_wmx4;
}
extern "C" int vox_hip_set_wmx4(int mode) {
    if (mode < 0 || mode > 2) return set_err("wmx4 mode: 0, 1 or 2 (got %d)", mode);
    g_wmx4 = mode;
    return 0;
}
extern "C" int vox_hip_wmx4(void) { return wmx4_mode(); }
// wmx4 fragment planes for the batched step, for models created from now on;
// VOX_HIP_WMX4_BATCH gives the initial value
static int g_wmx4_batch = -1;
static int wmx4_batch_mode() {
    if (g_wmx4_batch < 0) {
        const char* e = getenv("VOX_HIP_WMX4_BATCH");
        g_wmx4_batch = e && atoi(e) == 1 ? 1 : 0;
    }
    return g_wmx4_batch;
}
extern "C" int vox_hip_set_wmx4_batch(int on) {
    g_wmx4_batch = on ? 1 : 0;
    return 0;
}
extern "C" int vox_hip_wmx4_batch(void) { return wmx4_batch_mode(); }
// k_gemmf over the int8 fragment copies of Q8 tensors, for models created from now on
// (include/voxtral_hip.h); VOX_HIP_GEMMF_Q8=1 gives the initial value
static int g_gemmf_q8 = -1;
static int gemmf_q8_mode() {
    if (g_gemmf_q8 < 0) {
        const char* e = getenv("VOX_HIP_GEMMF_Q8");
        g_gemmf_q8 = e && atoi(e) == 1 ? 1 : 0;
    }
    return g_gemmf_q8;
}
extern "C" int vox_hip_set_gemmf_q8(int on) {
    g_gemmf_q8 = on ? 1 : 0;
    return 0;
}
extern "C" int vox_hip_gemmf_q8(void) { return gemmf_q8_mode(); }
// first capacity (rows) of the adapter buffer of streams created from now on; it doubles from
// there (include/voxtral_hip.h).  Host state only: no device call.
static const int ADAPTER_ROWS0 = 1024;
static int g_adapter_rows0 = ADAPTER_ROWS0;
extern "C" int vox_hip_set_adapter_rows0(int rows) {
    if (rows == 0) rows = ADAPTER_ROWS0;
    if (rows < 16 || rows > ADAPTER_ROWS0 || (rows & (rows - 1)))
        return set_err("adapter rows0: 0 (the default of %d) or a power of two in 16..%d (got %d)", ADAPTER_ROWS0,
                       ADAPTER_ROWS0, rows);
    g_adapter_rows0 = rows;
    return 0;
}

// smallest first capacity of a growing decoder ring (vox_hip_model_set_kv_grow): the ring's
// slack, which holds the longest prompt (32 + 30 rows); the full ring is the window plus it
static const int KV_GROW_MIN = 64;

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Mode 2: the MXFP4 rounding of a host bf16 matrix (vox_wmx4_round), into `out`
static void wmx4_round_host(vox_hip_wmx4_stats_t& S, const void* w, int rows, int K, std::vector<uint16_t>& out) {
    const auto t0 = std::chrono::steady_clock::now();
    out.resize((size_t)rows * K);
    const uint16_t* in = (const uint16_t*)w;
    par_range(rows, [&](long long r0, long long r1) { vox_wmx4_round_rows(in, r0, r1, K, out.data()); });
    S.round_ms += ms_since(t0);
}

// The wmx4 plane of a bf16 matrix whose rows are in device order (host copy), for the wmx4
// row groups of this shape.  A tensor that fails vox_wmx4_scan, or of a shape the wmx4
// instances do not take, gets none: M->plane stays null and the tensor streams as before.
// fstats != null (and rows % 16 == 0, K % 64 == 0): the tensor's fragment plane for the batched
// step as well, from the same nibbles and scales.
static int wmx4_make(int enabled, vox_hip_wmx4_stats_t& S, WMx4D* M, const uint16_t* w, int rows, int K, int swiglu,
                     long long* fstats = nullptr) {
    M->plane = M->frag = nullptr;
    if (!enabled) return 0;
    if (!w) return set_err("null weight pointer");
    const size_t n = (size_t)rows * K;
    auto t0 = std::chrono::steady_clock::now();
    std::atomic<int> ok{gemv_ok_mx4(rows, K) ? 1 : 0};
    if (ok) {
        // every thread starts at the head of its range and stops at its first failing block
        par_range(rows, [&](long long r0, long long r1) {
            for (long long r = r0; r < r1 && ok.load(std::memory_order_relaxed); r++)
                if (!vox_wmx4_scan_rows(w, r, r + 1, K)) ok = 0;
        });
    }
    S.scan_ms += ms_since(t0);
    if (!ok) {
        S.refused_tensors++;
        return 0;
    }
    t0 = std::chrono::steady_clock::now();
    const int rb = gemv_rowgroup_mx4(rows);
    const size_t words = (size_t)vox_wmx4_plane_words(rows, K, rb);
    std::vector<uint32_t> nib(n / 8), plane(words);
    std::vector<uint8_t> scl(n / VOX_WMX4_BLOCK);
    par_range(rows, [&](long long r0, long long r1) { vox_wmx4_pack_rows(w, r0, r1, K, nib.data(), scl.data()); });
    par_range(rows / rb, [&](long long g0, long long g1) {
        vox_wmx4_plane_groups(nib.data(), scl.data(), g0, g1, K, rb, swiglu, plane.data());
    });
    CK(dalloc(&M->plane, words * 4));
    if (upload(M->plane, plane.data(), words * 4)) return -1;
    S.wmx4_tensors++;
    S.plane_bytes += (long long)words * 4;
    S.bf16_bytes += (long long)n * 2;
    S.bits_per_weight = S.plane_bytes * 8.0 / (S.bf16_bytes / 2);
    S.pack_ms += ms_since(t0);
    const size_t fwords = fstats ? (size_t)vox_wmx4_frag_words(rows, K) : 0;
    if (fwords) {
        t0 = std::chrono::steady_clock::now();
        std::vector<uint32_t>().swap(plane);
        std::vector<uint32_t> fp(fwords);
        par_range(rows / 16, [&](long long g0, long long g1) { vox_wmx4_frag_groups(nib.data(), scl.data(), g0, g1, K, fp.data()); });
        CK(dalloc(&M->frag, fwords * 4));
        if (upload(M->frag, fp.data(), fwords * 4)) return -1;
        fstats[0]++;
        fstats[1] += (long long)fwords * 4;
        fstats[2] += (long long)n * 2;
        fstats[3] += (long long)(ms_since(t0) * 1000.0);
    }
    return 0;
}
// (VOX_HIP_WPACK=0 streams raw rows everywhere: such a model builds no plane)
static void wmx4_args(GemvArgs& a, const WMx4D& M) { a.wm_plane = M.plane; }
// blocks of the single-stream LM head launch (its argmax partials)
static int lm_head_grid(const vox_hip_model* m) {
    return m->mlm.plane ? gemv_grid_mx4(m->c.vocab) : gemv_grid(m->c.vocab);
}

// the ada table [dec_layers][dec_dim] of a delay: vox_update_time_conditioning (voxtral.c:31-80)
static void model_ada_host(const vox_hip_model_t* m, int delay_tokens, std::vector<float>& out) {
    const vox_hip_config_t& c = m->c;
    int D = c.dec_dim, A = c.ada_dim;
    std::vector<float> t_cond(D), hidden(A);
    int half = D / 2;
    float log_theta = logf(10000.0f);
    float t = (float)delay_tokens;
    for (int i = 0; i < half; i++) {
        float inv_freq = expf(-log_theta * (float)i / (float)half);
        float emb = t * inv_freq;
        t_cond[i] = cosf(emb);
        t_cond[i + half] = sinf(emb);
    }
    out.assign((size_t)c.dec_layers * D, 0.f);
    for (int l = 0; l < c.dec_layers; l++) {
        const float* down = m->ada_down[l].data();
        const float* up = m->ada_up[l].data();
        for (int i = 0; i < A; i++) {
            float sum = 0.f;
            for (int j = 0; j < D; j++) sum += down[(size_t)i * D + j] * t_cond[j];
            hidden[i] = host_gelu(sum, c.gelu_erf);
        }
        float* sc = out.data() + (size_t)l * D;
        for (int i = 0; i < D; i++) {
            float sum = 0.f;
            for (int j = 0; j < A; j++) sum += up[(size_t)i * A + j] * hidden[j];
            sc[i] = sum;
        }
    }
}

static int model_update_ada(vox_hip_model_t* m) {
    model_ada_host(m, m->delay_tokens, m->ada_host);
    CK(h2d(m->ada_scale, m->ada_host.data(), m->ada_host.size() * 4));
    return 0;
}

// the model's table of delay d (0 .. VOX_HIP_MAX_DELAY_TOKENS), made on first use
static int model_ada_table(vox_hip_model_t* m, int d) {
    if (d < 0 || d > VOX_HIP_MAX_DELAY_TOKENS) return set_err("delay of %d tokens is not 0..%d", d, VOX_HIP_MAX_DELAY_TOKENS);
    if (m->ada_tab[d]) return 0;
    model_ada_host(m, d, m->ada_tab_host[d]);
    float* t = nullptr;
    CK(dalloc(&t, m->ada_tab_host[d].size()));
    if (hipError_t e = h2d(t, m->ada_tab_host[d].data(), m->ada_tab_host[d].size() * 4); e != hipSuccess) {
        dfree(t);
        return set_err("ada table upload: %s", hipGetErrorString(e));
    }
    m->ada_tab[d] = t;
    return 0;
}

static int model_rope_tables(vox_hip_model_t* m, int positions) {
    const vox_hip_config_t& c = m->c;
    dfree(m->rope_enc);
    dfree(m->rope_dec);
    std::vector<float> t((size_t)positions * std::max(c.enc_head_dim, c.dec_head_dim));
    CK(dalloc(&m->rope_enc, (size_t)positions * c.enc_head_dim));
    host_rope(t.data(), 0, positions, c.enc_head_dim, c.rope_theta);
    CK(h2d(m->rope_enc, t.data(), (size_t)positions * c.enc_head_dim * 4));
    CK(dalloc(&m->rope_dec, (size_t)positions * c.dec_head_dim));
    host_rope(t.data(), 0, positions, c.dec_head_dim, c.rope_theta);
    CK(h2d(m->rope_dec, t.data(), (size_t)positions * c.dec_head_dim * 4));
    m->rope_positions = positions;
    m->rope_gen++;
    return 0;
}

static int check_config(const vox_hip_config_t* c) {
    if (c->enc_head_dim != 64 && c->enc_head_dim != 128) return set_err("enc_head_dim must be 64/128");
    if (c->dec_head_dim != 64 && c->dec_head_dim != 128) return set_err("dec_head_dim must be 64/128");
    if (c->enc_heads % c->enc_kv_heads || c->dec_heads % c->dec_kv_heads)
        return set_err("heads must be a multiple of kv heads");
    if (c->dec_heads / c->dec_kv_heads > 4 || c->enc_heads / c->enc_kv_heads > 4)
        return set_err("GQA ratio > 4 unsupported");
    int dims[] = {c->enc_dim, c->enc_hidden, c->dec_dim, c->dec_hidden,
                  c->enc_heads * c->enc_head_dim, c->dec_heads * c->dec_head_dim,
                  c->dec_kv_heads * c->dec_head_dim, c->mel_bins * 3};
    for (int d : dims)
        if (d % 64) return set_err("dimension %d not a multiple of 64", d);
    if (c->vocab % 2) return set_err("vocab must be even");
    if (c->downsample != 4) return set_err("downsample must be 4");
    return 0;
}

extern "C" void vox_hip_model_free(vox_hip_model_t* m);

extern "C" vox_hip_model_t* vox_hip_model_create(const vox_hip_config_t* cfg,
                                                 const vox_hip_weights_t* w, int delay_tokens) {
    if (!g_inited && !vox_hip_init()) return nullptr;
    if (check_config(cfg)) return nullptr;
    vox_hip_model_t* m = new vox_hip_model_t();
    memset(&m->c, 0, sizeof m->c);
    m->c = *cfg;
    m->delay_tokens = delay_tokens;
    {
        // the reference's VOX_DECODER_KV_FP16 (voxtral.c:189-190); opt-in here (unset = f32,
        // the CPU reference's cache), vox_hip_model_set_kv_fp16 overrides
        const char* e = getenv("VOX_DECODER_KV_FP16");
        m->kvt = (e && atoi(e) != 0 && cfg->dec_head_dim == 128) ? KV_F16 : KV_F32;
        // the one-byte rings (FP8 E4M3, vox_kv8.h): opt-in, before the 16-bit variable when both
        // are set, head_dim 128 only like it; vox_hip_model_set_kv_dtype overrides
        const char* e8 = getenv("VOX_HIP_KV_FP8");
        if (e8 && atoi(e8) != 0 && cfg->dec_head_dim == 128) m->kvt = KV_FP8;
        // the encoder's rings (no reference counterpart: VOX_DECODER_KV_FP16 is decoder-only):
        // IEEE half when VOX_HIP_ENC_KV_FP16 is set nonzero, head_dim 64 only;
        // vox_hip_model_set_enc_kv_fp16 overrides
        const char* ee = getenv("VOX_HIP_ENC_KV_FP16");
        m->ekvt = (ee && atoi(ee) != 0 && cfg->enc_head_dim == 64) ? KV_F16 : KV_F32;
        // one-byte encoder rings (FP8 E4M3, vox_kv8.h) when VOX_HIP_ENC_KV_FP8 is set nonzero: before
        // the 16-bit variable when both are set, head_dim 64 only; vox_hip_model_set_enc_kv_dtype overrides
        const char* ee8 = getenv("VOX_HIP_ENC_KV_FP8");
        if (ee8 && atoi(ee8) != 0 && cfg->enc_head_dim == 64) m->ekvt = KV_FP8;
        // decoder rings that start at VOX_HIP_KV_GROW slots and grow with the stream's position
        // (unset or 0: the full ring from the start); vox_hip_model_set_kv_grow overrides
        const char* eg = getenv("VOX_HIP_KV_GROW");
        m->kv_grow = 0;
        if (eg && atoi(eg) > 0) m->kv_grow = std::min(std::max(atoi(eg), KV_GROW_MIN), cfg->dec_window + KV_GROW_MIN);
    }
    m->conv0_w = m->conv1_w = nullptr;
    m->ad0 = m->ad1 = m->tok_emb = nullptr;
    m->ad0_s = m->ad1_s = m->tok_emb_s = nullptr;
    m->conv0_b = m->conv1_b = m->enc_norm = m->dec_norm = m->ada_scale = nullptr;
    for (float*& t : m->ada_tab) t = nullptr;
    m->rope_enc = m->rope_dec = nullptr;
    memset(&m->plm, 0, sizeof m->plm);
    memset(&m->wstats, 0, sizeof m->wstats);
    memset(&m->mlm, 0, sizeof m->mlm);
    memset(&m->mstats, 0, sizeof m->mstats);
    m->wmx4 = wmx4_mode();
    m->wmx4_batch = m->wmx4 ? wmx4_batch_mode() : 0;
    memset(m->fstats, 0, sizeof m->fstats);
    m->gemmf_q8 = gemmf_q8_mode();
    m->n_gemmf_q8 = 0;
    long long* const fst = m->wmx4_batch ? m->fstats : nullptr;
    {
        // VOX_HIP_WPACK=0: every GEMV weight stays raw bf16 (same-machine A/B runs)
        const char* e = getenv("VOX_HIP_WPACK");
        m->wpack = (e && atoi(e) == 0) ? 0 : 1;
    }
    const vox_hip_config_t& c = *cfg;
    const int ED = c.enc_dim, EQ = c.enc_heads * c.enc_head_dim, EKV = c.enc_kv_heads * c.enc_head_dim;
    const int EH = c.enc_hidden;
    const int DD = c.dec_dim, DQ = c.dec_heads * c.dec_head_dim, DKV = c.dec_kv_heads * c.dec_head_dim;
    const int DH = c.dec_hidden;
    auto fail = [&]() -> vox_hip_model_t* { vox_hip_model_free(m); return nullptr; };
#define TRY(x) do { if ((x) != 0) return fail(); } while (0)
#define TRYH(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { set_err("%s: %s", #x, hipGetErrorString(e__)); return fail(); } } while (0)
#define SCL(field, l) (w->field ? w->field[l] : nullptr)
    // conv stem
    TRYH(dalloc(&m->conv0_w, (size_t)ED * c.mel_bins * 3));
    TRY(upload_f32_as_bf16(m->conv0_w, w->conv0_w, (size_t)ED * c.mel_bins * 3));
    TRYH(dalloc(&m->conv1_w, (size_t)ED * ED * 3));
    TRY(upload_f32_as_bf16(m->conv1_w, w->conv1_w, (size_t)ED * ED * 3));
    TRYH(dalloc(&m->conv0_b, ED));
    TRY(upload(m->conv0_b, w->conv0_b, ED * 4));
    TRYH(dalloc(&m->conv1_b, ED));
    TRY(upload(m->conv1_b, w->conv1_b, ED * 4));
    // encoder layers
    m->enc.resize(c.enc_layers);
    for (int l = 0; l < c.enc_layers; l++) {
        EncLayerD& L = m->enc[l];
        memset(&L, 0, sizeof L);
        TRY(upload_qkv(&L.wqkv, &L.sqkv, w->enc_wq[l], SCL(enc_wq_s, l), w->enc_wk[l], SCL(enc_wk_s, l),
                       w->enc_wv[l], SCL(enc_wv_s, l), EQ, EKV, ED));
        TRYH(dalloc(&L.bqkv, EQ + 2 * EKV));  // k part stays zero: wk has no bias
        TRY(upload(L.bqkv, w->enc_wq_b[l], EQ * 4));
        TRY(upload(L.bqkv + EQ + EKV, w->enc_wv_b[l], EKV * 4));
        TRY(upload_mat(&L.wo, &L.so, w->enc_wo[l], SCL(enc_wo_s, l), ED, EQ));
        TRYH(dalloc(&L.bo, ED));
        TRY(upload(L.bo, w->enc_wo_b[l], ED * 4));
        TRY(upload_w13(&L.w13, &L.s13, w->enc_w1[l], SCL(enc_w1_s, l), w->enc_w3[l], SCL(enc_w3_s, l), EH, ED));
        TRY(upload_mat(&L.w2, &L.s2, w->enc_w2[l], SCL(enc_w2_s, l), ED, EH));
        TRYH(dalloc(&L.b2, ED));
        TRY(upload(L.b2, w->enc_w2_b[l], ED * 4));
        TRYH(dalloc(&L.attn_norm, ED));
        TRY(upload(L.attn_norm, w->enc_attn_norm[l], ED * 4));
        TRYH(dalloc(&L.ffn_norm, ED));
        TRY(upload(L.ffn_norm, w->enc_ffn_norm[l], ED * 4));
    }
    TRYH(dalloc(&m->enc_norm, ED));
    TRY(upload(m->enc_norm, w->enc_norm, ED * 4));
    // adapter
    TRY(upload_mat(&m->ad0, &m->ad0_s, w->ad0, w->ad0_s, DD, (size_t)ED * c.downsample));
    TRY(upload_mat(&m->ad1, &m->ad1_s, w->ad1, w->ad1_s, DD, DD));
    // decoder
    // wmx4 mode 2: the bf16 matrices of the decode step are rounded to MXFP4 values here, on
    // the host, before anything is uploaded: raw rows, fragment-major copies, wpack13 and wmx4
    // planes all hold the one rounded model (Q8 tensors are left alone)
    std::vector<uint16_t> rnd[7];
    auto rounded = [&](int slot, const void* src, const float* scale, int rows, int K) -> const void* {
        if (m->wmx4 != 2 || scale || !src) return src;
        wmx4_round_host(m->mstats, src, rows, K, rnd[slot]);
        return rnd[slot].data();
    };
    const void* h_tok = rounded(0, w->tok_emb, w->tok_emb_s, c.vocab, DD);
    TRY(upload_mat(&m->tok_emb, &m->tok_emb_s, h_tok, w->tok_emb_s, c.vocab, DD));
    // wpack13 copies of the bf16 matrices the single-stream decode step streams (made here,
    // not in the first step); the raw copies stay for every other path
    if (!w->tok_emb_s) {
        TRY(wpack_make(m->wpack, m->wstats, &m->plm, (const uint16_t*)h_tok, c.vocab, DD, 0));
        TRY(wmx4_make(m->wmx4 && m->wpack, m->mstats, &m->mlm, (const uint16_t*)h_tok, c.vocab, DD, 0, fst));
    }
    rnd[0] = std::vector<uint16_t>();
    std::vector<uint16_t> hrows;  // a matrix in device row order (merged Q|K|V, interleaved W1|W3)
    m->dec.resize(c.dec_layers);
    m->ada_down.resize(c.dec_layers);
    m->ada_up.resize(c.dec_layers);
    for (int l = 0; l < c.dec_layers; l++) {
        DecLayerD& L = m->dec[l];
        memset(&L, 0, sizeof L);
        // blocks lie within a row, so rounding wq, wk, wv (w1, w3) one by one rounds Q|K|V (W1|W3)
        const void* h_wq = rounded(0, w->dec_wq[l], SCL(dec_wq_s, l), DQ, DD);
        const void* h_wk = rounded(1, w->dec_wk[l], SCL(dec_wk_s, l), DKV, DD);
        const void* h_wv = rounded(2, w->dec_wv[l], SCL(dec_wv_s, l), DKV, DD);
        const void* h_wo = rounded(3, w->dec_wo[l], SCL(dec_wo_s, l), DD, DQ);
        const void* h_w1 = rounded(4, w->dec_w1[l], SCL(dec_w1_s, l), DH, DD);
        const void* h_w3 = rounded(5, w->dec_w3[l], SCL(dec_w3_s, l), DH, DD);
        const void* h_w2 = rounded(6, w->dec_w2[l], SCL(dec_w2_s, l), DD, DH);
        TRY(upload_qkv(&L.wqkv, &L.sqkv, h_wq, SCL(dec_wq_s, l), h_wk, SCL(dec_wk_s, l), h_wv, SCL(dec_wv_s, l), DQ,
                       DKV, DD));
        TRY(upload_mat(&L.wo, &L.so, h_wo, SCL(dec_wo_s, l), DD, DQ));
        TRY(upload_w13(&L.w13, &L.s13, h_w1, SCL(dec_w1_s, l), h_w3, SCL(dec_w3_s, l), DH, DD));
        TRY(upload_mat(&L.w2, &L.s2, h_w2, SCL(dec_w2_s, l), DD, DH));
        if (!L.sqkv) {
            hrows.resize((size_t)(DQ + 2 * DKV) * DD);
            memcpy(hrows.data(), h_wq, (size_t)DQ * DD * 2);
            memcpy(hrows.data() + (size_t)DQ * DD, h_wk, (size_t)DKV * DD * 2);
            memcpy(hrows.data() + (size_t)(DQ + DKV) * DD, h_wv, (size_t)DKV * DD * 2);
            TRY(wpack_make(m->wpack, m->wstats, &L.pqkv, hrows.data(), DQ + 2 * DKV, DD, 0));
            TRY(wmx4_make(m->wmx4 && m->wpack, m->mstats, &L.mqkv, hrows.data(), DQ + 2 * DKV, DD, 0, fst));
        }
        if (!L.so) {
            TRY(wpack_make(m->wpack, m->wstats, &L.po, (const uint16_t*)h_wo, DD, DQ, 0));
            TRY(wmx4_make(m->wmx4 && m->wpack, m->mstats, &L.mo, (const uint16_t*)h_wo, DD, DQ, 0, fst));
        }
        if (!L.s13) {
            hrows.resize((size_t)2 * DH * DD);
            const size_t grp = (size_t)16 * DD;
            for (int g = 0; g < DH / 16; g++) {
                memcpy(hrows.data() + 2 * g * grp, (const uint16_t*)h_w1 + g * grp, grp * 2);
                memcpy(hrows.data() + (2 * g + 1) * grp, (const uint16_t*)h_w3 + g * grp, grp * 2);
            }
            TRY(wpack_make(m->wpack, m->wstats, &L.p13, hrows.data(), 2 * DH, DD, 1));
            TRY(wmx4_make(m->wmx4 && m->wpack, m->mstats, &L.m13, hrows.data(), 2 * DH, DD, 1, fst));
        }
        if (!L.s2) {
            TRY(wpack_make(m->wpack, m->wstats, &L.p2, (const uint16_t*)h_w2, DD, DH, 0));
            TRY(wmx4_make(m->wmx4 && m->wpack, m->mstats, &L.m2, (const uint16_t*)h_w2, DD, DH, 0, fst));
        }
        TRYH(dalloc(&L.attn_norm, DD));
        TRY(upload(L.attn_norm, w->dec_attn_norm[l], DD * 4));
        TRYH(dalloc(&L.ffn_norm, DD));
        TRY(upload(L.ffn_norm, w->dec_ffn_norm[l], DD * 4));
        if (!w->dec_ada_down[l] || !w->dec_ada_up[l]) { set_err("null ada weights"); return fail(); }
        m->ada_down[l].assign(w->dec_ada_down[l], w->dec_ada_down[l] + (size_t)c.ada_dim * DD);
        m->ada_up[l].assign(w->dec_ada_up[l], w->dec_ada_up[l] + (size_t)DD * c.ada_dim);
    }
    TRYH(dalloc(&m->dec_norm, DD));
    TRY(upload(m->dec_norm, w->dec_norm, DD * 4));
    TRYH(dalloc(&m->ada_scale, (size_t)c.dec_layers * DD));
    TRY(model_update_ada(m));
    TRY(model_rope_tables(m, 32768));
#undef TRY
#undef TRYH
#undef SCL
    return m;
}

extern "C" void vox_hip_model_free(vox_hip_model_t* m) {
    if (!m) return;
    dfree(m->conv0_w); dfree(m->conv1_w); dfree(m->conv0_b); dfree(m->conv1_b);
    for (auto& L : m->enc) {
        dfree(L.wqkv); dfree(L.wo); dfree(L.w13); dfree(L.w2);
        dfree(L.sqkv); dfree(L.so); dfree(L.s13); dfree(L.s2);
        dfree(L.bqkv); dfree(L.bo); dfree(L.b2); dfree(L.attn_norm); dfree(L.ffn_norm);
    }
    for (auto& L : m->dec) {
        dfree(L.wqkv); dfree(L.wo); dfree(L.w13); dfree(L.w2);
        dfree(L.sqkv); dfree(L.so); dfree(L.s13); dfree(L.s2);
        dfree(L.attn_norm); dfree(L.ffn_norm);
        for (WPackD* P : {&L.pqkv, &L.po, &L.p13, &L.p2}) { dfree(P->main); dfree(P->side); }
        for (WMx4D* M : {&L.mqkv, &L.mo, &L.m13, &L.m2}) { dfree(M->plane); dfree(M->frag); }
    }
    dfree(m->plm.main); dfree(m->plm.side); dfree(m->mlm.plane); dfree(m->mlm.frag);
    for (auto& F : m->dfrag) {
        dfree(F.wqkv); dfree(F.wo); dfree(F.w13); dfree(F.w2);
    }
    for (auto& F : m->efrag) {
        dfree(F.wqkv); dfree(F.wo); dfree(F.w13); dfree(F.w2);
    }
    dfree(m->lm_frag);
    dfree(m->enc_norm); dfree(m->ad0); dfree(m->ad1); dfree(m->tok_emb); dfree(m->dec_norm);
    dfree(m->ad0_s); dfree(m->ad1_s); dfree(m->tok_emb_s);
    dfree(m->ada_scale); dfree(m->rope_enc); dfree(m->rope_dec);
    for (float* t : m->ada_tab) dfree(t);
    delete m;
}

extern "C" int vox_hip_model_wpack_stats(const vox_hip_model_t* m, vox_hip_wpack_stats_t* out) {
    if (!m || !out) return set_err("wpack_stats: null argument");
    *out = m->wstats;
    return 0;
}

extern "C" int vox_hip_model_wmx4_stats(const vox_hip_model_t* m, vox_hip_wmx4_stats_t* out) {
    if (!m || !out) return set_err("wmx4_stats: null argument");
    *out = m->mstats;
    return 0;
}

extern "C" int vox_hip_model_wmx4_batch_stats(const vox_hip_model_t* m, long long out4[4]) {
    if (!m || !out4) return set_err("wmx4_batch_stats: null argument");
    memcpy(out4, m->fstats, sizeof m->fstats);
    return 0;
}

// [0] the switch the model took, [1] k_gemmf launches on int8 fragments, [2] / [3] Q8 matrices
// (merged Q|K|V and W1|W3 count once each, the LM head once) whose shape k_gemmf takes / refuses
extern "C" int vox_hip_model_gemmf_q8_stats(const vox_hip_model_t* m, long long out4[4]) {
    if (!m || !out4) return set_err("gemmf_q8_stats: null argument");
    const vox_hip_config_t& c = m->c;
    const int ED = c.enc_dim, EQ = c.enc_heads * c.enc_head_dim, EKV = c.enc_kv_heads * c.enc_head_dim;
    const int DD = c.dec_dim, DQ = c.dec_heads * c.dec_head_dim, DKV = c.dec_kv_heads * c.dec_head_dim;
    long long ok = 0, no = 0;
    auto tensor = [&](const float* scale, int N, int K) {
        if (scale) (gemmf_ok(1, N, K) ? ok : no)++;
    };
    for (const EncLayerD& L : m->enc) {
        tensor(L.sqkv, EQ + 2 * EKV, ED);
        tensor(L.so, ED, EQ);
        tensor(L.s13, 2 * c.enc_hidden, ED);
        tensor(L.s2, ED, c.enc_hidden);
    }
    for (const DecLayerD& L : m->dec) {
        tensor(L.sqkv, DQ + 2 * DKV, DD);
        tensor(L.so, DD, DQ);
        tensor(L.s13, 2 * c.dec_hidden, DD);
        tensor(L.s2, DD, c.dec_hidden);
    }
    tensor(m->tok_emb_s, c.vocab, DD);
    out4[0] = m->gemmf_q8;
    out4[1] = m->n_gemmf_q8;
    out4[2] = ok;
    out4[3] = no;
    return 0;
}

extern "C" int vox_hip_model_set_delay(vox_hip_model_t* m, int delay_tokens) {
    // the slots of a begun call read the model's ada table on every step
    if (m->begun_calls > 0) return set_err("model_set_delay: a begun call of this model was not finished");
    m->delay_tokens = delay_tokens;
    return model_update_ada(m);
}

extern "C" int vox_hip_set_gemm_planes(int planes) {
    if (set_gemm_planes(planes)) return set_err("gemm planes: 2 or 3 (got %d)", planes);
    return 0;
}

extern "C" int vox_hip_gemm_planes(void) { return gemm_planes_np(); }
extern "C" int vox_hip_set_gemmf_wait(int ticks) { return set_gemmf_wait(ticks); }

extern "C" int vox_hip_model_set_kv_fp16(vox_hip_model_t* m, int on) {
    if (on && m->c.dec_head_dim != 128) return set_err("16-bit decoder KV: head_dim 128 only (got %d)", m->c.dec_head_dim);
    m->kvt = on ? KV_F16 : KV_F32;
    return 0;
}

extern "C" int vox_hip_model_set_kv_dtype(vox_hip_model_t* m, int dtype) {
    if (dtype < KV_F32 || dtype > KV_FP8) return set_err("decoder KV element type: 0 (f32), 1 (half) or 2 (fp8), got %d", dtype);
    if (dtype != KV_F32 && m->c.dec_head_dim != 128)
        return set_err("%s decoder KV: head_dim 128 only (got %d)", dtype == KV_FP8 ? "FP8" : "16-bit", m->c.dec_head_dim);
    m->kvt = dtype;
    return 0;
}

extern "C" int vox_hip_model_set_enc_kv_fp16(vox_hip_model_t* m, int on) {
    if (!m) return set_err("model_set_enc_kv_fp16: null model");
    if (on && m->c.enc_head_dim != 64) return set_err("16-bit encoder KV: head_dim 64 only (got %d)", m->c.enc_head_dim);
    m->ekvt = on ? KV_F16 : KV_F32;
    return 0;
}

extern "C" int vox_hip_model_set_enc_kv_dtype(vox_hip_model_t* m, int dtype) {
    if (!m) return set_err("model_set_enc_kv_dtype: null model");
    if (dtype < KV_F32 || dtype > KV_FP8) return set_err("encoder KV element type: 0 (f32), 1 (half) or 2 (fp8), got %d", dtype);
    if (dtype != KV_F32 && m->c.enc_head_dim != 64)
        return set_err("%s encoder KV: head_dim 64 only (got %d)", dtype == KV_FP8 ? "FP8" : "16-bit", m->c.enc_head_dim);
    m->ekvt = dtype;
    return 0;
}

extern "C" int vox_hip_stream_kv_fp16(const vox_hip_stream_t* s);

// Streams created afterwards start with decoder rings of slots0 slots (clamped to [64, window +
// 64]: 64 holds the longest prompt, 32 + 30 rows) that double as the stream's position needs
// them, up to the full window + 64 (stream_grow_dec).  0: the full ring from the start (default).
extern "C" int vox_hip_model_set_kv_grow(vox_hip_model_t* m, int slots0) {
    if (!m) return set_err("model_set_kv_grow: null model");
    if (slots0 < 0) return set_err("model_set_kv_grow: %d slots (0: off, or the first ring capacity)", slots0);
    m->kv_grow = slots0 ? std::min(std::max(slots0, KV_GROW_MIN), m->c.dec_window + KV_GROW_MIN) : 0;
    return 0;
}

extern "C" int vox_hip_model_ada_scale(vox_hip_model_t* m, float* out) {
    memcpy(out, m->ada_host.data(), m->ada_host.size() * 4);
    return 0;
}

// ---------------------------------------------------------------------------
// Stream
// ---------------------------------------------------------------------------
static const int ENC_SUB = 1024;      // encoder rows per pass through the 32 layers
static const int DEC_SLACK = 64;      // decoder ring capacity = window + slack
static_assert(DEC_SLACK == KV_GROW_MIN, "a growing ring starts no smaller than the slack");
static const int STEP_BATCH = 16;     // graph replays between EOS checks
static const size_t GEMM_WS_ELEMS = (size_t)8 << 20;  // split-K workspace (32 MB)
static const int TOKENS_CAP = 1 << 16;  // per-stream token / alternatives ring entries

struct vox_hip_stream {
    vox_hip_stream() { memset((void*)this, 0, offsetof(vox_hip_stream, pev)); }
    vox_hip_model_t* m;
    unsigned long long uid;  // unique per stream object ever created (batch graph keys)
    hipStream_t st;
    // rolling KV caches [layers][cap][kv_dim]
    float *ek, *ev, *dk, *dv;   // dk / dv: elements of type kvt (f32, IEEE half or FP8 E4M3 bytes)
    int ecap, dcap;             // ek / ev: elements of type ekvt (f32, IEEE half or FP8 E4M3 bytes)
    int kvt, ekvt;
    // growing decoder rings (vox_hip_model_set_kv_grow): the first capacity (0: the full ring from
    // the start, dcap never moves), an upper bound of the rows the ring holds (the last position + 1
    // of the calls that appended so far: each of them passes through stream_grow_dec first; a
    // growth copies that many rows), growths and bytes copied by them
    int dslots0, drows;
    long long kv_grows, kv_copied;
    // encoder passes of this stream by path (vox_hip_stream_enc_paths): one-row GEMV, fused
    // skinny chain (k_sklx), slab skinny chain, M > 1 rows pass, and layer-0 attention launches
    // that took a split key grid
    long long enc_paths[5];
    long long enc_pos;  // next encoder logical position
    // conv stem
    float *mel_p, *mel_tail, *c0_p, *c0_tail, *c0_res, *im2col;
    int res_count;
    int frames_cap;   // capacity (mel frames) of the conv buffers
    // encoder
    float *x_enc, *xn, *qkv, *q, *att, *gate, *enc_res;
    int x_rows_cap;
    int enc_res_count;
    float *rope_rows;  // per-call rope rows for the boundary twins
    int rope_rows_cap;
    // adapter
    float *adapter, *ad_mid;
    int adapter_cap, total_adapter;
    // the begun, unfinished batched call that lists this stream (vox_hip_batch_begin_rows ..
    // vox_hip_batch_finish), null otherwise: its slot table holds the stream's buffer pointers
    struct vox_hip_batch* held;
    long long ad_grows, ad_grows_held;  // adapter buffer growths / of them inside such a call
    // decoder
    float *xd, *xnd, *qkvd, *qd_, *attd, *gated, *part, *logits, *pval;
    float *part_alt, *alts;  // stream_fill_alts partials / per-step records [tokens_cap][ALT_REC]
    float* gws;              // split-K GEMM partials (encoder / prefill / adapter)
    size_t gws_n;
    uint16_t* exp_;          // skinny encoder: row planes [4][3][16][max K] (fragment order)
    float* eslab;            // skinny encoder: split-K slabs [4][S][16][N]
    uint16_t* exp2;          // k_sklx: the second planes buffer (wo / w2 inputs)
    int* eticket;            // k_sklx slice tickets [SKX_TICKETS] (zeroed, self-resetting)
    int enc_async;           // vox_hip_stream_encode_mel returns without a stream sync
    float* xbatch;           // stacked encoder rows of a batched pass led by this stream
    float *cs_im, *cs_c0;    // its stacked conv-stem im2col rows / conv0 rows (enc_prefix_batch)
    float *abatch, *abatch_out;  // its stacked adapter input rows (4 x enc_dim) / adapter rows
    float* essq;             // k_sklx row sums of squares per column slice [2][slices][16]
    uint16_t *gpa, *gpc;     // k_gemmf planes: norm / attention rows (K <= max(enc_dim, heads x hd)), gate rows
    int* gflags;             // k_gemmf partial-tile flags + the recompute counter (gemmf_flag_ints())
    int gepoch;              // k_gemmf launch epoch on this stream
    uint16_t *dpa, *dpc;     // decoder prefill planes on k_gemmf: [rb][3][16][max(dim, heads x hd)], [rb][3][16][hidden]
    int dp_rows;             // rows they hold
    int n_alt;               // vox_stream_set_alt (voxtral.c:1329-1337); 1 = off
    float alt_cutoff;
    int graph_alt;           // alt mode the step graphs were captured with
    int graph_rope_gen;      // model rope table generation the step graphs were captured with
    int *pidx, *state, *tokens;   // tokens: ring of tokens_cap ids, index = step % tokens_cap
    int* twin_state;              // decoder_full_step's argmax state (the graph state stays untouched)
    int dec_rows_cap, tokens_cap;
    hipGraphExec_t step_exec[STEP_GRAPHS];  // [g]: attention with 2^g key splits (g = 0: no combine)
    int graph_ready;              // bit mask of built graphs
    int started, eos_seen, n_generated;
    int h_state[4];
    int delay;                    // vox_hip_stream_set_delay: the stream's own delay in tokens, -1: the model's
    // profiling
    int profiling;
    int graph_prof;               // the last (eager, profiled) steps recorded W1|W3 events
    int capturing;
    hipEvent_t evt[2];
    hipEvent_t sev;               // cross-queue ordering (batched encoder pass), no timing
    std::vector<hipEvent_t> pev;  // [2*dec_layers] start/stop of each layer's W1|W3 GEMV
    double prof_ms, prof_bytes;
    long long prof_launches;
};

static int stream_alloc_frames(vox_hip_stream_t* s, int frames) {
    if (frames <= s->frames_cap) return 0;
    const vox_hip_config_t& c = s->m->c;
    int f = 256;
    while (f < frames) f *= 2;
    dfree(s->mel_p); dfree(s->c0_p); dfree(s->im2col); dfree(s->x_enc);
    CK(dalloc(&s->mel_p, (size_t)(f + 2) * c.mel_bins));
    CK(dalloc(&s->c0_p, (size_t)(f + 3) * c.enc_dim));
    size_t im = std::max((size_t)f * c.mel_bins * 3, (size_t)(f / 2 + 2) * c.enc_dim * 3);
    CK(dalloc(&s->im2col, im));
    CK(dalloc(&s->x_enc, (size_t)(f / 2 + 8) * c.enc_dim));
    s->frames_cap = f;
    return 0;
}

static int batch_park(struct vox_hip_batch* b, float* p);
static const char* HELD_MSG = "the stream is in a begun call that was not finished (vox_hip_batch_finish first)";

// The adapter buffer holds `need` rows: a larger one is allocated, the rows copied on the
// stream's queue, the old one freed.  Inside a begun batched call that lists the stream
// (s->held) the old buffer is not freed: the call's slot table holds its address and the steps
// batch_finish has yet to enqueue read the call's rows[i] first rows through it.  All of those
// exist there, and nothing writes the old buffer again, so the call reads the same rows it
// would have read without the growth; the batch frees the buffer after its last wait.
static int stream_alloc_adapter(vox_hip_stream_t* s, int need) {
    if (need <= s->adapter_cap) return 0;
    const int D = s->m->c.dec_dim;
    int nc = s->adapter_cap ? s->adapter_cap : g_adapter_rows0;
    while (nc < need) nc *= 2;
    float* na = nullptr;
    CK(dalloc(&na, (size_t)nc * D));
    if (s->adapter && s->total_adapter > 0)
        if (hipError_t e = hipMemcpyAsync(na, s->adapter, (size_t)s->total_adapter * D * 4, hipMemcpyDeviceToDevice, s->st);
            e != hipSuccess) {
            dfree(na);
            return set_err("adapter rows copy: %s", hipGetErrorString(e));
        }
    if (hipError_t e = hipStreamSynchronize(s->st); e != hipSuccess) {
        dfree(na);
        return set_err("adapter rows copy: %s", hipGetErrorString(e));
    }
    if (s->adapter_cap) {
        s->ad_grows++;
        s->ad_grows_held += s->held != nullptr;
    }
    if (s->held && s->adapter) {
        if (batch_park(s->held, s->adapter)) {
            dfree(na);
            return -1;
        }
        s->adapter = nullptr;
    } else {
        dfree(s->adapter);
    }
    s->adapter = na;
    s->adapter_cap = nc;
    s->graph_ready = 0;  // the step graph captured the old pointer
    return 0;
}

static int stream_alloc_dec_rows(vox_hip_stream_t* s, int rows) {
    if (rows <= s->dec_rows_cap) return 0;
    const vox_hip_config_t& c = s->m->c;
    int r = 64;
    while (r < rows) r *= 2;
    const int DQ = c.dec_heads * c.dec_head_dim, DKV = c.dec_kv_heads * c.dec_head_dim;
    dfree(s->xd); dfree(s->xnd); dfree(s->qkvd); dfree(s->qd_); dfree(s->attd); dfree(s->gated);
    CK(dalloc(&s->xd, (size_t)r * c.dec_dim));
    CK(dalloc(&s->xnd, (size_t)r * c.dec_dim));
    CK(dalloc(&s->qkvd, (size_t)r * (DQ + 2 * DKV)));
    CK(dalloc(&s->qd_, (size_t)r * DQ));
    CK(dalloc(&s->attd, (size_t)r * DQ));
    CK(dalloc(&s->gated, (size_t)r * c.dec_hidden));
    s->dec_rows_cap = r;
    s->graph_ready = 0;
    return 0;
}

extern "C" void vox_hip_stream_free(vox_hip_stream_t* s);

extern "C" vox_hip_stream_t* vox_hip_stream_create(vox_hip_model_t* m) {
    static std::atomic<unsigned long long> next_uid{1};
    vox_hip_stream_t* s = new vox_hip_stream_t();
    s->m = m;
    s->uid = next_uid++;
    s->delay = -1;
    const vox_hip_config_t& c = m->c;
    auto fail = [&]() -> vox_hip_stream_t* { vox_hip_stream_free(s); return nullptr; };
#define TRYH(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { set_err("%s: %s", #x, hipGetErrorString(e__)); return fail(); } } while (0)
#define SCL(field, l) (w->field ? w->field[l] : nullptr)
    TRYH(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
    const int EKV = c.enc_kv_heads * c.enc_head_dim, DKV = c.dec_kv_heads * c.dec_head_dim;
    const int EQ = c.enc_heads * c.enc_head_dim;
    s->ecap = c.enc_window + ENC_SUB + 64;
    s->dcap = c.dec_window + DEC_SLACK;
    // (a first capacity of the full size is the plain ring)
    s->dslots0 = m->kv_grow < s->dcap ? m->kv_grow : 0;
    if (s->dslots0) s->dcap = s->dslots0;
    s->kvt = m->kvt;
    s->ekvt = m->ekvt;
    // (a half or one-byte encoder ring has head_dim 64, so EKV is a multiple of 4)
    TRYH(dalloc(&s->ek, (size_t)c.enc_layers * s->ecap * EKV / (4 / kv_esize(s->ekvt))));
    TRYH(dalloc(&s->ev, (size_t)c.enc_layers * s->ecap * EKV / (4 / kv_esize(s->ekvt))));
    // (dalloc counts floats: a half ring takes half of them, a one-byte ring a quarter; the
    // narrow modes have head_dim 128, so DKV is a multiple of 4)
    TRYH(dalloc(&s->dk, (size_t)c.dec_layers * s->dcap * DKV / (4 / kv_esize(s->kvt))));
    TRYH(dalloc(&s->dv, (size_t)c.dec_layers * s->dcap * DKV / (4 / kv_esize(s->kvt))));
    TRYH(dalloc(&s->mel_tail, (size_t)2 * c.mel_bins));
    TRYH(dalloc(&s->c0_tail, (size_t)2 * c.enc_dim));
    TRYH(dalloc(&s->c0_res, (size_t)c.enc_dim));
    TRYH(dalloc(&s->enc_res, (size_t)4 * c.enc_dim));
    TRYH(dalloc(&s->xn, (size_t)ENC_SUB * c.enc_dim));
    TRYH(dalloc(&s->qkv, (size_t)ENC_SUB * (EQ + 2 * EKV)));
    TRYH(dalloc(&s->q, (size_t)ENC_SUB * EQ));
    TRYH(dalloc(&s->att, (size_t)ENC_SUB * EQ));
    TRYH(dalloc(&s->gate, (size_t)ENC_SUB * c.enc_hidden));
    TRYH(dalloc(&s->ad_mid, (size_t)(ENC_SUB / 4 + 4) * c.dec_dim));
    // decode-attention partials + one arrival count per kv head after them (zeroed here,
    // reset by the merging block after every launch)
    TRYH(dalloc(&s->part, (size_t)c.dec_heads * attn_maxch(c.dec_window) * (c.dec_head_dim + 2) + c.dec_kv_heads));
    TRYH(dalloc(&s->part_alt, (size_t)GEMV_MAX_BLOCKS * ALT_PART));
    s->gws_n = GEMM_WS_ELEMS;
    TRYH(dalloc(&s->gws, s->gws_n));
    TRYH(dalloc(&s->logits, (size_t)c.vocab));
    TRYH(dalloc(&s->pval, GEMV_MAX_BLOCKS));
    TRYH(dalloc(&s->pidx, GEMV_MAX_BLOCKS));
    TRYH(dalloc(&s->state, 4));
    TRYH(dalloc(&s->twin_state, 4));
    s->tokens_cap = TOKENS_CAP;
    TRYH(dalloc(&s->tokens, s->tokens_cap));
    TRYH(dalloc(&s->alts, (size_t)s->tokens_cap * ALT_REC));
    s->n_alt = 1;
    s->alt_cutoff = 0.f;
    TRYH(hipEventCreate(&s->evt[0]));
    TRYH(hipEventCreate(&s->evt[1]));
    TRYH(hipEventCreateWithFlags(&s->sev, hipEventDisableTiming));
#undef TRYH
    if (stream_alloc_frames(s, 2048) || stream_alloc_adapter(s, g_adapter_rows0) || stream_alloc_dec_rows(s, 64))
        return fail();
    if (vox_hip_stream_reset(s)) return fail();
    return s;
}

// the batched steps' queue: the highest stream priority, so beside a cross-stream encoder pass
// (vox_hip_batch_decode_rows) the latency-bound step kernels go first
static hipError_t queue_high_priority(hipStream_t* q) {
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) {
        (void)hipGetLastError();  // not left pending for the next launch check
        hi = 0;
    }
    // VOX_HIP_BATCH_PRIORITY=0: a normal-priority batch queue (A/B of the served overlap)
    const char* e = getenv("VOX_HIP_BATCH_PRIORITY");
    if (e && atoi(e) == 0) return hipStreamCreateWithFlags(q, hipStreamNonBlocking);
    return hipStreamCreateWithPriority(q, hipStreamNonBlocking, hi);
}

// the stream's delay and ada table: its own (vox_hip_stream_set_delay), or the model's read at use
static int stream_delay(const vox_hip_stream_t* s) { return s->delay < 0 ? s->m->delay_tokens : s->delay; }
static const float* stream_ada(const vox_hip_stream_t* s) { return s->delay < 0 ? s->m->ada_scale : s->m->ada_tab[s->delay]; }

extern "C" int vox_hip_stream_set_delay(vox_hip_stream_t* s, int delay_tokens) {
    if (!s) return set_err("stream_set_delay: null stream");
    if (s->held) return set_err("stream_set_delay: %s", HELD_MSG);
    if (delay_tokens < -1 || delay_tokens > VOX_HIP_MAX_DELAY_TOKENS)
        return set_err("stream_set_delay: %d tokens is not -1 (the model's delay) or 0..%d", delay_tokens, VOX_HIP_MAX_DELAY_TOKENS);
    if (s->started)
        return set_err("stream_set_delay: the stream's decoder has started (vox_hip_stream_reset or _reset_decoder first)");
    if (delay_tokens >= 0 && model_ada_table(s->m, delay_tokens)) return -1;
    s->delay = delay_tokens;
    // the step graphs hold the ada pointer
    for (int g = 0; g < STEP_GRAPHS; g++)
        if (s->step_exec[g]) {
            hipGraphExecDestroy(s->step_exec[g]);
            s->step_exec[g] = nullptr;
        }
    s->graph_ready = 0;
    return 0;
}

extern "C" int vox_hip_stream_delay(const vox_hip_stream_t* s) { return s ? stream_delay(s) : -1; }

extern "C" int vox_hip_stream_ada_scale(vox_hip_stream_t* s, float* out) {
    if (!s || !out) return set_err("stream_ada_scale: null argument");
    const std::vector<float>& t = s->delay < 0 ? s->m->ada_host : s->m->ada_tab_host[s->delay];
    memcpy(out, t.data(), t.size() * 4);
    return 0;
}

extern "C" int vox_hip_stream_kv_fp16(const vox_hip_stream_t* s) { return s->kvt == KV_F16; }
extern "C" int vox_hip_stream_kv_dtype(const vox_hip_stream_t* s) { return s->kvt; }

extern "C" int vox_hip_stream_enc_kv_fp16(const vox_hip_stream_t* s) { return s && s->ekvt == KV_F16; }
extern "C" int vox_hip_stream_enc_kv_dtype(const vox_hip_stream_t* s) { return s ? s->ekvt : -1; }
extern "C" int vox_hip_stream_enc_paths(const vox_hip_stream_t* s, long long out5[5]) {
    if (!s || !out5) return set_err("stream_enc_paths: null argument");
    for (int i = 0; i < 5; i++) out5[i] = s->enc_paths[i];
    return 0;
}
// bytes of the stream's encoder K and V rings together
extern "C" long long vox_hip_stream_enc_kv_bytes(const vox_hip_stream_t* s) {
    if (!s) return -1;
    const vox_hip_config_t& c = s->m->c;
    return 2LL * c.enc_layers * s->ecap * c.enc_kv_heads * c.enc_head_dim * (long long)kv_esize(s->ekvt);
}

// layer l's encoder K or V ring (base = s->ek or s->ev) in the stream's element type
static float* enc_ring(const vox_hip_stream_t* s, float* base, int l) {
    const vox_hip_config_t& c = s->m->c;
    const size_t elems = (size_t)l * s->ecap * c.enc_kv_heads * c.enc_head_dim;
    return reinterpret_cast<float*>(reinterpret_cast<char*>(base) + elems * kv_esize(s->ekvt));
}

// layer l's decoder K or V ring (base = s->dk or s->dv) in the stream's element type
static float* dec_ring(const vox_hip_stream_t* s, float* base, int l) {
    const vox_hip_config_t& c = s->m->c;
    const size_t elems = (size_t)l * s->dcap * c.dec_kv_heads * c.dec_head_dim;
    return reinterpret_cast<float*>(reinterpret_cast<char*>(base) + elems * kv_esize(s->kvt));
}

// ---------------------------------------------------------------------------
// Growing decoder rings.  A ring of fewer slots than window + slack has not
// wrapped: slot = position, so a longer ring holds the same rows at the same slots and growth
// is a copy of each layer's first rows from pitch cap0 * DKV * esize to pitch cap1 * DKV * esize.
// ---------------------------------------------------------------------------
static int dec_ring_full(const vox_hip_stream_t* s) { return s->m->c.dec_window + DEC_SLACK; }
// floats (dalloc's unit) of one of the stream's two decoder rings at `cap` slots
static size_t dec_ring_floats(const vox_hip_stream_t* s, int cap) {
    const vox_hip_config_t& c = s->m->c;
    return (size_t)c.dec_layers * cap * c.dec_kv_heads * c.dec_head_dim / (4 / kv_esize(s->kvt));
}
// a ring buffer leaves: vox_hip_memory_used follows the rings down as well as up
static void dec_ring_free(float*& p, size_t floats) {
    if (!p) return;
    dfree(p);
    g_mem_used -= std::max(floats, (size_t)1) * sizeof(float);
}
// the smallest slots0 * 2^k that holds `need` positions, capped at the full ring
static int kv_grow_cap(int slots0, int full, int need) {
    long long c = slots0;
    while (c < need && c < full) c *= 2;
    return (int)std::min<long long>(c, full);
}

// One stream's pending growth: the new rings are allocated first (dec_grow_alloc; nothing is
// enqueued and the stream is untouched, so a failure leaves it whole at its old capacity), then
// every growth of a call is committed together (dec_grow_commit).
struct DecGrow {
    vox_hip_stream_t* s;
    int need, cap;      // positions the rings are to hold; the new capacity (0: no growth)
    bool appends;       // the caller goes on to append up to `need` positions (a reservation does not)
    float *nk, *nv;
};

static int dec_grow_alloc(vox_hip_stream_t* s, int need, bool appends, DecGrow* g) {
    const int full = dec_ring_full(s);
    *g = DecGrow{s, std::min(std::max(need, 0), full), 0, appends, nullptr, nullptr};
    if (!s->dslots0 || g->need <= s->dcap) return 0;
    const int nc = kv_grow_cap(s->dslots0, full, g->need);
    const size_t nf = dec_ring_floats(s, nc);
    hipError_t e = dalloc(&g->nk, nf);
    if (e == hipSuccess) {
        e = dalloc(&g->nv, nf);
        if (e != hipSuccess) dec_ring_free(g->nk, nf);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();  // the failed hipMalloc, so no later launch check reports it
        g->nk = g->nv = nullptr;
        return set_err("decoder KV ring growth %d -> %d slots (%zu bytes): %s", s->dcap, nc, 2 * nf * sizeof(float),
                       hipGetErrorString(e));
    }
    g->cap = nc;
    return 0;
}

static void dec_grow_drop(DecGrow* g, int n) {
    for (int i = 0; i < n; i++)
        if (g[i].cap) {
            const size_t nf = dec_ring_floats(g[i].s, g[i].cap);
            dec_ring_free(g[i].nk, nf);
            dec_ring_free(g[i].nv, nf);
            g[i].cap = 0;
        }
}

// The copies of every pending growth on queue q (the queue that reads the rings next), one 2D
// copy per ring: the first s->drows rows of every layer (what the ring holds; the positions a
// growth reserves enter s->drows only where the caller appends them).  Every earlier writer of a ring is done by
// now: each entry point that appends waits for its queue before it returns, and a begun
// batched call refuses its members to all of them.  The old rings are freed after the wait for
// q, when their last reader, the copy, is done; the stream's step graphs hold their addresses
// and the capacity, so they are captured again.
static int dec_grow_commit(DecGrow* g, int n, hipStream_t q) {
    bool any = false;
    for (int i = 0; i < n; i++) {
        vox_hip_stream_t* s = g[i].s;
        if (!g[i].cap) continue;
        any = true;
        const vox_hip_config_t& c = s->m->c;
        const size_t row = (size_t)c.dec_kv_heads * c.dec_head_dim * kv_esize(s->kvt);
        const int rows = std::min(s->drows, s->dcap);
        if (rows > 0) {
            float* src[2] = {s->dk, s->dv};
            float* dst[2] = {g[i].nk, g[i].nv};
            for (int w = 0; w < 2; w++)
                if (hipError_t e = hipMemcpy2DAsync(dst[w], (size_t)g[i].cap * row, src[w], (size_t)s->dcap * row,
                                                    (size_t)rows * row, c.dec_layers, hipMemcpyDeviceToDevice, q);
                    e != hipSuccess) {
                    (void)hipStreamSynchronize(q);
                    dec_grow_drop(g, n);
                    return set_err("decoder KV ring growth copy: %s", hipGetErrorString(e));
                }
        }
    }
    if (any)
        if (hipError_t e = hipStreamSynchronize(q); e != hipSuccess) {
            dec_grow_drop(g, n);
            return set_err("decoder KV ring growth copy: %s", hipGetErrorString(e));
        }
    for (int i = 0; i < n; i++) {
        vox_hip_stream_t* s = g[i].s;
        if (g[i].cap) {
            const vox_hip_config_t& c = s->m->c;
            const size_t of = dec_ring_floats(s, s->dcap);
            s->kv_grows++;
            s->kv_copied += 2LL * c.dec_layers * std::min(s->drows, s->dcap) * c.dec_kv_heads * c.dec_head_dim *
                            (long long)kv_esize(s->kvt);
            dec_ring_free(s->dk, of);
            dec_ring_free(s->dv, of);
            s->dk = g[i].nk;
            s->dv = g[i].nv;
            s->dcap = g[i].cap;
            s->graph_ready = 0;
            g[i].cap = 0;
        }
        if (g[i].appends) s->drows = std::max(s->drows, g[i].need);
    }
    return 0;
}

// the stream's rings hold min(full, need) positions before a call on its own queue appends them
// (appends = false: a reservation, nothing is appended)
static int stream_grow_dec(vox_hip_stream_t* s, int need, bool appends = true) {
    DecGrow g;
    if (dec_grow_alloc(s, need, appends, &g)) return -1;
    return dec_grow_commit(&g, 1, s->st);
}

// a stream that grew goes back to its first capacity (new audio: vox_hip_stream_reset).  The
// small rings are allocated before anything is freed, and vox_hip_stream_reset calls this before
// it touches any other state: a failure leaves the whole stream as it was.
static int stream_shrink_dec(vox_hip_stream_t* s) {
    if (!s->dslots0 || s->dcap == s->dslots0) return 0;
    const size_t nf = dec_ring_floats(s, s->dslots0), of = dec_ring_floats(s, s->dcap);
    // the small rings first: a failure leaves the stream whole at the capacity it had
    float *nk = nullptr, *nv = nullptr;
    if (dalloc(&nk, nf) != hipSuccess || dalloc(&nv, nf) != hipSuccess) {
        (void)hipGetLastError();
        dec_ring_free(nk, nf);
        dec_ring_free(nv, nf);
        return set_err("stream_reset: decoder KV rings of %d slots could not be allocated", s->dslots0);
    }
    CK(hipStreamSynchronize(s->st));
    dec_ring_free(s->dk, of);
    dec_ring_free(s->dv, of);
    s->dk = nk;
    s->dv = nv;
    s->dcap = s->dslots0;
    s->drows = 0;
    s->graph_ready = 0;
    return 0;
}

extern "C" int vox_hip_stream_kv_slots(const vox_hip_stream_t* s) { return s ? s->dcap : -1; }
// bytes of the stream's decoder K and V rings together
extern "C" long long vox_hip_stream_kv_bytes(const vox_hip_stream_t* s) {
    if (!s) return -1;
    const vox_hip_config_t& c = s->m->c;
    return 2LL * c.dec_layers * s->dcap * c.dec_kv_heads * c.dec_head_dim * (long long)kv_esize(s->kvt);
}
extern "C" int vox_hip_stream_kv_grow_stats(const vox_hip_stream_t* s, long long out3[3]) {
    if (!s || !out3) return set_err("stream_kv_grow_stats: null argument");
    out3[0] = s->kv_grows;
    out3[1] = s->kv_copied;
    out3[2] = s->dcap;
    return 0;
}
// the rings hold `positions` positions (the full ring at most) from now on: a server grows
// ahead of the calls that would, and takes a failure here as its admission test
extern "C" int vox_hip_stream_reserve_kv(vox_hip_stream_t* s, int positions) {
    if (!s) return set_err("stream_reserve_kv: null stream");
    if (s->held) return set_err("stream_reserve_kv: %s", HELD_MSG);
    if (positions < 0) return set_err("stream_reserve_kv: %d positions", positions);
    return stream_grow_dec(s, positions, false);
}

extern "C" void vox_hip_stream_free(vox_hip_stream_t* s) {
    if (!s) return;
    if (s->held) {
        // (void: reported through vox_hip_last_error; the stream stays whole for the call)
        set_err("stream_free: %s", HELD_MSG);
        return;
    }
    if (s->st) hipStreamSynchronize(s->st);
    for (int g = 0; g < STEP_GRAPHS; g++)
        if (s->step_exec[g]) hipGraphExecDestroy(s->step_exec[g]);
    dfree(s->ek); dfree(s->ev); dfree(s->dk); dfree(s->dv);
    dfree(s->mel_p); dfree(s->mel_tail); dfree(s->c0_p); dfree(s->c0_tail); dfree(s->c0_res);
    dfree(s->im2col); dfree(s->x_enc); dfree(s->xn); dfree(s->qkv); dfree(s->q); dfree(s->att);
    dfree(s->gate); dfree(s->enc_res); dfree(s->rope_rows); dfree(s->adapter); dfree(s->ad_mid);
    dfree(s->xd); dfree(s->xnd); dfree(s->qkvd); dfree(s->qd_); dfree(s->attd); dfree(s->gated);
    dfree(s->part); dfree(s->logits); dfree(s->pval); dfree(s->pidx); dfree(s->state); dfree(s->twin_state); dfree(s->tokens);
    dfree(s->part_alt); dfree(s->alts); dfree(s->gws); dfree(s->exp_); dfree(s->eslab); dfree(s->eticket); dfree(s->essq); dfree(s->exp2); dfree(s->xbatch); dfree(s->abatch); dfree(s->abatch_out); dfree(s->cs_im); dfree(s->cs_c0);
    dfree(s->gpa); dfree(s->gpc); dfree(s->gflags); dfree(s->dpa); dfree(s->dpc);
    if (s->evt[0]) hipEventDestroy(s->evt[0]);
    if (s->evt[1]) hipEventDestroy(s->evt[1]);
    if (s->sev) hipEventDestroy(s->sev);
    for (hipEvent_t e : s->pev) hipEventDestroy(e);
    if (s->st) hipStreamDestroy(s->st);
    delete s;
}

extern "C" int vox_hip_stream_reset_decoder(vox_hip_stream_t* s) {
    // stream_reset_decoder_state (voxtral.c:766-783): KV length 0, adapter backlog dropped
    if (s->held) return set_err("stream_reset_decoder: %s", HELD_MSG);
    s->total_adapter = 0;
    s->started = 0;
    s->eos_seen = 0;
    s->n_generated = 0;
    s->drows = 0;  // (a grown ring keeps its capacity; it holds no row worth copying)
    int st[4] = {0, 0, TOKEN_BOS, 0};
    memcpy(s->h_state, st, sizeof st);
    CK(hipMemcpyAsync(s->state, st, sizeof st, hipMemcpyHostToDevice, s->st));
    CK(hipStreamSynchronize(s->st));
    return 0;
}

extern "C" int vox_hip_stream_reset(vox_hip_stream_t* s) {
    // stream_reset_full_state (voxtral.c:786-814)
    if (s->held) return set_err("stream_reset: %s", HELD_MSG);
    const vox_hip_config_t& c = s->m->c;
    // new audio: a ring that grew returns to its first capacity (first: if the small rings
    // cannot be allocated the stream is left exactly as it was)
    if (stream_shrink_dec(s)) return -1;
    s->enc_pos = 0;
    s->res_count = 0;
    s->enc_res_count = 0;
    CK(hipMemsetAsync(s->mel_tail, 0, (size_t)2 * c.mel_bins * 4, s->st));
    CK(hipMemsetAsync(s->c0_tail, 0, (size_t)2 * c.enc_dim * 4, s->st));
    return vox_hip_stream_reset_decoder(s);
}

extern "C" int vox_hip_stream_sync(vox_hip_stream_t* s) {
    CK(hipStreamSynchronize(s->st));
    return 0;
}

// ---------------------------------------------------------------------------
// Incremental log-mel on the device: the vox_mel_ctx_t of
// voxtral_audio.c:405-671 with its padded sample buffer and its frames in HBM.  The
// kernels run on the owning stream's queue, ahead of the encoder that reads the frames.
// ---------------------------------------------------------------------------
static const int MEL_FFT = 400, MEL_FREQ = 201, MEL_HOP = 160, MEL_BINS = 128, MEL_SR = 16000;
static const float MEL_LOG_MAX = 1.5f;                // LOG_MEL_MAX (voxtral_audio.c:25)
static const long long MEL_COMPACT_MIN = 16000;       // MEL_SAMPLE_COMPACT_MIN (:429)

struct vox_hip_mel {
    vox_hip_stream_t* s;
    float *window, *dcosT, *dsinT, *filtT;  // device tables (built on the host as the reference does)
    float* samples;                         // padded audio; samples[0] = global sample sample_offset
    long long n_samples, samples_cap, sample_offset;
    float* mel;                             // frames; mel[0] = global frame mel_phys0
    int mel_cap, mel_phys0;
    int frame_offset, n_frames;             // live frames: global [frame_offset, frame_offset + n_frames)
    int finished;
};

// hertz_to_mel / mel_to_hertz / build_mel_filters (voxtral_audio.c:223-285), f32 as there
static float mel_hz_to_mel(float f) {
    const float logstep = 27.0f / logf(6.4f);
    float m = 3.0f * f / 200.0f;
    if (f >= 1000.0f) m = 15.0f + logf(f / 1000.0f) * logstep;
    return m;
}
static float mel_mel_to_hz(float m) {
    const float logstep = logf(6.4f) / 27.0f;
    float f = 200.0f * m / 3.0f;
    if (m >= 15.0f) f = 1000.0f * expf(logstep * (m - 15.0f));
    return f;
}

extern "C" void vox_hip_mel_free(vox_hip_mel_t* m) {
    if (!m) return;
    if (m->s) hipStreamSynchronize(m->s->st);
    dfree(m->window); dfree(m->dcosT); dfree(m->dsinT); dfree(m->filtT); dfree(m->samples); dfree(m->mel);
    delete m;
}

extern "C" vox_hip_mel_t* vox_hip_mel_create(vox_hip_stream_t* s, int left_pad_samples) {
    if (!s || left_pad_samples < 0) {
        set_err("vox_hip_mel_create: bad arguments");
        return nullptr;
    }
    vox_hip_mel_t* m = new vox_hip_mel_t();
    memset((void*)m, 0, sizeof *m);
    m->s = s;
    auto fail = [&]() -> vox_hip_mel_t* { vox_hip_mel_free(m); return nullptr; };
    std::vector<float> win(MEL_FFT), dc((size_t)MEL_FFT * MEL_FREQ), ds((size_t)MEL_FFT * MEL_FREQ),
        ft((size_t)MEL_FREQ * MEL_BINS, 0.f);
    // DFT tables and periodic Hann window (voxtral_audio.c:531-545)
    for (int k = 0; k < MEL_FREQ; k++)
        for (int n = 0; n < MEL_FFT; n++) {
            const float ang = 2.0f * (float)M_PI * (float)k * (float)n / (float)MEL_FFT;
            dc[(size_t)n * MEL_FREQ + k] = cosf(ang);
            ds[(size_t)n * MEL_FREQ + k] = sinf(ang);
        }
    for (int i = 0; i < MEL_FFT; i++) win[i] = 0.5f * (1.0f - cosf(2.0f * (float)M_PI * (float)i / (float)MEL_FFT));
    // Slaney filters (voxtral_audio.c:248-285), stored [freq][bin]
    float fft_freqs[MEL_FREQ], ffq[MEL_BINS + 2], fdf[MEL_BINS + 1];
    for (int i = 0; i < MEL_FREQ; i++) fft_freqs[i] = (float)i * ((float)MEL_SR / 2.0f) / (float)(MEL_FREQ - 1);
    const float mmin = mel_hz_to_mel(0.0f), mmax = mel_hz_to_mel((float)MEL_SR / 2.0f);
    for (int i = 0; i < MEL_BINS + 2; i++) ffq[i] = mel_mel_to_hz(mmin + (mmax - mmin) * (float)i / (float)(MEL_BINS + 1));
    for (int i = 0; i < MEL_BINS + 1; i++) {
        fdf[i] = ffq[i + 1] - ffq[i];
        if (fdf[i] == 0.0f) fdf[i] = 1e-6f;
    }
    for (int b = 0; b < MEL_BINS; b++) {
        const float enorm = 2.0f / (ffq[b + 2] - ffq[b]);
        for (int f = 0; f < MEL_FREQ; f++) {
            const float down = (fft_freqs[f] - ffq[b]) / fdf[b];
            const float up = (ffq[b + 2] - fft_freqs[f]) / fdf[b + 1];
            float v = fminf(down, up);
            if (v < 0.0f) v = 0.0f;
            ft[(size_t)f * MEL_BINS + b] = v * enorm;
        }
    }
#define TRYH(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { set_err("%s: %s", #x, hipGetErrorString(e__)); return fail(); } } while (0)
    TRYH(dalloc(&m->window, win.size()));
    TRYH(dalloc(&m->dcosT, dc.size()));
    TRYH(dalloc(&m->dsinT, ds.size()));
    TRYH(dalloc(&m->filtT, ft.size()));
    TRYH(h2d(m->window, win.data(), win.size() * 4));
    TRYH(h2d(m->dcosT, dc.data(), dc.size() * 4));
    TRYH(h2d(m->dsinT, ds.data(), ds.size() * 4));
    TRYH(h2d(m->filtT, ft.data(), ft.size() * 4));
    // left padding: 200 (center reflect over silence) + left_pad_samples zeros (:547-557)
    m->n_samples = 200 + (long long)left_pad_samples;
    m->samples_cap = m->n_samples + 16000;
    TRYH(dalloc(&m->samples, (size_t)m->samples_cap));   // zeroed
    m->mel_cap = 1024;
    TRYH(dalloc(&m->mel, (size_t)m->mel_cap * MEL_BINS));
#undef TRYH
    return m;
}

static int mel_reserve_samples(vox_hip_mel_t* m, long long need) {
    if (need <= m->samples_cap) return 0;
    long long nc = m->samples_cap;
    while (nc < need) nc *= 2;
    float* nb = nullptr;
    CK(dalloc(&nb, (size_t)nc));
    CK(hipMemcpyAsync(nb, m->samples, (size_t)m->n_samples * 4, hipMemcpyDeviceToDevice, m->s->st));
    CK(hipStreamSynchronize(m->s->st));
    dfree(m->samples);
    m->samples = nb;
    m->samples_cap = nc;
    return 0;
}

// mel_compute_available (voxtral_audio.c:454-513): every frame whose window fits
static int mel_compute(vox_hip_mel_t* m) {
    const long long next = (long long)m->frame_offset + m->n_frames;  // global index of the next frame
    long long nf = 0;
    while ((next + nf) * MEL_HOP - m->sample_offset + MEL_FFT <= m->n_samples) nf++;
    if (nf == 0) return 0;
    const long long need = next + nf - m->mel_phys0;  // physical frames after this call
    if (need > m->mel_cap) {
        // grow, keeping only the live frames (discarded ones are dropped here)
        int nc = m->mel_cap;
        while (nc < need - (m->frame_offset - m->mel_phys0)) nc *= 2;
        float* nb = nullptr;
        CK(dalloc(&nb, (size_t)nc * MEL_BINS));
        if (m->n_frames)
            CK(hipMemcpyAsync(nb, m->mel + (size_t)(m->frame_offset - m->mel_phys0) * MEL_BINS,
                              (size_t)m->n_frames * MEL_BINS * 4, hipMemcpyDeviceToDevice, m->s->st));
        CK(hipStreamSynchronize(m->s->st));
        dfree(m->mel);
        m->mel = nb;
        m->mel_cap = nc;
        m->mel_phys0 = m->frame_offset;
    }
    CK(launch_mel_frames(m->samples, next * MEL_HOP - m->sample_offset, (int)nf, m->window, m->dcosT, m->dsinT,
                         m->filtT, MEL_LOG_MAX - 8.0f, m->mel + (size_t)(next - m->mel_phys0) * MEL_BINS, m->s->st));
    m->n_frames += (int)nf;
    return (int)nf;
}

// mel_compact_samples (voxtral_audio.c:432-451): samples no future frame reads are dropped
// once they reach 1 s (and never overlap the kept tail, so one device copy moves it)
static int mel_compact(vox_hip_mel_t* m) {
    const long long needed_from = ((long long)m->frame_offset + m->n_frames) * MEL_HOP;
    long long discard = needed_from - m->sample_offset;
    if (discard <= 0) return 0;
    if (discard > m->n_samples) discard = m->n_samples;
    const long long remain = m->n_samples - discard;
    if (discard < MEL_COMPACT_MIN || remain > discard) return 0;
    if (remain > 0)
        CK(hipMemcpyAsync(m->samples, m->samples + discard, (size_t)remain * 4, hipMemcpyDeviceToDevice, m->s->st));
    m->n_samples = remain;
    m->sample_offset += discard;
    return 0;
}

extern "C" int vox_hip_mel_reset(vox_hip_mel_t* m, int left_pad_samples) {
    if (!m || left_pad_samples < 0) return set_err("vox_hip_mel_reset: bad arguments");
    const long long n0 = 200 + (long long)left_pad_samples;
    if (mel_reserve_samples(m, n0)) return -1;
    CK(hipMemsetAsync(m->samples, 0, (size_t)n0 * 4, m->s->st));
    m->n_samples = n0;
    m->sample_offset = 0;
    m->mel_phys0 = 0;
    m->frame_offset = 0;
    m->n_frames = 0;
    m->finished = 0;
    return 0;
}

extern "C" int vox_hip_mel_feed(vox_hip_mel_t* m, const float* samples, int n) {
    if (!m || m->finished) return set_err("vox_hip_mel_feed: no context or already finished");
    if (n <= 0) return 0;
    if (mel_reserve_samples(m, m->n_samples + n)) return -1;
    CK(hipMemcpyAsync(m->samples + m->n_samples, samples, (size_t)n * 4, hipMemcpyHostToDevice, m->s->st));
    m->n_samples += n;
    const int nf = mel_compute(m);
    if (nf < 0 || mel_compact(m)) return -1;
    return nf;
}

extern "C" int vox_hip_mel_finish(vox_hip_mel_t* m, int right_pad) {
    if (!m) return set_err("vox_hip_mel_finish: no context");
    if (m->finished) return m->n_frames;
    if (right_pad < 0) right_pad = 0;
    if (mel_reserve_samples(m, m->n_samples + right_pad + 200)) return -1;
    if (right_pad > 0)
        CK(hipMemsetAsync(m->samples + m->n_samples, 0, (size_t)right_pad * 4, m->s->st));
    m->n_samples += right_pad;
    // right reflect over the last real samples (voxtral_audio.c:609-624)
    CK(launch_mel_reflect(m->samples, m->n_samples, m->n_samples - right_pad, 200, m->s->st));
    m->n_samples += 200;
    if (mel_compute(m) < 0) return -1;
    if (m->n_frames > 0) m->n_frames--;  // the last frame is dropped (:629-630)
    m->finished = 1;
    return m->n_frames;
}

extern "C" int vox_hip_mel_frames(const vox_hip_mel_t* m, int* frame_offset) {
    if (!m) return -1;
    if (frame_offset) *frame_offset = m->frame_offset;
    return m->n_frames;
}

extern "C" const float* vox_hip_mel_frame_ptr(const vox_hip_mel_t* m, int global_frame) {
    if (!m || global_frame < m->frame_offset || global_frame > m->frame_offset + m->n_frames) {
        set_err("vox_hip_mel_frame_ptr: frame %d outside the live range", global_frame);
        return nullptr;
    }
    return m->mel + (size_t)(global_frame - m->mel_phys0) * MEL_BINS;
}

// vox_mel_discard_before (voxtral_audio.c:645-662): frames before keep_from_frame leave the
// live range (their memory is reclaimed at the next growth)
extern "C" int vox_hip_mel_discard_before(vox_hip_mel_t* m, int keep_from_frame) {
    if (!m) return -1;
    if (keep_from_frame <= m->frame_offset) return 0;
    int d = keep_from_frame - m->frame_offset;
    if (d > m->n_frames) d = m->n_frames;
    m->frame_offset += d;
    m->n_frames -= d;
    return mel_compact(m);
}

extern "C" int vox_hip_mel_read(vox_hip_mel_t* m, int global_first, int n, float* out) {
    if (!m || n < 0 || global_first < m->frame_offset || global_first + n > m->frame_offset + m->n_frames)
        return set_err("vox_hip_mel_read: range outside the live frames");
    if (n == 0) return 0;
    CK(hipMemcpyAsync(out, m->mel + (size_t)(global_first - m->mel_phys0) * MEL_BINS, (size_t)n * MEL_BINS * 4,
                      hipMemcpyDeviceToHost, m->s->st));
    CK(hipStreamSynchronize(m->s->st));
    return 0;
}

// ---------------------------------------------------------------------------
// Encoder: 32 layers on rows [0, n) of x (logical positions pos0..), in place.
// voxtral_encoder.c:562-686.  rope: rows for these positions (table slice or per-call).
// ---------------------------------------------------------------------------
// Short encoder chunks (streaming -I: ~25 rows per 0.5 s) sit far below the MFMA ridge:
// their projections run as skinny GEMMs over fragment-major encoder weights (k_skl, the
// batched decoder's kernel: rows = up to 2 B fragments of 16, every weight byte streamed
// once per row block) with the consumers fused (residual + bias + RMSNorm into planes,
// SwiGLU into planes, bias into the QKV rows).  Longer chunks keep k_gemm2.
static const int ENC_SKINNY_MAX = SK_MAX_ROWS;  // buffers: up to SK_MAX_ROWS / 16 row blocks
static int enc_skinny_rows() {
    // chunks of up to this many rows take the skinny path (VOX_HIP_ENC_SKINNY_ROWS, <= 96).
    // 80: the ~70-row flush chunk of a one-shot clip too (jfk encoder RTF 0.00129 -> 0.00118:
    // five 16-row blocks re-reading each weight slice from the XCD's L2 beat a mostly empty
    // 128-row k_gemm2 tile)
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("VOX_HIP_ENC_SKINNY_ROWS");
        v = e ? std::max(0, std::min(ENC_SKINNY_MAX, atoi(e))) : 80;
    }
    return v;
}

static int model_enc_frag(vox_hip_model_t* m) {
    if (!m->efrag.empty()) return 0;
    const vox_hip_config_t& c = m->c;
    const int ED = c.enc_dim, EQ = c.enc_heads * c.enc_head_dim, EKV = c.enc_kv_heads * c.enc_head_dim;
    const int EH = c.enc_hidden;
    std::vector<DecFragD> F(c.enc_layers, DecFragD{});
    for (int l = 0; l < c.enc_layers; l++) {
        const EncLayerD& L = m->enc[l];
        if (frag_copy(&F[l].wqkv, L.wqkv, EQ + 2 * EKV, ED, L.sqkv != nullptr) ||
            frag_copy(&F[l].wo, L.wo, ED, EQ, L.so != nullptr) ||
            frag_copy(&F[l].w13, L.w13, 2 * EH, ED, L.s13 != nullptr) ||
            frag_copy(&F[l].w2, L.w2, ED, EH, L.s2 != nullptr)) {
            for (auto& f : F) { dfree(f.wqkv); dfree(f.wo); dfree(f.w13); dfree(f.w2); }
            return -1;
        }
    }
    m->efrag.swap(F);
    return 0;
}

static bool enc_skinny_ok(const vox_hip_config_t& c) {
    const int ED = c.enc_dim, EQ = c.enc_heads * c.enc_head_dim, EKV = c.enc_kv_heads * c.enc_head_dim;
    const int EH = c.enc_hidden;
    return skl_splits(ED) && skl_splits(EQ) && skl_splits(EH) && ED % 64 == 0 && (EQ + 2 * EKV) % 64 == 0 &&
           (2 * EH) % 64 == 0 && ED <= 8 * 512;
}

static int enc_fused_env() {
    static const int v = env_on("VOX_HIP_ENC_FUSED");
    return v;
}

static int run_encoder_rows_skinny(vox_hip_stream_t* s, float* x, int n, long long pos0, const float* rope) {
    vox_hip_model_t* m = s->m;
    const vox_hip_config_t& c = m->c;
    const int ED = c.enc_dim, H = c.enc_heads, KVH = c.enc_kv_heads, hd = c.enc_head_dim;
    const int EQ = H * hd, EKV = KVH * hd, EH = c.enc_hidden, NQKV = EQ + 2 * EKV;
    const float scale = 1.0f / sqrtf((float)hd);
    hipStream_t st = s->st;
    if (model_enc_frag(m)) return -1;
    if (!s->exp_) {
        const int kmax = std::max(ED, std::max(EQ, EH));
        const size_t slab = std::max(std::max((size_t)skl_splits(ED, NQKV) * NQKV, (size_t)skl_splits(EQ, ED) * ED),
                                     std::max((size_t)skl_splits(ED, 2 * EH) * 2 * EH, (size_t)skl_splits(EH, ED) * ED));
        const int RB = ENC_SKINNY_MAX / SK_ROWS;
        CK(dalloc(&s->exp_, (size_t)RB * 3 * SK_ROWS * kmax));
        CK(dalloc(&s->eslab, (size_t)RB * SK_ROWS * slab));
        CK(dalloc(&s->eticket, (size_t)SKX_TICKETS));
        CK(dalloc(&s->essq, (size_t)RB * SK_ROWS * (ED / 64)));
    }
    uint16_t* xp = s->exp_;
    float* sl = s->eslab;
    if (enc_fused_env() && !m->enc[0].sqkv) {
        // bf16: the row kernels folded into the projections (k_sklx): 5 launches per layer.
        // Planes alternate between two buffers so that no launch overwrites its own input:
        // xa = the QKV / W1|W3 inputs (x * norm weight), xq = the wo / w2 inputs.
        if (!s->exp2)
            CK(dalloc(&s->exp2, (size_t)(ENC_SKINNY_MAX / SK_ROWS) * 3 * SK_ROWS * std::max(ED, std::max(EQ, EH))));
        uint16_t *xa = xp, *xq = s->exp2;
        SklFused f;
        f.part = sl;
        f.ticket = s->eticket;
        f.eps = c.enc_eps;
        const int nsl_wo = sklx_slices(ED, EQ), nsl_w2 = sklx_slices(ED, EH);
        CK(launch_rmsnorm_fplanes(x, n, ED, m->enc[0].attn_norm, nullptr, c.enc_eps, xa, nullptr, 0, st));
        s->enc_paths[1]++;
        for (int l = 0; l < c.enc_layers; l++) {
            const EncLayerD& L = m->enc[l];
            const DecFragD& F = m->efrag[l];
            float* Kc = enc_ring(s, s->ek, l);
            float* Vc = enc_ring(s, s->ev, l);
            // QKV (attention RMSNorm: layer 0 normalised planes, then x * w planes scaled by
            // the inverse RMS), bias + RoPE + K/V append epilogue (encoder.c:562-607)
            SklFused q = f;
            q.ssq_in = s->essq;
            q.nsl = nsl_w2;
            q.bias = L.bqkv;
            q.rope = rope;
            q.qd = EQ;
            q.kvd = EKV;
            q.hd = hd;
            q.pos0 = (int)pos0;
            q.cap = s->ecap;
            q.q = s->q;
            q.Kc = Kc;
            q.Vc = Vc;
            q.kvt = s->ekvt;
            int ns = 0;
            CK(launch_gemm_sklx(l ? SKX_PRO_SCALE : SKX_PRO_PLANES, SKX_EPI_QKV, xa, ED, F.wqkv, NQKV, n, q, st));
            CK(launch_attn_rows_mf(hd, s->q, EQ, Kc, Vc, s->ecap, s->att, EQ, n, H, KVH, (int)pos0, 0, c.enc_window, scale,
                                 st, s->gws, s->gws_n, xq, s->ekvt, &ns));
            if (l == 0) s->enc_paths[4] += ns > 1;
            // wo + bias residual (encoder.c:640-644); the FFN norm's planes and row sums of squares
            SklFused o = f;
            o.x = x;
            o.bias = L.bo;
            o.ssq_out = s->essq;
            o.planes = xa;
            o.nw = L.ffn_norm;
            CK(launch_gemm_sklx(SKX_PRO_PLANES, SKX_EPI_RESID, xq, EQ, F.wo, ED, n, o, st));
            // W1|W3 (FFN RMSNorm), SwiGLU epilogue into the w2 planes (encoder.c:646-676)
            SklFused u = f;
            u.ssq_in = s->essq;
            u.nsl = nsl_wo;
            u.planes = xq;
            CK(launch_gemm_sklx(SKX_PRO_SCALE, SKX_EPI_SWIGLU, xa, ED, F.w13, 2 * EH, n, u, st));
            // w2 + bias residual (encoder.c:678-684); the next layer's attention-norm planes
            SklFused d = f;
            d.x = x;
            d.bias = L.b2;
            d.ssq_out = s->essq;
            if (l + 1 < c.enc_layers) {
                d.planes = xa;
                d.nw = m->enc[l + 1].attn_norm;
            }
            CK(launch_gemm_sklx(SKX_PRO_PLANES, SKX_EPI_RESID, xq, EH, F.w2, ED, n, d, st));
        }
        CK(launch_rmsnorm_rows(x, ED, x, ED, m->enc_norm, nullptr, n, ED, c.enc_eps, st));
        return 0;
    }
    s->enc_paths[2]++;
    for (int l = 0; l < c.enc_layers; l++) {
        const EncLayerD& L = m->enc[l];
        const DecFragD& F = m->efrag[l];
        float* Kc = enc_ring(s, s->ek, l);
        float* Vc = enc_ring(s, s->ev, l);
        // previous layer's w2 residual (+ bias) then RMSNorm -> planes (encoder.c:562-566, 680-684)
        CK(launch_rmsnorm_fplanes(x, n, ED, L.attn_norm, nullptr, c.enc_eps, xp, l ? sl : nullptr,
                                  l ? skl_splits(EH, ED) : 0, st, l ? m->enc[l - 1].b2 : nullptr));
        CK(launch_gemm_skl(xp, ED, F.wqkv, L.sqkv, NQKV, n, sl, st));
        // QKV slabs + biases -> RoPE -> K/V append (one pass), attention with its output
        // merged straight into the wo planes
        CK(launch_slabs_rope_kv(sl, skl_splits(ED, NQKV), n, L.bqkv, EQ, EKV, hd, rope, (int)pos0, s->q, Kc, Vc, s->ecap, st,
                                s->ekvt));
        CK(launch_attn_rows_mf(hd, s->q, EQ, Kc, Vc, s->ecap, s->att, EQ, n, H, KVH, (int)pos0, 0, c.enc_window, scale, st,
                             s->gws, s->gws_n, xp, s->ekvt));
        CK(launch_gemm_skl(xp, EQ, F.wo, L.so, ED, n, sl, st));
        // wo residual (+ bias) then the FFN RMSNorm -> planes (encoder.c:640-650)
        CK(launch_rmsnorm_fplanes(x, n, ED, L.ffn_norm, nullptr, c.enc_eps, xp, sl, skl_splits(EQ, ED), st, L.bo));
        CK(launch_gemm_skl(xp, ED, F.w13, L.s13, 2 * EH, n, sl, st));
        CK(launch_swiglu_fplanes(sl, skl_splits(ED, 2 * EH), EH, n, xp, st));
        CK(launch_gemm_skl(xp, EH, F.w2, L.s2, ED, n, sl, st));
    }
    CK(launch_resid_slabs(x, n, ED, sl, skl_splits(EH, ED), m->enc[c.enc_layers - 1].b2, st));
    CK(launch_rmsnorm_rows(x, ED, x, ED, m->enc_norm, nullptr, n, ED, c.enc_eps, st));
    return 0;
}

// Encoder passes of more rows (one-shot chunks: 677 rows for jfk, 1024-row passes of long
// clips): the projections on k_gemmf (stream-K MFMA over fragment-major weights), their
// inputs written as planes by the producers (RMSNorm rows, the attention output, the W1|W3
// SwiGLU epilogue), so no GEMM re-splits f32 activations per column tile.
static int enc_gemmf_env() {
    static const int v = env_on("VOX_HIP_GEMMF");
    return v;
}

// Q8 tensors among a pass's layers: k_gemmf takes them only where the model took the
// vox_hip_set_gemmf_q8 switch (their int8 fragment copies, each launch by its own tensor's format)
template <class Layer>
static bool gemmf_fmt_ok(const vox_hip_model_t* m, const std::vector<Layer>& layers) {
    if (m->gemmf_q8) return true;
    for (const Layer& L : layers)
        if (L.sqkv || L.so || L.s13 || L.s2) return false;
    return true;
}

static bool enc_gemmf_ok(const vox_hip_model_t* m, int n) {
    const vox_hip_config_t& c = m->c;
    const int ED = c.enc_dim, EQ = c.enc_heads * c.enc_head_dim, EKV = c.enc_kv_heads * c.enc_head_dim;
    return enc_gemmf_env() && gemmf_fmt_ok(m, m->enc) && gemmf_ok(n, EQ + 2 * EKV, ED) && gemmf_ok(n, ED, EQ) &&
           gemmf_ok(n, 2 * c.enc_hidden, ED) && gemmf_ok(n, ED, c.enc_hidden) && c.enc_hidden % 64 == 0 &&
           ED <= 4 * 512;
}

// k_gemmf launches on queue st with their split workspace, partial-tile flags and hand-off
// epochs (a queue's own: two k_gemmf launches in flight on two queues must not share flags).
// Two epoch disciplines:
//   epoch_dev == null: *epoch is a host counter baked into each launch.  A captured (replayed)
//     k_gemmf would reuse it and read stale partial tiles, so capture is refused.
//   epoch_dev != null (the wide batched step): *epoch is the launch's index within the step, the
//     kernel adds the device word, and the step's last kernel advances the word past the indices
//     (launch_gemmf_epoch_bump), so the launches may be captured and replayed.  Tiles by
//     gemmf_wide_rb; step_q8 counts the step's launches on int8 fragments (batch_run multiplies
//     it by the replays).
struct GemmfQ {
    hipStream_t st;
    float* ws;
    size_t ws_n;
    int* flags;
    int* epoch;
    long long* n_q8;  // the model's count of launches on int8 fragments
    const int* epoch_dev;
    int* step_q8;
};

// W: the tensor's fragment-major copy, int8 where wscale (its Q8 row scales) is set
static int gemmf_on(const GemmfQ& q, int epi, const uint16_t* xs, int K, int n, const uint8_t* W, const float* wscale,
                    int N, const float* bias, float* C, int ldc, uint16_t* xo) {
    if (!q.epoch_dev) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        CK(hipStreamIsCapturing(q.st, &cs));
        if (cs != hipStreamCaptureStatusNone) return set_err("k_gemmf launch while the stream is capturing");
    }
    if (++*q.epoch <= 0) *q.epoch = 1;
    // the launcher's shape / workspace checks, reported with the shape (launch_gemmf has one
    // error code for all of them)
    if (!gemmf_ok(n, N, K) || !q.ws || !q.flags)
        return set_err("k_gemmf: unsupported shape M %d N %d K %d (ws %p flags %p)", n, N, K, (void*)q.ws, (void*)q.flags);
    if (!q.epoch_dev) {
        // an error an earlier unchecked call left pending (the launcher's hipGetLastError would
        // report it as this launch's); not where the launch may be inside a capture, which gets
        // no HIP call but the launch itself
        const hipError_t pend = hipGetLastError();
        if (pend != hipSuccess) return set_err("k_gemmf: HIP error pending before the launch: %s", hipGetErrorString(pend));
    }
    CK(launch_gemmf(epi, gemm_planes_np(), xs, K, n, W, N, bias, C, ldc, xo, q.ws, q.ws_n, q.flags, *q.epoch, q.st,
                    q.epoch_dev, q.epoch_dev ? gemmf_wide_rb(n, N, K) : 0, wscale));
    if (wscale) {
        ++*q.n_q8;
        if (q.step_q8) ++*q.step_q8;
    }
    return 0;
}

// a stream's own queue, workspace, flags and host epoch counter
static GemmfQ stream_gemmfq(vox_hip_stream_t* s) {
    return GemmfQ{s->st, s->gws, s->gws_n, s->gflags, &s->gepoch, &s->m->n_gemmf_q8, nullptr, nullptr};
}

// ---------------------------------------------------------------------------
// The transformer layers of a pass of M > 1 rows, for every caller: encoder
// passes of one stream and of several, decoder prefills of one stream and of several, and the
// wide batched step.  rows_layers is the one place the launch sequence is written.
// ---------------------------------------------------------------------------
// One layer's tensors.  f*: the fragment-major copies (null until model_enc_frag / model_frag);
// s*: Q8 row scales (null: bf16); b*: biases (encoder; null in the decoder); ada: the layer's
// ada scale row (decoder; null in the encoder).
struct RowsLayer {
    const uint8_t *wqkv, *wo, *w13, *w2;
    const uint8_t *fqkv, *fo, *f13, *f2;
    const float *sqkv, *so, *s13, *s2;
    const float *bqkv, *bo, *b2;
    const float *attn_norm, *ffn_norm, *ada;
};
struct RowsStack {
    int D, Q, KV, hidden, layers;  // Q = heads x head_dim, KV = kv heads x head_dim
    float eps;
    RowsLayer (*layer)(const vox_hip_model_t* m, int l);
};
// The rows between the launches; the caller owns them.  xn, att, hid: the row-major form's
// normalised rows, wo input and w2 input; pa, pc: the plane form's two plane buffers.
struct RowsScratch {
    float *x, *qkv, *xn, *att, *hid;
    uint16_t *pa, *pc;
};
// Where a decoder pass takes its ada rows when not from the model's table (the layer
// descriptor's): table: another table [layers][D] for all rows (a stream's own delay); slots: row
// r from slots[r].ada (the wide batched step of a call with delays of its own: the per-slot norm
// instances)
struct RowsAda {
    const float* table = nullptr;
    const BatchSlot* slots = nullptr;
};

static RowsLayer enc_rows_layer(const vox_hip_model_t* m, int l) {
    const EncLayerD& L = m->enc[l];
    const DecFragD F = m->efrag.empty() ? DecFragD{} : m->efrag[l];
    return RowsLayer{L.wqkv, L.wo, L.w13, L.w2, F.wqkv, F.wo, F.w13, F.w2, L.sqkv, L.so, L.s13, L.s2,
                     L.bqkv, L.bo, L.b2, L.attn_norm, L.ffn_norm, nullptr};
}
static RowsLayer dec_rows_layer(const vox_hip_model_t* m, int l) {
    const DecLayerD& L = m->dec[l];
    const DecFragD F = m->dfrag.empty() ? DecFragD{} : m->dfrag[l];
    return RowsLayer{L.wqkv, L.wo, L.w13, L.w2, F.wqkv, F.wo, F.w13, F.w2, L.sqkv, L.so, L.s13, L.s2,
                     nullptr, nullptr, nullptr, L.attn_norm, L.ffn_norm, m->ada_scale + (size_t)l * m->c.dec_dim};
}
static RowsStack enc_rows_stack(const vox_hip_config_t& c) {
    return RowsStack{c.enc_dim, c.enc_heads * c.enc_head_dim, c.enc_kv_heads * c.enc_head_dim, c.enc_hidden, c.enc_layers,
                     c.enc_eps, enc_rows_layer};
}
static RowsStack dec_rows_stack(const vox_hip_config_t& c) {
    return RowsStack{c.dec_dim, c.dec_heads * c.dec_head_dim, c.dec_kv_heads * c.dec_head_dim, c.dec_hidden, c.dec_layers,
                     c.dec_eps, dec_rows_layer};
}

// Rows B.x[0..n) through the stack's layers in place, on queue q.st (encoder.c:562-684,
// decoder.c:509-606).  gf: the projections on k_gemmf over the fragment-major copies, their inputs
// written as planes by the producers (RMSNorm rows, the attention output, the W1|W3 SwiGLU
// epilogue); otherwise on launch_gemm (k_gemm2) over the row-major tensors, the same arithmetic.
// attn(l, planes): layer l's RoPE + K/V append + attention from B.qkv, its rows into B.att and /
// or, planes != null, as the wo input planes.
template <class Attn>
static int rows_layers(const vox_hip_model_t* m, const RowsStack& S, const RowsScratch& B, const GemmfQ& q, bool gf, int n,
                       Attn attn, const RowsAda& ada = RowsAda{}) {
    const int D = S.D, NQKV = S.Q + 2 * S.KV, HID = S.hidden;
    hipStream_t st = q.st;
    for (int l = 0; l < S.layers; l++) {
        RowsLayer L = S.layer(m, l);
        if (ada.table) L.ada = ada.table + (size_t)l * D;
        // RMSNorm, QKV (+ bias)
        if (gf) {
            CK(launch_rmsnorm_fplanes(B.x, n, D, L.attn_norm, nullptr, S.eps, B.pa, nullptr, 0, st));
            if (gemmf_on(q, EPI_STORE, B.pa, D, n, L.fqkv, L.sqkv, NQKV, L.bqkv, B.qkv, NQKV, nullptr)) return -1;
        } else {
            CK(launch_rmsnorm_rows(B.x, D, B.xn, D, L.attn_norm, nullptr, n, D, S.eps, st));
            CK(launch_gemm(EPI_STORE, 3, B.xn, D, L.wqkv, L.sqkv, D, n, NQKV, L.bqkv, B.qkv, NQKV, st, q.ws, q.ws_n));
        }
        if (attn(l, gf ? B.pa : nullptr)) return -1;
        // wo (+ bias) residual; RMSNorm (x (1 + ada)), W1|W3 with SwiGLU, w2 (+ bias) residual
        if (gf) {
            if (gemmf_on(q, EPI_RESID, B.pa, S.Q, n, L.fo, L.so, D, L.bo, B.x, D, nullptr)) return -1;
            if (ada.slots) CK(launch_rmsnorm_fplanes_slots(B.x, n, D, L.ffn_norm, ada.slots, (size_t)l * D, S.eps, B.pa, st));
            else CK(launch_rmsnorm_fplanes(B.x, n, D, L.ffn_norm, L.ada, S.eps, B.pa, nullptr, 0, st));
            if (gemmf_on(q, EPI_SWIGLU, B.pa, D, n, L.f13, L.s13, 2 * HID, nullptr, nullptr, HID, B.pc)) return -1;
            if (gemmf_on(q, EPI_RESID, B.pc, HID, n, L.f2, L.s2, D, L.b2, B.x, D, nullptr)) return -1;
        } else {
            CK(launch_gemm(EPI_RESID, 3, B.att, S.Q, L.wo, L.so, S.Q, n, D, L.bo, B.x, D, st, q.ws, q.ws_n));
            if (ada.slots) CK(launch_rmsnorm_rows_slots(B.x, D, B.xn, D, L.ffn_norm, ada.slots, (size_t)l * D, n, D, S.eps, st));
            else CK(launch_rmsnorm_rows(B.x, D, B.xn, D, L.ffn_norm, L.ada, n, D, S.eps, st));
            CK(launch_gemm(EPI_SWIGLU, 3, B.xn, D, L.w13, L.s13, D, n, 2 * HID, nullptr, B.hid, HID, st, q.ws, q.ws_n));
            CK(launch_gemm(EPI_RESID, 3, B.hid, HID, L.w2, L.s2, HID, n, D, L.b2, B.x, D, st, q.ws, q.ws_n));
        }
    }
    return 0;
}

// What a k_gemmf encoder pass on s's queue needs besides its row buffers: the fragment-major
// encoder copies, the stream's plane buffers (one pass of ENC_SUB rows) and hand-off flags
static int stream_enc_planes(vox_hip_stream_t* s) {
    const vox_hip_config_t& c = s->m->c;
    if (model_enc_frag(s->m)) return -1;
    if (!s->gpa) {
        const size_t rb = PLANE_MAX_ROWS / SK_ROWS;
        CK(dalloc(&s->gpa, rb * 3 * SK_ROWS * std::max(c.enc_dim, c.enc_heads * c.enc_head_dim)));
        CK(dalloc(&s->gpc, rb * 3 * SK_ROWS * c.enc_hidden));
    }
    if (!s->gflags) CK(dalloc(&s->gflags, gemmf_flag_ints()));
    return 0;
}
static RowsScratch enc_rows_scratch(vox_hip_stream_t* s, float* x) {
    return RowsScratch{x, s->qkv, s->xn, s->att, s->gate, s->gpa, s->gpc};
}

// A single new encoder row (the 1-frame final chunk of a one-shot clip, a live stream's odd
// frame): the decode GEMVs -- every weight byte read once at the weight-streaming rate, with
// the RMSNorm prologues and the bias / RoPE + K/V append / SwiGLU / residual epilogues
// (encoder.c:562-684) -- and the M > 1 attention kernel for the one query row.  Five
// launches per layer instead of the skinny chain's row blocks of 16.
static bool enc_gemv_ok(const vox_hip_model_t* m) {
    const vox_hip_config_t& c = m->c;
    const int ED = c.enc_dim, EQ = c.enc_heads * c.enc_head_dim, EKV = c.enc_kv_heads * c.enc_head_dim;
    const bool q8 = m->enc[0].sqkv != nullptr;
    return gemv_ok(EQ + 2 * EKV, ED, q8) && gemv_ok(ED, EQ, q8) && gemv_ok(2 * c.enc_hidden, ED, q8) &&
           gemv_ok(ED, c.enc_hidden, q8) && c.enc_head_dim % 2 == 0 && c.enc_hidden % 16 == 0;
}

static int run_encoder_row_gemv(vox_hip_stream_t* s, float* x, long long pos0, const float* rope) {
    vox_hip_model_t* m = s->m;
    const vox_hip_config_t& c = m->c;
    const int ED = c.enc_dim, H = c.enc_heads, KVH = c.enc_kv_heads, hd = c.enc_head_dim;
    const int EQ = H * hd, EKV = KVH * hd, EH = c.enc_hidden;
    const float scale = 1.0f / sqrtf((float)hd);
    hipStream_t st = s->st;
    for (int l = 0; l < c.enc_layers; l++) {
        const EncLayerD& L = m->enc[l];
        float* Kc = enc_ring(s, s->ek, l);
        float* Vc = enc_ring(s, s->ev, l);
        GemvArgs a;
        // RMSNorm -> QKV + bias -> RoPE -> K/V append (encoder.c:562-607)
        memset(&a, 0, sizeof a);
        a.x = x; a.K = ED; a.W = L.wqkv; a.wscale = L.sqkv; a.rows = EQ + 2 * EKV; a.bias = L.bqkv;
        a.norm_w = L.attn_norm; a.eps = c.enc_eps; a.y = s->q;
        a.qd = EQ; a.kvd = EKV; a.hd = hd; a.pos = (int)pos0; a.rope = rope - (size_t)pos0 * hd;
        a.Kc = Kc; a.Vc = Vc; a.cap = s->ecap; a.kvt = s->ekvt;
        CK(launch_gemv(PRO_NORM, EPI_QKV_BIAS, a, st));
        // windowed attention of the one query (encoder.c:609-638)
        CK(launch_attn_rows_mf(hd, s->q, EQ, Kc, Vc, s->ecap, s->att, EQ, 1, H, KVH, (int)pos0, 0, c.enc_window, scale,
                               st, s->gws, s->gws_n, nullptr, s->ekvt));
        // wo + bias residual (encoder.c:640-644)
        memset(&a, 0, sizeof a);
        a.x = s->att; a.K = EQ; a.W = L.wo; a.wscale = L.so; a.rows = ED; a.bias = L.bo; a.y = x;
        CK(launch_gemv(PRO_NONE, EPI_RESID, a, st));
        // RMSNorm -> W1|W3 -> silu * up (encoder.c:646-676)
        memset(&a, 0, sizeof a);
        a.x = x; a.K = ED; a.W = L.w13; a.wscale = L.s13; a.rows = 2 * EH; a.norm_w = L.ffn_norm; a.eps = c.enc_eps;
        a.y = s->gate;
        CK(launch_gemv(PRO_NORM, EPI_SWIGLU, a, st));
        // w2 + bias residual (encoder.c:678-684)
        memset(&a, 0, sizeof a);
        a.x = s->gate; a.K = EH; a.W = L.w2; a.wscale = L.s2; a.rows = ED; a.bias = L.b2; a.y = x;
        CK(launch_gemv(PRO_NONE, EPI_RESID, a, st));
    }
    CK(launch_rmsnorm_rows(x, ED, x, ED, m->enc_norm, nullptr, 1, ED, c.enc_eps, st));
    return 0;
}

static int enc_skinny_env() {
    static const int v = env_on("VOX_HIP_ENC_SKINNY");
    return v;
}

static int run_encoder_rows(vox_hip_stream_t* s, float* x, int n, long long pos0, const float* rope) {
    vox_hip_model_t* m = s->m;
    const vox_hip_config_t& c = m->c;
    const int ED = c.enc_dim, H = c.enc_heads, KVH = c.enc_kv_heads, hd = c.enc_head_dim;
    const int EQ = H * hd, EKV = KVH * hd;
    const float scale = 1.0f / sqrtf((float)hd);
    hipStream_t st = s->st;
    if (n > ENC_SUB) return set_err("encoder pass of %d rows > %d", n, ENC_SUB);
    if (n == 1 && enc_gemv_ok(m)) {
        s->enc_paths[0]++;
        return run_encoder_row_gemv(s, x, pos0, rope);
    }
    if (n <= enc_skinny_rows() && enc_skinny_env() && enc_skinny_ok(c)) return run_encoder_rows_skinny(s, x, n, pos0, rope);
    s->enc_paths[3]++;
    const bool gf = enc_gemmf_ok(m, n);
    if (gf && stream_enc_planes(s)) return -1;
    // RoPE + K/V append (encoder.c:562-607), windowed attention (:609-638)
    if (rows_layers(m, enc_rows_stack(c), enc_rows_scratch(s, x), stream_gemmfq(s), gf, n, [&](int l, uint16_t* planes) -> int {
            float* Kc = enc_ring(s, s->ek, l);
            float* Vc = enc_ring(s, s->ev, l);
            CK(launch_rope_kv(s->qkv, n, EQ, EKV, hd, rope, (int)pos0, s->q, Kc, Vc, s->ecap, st, s->ekvt));
            CK(launch_attn_rows_mf(hd, s->q, EQ, Kc, Vc, s->ecap, s->att, EQ, n, H, KVH, (int)pos0, 0, c.enc_window, scale,
                                   st, s->gws, s->gws_n, planes, s->ekvt));
            return 0;
        }))
        return -1;
    CK(launch_rmsnorm_rows(x, ED, x, ED, m->enc_norm, nullptr, n, ED, c.enc_eps, st));
    return 0;
}

// The model's rope tables cover last_pos.  Growing them waits for the whole device and moves
// the tables.  An encoder pass enqueued inside a begun batched call (the scheduler's steps-first
// order) can get here: the wait then covers the call's chunk in flight too, which is deliberate
// -- the old tables are freed only once nothing reads them, and batch_run captures its graphs
// again when rope_gen moved, so the later chunks read the new ones.  The overlap of that one
// run is lost; the tables double, so this happens a handful of times per process.
static int ensure_rope(vox_hip_stream_t* s, long long last_pos) {
    vox_hip_model_t* m = s->m;
    if (last_pos < m->rope_positions) return 0;
    int p = m->rope_positions;
    while (p <= last_pos) p *= 2;
    CK(hipDeviceSynchronize());
    if (model_rope_tables(m, p)) return -1;
    s->graph_ready = 0;
    return 0;
}

// stream_run_encoder in three phases, so a batch of streams can share the layer passes
// (vox_hip_stream_encode_mel_batch): (1) conv stem of n new mel frames on the stream's queue,
// *T1 encoder rows left at *xin (-1 error); (2) the 32 layers over those rows; (3) 4x
// downsample + adapter, returning the adapter rows added.
static int enc_prefix(vox_hip_stream_t* s, const float* mel, int n, int mel_on_device, int* T1o, float** xino) {
    vox_hip_model_t* m = s->m;
    const vox_hip_config_t& c = m->c;
    const int MB = c.mel_bins, ED = c.enc_dim;
    hipStream_t st = s->st;
    *T1o = 0;
    *xino = nullptr;
    if (n <= 0) return 0;
    if (stream_alloc_frames(s, n + 4)) return -1;
    // ---- conv0 over [mel_tail(2) | new n] (voxtral.c:594-651) ----
    CK(hipMemcpyAsync(s->mel_p, s->mel_tail, (size_t)2 * MB * 4, hipMemcpyDeviceToDevice, st));
    CK(hipMemcpyAsync(s->mel_p + (size_t)2 * MB, mel, (size_t)n * MB * 4,
                      mel_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    CK(launch_mel_tail(s->mel_p, n, MB, s->mel_tail, st));
    // c0_p rows: [c0_tail(2) | residual(res_count) | conv0 new (n)]
    CK(hipMemcpyAsync(s->c0_p, s->c0_tail, (size_t)2 * ED * 4, hipMemcpyDeviceToDevice, st));
    if (s->res_count)
        CK(hipMemcpyAsync(s->c0_p + (size_t)2 * ED, s->c0_res, (size_t)ED * 4, hipMemcpyDeviceToDevice, st));
    float* c0_new = s->c0_p + (size_t)(2 + s->res_count) * ED;
    CK(launch_im2col3(s->mel_p, MB, n, 1, 0, s->im2col, st));
    CK(launch_gemm(c.gelu_erf ? EPI_GELU_ERF : EPI_GELU, 3, s->im2col, MB * 3, m->conv0_w, nullptr, MB * 3, n, ED,
                   m->conv0_b, c0_new, ED, st, s->gws, s->gws_n));
    // ---- stride alignment (voxtral.c:653-692) ----
    const int total = s->res_count + n;
    const int new_res = total & 1;
    const int feed = total - new_res;
    if (new_res)
        CK(hipMemcpyAsync(s->c0_res, s->c0_p + (size_t)(2 + total - 1) * ED, (size_t)ED * 4,
                          hipMemcpyDeviceToDevice, st));
    s->res_count = new_res;
    if (feed <= 0) return 0;
    // ---- conv1 over [c0_tail(2) | feed], first output discarded (voxtral.c:694-756) ----
    const int T1 = feed / 2;
    float* xin = s->x_enc + (size_t)4 * ED;  // 4 spare rows in front for the downsample residual
    CK(launch_im2col3(s->c0_p, ED, T1, 2, 1, s->im2col, st));
    CK(launch_gemm(c.gelu_erf ? EPI_GELU_ERF : EPI_GELU, 3, s->im2col, ED * 3, m->conv1_w, nullptr, ED * 3, T1, ED,
                   m->conv1_b, xin, ED, st, s->gws, s->gws_n));
    CK(hipMemcpyAsync(s->c0_tail, s->c0_p + (size_t)(2 + feed - 2) * ED, (size_t)2 * ED * 4,
                      hipMemcpyDeviceToDevice, st));
    if (ensure_rope(s, s->enc_pos + T1 + 1)) return -1;
    *T1o = T1;
    *xino = xin;
    return 0;
}

// enc_prefix for several streams at once, on lead's queue, the two conv GEMMs run once over
// every stream's rows (the conv weights read once per pass; 2 launches instead of 2 per
// stream).  Stream b's conv0 rows form segment [c0_tail(2) | residual (res) | new (n)] of one
// stacked buffer, laid out as enc_prefix's c0_p: the GEMM also computes the tail / residual
// rows (from stale im2col rows; rows are independent) and the true ones are copied over them;
// conv1 writes stream b's T1[b] encoder rows straight to X at its stacked offset.  Per row the
// same products as enc_prefix (voxtral.c:594-756).  Returns the stacked rows N (-1 error).
static const int CS_ROWS = 2 * ENC_SUB + 5 * VOX_MAX_BATCH;  // conv0 rows of a batched pass
static bool enc_prefix_batch_fits(vox_hip_stream_t* const* ss, const int* n, int B) {
    long long r0 = 0, r1 = 0;
    for (int b = 0; b < B; b++)
        if (n[b] > 0) {
            r0 += 2 + ss[b]->res_count + n[b];
            r1 += (ss[b]->res_count + n[b]) / 2;
        }
    return r0 <= CS_ROWS && r1 <= ENC_SUB;
}

static int enc_prefix_batch(vox_hip_stream_t* lead, vox_hip_stream_t* const* ss, const float* const* mels,
                            const int* n, int B, int mel_on_device, float* X, int* T1, int* off) {
    vox_hip_model_t* m = lead->m;
    const vox_hip_config_t& c = m->c;
    const int MB = c.mel_bins, ED = c.enc_dim;
    hipStream_t st = lead->st;
    if (!lead->cs_im) {
        CK(dalloc(&lead->cs_im, std::max((size_t)CS_ROWS * MB * 3, (size_t)ENC_SUB * ED * 3)));
        CK(dalloc(&lead->cs_c0, (size_t)CS_ROWS * ED));
    }
    std::vector<int> seg(B, 0), res(B, 0), tot(B, 0);
    int R0 = 0, N = 0;
    for (int b = 0; b < B; b++) {
        T1[b] = 0;
        off[b] = N;
        if (n[b] <= 0) continue;
        vox_hip_stream_t* s = ss[b];
        if (stream_alloc_frames(s, n[b] + 4)) return -1;
        seg[b] = R0;
        res[b] = s->res_count;
        tot[b] = s->res_count + n[b];
        R0 += 2 + s->res_count + n[b];
        const int feed = tot[b] - (tot[b] & 1);
        T1[b] = feed > 0 ? feed / 2 : 0;
        N += T1[b];
    }
    // the members' queues (their mel frames) before the lead's
    for (int b = 0; b < B; b++)
        if (ss[b] != lead && n[b] > 0) {
            CK(hipEventRecord(ss[b]->sev, ss[b]->st));
            CK(hipStreamWaitEvent(st, ss[b]->sev, 0));
        }
    // ---- conv0 (voxtral.c:594-651) over every stream's [mel_tail(2) | new n] ----
    for (int b = 0; b < B; b++) {
        if (n[b] <= 0) continue;
        vox_hip_stream_t* s = ss[b];
        CK(hipMemcpyAsync(s->mel_p, s->mel_tail, (size_t)2 * MB * 4, hipMemcpyDeviceToDevice, st));
        CK(hipMemcpyAsync(s->mel_p + (size_t)2 * MB, mels[b], (size_t)n[b] * MB * 4,
                          mel_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        CK(launch_mel_tail(s->mel_p, n[b], MB, s->mel_tail, st));
        CK(launch_im2col3(s->mel_p, MB, n[b], 1, 0, lead->cs_im + (size_t)(seg[b] + 2 + res[b]) * MB * 3, st));
    }
    CK(launch_gemm(c.gelu_erf ? EPI_GELU_ERF : EPI_GELU, 3, lead->cs_im, MB * 3, m->conv0_w, nullptr, MB * 3, R0, ED,
                   m->conv0_b, lead->cs_c0, ED, st, lead->gws, lead->gws_n));
    // the true tail / residual rows over the computed ones; the new residual row kept
    for (int b = 0; b < B; b++) {
        if (n[b] <= 0) continue;
        vox_hip_stream_t* s = ss[b];
        float* c0p = lead->cs_c0 + (size_t)seg[b] * ED;
        CK(hipMemcpyAsync(c0p, s->c0_tail, (size_t)2 * ED * 4, hipMemcpyDeviceToDevice, st));
        if (res[b]) CK(hipMemcpyAsync(c0p + (size_t)2 * ED, s->c0_res, (size_t)ED * 4, hipMemcpyDeviceToDevice, st));
        const int new_res = tot[b] & 1;
        if (new_res)
            CK(hipMemcpyAsync(s->c0_res, c0p + (size_t)(2 + tot[b] - 1) * ED, (size_t)ED * 4, hipMemcpyDeviceToDevice, st));
        s->res_count = new_res;
        // ---- conv1 im2col over [c0_tail(2) | feed], first output discarded (voxtral.c:694-756) ----
        if (T1[b] > 0) {
            const int feed = 2 * T1[b];
            CK(launch_im2col3(c0p, ED, T1[b], 2, 1, lead->cs_im + (size_t)off[b] * ED * 3, st));
            CK(hipMemcpyAsync(s->c0_tail, c0p + (size_t)feed * ED, (size_t)2 * ED * 4, hipMemcpyDeviceToDevice, st));
        }
    }
    if (N > 0)
        CK(launch_gemm(c.gelu_erf ? EPI_GELU_ERF : EPI_GELU, 3, lead->cs_im, ED * 3, m->conv1_w, nullptr, ED * 3, N, ED,
                       m->conv1_b, X, ED, st, lead->gws, lead->gws_n));
    for (int b = 0; b < B; b++)
        if (T1[b] > 0 && ensure_rope(ss[b], ss[b]->enc_pos + T1[b] + 1)) return -1;
    return N;
}

static int enc_suffix(vox_hip_stream_t* s, float* xin, int T1) {
    vox_hip_model_t* m = s->m;
    const vox_hip_config_t& c = m->c;
    const int ED = c.enc_dim, D = c.dec_dim;
    hipStream_t st = s->st;
    s->enc_pos += T1;
    // ---- 4x downsample with residual + adapter (voxtral.c:868-934, encoder.c:699-737) ----
    const int R = s->enc_res_count;
    const int tot = R + T1;
    const int usable = (tot / 4) * 4;
    const int left = tot - usable;
    int added = 0;
    if (usable > 0) {
        if (R) CK(hipMemcpyAsync(xin - (size_t)R * ED, s->enc_res, (size_t)R * ED * 4, hipMemcpyDeviceToDevice, st));
        const float* ain = xin - (size_t)R * ED;
        const int n4 = usable / 4;
        if (stream_alloc_adapter(s, s->total_adapter + n4)) return -1;
        for (int r0 = 0; r0 < n4; r0 += ENC_SUB / 4) {
            int nr = std::min(ENC_SUB / 4, n4 - r0);
            CK(launch_gemm(c.gelu_erf ? EPI_GELU_ERF : EPI_GELU, 3, ain + (size_t)r0 * 4 * ED, 4 * ED, m->ad0, m->ad0_s,
                           4 * ED, nr, D, nullptr, s->ad_mid, D, st, s->gws, s->gws_n));
            CK(launch_gemm(EPI_STORE, 3, s->ad_mid, D, m->ad1, m->ad1_s, D, nr, D, nullptr,
                           s->adapter + (size_t)(s->total_adapter + r0) * D, D, st, s->gws, s->gws_n));
        }
        s->total_adapter += n4;
        added = n4;
        if (left)
            CK(hipMemcpyAsync(s->enc_res, ain + (size_t)usable * ED, (size_t)left * ED * 4, hipMemcpyDeviceToDevice, st));
    } else if (T1 > 0) {
        // fewer than 4 rows in total: keep all of them (old residual followed by new rows)
        CK(hipMemcpyAsync(s->enc_res + (size_t)R * ED, xin, (size_t)T1 * ED * 4, hipMemcpyDeviceToDevice, st));
    }
    s->enc_res_count = left;
    return added;
}

// enc_suffix for several streams at once, on lead's queue: stream b's new encoder rows are
// X[off[b] ..+ T1[b]); its 4-row groups (residual rows first) are stacked into one adapter
// input, the two adapter projections run once over all of them (the adapter weights read once
// per pass instead of once per stream), and each stream's rows are copied to its adapter
// buffer.  Per row the same products as enc_suffix (voxtral.c:868-934).
static int enc_suffix_batch(vox_hip_stream_t* lead, const float* X, vox_hip_stream_t* const* ss, const int* T1,
                            const int* off, int B, int* added) {
    vox_hip_model_t* m = lead->m;
    const vox_hip_config_t& c = m->c;
    const int ED = c.enc_dim, D = c.dec_dim;
    hipStream_t st = lead->st;
    const size_t ain_rows = (size_t)ENC_SUB + 4 * VOX_MAX_BATCH;  // encoder rows (+ residuals)
    if (!lead->abatch) {
        CK(dalloc(&lead->abatch, ain_rows * ED));
        CK(dalloc(&lead->abatch_out, ain_rows / 4 * D));
    }
    std::vector<int> aoff(B, 0), n4v(B, 0);
    int NA = 0;  // stacked adapter rows
    // the stacked rows are bounded before any copy is queued; every adapter buffer was sized
    // before the pass was enqueued (vox_hip_stream_encode_mel_batch), so nothing here waits on a queue
    for (int b = 0; b < B; b++)
        if (T1[b] > 0) {
            const int tot = ss[b]->enc_res_count + T1[b];
            if (ss[b]->total_adapter + tot / 4 > ss[b]->adapter_cap) return set_err("enc_suffix_batch: adapter buffer");
            NA += tot / 4;
        }
    if ((size_t)NA * 4 > ain_rows) return set_err("enc_suffix_batch: %d adapter rows", NA);
    NA = 0;
    for (int b = 0; b < B; b++) {
        added[b] = 0;
        if (T1[b] <= 0) continue;
        vox_hip_stream_t* s = ss[b];
        s->enc_pos += T1[b];
        const int R = s->enc_res_count, tot = R + T1[b], usable = (tot / 4) * 4, left = tot - usable;
        const float* xb = X + (size_t)off[b] * ED;
        if (usable > 0) {
            float* dst = lead->abatch + (size_t)NA * 4 * ED;
            if (R) CK(hipMemcpyAsync(dst, s->enc_res, (size_t)R * ED * 4, hipMemcpyDeviceToDevice, st));
            CK(hipMemcpyAsync(dst + (size_t)R * ED, xb, (size_t)(usable - R) * ED * 4, hipMemcpyDeviceToDevice, st));
            if (left)
                CK(hipMemcpyAsync(s->enc_res, xb + (size_t)(usable - R) * ED, (size_t)left * ED * 4,
                                  hipMemcpyDeviceToDevice, st));
            aoff[b] = NA;
            n4v[b] = usable / 4;
            NA += usable / 4;
        } else {
            CK(hipMemcpyAsync(s->enc_res + (size_t)R * ED, xb, (size_t)T1[b] * ED * 4, hipMemcpyDeviceToDevice, st));
        }
        s->enc_res_count = left;
    }
    for (int r0 = 0; r0 < NA; r0 += ENC_SUB / 4) {
        const int nr = std::min(ENC_SUB / 4, NA - r0);
        CK(launch_gemm(c.gelu_erf ? EPI_GELU_ERF : EPI_GELU, 3, lead->abatch + (size_t)r0 * 4 * ED, 4 * ED, m->ad0,
                       m->ad0_s, 4 * ED, nr, D, nullptr, lead->ad_mid, D, st, lead->gws, lead->gws_n));
        CK(launch_gemm(EPI_STORE, 3, lead->ad_mid, D, m->ad1, m->ad1_s, D, nr, D, nullptr,
                       lead->abatch_out + (size_t)r0 * D, D, st, lead->gws, lead->gws_n));
    }
    for (int b = 0; b < B; b++) {
        if (!n4v[b]) continue;
        vox_hip_stream_t* s = ss[b];
        CK(hipMemcpyAsync(s->adapter + (size_t)s->total_adapter * D, lead->abatch_out + (size_t)aoff[b] * D,
                          (size_t)n4v[b] * D * 4, hipMemcpyDeviceToDevice, st));
        s->total_adapter += n4v[b];
        added[b] = n4v[b];
    }
    return 0;
}

// The 32 encoder layers over the stacked new rows of several streams (row block b = rows
// [off[b], off[b] + nr[b]) of X belongs to ss[b], at its logical positions from pos0[b]): one
// rows_layers call over all rows (every weight byte read once for the batch) whose attention
// step runs RoPE + K/V append and the windowed attention per stream against its own ring.
// Launched on lead->st with lead's scratch (ENC_SUB rows); the caller orders the streams.
static int run_encoder_rows_batch(vox_hip_stream_t* lead, float* X, int N, vox_hip_stream_t* const* ss,
                                  const int* off, const int* nr, const long long* pos0, int B) {
    vox_hip_model_t* m = lead->m;
    const vox_hip_config_t& c = m->c;
    const int ED = c.enc_dim, H = c.enc_heads, KVH = c.enc_kv_heads, hd = c.enc_head_dim;
    const int EQ = H * hd, EKV = KVH * hd;
    const float scale = 1.0f / sqrtf((float)hd);
    hipStream_t st = lead->st;
    const bool gf = enc_gemmf_ok(m, N);
    if (gf && stream_enc_planes(lead)) return -1;
    EncRows er;
    memset(&er, 0, sizeof er);
    er.B = B;
    for (int b = 0; b < B; b++) {
        er.off[b] = off[b];
        er.nr[b] = nr[b];
        er.pos0[b] = (int)pos0[b];
    }
    // every stream's RoPE + K/V append and attention in one launch each (row offsets)
    if (rows_layers(m, enc_rows_stack(c), enc_rows_scratch(lead, X), stream_gemmfq(lead), gf, N, [&](int l, uint16_t* planes) -> int {
            for (int b = 0; b < B; b++) {
                er.Kc[b] = enc_ring(ss[b], ss[b]->ek, l);
                er.Vc[b] = enc_ring(ss[b], ss[b]->ev, l);
            }
            // (one ring type per pass: vox_hip_stream_encode_mel_batch groups the streams by it)
            CK(launch_rope_kv_rows(lead->qkv, N, EQ, EKV, hd, m->rope_enc, er, lead->q, lead->ecap, st, lead->ekvt));
            CK(launch_attn_rows(hd, lead->q, er, N, lead->ecap, lead->att, H, KVH, c.enc_window, scale, lead->gws,
                                lead->gws_n, st, planes, lead->ekvt));
            return 0;
        }))
        return -1;
    CK(launch_rmsnorm_rows(X, ED, X, ED, m->enc_norm, nullptr, N, ED, c.enc_eps, st));
    return 0;
}

// Several streams' new mel frames through one encoder pass (SURVEY 8f#1's batching applied
// to the encoder): each stream's conv stem on its own queue, then the stacked rows through the
// 32 layers once on ss[0]'s queue (weights read once for the batch), then each stream's
// downsample + adapter on its own queue; HIP events order the queues.  Falls back to one
// stream at a time when the stacked rows exceed one pass (ENC_SUB).  added[b] = adapter rows
// appended to stream b.  Synchronous unless every stream is in async-encode mode.
// encode_mel_batch_pass: the streams of one encoder ring type (one stacked pass, ss[0] leads).
// sync: wait for every stream's queue at the end unless all of them are in async-encode mode
// (false: the caller, which holds the whole list, does)
static int encode_mel_batch_pass(vox_hip_stream_t* const* ss, const float* const* mels, const int* n, int B,
                                 int mel_on_device, int* added, bool sync = true) {
    vox_hip_stream_t* lead = ss[0];
    const vox_hip_config_t& c = lead->m->c;
    const int ED = c.enc_dim;
    std::vector<int> T1(B), off(B);
    std::vector<float*> xin(B);
    std::vector<long long> pos0(B);
    int N = 0;
    bool all_async = true;
    // encoder rows each stream's frames complete (enc_prefix's stride alignment, on the host)
    int active = 0;
    for (int b = 0; b < B; b++) {
        all_async = all_async && ss[b]->enc_async;
        if (n[b] > 0) {
            const int tot = ss[b]->res_count + n[b];
            active += tot - (tot & 1) > 0;
        }
    }
    // several streams with rows: the conv stems stacked on the lead's queue (one GEMM per
    // conv for all of them, VOX_HIP_ENC_STEM_BATCH=0: one stream at a time), rows straight
    // into the stacked layer input
    static const int stem_batch = env_on("VOX_HIP_ENC_STEM_BATCH");
    const bool stacked = stem_batch && active > 1 && enc_prefix_batch_fits(ss, n, B);
    if (stacked) {
        if (!lead->xbatch) CK(dalloc(&lead->xbatch, (size_t)ENC_SUB * ED));
        N = enc_prefix_batch(lead, ss, mels, n, B, mel_on_device, lead->xbatch, T1.data(), off.data());
        if (N < 0) return -1;
        for (int b = 0; b < B; b++) pos0[b] = ss[b]->enc_pos;
    } else {
        for (int b = 0; b < B; b++) {
            if (enc_prefix(ss[b], mels[b], n[b], mel_on_device, &T1[b], &xin[b])) return -1;
            off[b] = N;
            pos0[b] = ss[b]->enc_pos;
            N += T1[b];
        }
    }
    if (!stacked && (N > ENC_SUB || active <= 1)) {
        // one stream at a time: rows beyond one pass, or a single stream with rows (its own
        // path keeps the skinny fused kernels for a short chunk)
        for (int b = 0; b < B; b++) {
            added[b] = 0;
            if (T1[b] <= 0) continue;
            for (int r0 = 0; r0 < T1[b]; r0 += ENC_SUB) {
                const int nrr = std::min(ENC_SUB, T1[b] - r0);
                const long long p0 = ss[b]->enc_pos + r0;
                if (run_encoder_rows(ss[b], xin[b] + (size_t)r0 * ED, nrr, p0, lead->m->rope_enc + (size_t)p0 * c.enc_head_dim))
                    return -1;
            }
            added[b] = enc_suffix(ss[b], xin[b], T1[b]);
            if (added[b] < 0) return -1;
        }
    } else {
        if (!stacked) {
            if (!lead->xbatch) CK(dalloc(&lead->xbatch, (size_t)ENC_SUB * ED));
            // the lead's queue waits for every member's conv stem (each stream's own reusable
            // event), stacks the rows, runs the layers
            for (int b = 1; b < B; b++) {
                CK(hipEventRecord(ss[b]->sev, ss[b]->st));
                CK(hipStreamWaitEvent(lead->st, ss[b]->sev, 0));
            }
            for (int b = 0; b < B; b++)
                if (T1[b] > 0)
                    CK(hipMemcpyAsync(lead->xbatch + (size_t)off[b] * ED, xin[b], (size_t)T1[b] * ED * 4,
                                      hipMemcpyDeviceToDevice, lead->st));
        }
        // adapter buffers sized now, before the pass is on the lead's queue: growing one later
        // (stream_alloc_adapter synchronises the stream's queue) would wait for the whole pass
        for (int b = 0; b < B; b++)
            if (T1[b] > 0 && stream_alloc_adapter(ss[b], ss[b]->total_adapter + (ss[b]->enc_res_count + T1[b]) / 4))
                return -1;
        if (run_encoder_rows_batch(lead, lead->xbatch, N, ss, off.data(), T1.data(), pos0.data(), B)) return -1;
        // downsample + adapter of every stream in one pass on the lead's queue; the members'
        // queues then wait for it
        if (enc_suffix_batch(lead, lead->xbatch, ss, T1.data(), off.data(), B, added)) return -1;
        CK(hipEventRecord(lead->sev, lead->st));
        for (int b = 1; b < B; b++) CK(hipStreamWaitEvent(ss[b]->st, lead->sev, 0));
    }
    if (sync && !all_async)
        for (int b = 0; b < B; b++) CK(hipStreamSynchronize(ss[b]->st));
    return 0;
}

// A list that mixes encoder ring types (vox_hip_model_set_enc_kv_dtype between the streams'
// creations): one stacked pass per type, each over its streams in list order with the type's
// first stream leading, the types (f32, half, FP8) in the order in which the list first names them.
// Every stream's own queue carries its work as in a single pass, and added[] keeps list order.
// Synchronous unless every listed stream, of any type, is in async-encode mode.
extern "C" int vox_hip_stream_encode_mel_batch(vox_hip_stream_t* const* ss, const float* const* mels, const int* n,
                                               int B, int mel_on_device, int* added) {
    if (B < 1 || !ss || !mels || !n || !added) return set_err("encode_mel_batch: bad arguments");
    if (B > VOX_MAX_BATCH) return set_err("encode_mel_batch: at most %d streams", VOX_MAX_BATCH);
    bool mixed = false, all_async = true;
    for (int b = 0; b < B; b++) {
        if (!ss[b] || ss[b]->m != ss[0]->m || ss[b]->ecap != ss[0]->ecap)
            return set_err("encode_mel_batch: streams of one model");
        all_async = all_async && ss[b]->enc_async;
        for (int j = 0; j < b; j++)
            if (ss[j] == ss[b]) return set_err("encode_mel_batch: stream listed twice");
        mixed = mixed || ss[b]->ekvt != ss[0]->ekvt;
    }
    if (!mixed) return encode_mel_batch_pass(ss, mels, n, B, mel_on_device, added);
    int order[3], ntypes = 0;  // the ring types in the order of their first stream
    for (int b = 0; b < B; b++) {
        int t = 0;
        while (t < ntypes && order[t] != ss[b]->ekvt) t++;
        if (t == ntypes) order[ntypes++] = ss[b]->ekvt;
    }
    for (int pass = 0; pass < ntypes; pass++) {
        std::vector<vox_hip_stream_t*> gs;
        std::vector<const float*> gm;
        std::vector<int> gn, gi;
        for (int b = 0; b < B; b++)
            if (ss[b]->ekvt == order[pass]) {
                gs.push_back(ss[b]);
                gm.push_back(mels[b]);
                gn.push_back(n[b]);
                gi.push_back(b);
            }
        std::vector<int> ga(gs.size(), 0);
        if (encode_mel_batch_pass(gs.data(), gm.data(), gn.data(), (int)gs.size(), mel_on_device, ga.data(), false))
            return -1;
        for (size_t i = 0; i < gi.size(); i++) added[gi[i]] = ga[i];
    }
    if (!all_async)
        for (int b = 0; b < B; b++) CK(hipStreamSynchronize(ss[b]->st));
    return 0;
}

extern "C" int vox_hip_stream_encode_mel(vox_hip_stream_t* s, const float* mel, int n, int mel_on_device) {
    const vox_hip_config_t& c = s->m->c;
    int T1 = 0;
    float* xin = nullptr;
    if (enc_prefix(s, mel, n, mel_on_device, &T1, &xin)) return -1;
    int added = 0;
    if (T1 > 0) {
        // ---- encoder (voxtral_encoder.c:495-693), sub-chunks through all layers ----
        for (int r0 = 0; r0 < T1; r0 += ENC_SUB) {
            int nr = std::min(ENC_SUB, T1 - r0);
            long long p0 = s->enc_pos + r0;
            if (run_encoder_rows(s, xin + (size_t)r0 * c.enc_dim, nr, p0,
                                 s->m->rope_enc + (size_t)p0 * c.enc_head_dim))
                return -1;
        }
        added = enc_suffix(s, xin, T1);
        if (added < 0) return -1;
    }
    if (!s->enc_async) CK(hipStreamSynchronize(s->st));
    return added;
}

extern "C" int vox_hip_stream_set_async_encode(vox_hip_stream_t* s, int on) {
    if (!s) return set_err("null stream");
    if (s->enc_async && !on) CK(hipStreamSynchronize(s->st));
    s->enc_async = on ? 1 : 0;
    return 0;
}

extern "C" int vox_hip_stream_adapter_tokens(vox_hip_stream_t* s) { return s->total_adapter; }

extern "C" int vox_hip_stream_adapter_stats(const vox_hip_stream_t* s, long long out3[3]) {
    if (!s || !out3) return set_err("stream_adapter_stats: null argument");
    out3[0] = s->adapter_cap;
    out3[1] = s->ad_grows;
    out3[2] = s->ad_grows_held;
    return 0;
}

extern "C" int vox_hip_stream_read_adapter(vox_hip_stream_t* s, int first, int n, float* out) {
    const int D = s->m->c.dec_dim;
    if (first < 0 || first + n > s->total_adapter) return set_err("adapter rows out of range");
    CK(hipMemcpyAsync(out, s->adapter + (size_t)first * D, (size_t)n * D * 4, hipMemcpyDeviceToHost, s->st));
    CK(hipStreamSynchronize(s->st));
    return 0;
}

// ---------------------------------------------------------------------------
// Decoder
// ---------------------------------------------------------------------------
// device state after the prompt's prefill rows 0..np-1: the next step reads row np with the
// streaming pad token (voxtral.c:1036-1061)
static int stream_prefilled(vox_hip_stream_t* s, hipStream_t q) {
    const int np = 32 + stream_delay(s);
    const int st4[4] = {np, np, TOKEN_STREAMING_PAD, s->n_generated};
    CK(hipMemcpyAsync(s->state, st4, sizeof st4, hipMemcpyHostToDevice, q));
    s->h_state[0] = np;
    s->h_state[1] = np;
    s->h_state[2] = TOKEN_STREAMING_PAD;
    s->h_state[3] = s->n_generated;
    s->started = 1;
    return 0;
}

// Decoder prefill rows on k_gemmf (bf16 weights): the projections read the fragment-major
// decoder copies of the batched path (model_frag) once per 64-row tile -- the 38-row prompt is
// one tile, where k_gemm2's 128 x 128 tiles were mostly padding and split K eight ways --, with
// the inputs written as planes by their producers (RMSNorm rows, the attention output, the
// W1|W3 SwiGLU epilogue), as the encoder's long passes do.
static int dec_gemmf_env() {
    // VOX_HIP_PREFILL_GEMMF=0: decoder prefills on k_gemm2 over the row-major weights (A/B, and
    // no fragment-major copies for a process that never batches)
    static const int v = env_on("VOX_HIP_PREFILL_GEMMF");
    return v;
}

static bool dec_gemmf_ok(const vox_hip_model_t* m, int n) {
    const vox_hip_config_t& c = m->c;
    const int DD = c.dec_dim, DQ = c.dec_heads * c.dec_head_dim, DKV = c.dec_kv_heads * c.dec_head_dim;
    return enc_gemmf_env() && dec_gemmf_env() && gemmf_fmt_ok(m, m->dec) && n >= 1 && n <= PLANE_MAX_ROWS && gemmf_ok(n, DQ + 2 * DKV, DD) &&
           gemmf_ok(n, DD, DQ) && gemmf_ok(n, 2 * c.dec_hidden, DD) && gemmf_ok(n, DD, c.dec_hidden) &&
           c.dec_hidden % 64 == 0;
}

static int stream_dec_planes(vox_hip_stream_t* s, int rows) {
    if (rows <= s->dp_rows) return 0;
    const vox_hip_config_t& c = s->m->c;
    const int DD = c.dec_dim, DQ = c.dec_heads * c.dec_head_dim;
    // whole 128-row tiles: k_gemmf reads every row block of a tile (rows past n are computed
    // and dropped)
    const int r = (rows + 127) / 128 * 128;
    dfree(s->dpa);
    dfree(s->dpc);
    s->dp_rows = 0;
    CK(dalloc(&s->dpa, (size_t)r * 3 * std::max(DD, DQ)));
    CK(dalloc(&s->dpc, (size_t)r * 3 * c.dec_hidden));
    if (!s->gflags) CK(dalloc(&s->gflags, gemmf_flag_ints()));
    s->dp_rows = r;
    return 0;
}

// the decoder rows of a pass led by s (its prefill scratch and planes), residual rows x
static RowsScratch dec_rows_scratch(vox_hip_stream_t* s, float* x) {
    return RowsScratch{x, s->qkvd, s->xnd, s->attd, s->gated, s->dpa, s->dpc};
}

// M>1 rows (prefill) at logical positions pos0.. (voxtral_decoder.c:496-606)
static int run_decoder_rows(vox_hip_stream_t* s, float* x, int n, int pos0, const float* rope) {
    vox_hip_model_t* m = s->m;
    const vox_hip_config_t& c = m->c;
    const int H = c.dec_heads, KVH = c.dec_kv_heads, hd = c.dec_head_dim;
    const int DQ = H * hd, DKV = KVH * hd;
    const float scale = 1.0f / sqrtf((float)hd);
    hipStream_t st = s->st;
    if (stream_alloc_dec_rows(s, n)) return -1;
    if (n > DEC_SLACK + 1 && pos0 > 0) return set_err("prefill of %d rows on a non-empty cache", n);
    // k_gemmf needs the fragment-major decoder copies (6.86 GB, made here on the first
    // prefill unless a batch made them) and the stream's plane buffers; when either cannot be
    // allocated the prefill takes the k_gemm2 form (same arithmetic, row-major weights)
    bool gf = n > 1 && dec_gemmf_ok(m, n);
    if (gf && (model_frag(m) || stream_dec_planes(s, n))) {
        vox_hip_clear_error();
        (void)hipGetLastError();  // the failed hipMalloc, so no later launch check reports it
        gf = false;
    }
    // (stream_dec_planes made the hand-off flags before the queue descriptor copies the pointer)
    return rows_layers(m, dec_rows_stack(c), dec_rows_scratch(s, x), stream_gemmfq(s), gf, n, [&](int l, uint16_t* planes) -> int {
        float* Kc = dec_ring(s, s->dk, l);
        float* Vc = dec_ring(s, s->dv, l);
        CK(launch_rope_kv(s->qkvd, n, DQ, DKV, hd, rope, pos0, s->qd_, Kc, Vc, s->dcap, st, s->kvt));
        CK(launch_attn_rows_mf(hd, s->qd_, DQ, Kc, Vc, s->dcap, s->attd, DQ, n, H, KVH, pos0, 0, c.dec_window, scale, st,
                               s->gws, s->gws_n, planes, s->kvt));
        return 0;
    }, RowsAda{s->delay < 0 ? nullptr : stream_ada(s), nullptr});
}

// The tensors a decode step streams (single-stream k_gemv and the R-row k_gemvr step): QKV, wo,
// W1|W3 and W2 of layer l, and the LM head (tied embeddings) as l == layers.  The one place that
// says what each is: matrix and Q8 scales, (rows, K), prologue / epilogue, norm weight and ada
// row, wpack13 and wmx4 planes.  The LM head's epilogue here is the batched steps' EPI_STORE; the
// single-stream step launches it with EPI_LOGITS[_ALT].
enum { T_QKV, T_WO, T_W13, T_W2 };
struct StepTensor {
    const uint8_t* W;
    const float* wscale;
    int rows, K, pro, epi;
    const float *norm_w, *ada;
    const WPackD* pack;
    const WMx4D* mx;
};
static StepTensor dec_step_tensor(const vox_hip_model_t* m, int l, int which) {
    const vox_hip_config_t& c = m->c;
    const int DD = c.dec_dim, DQ = c.dec_heads * c.dec_head_dim, DKV = c.dec_kv_heads * c.dec_head_dim, DH = c.dec_hidden;
    if (l == (int)m->dec.size())
        return StepTensor{m->tok_emb, m->tok_emb_s, c.vocab, DD, PRO_NORM, EPI_STORE, m->dec_norm, nullptr, &m->plm, &m->mlm};
    const DecLayerD& L = m->dec[l];
    switch (which) {
    case T_QKV: return StepTensor{L.wqkv, L.sqkv, DQ + 2 * DKV, DD, PRO_NORM, EPI_QKV, L.attn_norm, nullptr, &L.pqkv, &L.mqkv};
    case T_WO: return StepTensor{L.wo, L.so, DD, DQ, PRO_NONE, EPI_RESID, nullptr, nullptr, &L.po, &L.mo};
    case T_W13:
        return StepTensor{L.w13, L.s13, 2 * DH, DD, PRO_NORM_ADA, EPI_SWIGLU, L.ffn_norm, m->ada_scale + (size_t)l * DD,
                          &L.p13, &L.m13};
    default: return StepTensor{L.w2, L.s2, DD, DH, PRO_NONE, EPI_RESID, nullptr, nullptr, &L.p2, &L.m2};
    }
}
// f(tensor) over the 4 tensors of every layer and the LM head, until one returns false
template <class F>
static bool all_step_tensors(const vox_hip_model_t* m, F f) {
    const int nl = (int)m->dec.size();
    for (int l = 0; l <= nl; l++)
        for (int w = 0; w < (l < nl ? 4 : 1); w++)
            if (!f(dec_step_tensor(m, l, w))) return false;
    return true;
}
// a zeroed GemvArgs with the tensor's own fields: y = epi(W pro(x)); wmx4: its wmx4 plane, if any
static void step_tensor_args(GemvArgs& a, const StepTensor& t, const float* x, float* y, float eps, int wmx4) {
    memset(&a, 0, sizeof a);
    a.x = x; a.K = t.K; a.W = t.W; a.wscale = t.wscale; a.rows = t.rows; a.y = y;
    a.norm_w = t.norm_w; a.ada = t.ada; a.eps = t.norm_w ? eps : 0.f;
    wpack_args(a, *t.pack);
    if (wmx4) wmx4_args(a, *t.mx);
}

// One decoder step for the token whose input is already in s->xd[0..D).
// state != nullptr: positions come from device state (graph mode);
// otherwise pos/rope_row are host values (boundary twin).
static int enqueue_lm_head(vox_hip_stream_t* s, const int* state);

static int enqueue_step_layers(vox_hip_stream_t* s, const int* state, int pos, const float* rope_row,
                               int splits) {
    vox_hip_model_t* m = s->m;
    const vox_hip_config_t& c = m->c;
    const int H = c.dec_heads, KVH = c.dec_kv_heads, hd = c.dec_head_dim;
    const float scale = 1.0f / sqrtf((float)hd);
    hipStream_t st = s->st;
    for (int l = 0; l < c.dec_layers; l++) {
        float* Kc = dec_ring(s, s->dk, l);
        float* Vc = dec_ring(s, s->dv, l);
        GemvArgs a;
        // norm -> QKV -> RoPE -> KV append (decoder.c:709-722)
        StepTensor t = dec_step_tensor(m, l, T_QKV);
        step_tensor_args(a, t, s->xd, s->qd_, c.dec_eps, 1);
        a.qd = H * hd; a.kvd = KVH * hd; a.hd = hd;
        a.state = state; a.pos = pos;
        a.rope = state ? m->rope_dec : rope_row - (size_t)pos * hd;
        a.Kc = Kc; a.Vc = Vc; a.cap = s->dcap; a.kvt = s->kvt;
        CK(launch_gemv(t.pro, t.epi, a, st));
        // attention over the last min(pos+1, window) keys (decoder.c:724-733)
        CK(launch_attn_decode(hd, s->qd_, Kc, Vc, s->dcap, state, pos, c.dec_window, scale, H, KVH,
                              s->part, s->attd, splits, st, s->kvt));
        // wo + residual (decoder.c:735-740)
        t = dec_step_tensor(m, l, T_WO);
        step_tensor_args(a, t, s->attd, s->xd, c.dec_eps, 1);
        CK(launch_gemv(t.pro, t.epi, a, st));
        // norm * (1 + ada) -> W1|W3 -> silu * up (decoder.c:742-758)
        t = dec_step_tensor(m, l, T_W13);
        if (s->delay >= 0) t.ada = stream_ada(s) + (size_t)l * c.dec_dim;
        step_tensor_args(a, t, s->xd, s->gated, c.dec_eps, 1);
        // profiling: HIP events recorded by the W1|W3 launch's own dispatch (eager steps)
        const bool gprof = s->profiling && state && !s->capturing && (int)s->pev.size() == 2 * c.dec_layers;
        if (gprof) CK(launch_gemv_timed(t.pro, t.epi, a, s->pev[2 * l], s->pev[2 * l + 1], st));
        else CK(launch_gemv(t.pro, t.epi, a, st));
        // W2 + residual (decoder.c:758-760)
        t = dec_step_tensor(m, l, T_W2);
        step_tensor_args(a, t, s->gated, s->xd, c.dec_eps, 1);
        CK(launch_gemv(t.pro, t.epi, a, st));
    }
    return enqueue_lm_head(s, state);
}

// final norm + LM head (tied embeddings) + argmax partials (decoder.c:762-779)
static int enqueue_lm_head(vox_hip_stream_t* s, const int* state) {
    vox_hip_model_t* m = s->m;
    const StepTensor t = dec_step_tensor(m, m->c.dec_layers, 0);
    GemvArgs a;
    step_tensor_args(a, t, s->xd, s->logits, m->c.dec_eps, 1);
    a.part_val = s->pval; a.part_idx = s->pidx;
    a.part_alt = s->part_alt;
    CK(launch_gemv(t.pro, (state && s->n_alt > 1) ? EPI_LOGITS_ALT : EPI_LOGITS, a, s->st));
    return 0;
}

// Step graph g serves contexts of up to 2^g * ATT_BLOCK_KEYS keys (the last one: the whole
// window); graph 0 runs one attention block per query head and no combine kernel.
static int graph_splits(const vox_hip_stream_t* s, int g) {
    return std::min(1 << g, attn_maxsplits(s->m->c.dec_window));
}

static int graph_index(const vox_hip_stream_t* s, int ctx) {
    const int need = (ctx + ATT_BLOCK_KEYS - 1) / ATT_BLOCK_KEYS;
    int g = 0;
    while ((1 << g) < need && (1 << g) < attn_maxsplits(s->m->c.dec_window)) g++;
    return g;
}

static int enqueue_graph_step(vox_hip_stream_t* s, int splits) {
    const vox_hip_config_t& c = s->m->c;
    if (enqueue_step_layers(s, s->state, 0, nullptr, splits)) return -1;
    CK(launch_argmax_final(s->pval, s->pidx, lm_head_grid(s->m), s->state, s->tokens, s->tokens_cap,
                           s->adapter, s->adapter_cap, s->m->tok_emb, s->m->tok_emb_s, c.dec_dim, s->xd,
                           s->part_alt, s->n_alt > 1 ? s->alts : nullptr, c.vocab, s->st));
    return 0;
}

static int build_step_graph(vox_hip_stream_t* s, int gi) {
    if (s->step_exec[gi]) {
        hipGraphExecDestroy(s->step_exec[gi]);
        s->step_exec[gi] = nullptr;
    }
    hipGraph_t g = nullptr;
    CK(hipStreamBeginCapture(s->st, hipStreamCaptureModeThreadLocal));
    s->capturing = 1;
    int rc = enqueue_graph_step(s, graph_splits(s, gi));
    s->capturing = 0;
    hipError_t e = hipStreamEndCapture(s->st, &g);
    if (rc || e != hipSuccess) {
        if (g) hipGraphDestroy(g);
        return set_err("graph capture failed: %s", hipGetErrorString(e));
    }
    e = hipGraphInstantiate(&s->step_exec[gi], g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (e != hipSuccess) return set_err("graph instantiate failed: %s", hipGetErrorString(e));
    s->graph_ready |= 1 << gi;
    s->graph_alt = s->n_alt > 1;
    s->graph_rope_gen = s->m->rope_gen;
    return 0;
}

// Sampled kernel timing: after a batch of profiled steps, each layer's W1|W3 event pair
// (recorded by the kernel's dispatch packet) holds the last step's kernel duration.
static int collect_graph_profile(vox_hip_stream_t* s) {
    if (!s->profiling || !s->graph_prof) return 0;
    const vox_hip_config_t& c = s->m->c;
    for (int l = 0; l < c.dec_layers; l++) {
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, s->pev[2 * l], s->pev[2 * l + 1]));
        s->prof_ms += ms;
        s->prof_bytes += (double)2 * c.dec_hidden * c.dec_dim * 2;
        s->prof_launches++;
    }
    return 0;
}

static int use_graphs() {
    static const int v = env_on("VOX_HIP_GRAPH");
    return v;
}

// n steps starting at logical kv position pos0 (host mirror): the replayed graph is the one
// with the fewest attention key splits that covers the longest context of the n steps.
static int run_steps(vox_hip_stream_t* s, int n, int pos0) {
    const vox_hip_config_t& c = s->m->c;
    const int gi = graph_index(s, std::min(pos0 + n, c.dec_window));
    const int splits = graph_splits(s, gi);
    if (s->profiling && use_graphs() && n > 1) {
        // profiled batch: the first n - 1 steps replay the graph, the last one (whose W1|W3
        // events collect_graph_profile reads) runs eagerly below
        s->profiling = 0;
        const int rc = run_steps(s, n - 1, pos0);
        s->profiling = 1;
        if (rc) return -1;
        pos0 += n - 1;
        n = 1;
    }
    if (!use_graphs() || s->profiling) {
        // eager launches of the same device-state kernels: profiling (the W1|W3 launches
        // carry dispatch-recorded HIP events, which a graph cannot hold), profilers that
        // cannot follow graph replays (VOX_HIP_GRAPH=0).
        if (s->profiling && s->pev.empty()) {
            s->pev.resize(2 * c.dec_layers);
            for (auto& e : s->pev) CK(hipEventCreate(&e));
        }
        s->graph_prof = s->profiling;
        for (int i = 0; i < n; i++)
            if (enqueue_graph_step(s, splits)) return -1;
        return 0;
    }
    if (s->graph_ready && (s->graph_alt != (s->n_alt > 1) || s->graph_rope_gen != s->m->rope_gen)) s->graph_ready = 0;
    if (!(s->graph_ready & (1 << gi)) && build_step_graph(s, gi)) return -1;
    for (int i = 0; i < n; i++) CK(hipGraphLaunch(s->step_exec[gi], s->st));
    return 0;
}

// copy ring entries [first, first + n) of a per-step device log (rec ints / floats per entry)
template <class T>
static int ring_read(const T* ring, int cap, int rec, long long first, int n, T* out, hipStream_t st) {
    while (n > 0) {
        const int slot = (int)(first % cap);
        const int k = std::min(n, cap - slot);
        CK(hipMemcpyAsync(out, ring + (size_t)slot * rec, (size_t)k * rec * sizeof(T), hipMemcpyDeviceToHost, st));
        out += (size_t)k * rec;
        first += k;
        n -= k;
    }
    return 0;
}

// prompt embeds + prefill rows 0..prompt_len-2 (voxtral.c:1036-1057) on the stream's queue;
// the first generated token then comes from row prompt_len-1 through a regular step
static int stream_prefill(vox_hip_stream_t* s) {
    vox_hip_model_t* m = s->m;
    const int np = 32 + stream_delay(s);
    if (stream_alloc_dec_rows(s, np)) return -1;
    if (ensure_rope(s, np + 2)) return -1;
    CK(launch_embed_rows(s->adapter, m->tok_emb, m->tok_emb_s, 0, np, TOKEN_BOS, TOKEN_STREAMING_PAD, m->c.dec_dim,
                         s->xd, s->st));
    if (run_decoder_rows(s, s->xd, np, 0, m->rope_dec)) return -1;
    return stream_prefilled(s, s->st);
}

extern "C" int vox_hip_stream_decode(vox_hip_stream_t* s, int max_steps, int stop_at_eos,
                                     int* tokens_out, float* logits_out) {
    vox_hip_model_t* m = s->m;
    const vox_hip_config_t& c = m->c;
    const int D = c.dec_dim, V = c.vocab, hd = c.dec_head_dim;
    const int prompt_len = 1 + 32 + stream_delay(s);
    int produced = 0;
    if (s->held) return set_err("stream_decode: %s", HELD_MSG);
    if (max_steps <= 0 || s->eos_seen) return 0;
    if (!s->started && s->total_adapter < prompt_len) return 0;
    if (s->dslots0) {
        // a growing ring holds the call's last position before anything is enqueued: the prompt
        // if the decoder has not started, then min(max_steps, adapter rows left) steps
        const int pos = s->started ? s->h_state[0] : prompt_len - 1;
        const int left = s->total_adapter - (s->started ? s->h_state[1] : prompt_len - 1);
        if (stream_grow_dec(s, pos + std::max(0, std::min(max_steps, left)))) return -1;
    }
    if (!s->started && stream_prefill(s)) return -1;
    const int step_base = s->n_generated;
    int avail = s->total_adapter - (s->h_state[1] > 0 ? s->h_state[1] : prompt_len - 1);
    {
        // host mirror of the device state (positions advance by exactly one per step)
        int st4[4];
        CK(hipMemcpyAsync(st4, s->state, sizeof st4, hipMemcpyDeviceToHost, s->st));
        CK(hipStreamSynchronize(s->st));
        memcpy(s->h_state, st4, sizeof st4);
        avail = s->total_adapter - st4[1];
    }
    if (ensure_rope(s, (long long)s->h_state[0] + avail + 1)) return -1;
    // step input for the first step of this call (later inputs are built by the previous
    // step's argmax kernel)
    if (avail > 0) CK(launch_embed_step(s->adapter, m->tok_emb, m->tok_emb_s, s->state, D, s->xd, s->st));
    int todo = std::min(max_steps, avail);
    std::vector<int> tok;
    while (produced < todo) {
        int b = std::min(STEP_BATCH, todo - produced);
        if (logits_out) b = 1;
        if (run_steps(s, b, s->h_state[0] + produced)) return -1;
        tok.resize(produced + b);
        if (ring_read(s->tokens, s->tokens_cap, 1, (long long)step_base + produced, b, tok.data() + produced, s->st))
            return -1;
        if (logits_out)
            CK(hipMemcpyAsync(logits_out + (size_t)produced * V, s->logits, (size_t)V * 4, hipMemcpyDeviceToHost, s->st));
        CK(hipStreamSynchronize(s->st));
        if (collect_graph_profile(s)) return -1;
        int eos_at = -1;
        if (stop_at_eos)
            for (int i = produced; i < produced + b; i++)
                if (tok[i] == TOKEN_EOS) { eos_at = i; break; }
        if (eos_at >= 0) {
            produced = eos_at + 1;
            s->eos_seen = 1;
            break;
        }
        produced += b;
    }
    if (tokens_out) memcpy(tokens_out, tok.data(), (size_t)produced * 4);
    s->n_generated += produced;
    // host mirror; after an EOS the device ran ahead by at most one batch (never read again
    // in non-continuous mode, voxtral.c:1140-1144)
    s->h_state[0] += produced;
    s->h_state[1] += produced;
    if (produced) s->h_state[2] = tok[produced - 1];
    s->h_state[3] = s->n_generated;
    (void)hd;
    return produced;
}

// vox_stream_set_alt (voxtral.c:1329-1337)
extern "C" int vox_hip_stream_set_alt(vox_hip_stream_t* s, int n_alt, float cutoff) {
    if (!s) return -1;
    // (the call's slot names the alternatives ring by the mode the stream had at begin)
    if (s->held) return set_err("stream_set_alt: %s", HELD_MSG);
    if (n_alt < 1) n_alt = 1;
    if (n_alt > VOX_HIP_MAX_ALT) n_alt = VOX_HIP_MAX_ALT;
    if (cutoff < 0) cutoff = 0;
    if (cutoff > 1) cutoff = 1;
    s->n_alt = n_alt;
    s->alt_cutoff = cutoff;
    return 0;
}

// stream_fill_alts (voxtral.c:955-1010) for generated steps [first, first+n): the device
// left, per step, p_best and the three most probable text tokens other than the chosen
// one; the reference's acceptance rule is applied here.  ids_out [n][VOX_HIP_MAX_ALT]:
// [0] = the chosen token, then accepted alternatives, -1 after the first rejection (or
// beyond n_alt).  probs_out (optional) holds the matching softmax probabilities.
extern "C" int vox_hip_stream_read_alts(vox_hip_stream_t* s, int first, int n, int* ids_out,
                                        float* probs_out) {
    if (!s || first < 0 || n < 0 || first + n > s->n_generated || first < s->n_generated - s->tokens_cap)
        return set_err("alt range out of bounds (the last %d steps are kept)", s->tokens_cap);
    if (n == 0) return 0;
    std::vector<float> rec((size_t)n * ALT_REC);
    std::vector<int> tok(n);
    if (ring_read(s->alts, s->tokens_cap, ALT_REC, first, n, rec.data(), s->st) ||
        ring_read(s->tokens, s->tokens_cap, 1, first, n, tok.data(), s->st))
        return -1;
    CK(hipStreamSynchronize(s->st));
    for (int i = 0; i < n; i++) {
        int* ids = ids_out + (size_t)i * VOX_HIP_MAX_ALT;
        float* pr = probs_out ? probs_out + (size_t)i * VOX_HIP_MAX_ALT : nullptr;
        const float* r = rec.data() + (size_t)i * ALT_REC;
        for (int k = 0; k < VOX_HIP_MAX_ALT; k++) {
            ids[k] = -1;
            if (pr) pr[k] = 0.f;
        }
        ids[0] = tok[i];
        if (s->n_alt <= 1) continue;
        const float best_prob = r[0];
        if (pr) pr[0] = best_prob;
        if (best_prob <= 0) continue;
        for (int k = 1; k < s->n_alt; k++) {
            int id;
            memcpy(&id, &r[1 + 2 * (k - 1)], 4);
            const float p = r[2 + 2 * (k - 1)];
            if (id < 0) break;
            const float rr = 1.0f - p / best_prob;
            if (rr > s->alt_cutoff) break;
            ids[k] = id;
            if (pr) pr[k] = p;
        }
    }
    return 0;
}

extern "C" int vox_hip_stream_state(vox_hip_stream_t* s, int* out6) {
    out6[0] = s->h_state[0];
    out6[1] = s->h_state[1];
    out6[2] = s->h_state[2];
    out6[3] = s->started;
    out6[4] = s->eos_seen;
    out6[5] = s->n_generated;
    return 0;
}

// Raw ring elements of logical positions [first, first + n) of one decoder layer, in the
// stream's element type, [n][kv_heads * head_dim] each (k_out / v_out may be null).  The
// positions must still be resident: appended (< the stream's position) and not overwritten
// by the ring's wrap (>= position - ring capacity).  Waits for the stream's queue.
extern "C" int vox_hip_stream_read_kv(vox_hip_stream_t* s, int layer, int first, int n, void* k_out, void* v_out) {
    const vox_hip_config_t& c = s->m->c;
    const int pos = s->h_state[0];
    if (layer < 0 || layer >= c.dec_layers) return set_err("read_kv: layer %d of %d", layer, c.dec_layers);
    if (n < 0 || first < 0 || (long long)first + n > pos)
        return set_err("read_kv: positions [%d, %d + %d) not appended yet (stream at %d)", first, first, n, pos);
    if (first < pos - s->dcap)
        return set_err("read_kv: position %d already overwritten (stream at %d, ring of %d)", first, pos, s->dcap);
    CK(hipStreamSynchronize(s->st));
    const size_t row = (size_t)c.dec_kv_heads * c.dec_head_dim * kv_esize(s->kvt);
    void* outs[2] = {k_out, v_out};
    float* bases[2] = {s->dk, s->dv};
    for (int w = 0; w < 2; w++) {
        if (!outs[w]) continue;
        const char* ring = reinterpret_cast<const char*>(dec_ring(s, bases[w], layer));
        for (int i = 0; i < n;) {
            const int slot = (first + i) % s->dcap;
            const int run = std::min(n - i, s->dcap - slot);  // up to the ring's end
            CK(hipMemcpy(static_cast<char*>(outs[w]) + (size_t)i * row, ring + (size_t)slot * row, (size_t)run * row,
                         hipMemcpyDeviceToHost));
            i += run;
        }
    }
    return 0;
}

// The encoder twin of vox_hip_stream_read_kv: raw ring elements of logical encoder positions
// [first, first + n) of one encoder layer, in the stream's element type (f32, IEEE half or FP8 codes),
// [n][enc_kv_heads * enc_head_dim] each.  Waits for the stream's queue.
extern "C" int vox_hip_stream_read_enc_kv(vox_hip_stream_t* s, int layer, int first, int n, void* k_out, void* v_out) {
    if (!s) return set_err("read_enc_kv: null stream");
    const vox_hip_config_t& c = s->m->c;
    const long long pos = s->enc_pos;
    if (layer < 0 || layer >= c.enc_layers) return set_err("read_enc_kv: layer %d of %d", layer, c.enc_layers);
    if (n < 0 || first < 0 || (long long)first + n > pos)
        return set_err("read_enc_kv: positions [%d, %d + %d) not appended yet (stream at %lld)", first, first, n, pos);
    if (first < pos - s->ecap)
        return set_err("read_enc_kv: position %d already overwritten (stream at %lld, ring of %d)", first, pos, s->ecap);
    CK(hipStreamSynchronize(s->st));
    const size_t row = (size_t)c.enc_kv_heads * c.enc_head_dim * kv_esize(s->ekvt);
    void* outs[2] = {k_out, v_out};
    float* bases[2] = {s->ek, s->ev};
    for (int w = 0; w < 2; w++) {
        if (!outs[w]) continue;
        const char* ring = reinterpret_cast<const char*>(enc_ring(s, bases[w], layer));
        for (int i = 0; i < n;) {
            const int slot = (first + i) % s->ecap;
            const int run = std::min(n - i, s->ecap - slot);  // up to the ring's end
            CK(hipMemcpy(static_cast<char*>(outs[w]) + (size_t)i * row, ring + (size_t)slot * row, (size_t)run * row,
                         hipMemcpyDeviceToHost));
            i += run;
        }
    }
    return 0;
}

// The kernels' own FP8 ring store (element pairs and single elements) and load helpers over n
// values on the device: codes[i] = what a ring slot would hold for x[i], back[i] = what the
// attention kernels read from it (tests against vox_kv8.h; codes / back may be null).
extern "C" int vox_hip_kv8_convert(const float* x, int n, uint8_t* codes, float* back) {
    if (!g_inited && !vox_hip_init()) return -1;
    if (n < 0 || (n > 0 && !x)) return set_err("kv8_convert: bad arguments");
    if (n == 0) return 0;
    const size_t np = ((size_t)n + 7) / 8 * 8;  // whole 8-element groups (the kernel's unit)
    float *dx = nullptr, *db = nullptr;
    uint8_t* dc = nullptr;
    int rc = -1;
    do {
        if (hipMalloc((void**)&dx, np * 4) != hipSuccess || hipMalloc((void**)&db, np * 4) != hipSuccess ||
            hipMalloc((void**)&dc, np) != hipSuccess) {
            set_err("kv8_convert: out of device memory");
            break;
        }
        if (hipMemset(dx, 0, np * 4) != hipSuccess || hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess ||
            launch_kv8_convert(dx, (int)(np / 8), dc, db, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            (codes && hipMemcpy(codes, dc, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) ||
            (back && hipMemcpy(back, db, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess)) {
            set_err("kv8_convert: %s", hipGetErrorString(hipGetLastError()));
            break;
        }
        rc = 0;
    } while (0);
    if (dx) hipFree(dx);
    if (db) hipFree(db);
    if (dc) hipFree(dc);
    return rc;
}

extern "C" int vox_hip_stream_set_profiling(vox_hip_stream_t* s, int enable) {
    s->profiling = enable;
    s->prof_ms = 0;
    s->prof_bytes = 0;
    s->prof_launches = 0;
    return 0;
}

extern "C" int vox_hip_stream_profile(vox_hip_stream_t* s, double* out8) {
    out8[0] = s->prof_ms;
    out8[1] = s->prof_bytes;
    out8[2] = (double)s->prof_launches;
    out8[3] = s->prof_launches ? s->prof_ms / s->prof_launches : 0.0;
    out8[4] = 0;  // what the events bracket: the W1|W3 GEMV of every layer
    out8[5] = s->prof_launches ? s->prof_bytes / s->prof_launches : 0.0;
    // k_gemmf stage ranges an owner recomputed because a partial did not arrive in time
    int rec = 0;
    if (s->gflags) {
        CK(hipMemcpyAsync(&rec, s->gflags + gemmf_grid(), sizeof rec, hipMemcpyDeviceToHost, s->st));
        CK(hipStreamSynchronize(s->st));
    }
    out8[6] = rec;
    out8[7] = 0.0;
    return 0;
}

// ---------------------------------------------------------------------------
// Reference-boundary twins (host pointers; voxtral_metal.h)
//
// Any M, N, K: a weight is uploaded once per (host pointer, N, K) into a zero-padded
// [Np, Kp] device copy (Np a multiple of 128, Kp of 64: the k_gemm2 tile), the activation
// rows go into [M, Kp] with zero columns, and C comes back through a pitched copy, so the
// padding never reaches the caller.  M = 1 takes the GEMV when the padded shape suits it.
// Every HIP call is checked; the void functions report through vox_hip_last_error().
// ---------------------------------------------------------------------------
struct TwinW {
    uint8_t* w;   // [Np, Kp] bf16 or int8
    float* s;     // Q8 row scales [Np] (null: bf16)
    int N, K, Np, Kp;
};
struct TwinKey {
    const void* p;
    int n, k;
    bool operator==(const TwinKey& o) const { return p == o.p && n == o.n && k == o.k; }
};
struct TwinKeyHash {
    size_t operator()(const TwinKey& t) const {
        return std::hash<const void*>()(t.p) ^ ((size_t)t.n * 0x9e3779b97f4a7c15ull) ^ ((size_t)t.k << 1);
    }
};
static std::mutex g_twin_mu;
static std::unordered_map<TwinKey, TwinW, TwinKeyHash> g_wcache;  // (host ptr, N, K) -> device copy
static hipStream_t g_twin_st = nullptr;
static float* g_twin_ws = nullptr;  // split-K partials of the twin GEMMs
static float *g_tA = nullptr, *g_tC = nullptr, *g_tQ = nullptr, *g_tK = nullptr, *g_tV = nullptr, *g_tO = nullptr;
static size_t g_tA_n = 0, g_tC_n = 0, g_tQ_n = 0, g_tK_n = 0, g_tV_n = 0, g_tO_n = 0;
static float* g_tWs = nullptr;  // attention key-range partials
static size_t g_tWs_n = 0;

static int pad_to(int v, int a) { return (v + a - 1) / a * a; }

static int twin_buf(float** p, size_t* cap, size_t n) {
    if (n <= *cap) return 0;
    dfree(*p);
    *cap = 0;
    CK(dalloc(p, n));
    *cap = n;
    return 0;
}

// device copy of a host weight [N, K] (+ Q8 row scales), zero-padded to the GEMM tile
static const TwinW* twin_weight(const void* host, const float* scales, int N, int K) {
    if (!host || N <= 0 || K <= 0) {
        set_err("twin weight: null pointer or empty shape (%d x %d)", N, K);
        return nullptr;
    }
    const TwinKey key{host, N, K};
    auto it = g_wcache.find(key);
    if (it != g_wcache.end()) return &it->second;
    TwinW t{nullptr, nullptr, N, K, pad_to(N, 128), pad_to(K, 64)};
    const size_t esz = scales ? 1 : 2;
    hipError_t e = dalloc(&t.w, (size_t)t.Np * t.Kp * esz);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(t.w, (size_t)t.Kp * esz, host, (size_t)K * esz, (size_t)K * esz, N,
                             hipMemcpyHostToDevice, g_twin_st);
    if (e == hipSuccess && scales) {
        e = dalloc(&t.s, (size_t)t.Np);
        if (e == hipSuccess) e = hipMemcpyAsync(t.s, scales, (size_t)N * 4, hipMemcpyHostToDevice, g_twin_st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g_twin_st);
    if (e != hipSuccess) {
        dfree(t.w);
        dfree(t.s);
        set_err("twin weight upload (%d x %d): %s", N, K, hipGetErrorString(e));
        return nullptr;
    }
    return &(g_wcache[key] = t);
}

static int twin_init() {
    if (!g_inited && !vox_hip_init()) return -1;
    if (!g_twin_st) CK(hipStreamCreateWithFlags(&g_twin_st, hipStreamNonBlocking));
    if (!g_twin_ws) CK(dalloc(&g_twin_ws, GEMM_WS_ELEMS));
    return 0;
}

// host rows [M, K] -> device [M, Kp] (zero columns past K)
static int twin_put_rows(float** buf, size_t* cap, const float* host, int M, int K, int Kp) {
    if (!host) return set_err("twin: null input");
    if (twin_buf(buf, cap, (size_t)M * Kp)) return -1;
    if (Kp != K) {
        CK(hipMemsetAsync(*buf, 0, (size_t)M * Kp * 4, g_twin_st));
        CK(hipMemcpy2DAsync(*buf, (size_t)Kp * 4, host, (size_t)K * 4, (size_t)K * 4, M, hipMemcpyHostToDevice,
                            g_twin_st));
    } else {
        CK(hipMemcpyAsync(*buf, host, (size_t)M * K * 4, hipMemcpyHostToDevice, g_twin_st));
    }
    return 0;
}

// device [M, Np] -> host [M, N]
static int twin_get_rows(float* host, const float* dev, int M, int N, int Np) {
    if (!host) return set_err("twin: null output");
    CK(hipMemcpy2DAsync(host, (size_t)N * 4, dev, (size_t)Np * 4, (size_t)N * 4, M, hipMemcpyDeviceToHost, g_twin_st));
    return 0;
}

// dC[M, W.Np] = dA[M, W.Kp] . W^T on the twin stream
static int twin_gemm_dev(int M, const float* dA, const TwinW& W, float* dC) {
    if (M == 1 && gemv_ok(W.Np, W.Kp, W.s != nullptr)) {
        GemvArgs a;
        memset(&a, 0, sizeof a);
        a.x = dA; a.K = W.Kp; a.W = W.w; a.wscale = W.s; a.rows = W.Np; a.y = dC;
        CK(launch_gemv(PRO_NONE, EPI_STORE, a, g_twin_st));
        return 0;
    }
    CK(launch_gemm(EPI_STORE, 3, dA, W.Kp, W.w, W.s, W.Kp, M, W.Np, nullptr, dC, W.Np, g_twin_st, g_twin_ws,
                   GEMM_WS_ELEMS));
    return 0;
}

static int twin_sgemm(int M, int N, int K, const float* A, const void* B, const float* scales, float* C) {
    if (M <= 0 || N <= 0 || K <= 0) return M == 0 ? 0 : set_err("sgemm: bad shape %d x %d x %d", M, N, K);
    if (twin_init()) return -1;
    const TwinW* W = twin_weight(B, scales, N, K);
    if (!W) return -1;
    if (twin_put_rows(&g_tA, &g_tA_n, A, M, K, W->Kp) || twin_buf(&g_tC, &g_tC_n, (size_t)M * W->Np) ||
        twin_gemm_dev(M, g_tA, *W, g_tC) || twin_get_rows(C, g_tC, M, N, W->Np))
        return -1;
    CK(hipStreamSynchronize(g_twin_st));
    return 0;
}

// Test entry: y = W x for one bf16 matrix [rows, K] through k_gemv's STORE instance, from the
// wpack13 planes (packed = 1), the wmx4 plane (packed = 2) or the raw rows.  Returns 1 when the
// wpack13 instance ran, 2 when the wmx4 instance ran, 0 when the raw one did (packed = 0, or W
// outside the format's window / not MXFP4-valued), -1 on error.
extern "C" int vox_hip_gemv_wpack(int rows, int K, const uint16_t* W, const float* x, float* y, int packed) {
    std::lock_guard<std::mutex> lk(g_twin_mu);
    if (!W || !x || !y) return set_err("gemv_wpack: null argument");
    if (!gemv_ok(rows, K, 0)) return set_err("gemv_wpack: shape %d x %d is not a GEMV shape", rows, K);
    if (twin_init()) return -1;
    uint8_t* dW = nullptr;
    float *dx = nullptr, *dy = nullptr;
    if (packed < 0 || packed > 2) return set_err("gemv_wpack: packed must be 0, 1 or 2 (got %d)", packed);
    WPackD P = {nullptr, nullptr, 0};
    WMx4D M = {nullptr, nullptr};
    vox_hip_wpack_stats_t S;
    vox_hip_wmx4_stats_t MS;
    memset(&S, 0, sizeof S);
    memset(&MS, 0, sizeof MS);
    auto run = [&]() -> int {
        CK(dalloc(&dW, (size_t)rows * K * 2));
        CK(dalloc(&dx, (size_t)K));
        CK(dalloc(&dy, (size_t)rows));
        if (upload(dW, W, (size_t)rows * K * 2) || upload(dx, x, (size_t)K * 4)) return -1;
        if (wpack_make(packed == 1, S, &P, W, rows, K, 0)) return -1;
        if (wmx4_make(packed == 2, MS, &M, W, rows, K, 0)) return -1;
        GemvArgs a;
        memset(&a, 0, sizeof a);
        a.x = dx; a.K = K; a.W = dW; a.rows = rows; a.y = dy;
        wpack_args(a, P);
        a.wm_plane = M.plane;
        CK(launch_gemv(PRO_NONE, EPI_STORE, a, g_twin_st));
        CK(hipStreamSynchronize(g_twin_st));
        CK(hipMemcpy(y, dy, (size_t)rows * 4, hipMemcpyDeviceToHost));
        return 0;
    };
    const int rc = run();
    const int ran = M.plane ? 2 : P.main ? 1 : 0;
    dfree(dW); dfree(dx); dfree(dy); dfree(P.main); dfree(P.side); dfree(M.plane);
    return rc ? -1 : ran;
}

// Test entry: y[R][rows] = W x[r] for R in 1..8 rows through k_gemvr's STORE instance of the
// bucket >= R (the bucket's unused rows are zero), from the wpack13 planes (packed = 1), the
// wmx4 plane built from W (packed = 2, as vox_hip_gemv_wpack) or the raw rows.  Returns flags:
// bit 0 the wpack13 instance ran, bit 1 the per-row summation order is k_gemv's (every shape:
// k_gemvr never splits K), bit 2 the wmx4 instance ran (clear, and the raw rows streamed, when W
// is not MXFP4-valued or the shape has no wmx4 instance); -1 on error.
extern "C" int vox_hip_gemv_rows(int rows, int K, const uint16_t* W, const float* x, int R, float* y, int packed) {
    std::lock_guard<std::mutex> lk(g_twin_mu);
    if (!W || !x || !y) return set_err("gemv_rows: null argument");
    if (R < 1 || R > GEMVR_MAX_ROWS) return set_err("gemv_rows: %d rows (1..%d)", R, GEMVR_MAX_ROWS);
    if (!gemvr_ok(PRO_NONE, EPI_STORE, rows, K)) return set_err("gemv_rows: no k_gemvr instance for %d x %d", rows, K);
    if (packed < 0 || packed > 2) return set_err("gemv_rows: packed must be 0, 1 or 2 (got %d)", packed);
    if (twin_init()) return -1;
    int Rb = 1;
    while (Rb < R) Rb *= 2;
    uint8_t* dW = nullptr;
    float *dx = nullptr, *dy = nullptr;
    WPackD P = {nullptr, nullptr, 0};
    WMx4D M = {nullptr, nullptr};
    vox_hip_wpack_stats_t S;
    vox_hip_wmx4_stats_t MS;
    memset(&S, 0, sizeof S);
    memset(&MS, 0, sizeof MS);
    auto run = [&]() -> int {
        CK(dalloc(&dW, (size_t)rows * K * 2));
        CK(dalloc(&dx, (size_t)Rb * K));
        CK(dalloc(&dy, (size_t)Rb * rows));
        CK(hipMemset(dx, 0, (size_t)Rb * K * 4));
        if (upload(dW, W, (size_t)rows * K * 2) || upload(dx, x, (size_t)R * K * 4)) return -1;
        if (wpack_make(packed == 1, S, &P, W, rows, K, 0)) return -1;
        if (wmx4_make(packed == 2 && gemvr_ok_mx4(PRO_NONE, EPI_STORE, rows, K), MS, &M, W, rows, K, 0)) return -1;
        GemvRArgs a;
        memset(&a, 0, sizeof a);
        a.g.x = dx; a.ldx = K; a.g.K = K; a.g.W = dW; a.g.rows = rows; a.g.y = dy; a.ldy = rows;
        wpack_args(a.g, P);
        wmx4_args(a.g, M);
        CK(launch_gemvr(PRO_NONE, EPI_STORE, Rb, a, g_twin_st));
        CK(hipStreamSynchronize(g_twin_st));
        CK(hipMemcpy(y, dy, (size_t)R * rows * 4, hipMemcpyDeviceToHost));
        return 0;
    };
    const int rc = run();
    const int ran = (P.main ? 1 : 0) | (M.plane ? 4 : 0);
    dfree(dW); dfree(dx); dfree(dy); dfree(P.main); dfree(P.side); dfree(M.plane);
    return rc ? -1 : (ran | 2);
}

// Test entries for Q8 rows (W int8 [rows][K], one f32 scale per row): y[R][rows] = scale * (W x[r])
// through k_gemvr's Q8 STORE instance of the bucket >= R (the bucket's unused rows are zero),
// and its single-row twin through k_gemv<WF_Q8>'s STORE instance.  0, or -1 on error.
static int gemv_q8_entry(const char* who, int rows, int K, const int8_t* W, const float* scales, const float* x, int R,
                         float* y, bool rowsk) {
    std::lock_guard<std::mutex> lk(g_twin_mu);
    if (!W || !scales || !x || !y) return set_err("%s: null argument", who);
    if (R < 1 || R > GEMVR_MAX_ROWS) return set_err("%s: %d rows (1..%d)", who, R, GEMVR_MAX_ROWS);
    if (rowsk ? !gemvr_ok_q8(PRO_NONE, EPI_STORE, rows, K) : !gemv_ok(rows, K, 1))
        return set_err("%s: no Q8 instance for %d x %d", who, rows, K);
    if (twin_init()) return -1;
    int Rb = 1;
    while (Rb < R) Rb *= 2;
    uint8_t* dW = nullptr;
    float *ds = nullptr, *dx = nullptr, *dy = nullptr;
    auto run = [&]() -> int {
        CK(dalloc(&dW, (size_t)rows * K));
        CK(dalloc(&ds, (size_t)rows));
        CK(dalloc(&dx, (size_t)Rb * K));
        CK(dalloc(&dy, (size_t)Rb * rows));
        CK(hipMemset(dx, 0, (size_t)Rb * K * 4));
        if (upload(dW, W, (size_t)rows * K) || upload(ds, scales, (size_t)rows * 4) || upload(dx, x, (size_t)R * K * 4))
            return -1;
        GemvRArgs a;
        memset(&a, 0, sizeof a);
        a.g.x = dx; a.ldx = K; a.g.K = K; a.g.W = dW; a.g.wscale = ds; a.g.rows = rows; a.g.y = dy; a.ldy = rows;
        if (rowsk) CK(launch_gemvr(PRO_NONE, EPI_STORE, Rb, a, g_twin_st));
        else CK(launch_gemv(PRO_NONE, EPI_STORE, a.g, g_twin_st));
        CK(hipStreamSynchronize(g_twin_st));
        CK(hipMemcpy(y, dy, (size_t)R * rows * 4, hipMemcpyDeviceToHost));
        return 0;
    };
    const int rc = run();
    dfree(dW); dfree(ds); dfree(dx); dfree(dy);
    return rc ? -1 : 0;
}

extern "C" int vox_hip_gemv_rows_q8(int rows, int K, const int8_t* W, const float* scales, const float* x, int R, float* y) {
    return gemv_q8_entry("gemv_rows_q8", rows, K, W, scales, x, R, y, true);
}

extern "C" int vox_hip_gemv_q8(int rows, int K, const int8_t* W, const float* scales, const float* x, float* y) {
    return gemv_q8_entry("gemv_q8", rows, K, W, scales, x, 1, y, false);
}

// Test entry: nb rows x [nb][K] against one bf16 matrix W [N][K] through the batched step's own
// launchers (include/voxtral_hip.h): planes by launch_split_fplanes, then launch_gemm_skl with
// pair = 1 and its slabs summed in slab order on the host (head = 0), or launch_gemm_skf /
// launch_gemm_skf2 (head = 1); fmt = 1 streams the wmx4 fragment plane.
extern "C" int vox_hip_skinny_wmx4(int N, int K, const uint16_t* W, const float* x, int nb, float* y, int fmt, int head) {
    std::lock_guard<std::mutex> lk(g_twin_mu);
    if (!W || !x || !y) return set_err("skinny_wmx4: null argument");
    if (nb < 1 || nb > VOX_MAX_BATCH) return set_err("skinny_wmx4: %d rows (1..%d)", nb, VOX_MAX_BATCH);
    if ((fmt != 0 && fmt != 1) || (head != 0 && head != 1)) return set_err("skinny_wmx4: fmt and head are 0 or 1");
    if (N < 64 || N % 64 || K < 64 || K % 64 || (!head && !skl_splits(K, N)))
        return set_err("skinny_wmx4: shape %d x %d is not a skinny GEMM shape", N, K);
    if (fmt && !vox_wmx4_scan_(W, N, K))
        return set_err("skinny_wmx4: the matrix is not MXFP4-valued inside the exponent window");
    if (twin_init()) return -1;
    const int S = head ? 1 : skl_splits(K, N), Z = 2;
    uint8_t *dW = nullptr, *dF = nullptr;
    float *dx = nullptr, *dout = nullptr;
    uint16_t* dxs = nullptr;
    const size_t nout = head ? (size_t)Z * SK_ROWS * N : (size_t)Z * S * SK_ROWS * N;
    std::vector<float> out(nout);
    auto run = [&]() -> int {
        if (fmt) {
            const size_t n = (size_t)N * K, words = (size_t)vox_wmx4_frag_words(N, K);
            std::vector<uint32_t> nib(n / 8), fp(words);
            std::vector<uint8_t> scl(n / VOX_WMX4_BLOCK);
            par_range(N, [&](long long r0, long long r1) { vox_wmx4_pack_rows(W, r0, r1, K, nib.data(), scl.data()); });
            par_range(N / 16, [&](long long g0, long long g1) { vox_wmx4_frag_groups(nib.data(), scl.data(), g0, g1, K, fp.data()); });
            CK(dalloc(&dF, words * 4));
            if (upload(dF, fp.data(), words * 4)) return -1;
        } else {
            CK(dalloc(&dW, (size_t)N * K * 2));
            if (upload(dW, W, (size_t)N * K * 2) || frag_copy(&dF, dW, N, K, 0)) return -1;
        }
        CK(dalloc(&dx, (size_t)nb * K));
        CK(dalloc(&dxs, (size_t)Z * 3 * SK_ROWS * K));
        CK(dalloc(&dout, nout));
        if (upload(dx, x, (size_t)nb * K * 4)) return -1;  // (dalloc zeroes: the planes of rows nb.. are 0)
        CK(launch_split_fplanes(dx, nb, K, dxs, g_twin_st));
        if (!head)
            CK(launch_gemm_skl(dxs, K, dF, nullptr, N, nb, dout, g_twin_st, nullptr, 0, 0.f, 1, fmt));
        else if (nb > SK_ROWS)
            CK(launch_gemm_skf2(dxs, K, dF, nullptr, N, nb, dout, N, g_twin_st, fmt));
        else
            CK(launch_gemm_skf(dxs, K, dF, nullptr, N, nb, dout, N, g_twin_st, fmt));
        CK(hipStreamSynchronize(g_twin_st));
        CK(hipMemcpy(out.data(), dout, nout * 4, hipMemcpyDeviceToHost));
        return 0;
    };
    const int rc = run();
    dfree(dW); dfree(dF); dfree(dx); dfree(dxs); dfree(dout);
    if (rc) return -1;
    for (int j = 0; j < nb; j++) {
        float* yr = y + (size_t)j * N;
        if (head) {
            memcpy(yr, out.data() + (size_t)j * N, (size_t)N * 4);
            continue;
        }
        // slabs [row block][s][16][N], added in slab order (psum)
        const float* p = out.data() + (size_t)(j >> 4) * S * SK_ROWS * N + (size_t)(j & 15) * N;
        for (int n = 0; n < N; n++) {
            float v = p[n];
            for (int sp = 1; sp < S; sp++) v += p[(size_t)sp * SK_ROWS * N + n];
            yr[n] = v;
        }
    }
    return 0;
}

// Test entry: M rows x [M][K] against one Q8 matrix (Wq [N][K] int8, scales [N]) through the
// engine's plane writer (launch_split_fplanes) and launch_gemmf with EPI_STORE, no bias, at the
// process's plane count (include/voxtral_hip.h).  fmt = 1: the int8 fragment copy with the
// scales; fmt = 0: the bf16 fragment copy of the same integers, no scale.
extern "C" int vox_hip_gemmf_q8_rows(int M, int N, int K, const float* x, const int8_t* Wq, const float* scales, float* y,
                                     int fmt) {
    std::lock_guard<std::mutex> lk(g_twin_mu);
    if (!x || !Wq || !y || (fmt && !scales)) return set_err("gemmf_q8_rows: null argument");
    if (fmt != 0 && fmt != 1) return set_err("gemmf_q8_rows: fmt is 0 or 1");
    if (!gemmf_ok(M, N, K) || M > PLANE_MAX_ROWS)
        return set_err("gemmf_q8_rows: k_gemmf does not take M %d N %d K %d (M 1..1024, N %% 128, K %% 64)", M, N, K);
    if (twin_init()) return -1;
    uint8_t *dW = nullptr, *dF = nullptr;
    float *dx = nullptr, *dy = nullptr, *ds = nullptr, *dws = nullptr;
    uint16_t* dxs = nullptr;
    int* dflags = nullptr;
    auto run = [&]() -> int {
        const size_t n = (size_t)N * K;
        if (fmt) {
            CK(dalloc(&dW, n));
            CK(dalloc(&ds, (size_t)N));
            if (upload(dW, Wq, n) || upload(ds, scales, (size_t)N * 4) || frag_copy(&dF, dW, N, K, 1)) return -1;
        } else {
            // every int8 is a bf16: the high half of its f32
            std::vector<uint16_t> wb(n);
            for (size_t i = 0; i < n; i++) {
                const float f = (float)Wq[i];
                uint32_t u;
                memcpy(&u, &f, 4);
                wb[i] = (uint16_t)(u >> 16);
            }
            CK(dalloc(&dW, n * 2));
            if (upload(dW, wb.data(), n * 2) || frag_copy(&dF, dW, N, K, 0)) return -1;
        }
        const size_t rows = (size_t)(M + 127) / 128 * 128;  // whole tiles (dalloc zeroes: rows past M are 0)
        const size_t ws_n = gemmf_ws_floats(gemmf_grid());
        CK(dalloc(&dx, (size_t)M * K));
        CK(dalloc(&dxs, rows * 3 * K));
        CK(dalloc(&dy, (size_t)M * N));
        CK(dalloc(&dws, ws_n));
        CK(dalloc(&dflags, gemmf_flag_ints()));
        if (upload(dx, x, (size_t)M * K * 4)) return -1;
        CK(launch_split_fplanes(dx, M, K, dxs, g_twin_st));
        CK(launch_gemmf(EPI_STORE, gemm_planes_np(), dxs, K, M, dF, N, nullptr, dy, N, nullptr, dws, ws_n, dflags, 1,
                        g_twin_st, nullptr, 0, fmt ? ds : nullptr));
        CK(hipStreamSynchronize(g_twin_st));
        CK(hipMemcpy(y, dy, (size_t)M * N * 4, hipMemcpyDeviceToHost));
        return 0;
    };
    const int rc = run();
    dfree(dW); dfree(dF); dfree(dx); dfree(dxs); dfree(dy); dfree(ds); dfree(dws); dfree(dflags);
    return rc ? -1 : 0;
}

extern "C" void vox_hip_sgemm_bf16(int M, int N, int K, const float* A, const uint16_t* B, float* C) {
    std::lock_guard<std::mutex> lk(g_twin_mu);
    twin_sgemm(M, N, K, A, B, nullptr, C);
}

extern "C" void vox_hip_sgemm_q8(int M, int N, int K, const float* A, const int8_t* B, const float* scales,
                                 float* C) {
    std::lock_guard<std::mutex> lk(g_twin_mu);
    if (!scales) { set_err("sgemm_q8: null scales"); return; }
    twin_sgemm(M, N, K, A, B, scales, C);
}

// voxtral_metal.m:1274-1414: the input uploaded once, three projections into three arrays
extern "C" void vox_hip_fused_qkv_bf16(int M, int K, const float* input, const uint16_t* wq, int Nq,
                                       const uint16_t* wk, int Nk, const uint16_t* wv, int Nv,
                                       float* q, float* k, float* v) {
    std::lock_guard<std::mutex> lk(g_twin_mu);
    if (M <= 0) return;
    if (twin_init()) return;
    const TwinW* W[3] = {twin_weight(wq, nullptr, Nq, K), twin_weight(wk, nullptr, Nk, K),
                         twin_weight(wv, nullptr, Nv, K)};
    if (!W[0] || !W[1] || !W[2]) return;
    float* outs[3] = {q, k, v};
    float* dO[3] = {nullptr, nullptr, nullptr};
    size_t* caps[3] = {&g_tQ_n, &g_tK_n, &g_tV_n};
    float** bufs[3] = {&g_tQ, &g_tK, &g_tV};
    if (twin_put_rows(&g_tA, &g_tA_n, input, M, K, W[0]->Kp)) return;
    for (int i = 0; i < 3; i++) {
        if (twin_buf(bufs[i], caps[i], (size_t)M * W[i]->Np) || twin_gemm_dev(M, g_tA, *W[i], *bufs[i])) return;
        dO[i] = *bufs[i];
    }
    for (int i = 0; i < 3; i++)
        if (twin_get_rows(outs[i], dO[i], M, W[i]->N, W[i]->Np)) return;
    if (hipStreamSynchronize(g_twin_st) != hipSuccess) set_err("fused_qkv: sync failed");
}

__global__ void k_silu_mul(float* g, const float* u, size_t n) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        float v = g[i];
        g[i] = v / (1.0f + expf(-v)) * u[i];
    }
}

// voxtral_metal.m:1416-1572: (silu(x w1^T) * x w3^T) w2^T; the caller adds the w2 bias
extern "C" void vox_hip_fused_ffn_bf16(int M, int dim, int hidden, const float* input,
                                       const uint16_t* w1, const uint16_t* w3, const uint16_t* w2,
                                       float* output) {
    std::lock_guard<std::mutex> lk(g_twin_mu);
    if (M <= 0) return;
    if (twin_init()) return;
    const TwinW* d1 = twin_weight(w1, nullptr, hidden, dim);
    const TwinW* d3 = twin_weight(w3, nullptr, hidden, dim);
    const TwinW* d2 = twin_weight(w2, nullptr, dim, hidden);
    if (!d1 || !d3 || !d2) return;
    // gate / up rows [M, Hp]; the padded hidden columns are silu(0) * 0 = 0 and meet the
    // zero K padding of w2
    const int Hp = d1->Np;
    if (d2->Kp != Hp) { set_err("fused_ffn: padded hidden %d != %d", d2->Kp, Hp); return; }
    if (twin_put_rows(&g_tA, &g_tA_n, input, M, dim, d1->Kp) || twin_buf(&g_tQ, &g_tQ_n, (size_t)M * Hp) ||
        twin_buf(&g_tK, &g_tK_n, (size_t)M * Hp) || twin_buf(&g_tC, &g_tC_n, (size_t)M * d2->Np) ||
        twin_gemm_dev(M, g_tA, *d1, g_tQ) || twin_gemm_dev(M, g_tA, *d3, g_tK))
        return;
    const size_t n = (size_t)M * Hp;
    hipLaunchKernelGGL(k_silu_mul, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_twin_st, g_tQ, g_tK, n);
    if (hipGetLastError() != hipSuccess) { set_err("fused_ffn: silu_mul launch failed"); return; }
    if (twin_gemm_dev(M, g_tQ, *d2, g_tC) || twin_get_rows(output, g_tC, M, dim, d2->Np)) return;
    if (hipStreamSynchronize(g_twin_st) != hipSuccess) set_err("fused_ffn: sync failed");
}

static int twin_attention(float* out, const float* Q, const float* K, const float* V, int seq_q, int seq_k,
                          int n_heads, int n_kv_heads, int head_dim, float scale, int window_size, int q_offset) {
    if (twin_init()) return -1;
    if (seq_q <= 0) return 0;
    if (!out || !Q || !K || !V) return set_err("encoder_attention: null pointer");
    if (q_offset < 0 || q_offset + seq_q > seq_k) return set_err("encoder_attention: queries beyond keys");
    if (n_kv_heads <= 0 || n_heads % n_kv_heads) return set_err("encoder_attention: heads %d / kv heads %d", n_heads, n_kv_heads);
    const size_t qn = (size_t)seq_q * n_heads * head_dim, kn = (size_t)seq_k * n_kv_heads * head_dim;
    if (twin_buf(&g_tQ, &g_tQ_n, qn) || twin_buf(&g_tK, &g_tK_n, kn) || twin_buf(&g_tV, &g_tV_n, kn) ||
        twin_buf(&g_tO, &g_tO_n, qn))
        return -1;
    CK(hipMemcpyAsync(g_tQ, Q, qn * 4, hipMemcpyHostToDevice, g_twin_st));
    CK(hipMemcpyAsync(g_tK, K, kn * 4, hipMemcpyHostToDevice, g_twin_st));
    CK(hipMemcpyAsync(g_tV, V, kn * 4, hipMemcpyHostToDevice, g_twin_st));
    const int W = window_size > 0 ? window_size : (1 << 30);
    // few query rows: the key-range split + combine path the streaming encoder takes
    float* ws = nullptr;
    size_t wsn = 0;
    if (n_heads * ((seq_q + 15) / 16) < 256) {
        wsn = (size_t)n_heads * seq_q * 16 * (head_dim + 2);
        if (twin_buf(&g_tWs, &g_tWs_n, wsn)) return -1;
        ws = g_tWs;
    }
    CK(launch_attn_rows_mf(head_dim, g_tQ, n_heads * head_dim, g_tK, g_tV, seq_k, g_tO, n_heads * head_dim, seq_q,
                         n_heads, n_kv_heads, q_offset, 0, W, scale, g_twin_st, ws, wsn));
    CK(hipMemcpyAsync(out, g_tO, qn * 4, hipMemcpyDeviceToHost, g_twin_st));
    CK(hipStreamSynchronize(g_twin_st));
    return 0;
}

extern "C" void vox_hip_encoder_attention(float* out, const float* Q, const float* K, const float* V,
                                          int seq_q, int seq_k, int n_heads, int n_kv_heads,
                                          int head_dim, float scale, int window_size, int q_offset) {
    std::lock_guard<std::mutex> lk(g_twin_mu);
    twin_attention(out, Q, K, V, seq_q, seq_k, n_heads, n_kv_heads, head_dim, scale, window_size, q_offset);
}

static int upload_rope_rows(vox_hip_stream_t* s, const float* rope, size_t n) {
    if (n > (size_t)s->rope_rows_cap) {
        dfree(s->rope_rows);
        CK(dalloc(&s->rope_rows, n));
        s->rope_rows_cap = (int)n;
    }
    CK(hipMemcpyAsync(s->rope_rows, rope, n * 4, hipMemcpyHostToDevice, s->st));
    return 0;
}

extern "C" int vox_hip_encoder_full_step(vox_hip_stream_t* s, float* x, int new_len,
                                         const float* rope_freqs, int logical_start) {
    const vox_hip_config_t& c = s->m->c;
    const int ED = c.enc_dim;
    if (stream_alloc_frames(s, 2 * new_len + 8)) return -1;
    float* xin = s->x_enc + (size_t)4 * ED;
    CK(hipMemcpyAsync(xin, x, (size_t)new_len * ED * 4, hipMemcpyHostToDevice, s->st));
    if (upload_rope_rows(s, rope_freqs, (size_t)new_len * c.enc_head_dim)) return -1;
    for (int r0 = 0; r0 < new_len; r0 += ENC_SUB) {
        int nr = std::min(ENC_SUB, new_len - r0);
        if (run_encoder_rows(s, xin + (size_t)r0 * ED, nr, (long long)logical_start + r0,
                             s->rope_rows + (size_t)r0 * c.enc_head_dim))
            return -1;
    }
    CK(hipMemcpyAsync(x, xin, (size_t)new_len * ED * 4, hipMemcpyDeviceToHost, s->st));
    CK(hipStreamSynchronize(s->st));
    return 0;
}

extern "C" int vox_hip_decoder_prefill_step(vox_hip_stream_t* s, float* x, int seq_len,
                                            const float* rope_freqs, int logical_start) {
    const vox_hip_config_t& c = s->m->c;
    if (s->held) return set_err("decoder_prefill_step: %s", HELD_MSG);
    if (s->dslots0 && stream_grow_dec(s, logical_start + seq_len)) return -1;
    if (stream_alloc_dec_rows(s, seq_len)) return -1;
    CK(hipMemcpyAsync(s->xd, x, (size_t)seq_len * c.dec_dim * 4, hipMemcpyHostToDevice, s->st));
    if (upload_rope_rows(s, rope_freqs, (size_t)seq_len * c.dec_head_dim)) return -1;
    if (run_decoder_rows(s, s->xd, seq_len, logical_start, s->rope_rows)) return -1;
    CK(hipMemcpyAsync(x, s->xd, (size_t)seq_len * c.dec_dim * 4, hipMemcpyDeviceToHost, s->st));
    CK(hipStreamSynchronize(s->st));
    return 0;
}

extern "C" void vox_hip_decoder_start(vox_hip_stream_t* s, const float* x, int dim) {
    if (!s || !x || dim != s->m->c.dec_dim) {
        set_err("decoder_start: dim %d != dec_dim", dim);
        return;
    }
    if (hipMemcpyAsync(s->xd, x, (size_t)dim * 4, hipMemcpyHostToDevice, s->st) != hipSuccess)
        set_err("decoder_start upload failed");
}

extern "C" void vox_hip_decoder_end(vox_hip_stream_t* s) {
    if (s && hipStreamSynchronize(s->st) != hipSuccess) set_err("decoder_end: stream sync failed");
}

extern "C" int vox_hip_decoder_full_step(vox_hip_stream_t* s, const float* rope_freqs, int logical_pos,
                                         float* logits) {
    const vox_hip_config_t& c = s->m->c;
    if (s->held) return set_err("decoder_full_step: %s", HELD_MSG);
    if (s->dslots0 && stream_grow_dec(s, logical_pos + 1)) return -1;
    if (upload_rope_rows(s, rope_freqs, (size_t)c.dec_head_dim)) return -1;
    const int ctx = std::min(logical_pos + 1, c.dec_window);
    if (enqueue_step_layers(s, nullptr, logical_pos, s->rope_rows, (ctx + ATT_BLOCK_KEYS - 1) / ATT_BLOCK_KEYS))
        return -1;
    // argmax into the twin's own state so the graph-mode device state is untouched
    int* tmp_state = s->twin_state;
    int st4[4] = {0, 0, 0, 0};
    CK(hipMemcpyAsync(tmp_state, st4, sizeof st4, hipMemcpyHostToDevice, s->st));
    CK(launch_argmax_final(s->pval, s->pidx, lm_head_grid(s->m), tmp_state, nullptr, 0, nullptr, 0,
                           nullptr, nullptr, c.dec_dim, nullptr, nullptr, nullptr, c.vocab, s->st));
    CK(hipMemcpyAsync(st4, tmp_state, sizeof st4, hipMemcpyDeviceToHost, s->st));
    if (logits) CK(hipMemcpyAsync(logits, s->logits, (size_t)c.vocab * 4, hipMemcpyDeviceToHost, s->st));
    CK(hipStreamSynchronize(s->st));
    return st4[2];
}

extern "C" void* vox_hip_device_upload(const void* host, size_t bytes) {
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) { set_err("device_upload: hipMalloc(%zu) failed", bytes); return nullptr; }
    if (h2d(d, host, bytes) != hipSuccess) { hipFree(d); set_err("device_upload: copy failed"); return nullptr; }
    return d;
}

extern "C" int vox_hip_device_free(void* dev) {
    CK(hipFree(dev));
    return 0;
}

// ---------------------------------------------------------------------------
// Cross-stream batched greedy decoding (C4).  Row i of every batch
// activation buffer belongs to stream i; the weight GEMMs run once per step for all rows
// (M = streams), attention / RoPE / KV append / argmax use each stream's own state, rings
// and adapter rows.  Each stream's device state and token log advance exactly as in
// vox_hip_stream_decode, so streams can switch between the two paths.
// ---------------------------------------------------------------------------
struct vox_hip_batch {
    vox_hip_model_t* m;
    int cap;
    // rows of the slot-indexed buffers (slot table, token log, x, q, att, logits, pval / pidx /
    // palt, attention partials): the capacity's bucket, 32 (cap <= 32), 64 or 128.  The skinny
    // step's own buffers (part, planes xp_*) hold VOX_MAX_BATCH rows at any capacity.
    int rows;
    hipStream_t st;
    float *x, *q, *att, *logits, *pval, *palt;
    float* part;     // split-K slabs of the current projection (k_skl), consumed by the next kernel
    float* ssq;      // row sums of squares per 256-column slice (k_resid_xw_fplanes -> k_skl)
    int* ticket;     // k_sklx slice tickets (W1|W3 with the SwiGLU folded in; VOX_HIP_BATCH_SWX=0: off)
    int* pidx;
    uint16_t *xp_d, *xp_q, *xp_h;  // skinny-GEMM inputs: [3][16][K] bf16 planes of the rows (fragment order)
    float* apart;    // decode-attention partials + arrival counters, apart_n floats per slot
    size_t apart_n;
    // the slot table (rows BatchSlot) followed by the token log [rows][BATCH_TOKLOG],
    // in device memory and mirrored in pinned host memory (one copy each way per step chunk)
    BatchSlot* slots;
    BatchSlot* hslots;
    // step graphs [ring element type][slot bucket 1, 2, 4, 8, 16, 32][attention splits bucket]: their kernel
    // arguments point at the slot table and the batch's buffers only, so they stay valid as
    // streams come and go; captured again only when the model's rope table moves
    // (wmx4: [3 wmx4 + element type], the two weight sources keep graphs of their own)
    // [mixed]: the steps of a call in which a stream carries a delay of its own launch the per-slot
    // norm instances, so they keep graphs of their own beside the plain calls'
    // [mixed + 2 ragged]: likewise the steps of a call in which a stream's decoder rings are shorter
    // than window + slack (vox_hip_model_set_kv_grow) launch the ragged attention instances
    hipGraphExec_t gexec[4][6][6][STEP_GRAPHS];
    int grope_gen;
    // the MFMA step streams the wmx4 fragment planes of the tensors that have one
    // (vox_hip_batch_set_wmx4); the graphs hold the weight pointers, hence the key above
    int wmx4;
    // the R-row GEMV step (batch_step_gemv): steps whose slot bucket is <= gemv_rows take it
    // (0: off).  Its graphs [element type][bucket 1, 2, 4, 8][splits bucket] have keys of their own, so
    // the mode changes between calls without a capture being dropped.
    int gemv_rows;
    float* hid;      // SwiGLU rows [GEMVR_MAX_ROWS][dec_hidden] (allocated when the mode is first set)
    // (gemv_wmx4: [3 gemv_wmx4 + element type], as gexec)
    hipGraphExec_t gvexec[6][4][STEP_GRAPHS];
    long long n_gemv_replays, n_gemv_rows, n_gemv_captures;
    // the GEMV step streams the wmx4 GEMV plane of every tensor that has one
    // (vox_hip_batch_set_gemv_wmx4); a tensor without one keeps its wpack13 or raw launch
    int gemv_wmx4;
    long long n_gemv_wmx4_replays;
    // the stacked prefill takes streams with 16-bit and one-byte rings too (default; 0: those
    // streams prefill one by one on their own queues, vox_hip_batch_set_prefill_kv)
    int prefill_kv;
    // rows of the last call (b->logits row i = stream luid[i], from its last step when llive[i])
    unsigned long long luid[VOX_MAX_SLOTS];
    int llive[VOX_MAX_SLOTS];
    int lnb;
    // the wide step (batch_step_wide: slot buckets 64 and 128, rows > VOX_MAX_BATCH only): QKV
    // rows, k_gemmf input planes [row block][3][16][K] (wpa: dec_dim / heads*head_dim columns,
    // wpc: dec_hidden), the row-major fallback's normalised and SwiGLU rows, hand-off flags of
    // its own and the device epoch word its captured k_gemmf launches add to their epochs;
    // graphs [ring element type][bucket 64, 128][attention splits bucket]
    float *wqkv, *wxn, *whid;
    uint16_t *wpa, *wpc;
    int* wflags;
    int* wepoch;
    hipGraphExec_t gwexec[4][3][2][STEP_GRAPHS];  // [mixed + 2 ragged], as gexec
    // the ragged steps' ring capacity per slot, device and pinned host (made by the first ragged
    // call; a batch that sees full rings only never allocates or reads them), their counters
    int* dcaps;
    int* hcaps;
    long long n_ragged_calls, n_ragged_replays, n_ragged_captures;
    int wide_q8;  // k_gemmf launches on int8 fragments in one wide step (set by batch_step_wide)
    long long n_calls, n_replays, n_rows, n_captures, n_prefill_passes, n_prefilled;
    // split-K workspace of the stacked prefills (not the lead stream's: with an encoder pass
    // running beside the batched steps, that stream's queue may be using its own), and the
    // k_gemmf partial-tile flags + epoch of the batch queue's prefill launches
    float* pgws;
    int* gflags;
    int gepoch;
    // a call begun by batch_begin and not yet finished (vox_hip_batch_begin_rows /
    // vox_hip_batch_finish): its streams, outputs and the steps left after the chunk in flight
    struct {
        int active, n, max_steps, stop_at_eos, K, nb, gb, gi, splits, kvt, done, k;
        int gemv;  // the call's steps take the GEMV path
        int mixed; // a stream of the call carries a delay of its own: the per-slot norm instances
        int ragged; // a stream of the call has rings shorter than the full size: the ragged attention instances
        vox_hip_stream_t* streams[VOX_MAX_SLOTS];
        int* tokens_out;
        int* counts_out;
    } call;
    // adapter buffers the begun call's members outgrew (stream_alloc_adapter): the slot table
    // still names them, so they live until the call's last wait (batch_release)
    float** parked;
    int n_parked, cap_parked;
};

static_assert(VOX_MAX_SLOTS == VOX_HIP_BATCH_MAX_SLOTS, "the public bound of vox_hip_batch_create");
static int* slot_toklog(BatchSlot* slots, int rows) { return reinterpret_cast<int*>(slots + rows); }
static size_t slot_bytes(int rows) { return (sizeof(BatchSlot) + sizeof(int) * BATCH_TOKLOG) * (size_t)rows; }

// The window of a begun call (batch_begin .. batch_finish).  Its slot table names each member's
// state, tokens, adapter, Kc, Vc, alts and ada buffers and is uploaded once, so until the call
// ends none of them may be freed or moved, and nothing else may advance a member's decoder:
// batch_hold marks the members (the stream entry points that would do either refuse a held
// stream; encoding stays allowed and parks an outgrown adapter buffer here), batch_release
// ends the window after the call's last wait on the batch queue.
static int batch_park(vox_hip_batch_t* b, float* p) {
    if (b->n_parked == b->cap_parked) {
        const int nc = b->cap_parked ? 2 * b->cap_parked : 16;
        float** np = static_cast<float**>(realloc(b->parked, sizeof(float*) * nc));
        if (!np) return set_err("batch: out of host memory for a parked adapter buffer");
        b->parked = np;
        b->cap_parked = nc;
    }
    b->parked[b->n_parked++] = p;
    return 0;
}
static void batch_hold(vox_hip_batch_t* b) {
    for (int i = 0; i < b->call.n; i++) b->call.streams[i]->held = b;
    b->m->begun_calls++;
}
static void batch_release(vox_hip_batch_t* b) {
    for (int i = 0; i < b->call.n; i++)
        if (b->call.streams[i]->held == b) b->call.streams[i]->held = nullptr;
    b->m->begun_calls--;
    for (int i = 0; i < b->n_parked; i++) dfree(b->parked[i]);
    b->n_parked = 0;
}

// pack one [N, K] matrix (bf16, or int8 when q8) into fragment order (k_frag_pack)
static int frag_copy(uint8_t** dst, const uint8_t* src, int N, int K, int q8) {
    CK(dalloc(dst, (size_t)N * K * (q8 ? 1 : 2)));
    CK(launch_frag_pack(src, N, K, q8, *dst, nullptr));
    CK(hipStreamSynchronize(nullptr));
    return 0;
}

// fragment-major copies of the decoder matrices and the LM head, made once per model, on the
// first batch or the first bf16 prefill of more than one row (6.86 GB bf16 / 3.83 GB Q8 beside
// the row-major weights the single-stream GEMVs read).  All or nothing: a failed copy frees
// what it had made, so the model holds either every copy or none.
static int model_frag(vox_hip_model_t* m) {
    if (m->lm_frag) return 0;
    const vox_hip_config_t& c = m->c;
    const int DD = c.dec_dim, DQ = c.dec_heads * c.dec_head_dim, DKV = c.dec_kv_heads * c.dec_head_dim;
    const int DH = c.dec_hidden;
    std::vector<DecFragD> F(c.dec_layers, DecFragD{});
    uint8_t* lm = nullptr;
    bool ok = true;
    for (int l = 0; l < c.dec_layers && ok; l++) {
        const DecLayerD& L = m->dec[l];
        ok = !frag_copy(&F[l].wqkv, L.wqkv, DQ + 2 * DKV, DD, L.sqkv != nullptr) &&
             !frag_copy(&F[l].wo, L.wo, DD, DQ, L.so != nullptr) &&
             !frag_copy(&F[l].w13, L.w13, 2 * DH, DD, L.s13 != nullptr) &&
             !frag_copy(&F[l].w2, L.w2, DD, DH, L.s2 != nullptr);
    }
    if (ok) ok = !frag_copy(&lm, m->tok_emb, c.vocab, DD, m->tok_emb_s != nullptr);
    if (!ok) {
        for (auto& f : F) { dfree(f.wqkv); dfree(f.wo); dfree(f.w13); dfree(f.w2); }
        dfree(lm);
        return -1;
    }
    m->dfrag.swap(F);
    m->lm_frag = lm;
    return 0;
}

static void batch_drop_graphs(vox_hip_batch_t* b) {
    for (auto& x : b->gexec)
        for (auto& k : x)
            for (auto& g : k)
                for (auto& e : g)
                    if (e) {
                        hipGraphExecDestroy(e);
                        e = nullptr;
                    }
    for (auto& k : b->gvexec)
        for (auto& g : k)
            for (auto& e : g)
                if (e) {
                    hipGraphExecDestroy(e);
                    e = nullptr;
                }
    for (auto& x : b->gwexec)
        for (auto& k : x)
            for (auto& g : k)
                for (auto& e : g)
                    if (e) {
                        hipGraphExecDestroy(e);
                        e = nullptr;
                    }
}

extern "C" void vox_hip_batch_free(vox_hip_batch_t* b) {
    if (!b) return;
    if (b->st) hipStreamSynchronize(b->st);
    // a begun call that was never finished ends here: its members are released, its parked
    // adapter buffers freed (the steps in flight are done, the later chunks never run)
    if (b->call.active) batch_release(b);
    free(b->parked);
    dfree(b->x); dfree(b->part); dfree(b->ssq); dfree(b->ticket); dfree(b->q); dfree(b->att);
    dfree(b->logits); dfree(b->pval); dfree(b->pidx); dfree(b->palt); dfree(b->apart);
    dfree(b->xp_d); dfree(b->xp_q); dfree(b->xp_h); dfree(b->pgws); dfree(b->gflags); dfree(b->hid);
    dfree(b->wqkv); dfree(b->wxn); dfree(b->whid); dfree(b->wpa); dfree(b->wpc); dfree(b->wflags); dfree(b->wepoch);
    if (b->slots) hipFree(b->slots);
    if (b->hslots) hipHostFree(b->hslots);
    dfree(b->dcaps);
    if (b->hcaps) hipHostFree(b->hcaps);
    batch_drop_graphs(b);
    if (b->st) hipStreamDestroy(b->st);
    delete b;
}

static int batch_set_gemv_rows(vox_hip_batch_t* b, int max_rows);
static int batch_set_gemv_rows_q8(vox_hip_batch_t* b, int max_rows);
static int model_gemv_q8_count(const vox_hip_model_t* m);
static int batch_set_gemv_wmx4(vox_hip_batch_t* b, int on, bool quiet);

extern "C" vox_hip_batch_t* vox_hip_batch_create(vox_hip_model_t* m, int max_streams) {
    if (!m || max_streams < 1 || max_streams > VOX_MAX_SLOTS) {
        set_err("batch size must be 1..%d", VOX_MAX_SLOTS);
        return nullptr;
    }
    const vox_hip_config_t& c = m->c;
    if (c.dec_head_dim != 128 || c.dec_heads % c.dec_kv_heads || c.dec_heads / c.dec_kv_heads > 4 ||
        c.dec_dim % 256 || c.dec_dim / 256 > SKL_MAX_SLICES) {
        set_err("batched decode needs head_dim 128, <= 4 query heads per kv head and dec_dim = 256 k <= 3072");
        return nullptr;
    }
    vox_hip_batch_t* b = new vox_hip_batch_t();
    memset((void*)b, 0, sizeof *b);
    b->m = m;
    b->cap = max_streams;
    b->rows = max_streams <= VOX_MAX_BATCH ? VOX_MAX_BATCH : max_streams <= 64 ? 64 : VOX_MAX_SLOTS;
    const size_t D = c.dec_dim, QKV = c.dec_heads * c.dec_head_dim + 2 * c.dec_kv_heads * c.dec_head_dim;
    const size_t S = b->rows;         // rows of the slot-indexed buffers (graphs of any bucket)
    const size_t SK = VOX_MAX_BATCH;  // rows of the skinny step's slabs and planes
    auto fail = [&]() -> vox_hip_batch_t* { vox_hip_batch_free(b); return nullptr; };
#define TRYH(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { set_err("%s: %s", #x, hipGetErrorString(e__)); return fail(); } } while (0)
    TRYH(queue_high_priority(&b->st));
    TRYH(dalloc(&b->x, S * D));
    {
        const size_t DQ = (size_t)c.dec_heads * c.dec_head_dim, DH = c.dec_hidden;
        const size_t n = std::max(std::max(skl_splits(D, (int)QKV) * QKV, skl_splits(DQ, D) * D),
                                  std::max(skl_splits(D, 2 * DH) * 2 * DH, skl_splits(DH, D) * D));
        if (!skl_splits(D) || !skl_splits(DQ) || !skl_splits(DH)) {
            set_err("batched decode needs dec_dim, heads*head_dim and dec_hidden divisible by 256");
            return fail();
        }
        TRYH(dalloc(&b->part, (size_t)SK * n));  // [row block][split][16][N] for the skinny step's rows
    }
    TRYH(dalloc(&b->ssq, (size_t)SK_ROWS * SKX_TICKETS));  // [slices][16], any slice count
    TRYH(dalloc(&b->ticket, (size_t)SKX_TICKETS));
    TRYH(dalloc(&b->q, S * c.dec_heads * c.dec_head_dim));
    TRYH(dalloc(&b->att, S * c.dec_heads * c.dec_head_dim));
    TRYH(dalloc(&b->logits, S * c.vocab));
    TRYH(dalloc(&b->pval, S * ARGB));
    TRYH(dalloc(&b->pidx, S * ARGB));
    TRYH(dalloc(&b->palt, S * ARGB * ALT_PART));
    // attention partials + one arrival count per kv head (zeroed; reset by the merging block)
    b->apart_n = (size_t)c.dec_heads * attn_maxch(c.dec_window) * (c.dec_head_dim + 2) + c.dec_kv_heads;
    TRYH(dalloc(&b->apart, S * b->apart_n));
    TRYH(hipMalloc((void**)&b->slots, slot_bytes(b->rows)));
    TRYH(hipMemset(b->slots, 0, slot_bytes(b->rows)));
    TRYH(hipHostMalloc((void**)&b->hslots, slot_bytes(b->rows), hipHostMallocDefault));
    memset((void*)b->hslots, 0, slot_bytes(b->rows));
    if (model_frag(m)) return fail();
    TRYH(dalloc(&b->xp_d, (size_t)3 * SK * D));  // [row block][3][16][K]
    TRYH(dalloc(&b->xp_q, (size_t)3 * SK * c.dec_heads * c.dec_head_dim));
    TRYH(dalloc(&b->xp_h, (size_t)3 * SK * c.dec_hidden));
    if (b->rows > VOX_MAX_BATCH) {
        // the wide step's own rows, planes (whole 128-row tiles: k_gemmf reads every row block
        // of a tile), split workspace, flags and epoch word
        const size_t DQ = (size_t)c.dec_heads * c.dec_head_dim, R = VOX_MAX_SLOTS;
        TRYH(dalloc(&b->wqkv, S * QKV));
        TRYH(dalloc(&b->wxn, S * D));
        TRYH(dalloc(&b->whid, S * c.dec_hidden));
        TRYH(dalloc(&b->wpa, R * 3 * std::max(D, DQ)));
        TRYH(dalloc(&b->wpc, R * 3 * c.dec_hidden));
        TRYH(dalloc(&b->wflags, gemmf_flag_ints()));
        TRYH(dalloc(&b->wepoch, (size_t)1));
        TRYH(dalloc(&b->pgws, GEMM_WS_ELEMS));
    }
#undef TRYH
    // VOX_HIP_BATCH_GEMV=<0|1|2|4|8>: the initial max_rows of the R-row GEMV step (unset: 0;
    // a Q8 model keeps 0)
    if (const char* e = getenv("VOX_HIP_BATCH_GEMV")) {
        const int r = atoi(e);
        if (r && !(m->tok_emb_s || m->dec[0].sqkv) && batch_set_gemv_rows(b, r)) return fail();
    }
    // VOX_HIP_BATCH_GEMV_Q8=<0|1|2|4|8>: the same for a model with Q8 step tensors (a model
    // without one ignores it)
    if (const char* e = getenv("VOX_HIP_BATCH_GEMV_Q8")) {
        const int r = atoi(e);
        if (r && model_gemv_q8_count(m) && batch_set_gemv_rows_q8(b, r)) return fail();
    }
    b->wmx4 = m->fstats[0] ? 1 : 0;
    // VOX_HIP_BATCH_GEMV_WMX4=1: the GEMV step's initial weight source (unset: 0; a model
    // without a wmx4 GEMV plane keeps 0)
    if (const char* e = getenv("VOX_HIP_BATCH_GEMV_WMX4"))
        if (atoi(e) == 1) batch_set_gemv_wmx4(b, 1, true);
    // VOX_HIP_BATCH_PREFILL_KV=0: new streams with 16-bit or one-byte rings take the per-stream
    // prefill on their own queues instead of the stacked pass (A/B; f32 streams ignore it)
    {
        const char* e = getenv("VOX_HIP_BATCH_PREFILL_KV");
        b->prefill_kv = (e && atoi(e) == 0) ? 0 : 1;
    }
    return b;
}

// the batched step's projections: k_skl, one burst of column groups per block
// mx: the tensor's wmx4 fragment plane when the step streams it (null: Wf, the 16-bit copy)
static hipError_t batch_gemm(const uint16_t* xs, int K, const void* Wf, const uint8_t* mx, const float* wscale, int N,
                             int nb, float* part, hipStream_t st, const float* ssq = nullptr, int nsl = 0,
                             float eps = 0.f) {
    return launch_gemm_skl(xs, K, mx ? mx : Wf, wscale, N, nb, part, st, ssq, nsl, eps, 1, mx != nullptr);
}

// one batched step over slots 0..nb-1 of the slot table (their input rows already in b->x)
// mixed: the FFN norm's ada row per slot (k_resid_xw_fplanes_slot), from the slot table
// ragged: each slot's ring capacity from b->dcaps (the ragged attention instances; the shared
// cap and ring_off are not read)
static int batch_step(vox_hip_batch_t* b, int nb, int splits, int kvt, int wmx4, int mixed, int ragged) {
    vox_hip_model_t* m = b->m;
    auto mx = [&](const WMx4D& M) -> const uint8_t* { return wmx4 ? M.frag : nullptr; };
    const vox_hip_config_t& c = m->c;
    const int DD = c.dec_dim, H = c.dec_heads, KVH = c.dec_kv_heads, hd = c.dec_head_dim;
    const int DQ = H * hd, DKV = KVH * hd, DH = c.dec_hidden;
    const float scale = 1.0f / sqrtf((float)hd);
    const int cap = c.dec_window + DEC_SLACK;
    const size_t ring_layer = (size_t)cap * DKV * kv_esize(kvt);
    hipStream_t st = b->st;
    AttnPtrsRag ap;  // (a plain step passes its AttnPtrs part alone)
    memset((void*)&ap, 0, sizeof ap);
    ap.slots = b->slots;
    ap.caps = b->dcaps;
    for (int i = 0; i < nb; i++) {
        ap.q[i] = b->q + (size_t)i * DQ;
        ap.part[i] = b->apart + (size_t)i * b->apart_n;
        ap.out[i] = b->att + (size_t)i * DQ;
    }
    const int Sres = skl_splits(DH, DD);  // slabs the previous layer's w2 left for the residual
    for (int l = 0; l < c.dec_layers; l++) {
        const DecLayerD& L = m->dec[l];
        const DecFragD& F = m->dfrag[l];
        ap.ring_off = (size_t)l * ring_layer;
        // skinny MFMA GEMMs over fragment-major weights: the slots are the 16-column B
        // operand, every weight byte read once per step; each projection leaves split-K slabs
        // in b->part that the next kernel sums (with the residual for wo / w2).
        // residual + RMSNorm as slice-parallel rows: x * w planes + slice sums of squares, the
        // inverse RMS applied by the projection
        CK(launch_resid_xw_fplanes(b->x, nb, DD, L.attn_norm, nullptr, b->xp_d, b->part, l ? Sres : 0, nullptr,
                                   b->ssq, st));
        CK(batch_gemm(b->xp_d, DD, F.wqkv, mx(L.mqkv), L.sqkv, DQ + 2 * DKV, nb, b->part, st, b->ssq, DD / 256, c.dec_eps));
        // RoPE + KV append + attention of every live slot, output into the wo planes (one
        // launch; past 256 keys the last key-range block of a kv head merges the partials)
        AttnFuse af;
        af.qkv = b->part; af.S = skl_splits(DD, DQ + 2 * DKV); af.N = DQ + 2 * DKV; af.rope = m->rope_dec; af.xs = b->xp_q;
        if (ragged) {
            ap.layer = l;
            CK(launch_attn_batch_fused_rag(hd, ap, af, nb, c.dec_window, scale, H, KVH, splits, st, kvt));
        } else {
            CK(launch_attn_batch_fused(hd, ap, af, nb, cap, c.dec_window, scale, H, KVH, splits, st, kvt));
        }
        CK(batch_gemm(b->xp_q, DQ, F.wo, mx(L.mo), L.so, DD, nb, b->part, st));
        if (mixed)
            CK(launch_resid_xw_fplanes_slots(b->x, nb, DD, L.ffn_norm, b->slots, (size_t)l * DD, b->xp_d, b->part,
                                             skl_splits(DQ, DD), nullptr, b->ssq, st));
        else
            CK(launch_resid_xw_fplanes(b->x, nb, DD, L.ffn_norm, m->ada_scale + (size_t)l * DD, b->xp_d, b->part,
                                       skl_splits(DQ, DD), nullptr, b->ssq, st));
        if (!L.s13) {
            // W1|W3 with the SwiGLU folded in (k_sklx: the last block of each column slice
            // sums its slabs and writes the w2 planes)
            SklFused f;
            f.ssq_in = b->ssq; f.nsl = DD / 256; f.eps = c.dec_eps;
            f.part = b->part; f.ticket = b->ticket;
            f.planes = b->xp_h;
            const uint8_t* m13 = mx(L.m13);
            CK(launch_gemm_sklx(SKX_PRO_SCALE, SKX_EPI_SWIGLU, b->xp_d, DD, m13 ? m13 : F.w13, 2 * DH, nb, f, st, m13 != nullptr));
        } else {
            // Q8: the int8 projection, then the SwiGLU rows
            CK(batch_gemm(b->xp_d, DD, F.w13, nullptr, L.s13, 2 * DH, nb, b->part, st, b->ssq, DD / 256, c.dec_eps));
            CK(launch_swiglu_fplanes(b->part, skl_splits(DD, 2 * DH), DH, nb, b->xp_h, st));
        }
        CK(batch_gemm(b->xp_h, DH, F.w2, mx(L.m2), L.s2, DD, nb, b->part, st));
    }
    // final norm (after the last w2 residual) + LM head (tied embeddings) + per-slot argmax,
    // state, token log and next inputs (decoder.c:762-779)
    CK(launch_rmsnorm_fplanes(b->x, nb, DD, m->dec_norm, nullptr, c.dec_eps, b->xp_d, b->part, Sres, st));
    // 17..32 rows: both 16-row blocks in one k_skf launch (the embeddings read once;
    // VOX_HIP_SKF2=0: one launch per 16-row block)
    static const int skf2 = env_on("VOX_HIP_SKF2");
    const uint8_t* mlm = mx(m->mlm);
    const void* lmw = mlm ? mlm : m->lm_frag;
    if (skf2 && nb > SK_ROWS)
        CK(launch_gemm_skf2(b->xp_d, DD, lmw, m->tok_emb_s, c.vocab, nb, b->logits, c.vocab, st, mlm != nullptr));
    else
        for (int r0 = 0; r0 < nb; r0 += SK_ROWS)
            CK(launch_gemm_skf(b->xp_d + (size_t)r0 * 3 * DD, DD, lmw, m->tok_emb_s, c.vocab,
                               std::min(SK_ROWS, nb - r0), b->logits + (size_t)r0 * c.vocab, c.vocab, st, mlm != nullptr));
    CK(launch_argmax_batch(b->logits, nb, c.vocab, b->pval, b->pidx, b->palt, b->slots, TOKENS_CAP, slot_toklog(b->slots, b->rows),
                           m->tok_emb, m->tok_emb_s, DD, b->x, st));
    return 0;
}

// The same step for a bucket of nb <= 8 slots on the R-row GEMV (k_gemvr): the
// single-stream step's five launches per layer with every weight byte (bf16 rows, the model's
// wpack13 planes, with wmx4 set the wmx4 GEMV plane of each tensor that has one, or the int8
// rows and scales of a Q8 tensor) read once for the nb rows, and no planes, slabs
// or tickets.  Between
// the launches the rows live in b->x (residual stream, updated in place), b->q, b->att and
// b->hid; attention is the slot-table kernel of the single-stream step.  b->x is complete
// before and after either step, so the two may alternate from one call to the next.
static int batch_step_gemv(vox_hip_batch_t* b, int nb, int splits, int kvt, int wmx4) {
    vox_hip_model_t* m = b->m;
    const vox_hip_config_t& c = m->c;
    const int DD = c.dec_dim, H = c.dec_heads, KVH = c.dec_kv_heads, hd = c.dec_head_dim;
    const int DQ = H * hd, DKV = KVH * hd, DH = c.dec_hidden;
    const float scale = 1.0f / sqrtf((float)hd);
    const int cap = c.dec_window + DEC_SLACK;
    const size_t ring_layer = (size_t)cap * DKV * kv_esize(kvt);
    hipStream_t st = b->st;
    AttnPtrs ap;
    memset(&ap, 0, sizeof ap);
    ap.slots = b->slots;
    for (int i = 0; i < nb; i++) {
        ap.q[i] = b->q + (size_t)i * DQ;
        ap.part[i] = b->apart + (size_t)i * b->apart_n;
        ap.out[i] = b->att + (size_t)i * DQ;
    }
    GemvRArgs a;
    // a = tensor t over the nb rows x (row stride ldx) into y (ldy)
    auto fill = [&](const StepTensor& t, const float* x, int ldx, float* y, int ldy) {
        memset(&a, 0, sizeof a);
        step_tensor_args(a.g, t, x, y, c.dec_eps, wmx4);
        a.ldx = ldx; a.ldy = ldy;
    };
    for (int l = 0; l < c.dec_layers; l++) {
        ap.ring_off = (size_t)l * ring_layer;
        // norm -> QKV -> RoPE -> KV append of every live slot
        StepTensor t = dec_step_tensor(m, l, T_QKV);
        fill(t, b->x, DD, b->q, DQ);
        a.g.qd = DQ; a.g.kvd = DKV; a.g.hd = hd; a.g.rope = m->rope_dec; a.g.cap = cap; a.g.kvt = kvt;
        a.slots = b->slots; a.ring_off = ap.ring_off;
        CK(launch_gemvr(t.pro, t.epi, nb, a, st));
        CK(launch_attn_decode_batch(hd, ap, nb, cap, c.dec_window, scale, H, KVH, splits, st, kvt));
        // wo + residual
        t = dec_step_tensor(m, l, T_WO);
        fill(t, b->att, DQ, b->x, DD);
        CK(launch_gemvr(t.pro, t.epi, nb, a, st));
        // norm * (1 + ada) -> W1|W3 -> silu * up
        t = dec_step_tensor(m, l, T_W13);
        fill(t, b->x, DD, b->hid, DH);
        CK(launch_gemvr(t.pro, t.epi, nb, a, st));
        // W2 + residual
        t = dec_step_tensor(m, l, T_W2);
        fill(t, b->hid, DH, b->x, DD);
        CK(launch_gemvr(t.pro, t.epi, nb, a, st));
    }
    // final norm + LM head rows, then the batched step's own end (argmax, alternatives, token
    // log, state, next inputs)
    const StepTensor t = dec_step_tensor(m, c.dec_layers, 0);
    fill(t, b->x, DD, b->logits, c.vocab);
    CK(launch_gemvr(t.pro, t.epi, nb, a, st));
    CK(launch_argmax_batch(b->logits, nb, c.vocab, b->pval, b->pidx, b->palt, b->slots, TOKENS_CAP, slot_toklog(b->slots, b->rows),
                           m->tok_emb, m->tok_emb_s, DD, b->x, st));
    return 0;
}

// the tensors of the step all have k_gemvr instances; wmx4: those that have a wmx4 GEMV plane
// have wmx4 instances too
static bool model_gemvr_ok(const vox_hip_model_t* m, int wmx4 = 0) {
    return all_step_tensors(m, [&](const StepTensor& t) {
        return gemvr_ok(t.pro, t.epi, t.rows, t.K) && (!wmx4 || !t.mx->plane || gemvr_ok_mx4(t.pro, t.epi, t.rows, t.K));
    });
}

// tensors of the GEMV step (4 per layer and the LM head) with / without a wmx4 GEMV plane
static void model_gemv_wmx4_count(const vox_hip_model_t* m, long long* with, long long* without) {
    long long n = 0, all = 0;
    all_step_tensors(m, [&](const StepTensor& t) { n += t.mx->plane != nullptr; all++; return true; });
    *with = n;
    *without = all - n;
}

static int batch_set_gemv_rows(vox_hip_batch_t* b, int max_rows) {
    if (max_rows != 0 && max_rows != 1 && max_rows != 2 && max_rows != 4 && max_rows != 8)
        return set_err("batch_set_gemv_rows: max_rows %d is not 0, 1, 2, 4 or 8", max_rows);
    if (b->call.active) return set_err("batch_set_gemv_rows: a begun call was not finished");
    if (max_rows) {
        const vox_hip_model_t* m = b->m;
        if (m->tok_emb_s || m->dec[0].sqkv) return set_err("batch_set_gemv_rows: the GEMV step takes bf16 weights, not Q8");
        if (!model_gemvr_ok(m)) return set_err("batch_set_gemv_rows: no k_gemvr instance for this model's shapes");
        if (!b->hid) CK(dalloc(&b->hid, (size_t)GEMVR_MAX_ROWS * m->c.dec_hidden));
    }
    b->gemv_rows = max_rows;
    return 0;
}

extern "C" int vox_hip_batch_set_gemv_rows(vox_hip_batch_t* b, int max_rows) {
    if (!b) return set_err("batch_set_gemv_rows: null batch");
    return batch_set_gemv_rows(b, max_rows);
}

// Q8 step tensors of the model (4 per layer and the LM head: those with a scale vector)
static int model_gemv_q8_count(const vox_hip_model_t* m) {
    int n = 0;
    all_step_tensors(m, [&](const StepTensor& t) { n += t.wscale != nullptr; return true; });
    return n;
}

// every step tensor has a k_gemvr instance in its own format: the Q8 one where it has scales,
// the bf16 / wpack13 one otherwise (a checkpoint may quantise only some tensors)
static bool model_gemvr_ok_q8(const vox_hip_model_t* m) {
    return all_step_tensors(m, [](const StepTensor& t) {
        return t.wscale ? gemvr_ok_q8(t.pro, t.epi, t.rows, t.K) : gemvr_ok(t.pro, t.epi, t.rows, t.K);
    });
}

// The Q8 model's opt-in of its own: the same gemv_rows field, so the bucket
// dispatch, graphs and counters are the bf16 mode's
static int batch_set_gemv_rows_q8(vox_hip_batch_t* b, int max_rows) {
    if (max_rows != 0 && max_rows != 1 && max_rows != 2 && max_rows != 4 && max_rows != 8)
        return set_err("batch_set_gemv_rows_q8: max_rows %d is not 0, 1, 2, 4 or 8", max_rows);
    if (b->call.active) return set_err("batch_set_gemv_rows_q8: a begun call was not finished");
    const vox_hip_model_t* m = b->m;
    if (!model_gemv_q8_count(m))
        return set_err("batch_set_gemv_rows_q8: the model has no Q8 step tensor (vox_hip_batch_set_gemv_rows is its switch)");
    if (max_rows) {
        if (!model_gemvr_ok_q8(m)) return set_err("batch_set_gemv_rows_q8: no k_gemvr instance for this model's shapes");
        if (!b->hid) CK(dalloc(&b->hid, (size_t)GEMVR_MAX_ROWS * m->c.dec_hidden));
    }
    b->gemv_rows = max_rows;
    return 0;
}

extern "C" int vox_hip_batch_set_gemv_rows_q8(vox_hip_batch_t* b, int max_rows) {
    if (!b) return set_err("batch_set_gemv_rows_q8: null batch");
    return batch_set_gemv_rows_q8(b, max_rows);
}

static int batch_set_gemv_wmx4(vox_hip_batch_t* b, int on, bool quiet) {
    if (b->call.active) return quiet ? -1 : set_err("batch_set_gemv_wmx4: a begun call was not finished");
    if (on) {
        const vox_hip_model_t* m = b->m;
        long long with = 0, without = 0;
        model_gemv_wmx4_count(m, &with, &without);
        if (!with)
            return quiet ? -1
                         : set_err("batch_set_gemv_wmx4: the model has no wmx4 GEMV plane (vox_hip_set_wmx4 before its creation; "
                                   "not Q8, not VOX_HIP_WPACK=0)");
        if (!model_gemvr_ok(m, 1))
            return quiet ? -1 : set_err("batch_set_gemv_wmx4: no wmx4 k_gemvr instance for this model's shapes");
    }
    b->gemv_wmx4 = on ? 1 : 0;
    return 0;
}

extern "C" int vox_hip_batch_set_gemv_wmx4(vox_hip_batch_t* b, int on) {
    if (!b) return set_err("batch_set_gemv_wmx4: null batch");
    return batch_set_gemv_wmx4(b, on, false);
}

extern "C" int vox_hip_batch_gemv_wmx4_stats(const vox_hip_batch_t* b, long long out4[4]) {
    if (!b || !out4) return set_err("batch_gemv_wmx4_stats: null argument");
    out4[0] = b->gemv_wmx4;
    out4[1] = b->n_gemv_wmx4_replays;
    model_gemv_wmx4_count(b->m, &out4[2], &out4[3]);
    return 0;
}

extern "C" int vox_hip_batch_set_wmx4(vox_hip_batch_t* b, int on) {
    if (!b) return set_err("batch_set_wmx4: null batch");
    if (b->call.active) return set_err("batch_set_wmx4: a begun call was not finished");
    if (on && !b->m->fstats[0])
        return set_err("batch_set_wmx4: the model has no wmx4 fragment planes (vox_hip_set_wmx4_batch before its creation)");
    b->wmx4 = on ? 1 : 0;
    return 0;
}

extern "C" int vox_hip_batch_set_prefill_kv(vox_hip_batch_t* b, int on) {
    if (!b) return set_err("batch_set_prefill_kv: null batch");
    if (b->call.active) return set_err("batch_set_prefill_kv: a begun call was not finished");
    b->prefill_kv = on ? 1 : 0;
    return 0;
}

extern "C" int vox_hip_batch_gemv_stats(const vox_hip_batch_t* b, long long* out4) {
    if (!b || !out4) return set_err("batch_gemv_stats: null argument");
    out4[0] = b->gemv_rows;
    out4[1] = b->n_gemv_replays;
    out4[2] = b->n_gemv_rows;
    out4[3] = b->n_gemv_captures;
    return 0;
}

// The step for a bucket of 64 or 128 slots: a rows_layers call, as the stacked
// prefill makes (k_gemmf, or the launch_gemm form where dec_gemmf_ok is false), on the batch's own
// planes and scratch, with the slot-table decode attention as its attention step in place of the
// prefill's causal one.  Every weight byte is read once per step for the nb rows: the layers stream
// the bf16 fragment-major copies (on a wmx4-rounded model they hold the planes' values), the
// fallback the row-major tensors.  Rows are complete in b->x before and after, as in the other
// two steps, so a batch moves between buckets from one call to the next.
// k_gemmf's hand-off epochs are i + *b->wepoch for the step's i-th launch (GemmfQ's device-word
// discipline); the step's last kernel advances the word past them, so the launches may be
// captured and replayed.
// mixed: the FFN norm's ada row per slot (rows_layers' RowsAda::slots)
// ragged: each slot's ring capacity from b->dcaps, as batch_step
static int batch_step_wide(vox_hip_batch_t* b, int nb, int splits, int kvt, int mixed, int ragged) {
    vox_hip_model_t* m = b->m;
    const vox_hip_config_t& c = m->c;
    const int DD = c.dec_dim, H = c.dec_heads, KVH = c.dec_kv_heads, hd = c.dec_head_dim;
    const int DQ = H * hd, DKV = KVH * hd, QKV = DQ + 2 * DKV;
    const float scale = 1.0f / sqrtf((float)hd);
    const int cap = c.dec_window + DEC_SLACK;
    const size_t ring_layer = (size_t)cap * DKV * kv_esize(kvt);
    hipStream_t st = b->st;
    const bool gf = dec_gemmf_ok(m, nb);
    const bool lm_gf = (!m->tok_emb_s || m->gemmf_q8) && enc_gemmf_env() && dec_gemmf_env() && gemmf_ok(nb, c.vocab, DD);
    int launches = 0;
    b->wide_q8 = 0;  // this step's launches on int8 fragments (batch_run counts them again per replay)
    const GemmfQ q{st, b->pgws, GEMM_WS_ELEMS, b->wflags, &launches, &m->n_gemmf_q8, b->wepoch, &b->wide_q8};
    AttnSlotsRag ap;  // (a plain step passes its AttnSlots part alone)
    ap.q = nullptr; ap.q_ld = 0;
    ap.part = b->apart; ap.part_ld = b->apart_n;
    ap.out = gf ? nullptr : b->att; ap.out_ld = DQ;
    ap.slots = b->slots;
    ap.ring_off = 0;
    ap.caps = b->dcaps; ap.layer = 0;
    AttnFuse af;
    af.qkv = b->wqkv; af.S = 1; af.N = QKV; af.rope = m->rope_dec; af.xs = b->wpa;
    // RoPE + K/V append at each live slot's own position + attention over its ring, the rows
    // as the wo planes (and, for the fallback, as f32 rows in b->att)
    if (rows_layers(m, dec_rows_stack(c), RowsScratch{b->x, b->wqkv, b->wxn, b->att, b->whid, b->wpa, b->wpc}, q, gf, nb,
                    [&](int l, uint16_t*) -> int {
                        ap.ring_off = (size_t)l * ring_layer;
                        ap.layer = l;
                        if (ragged) CK(launch_attn_batch_wide_rag(hd, ap, af, nb, c.dec_window, scale, H, KVH, splits, st, kvt));
                        else CK(launch_attn_batch_wide(hd, ap, af, nb, cap, c.dec_window, scale, H, KVH, splits, st, kvt));
                        return 0;
                    }, RowsAda{nullptr, mixed ? b->slots : nullptr}))
        return -1;
    // final norm + LM head (tied embeddings) into b->logits, then the per-slot argmax, state,
    // token log and next inputs (decoder.c:762-779)
    if (lm_gf) {
        CK(launch_rmsnorm_fplanes(b->x, nb, DD, m->dec_norm, nullptr, c.dec_eps, b->wpa, nullptr, 0, st));
        if (gemmf_on(q, EPI_STORE, b->wpa, DD, nb, m->lm_frag, m->tok_emb_s, c.vocab, nullptr, b->logits, c.vocab, nullptr)) return -1;
    } else {
        CK(launch_rmsnorm_rows(b->x, DD, b->wxn, DD, m->dec_norm, nullptr, nb, DD, c.dec_eps, st));
        CK(launch_gemm(EPI_STORE, 3, b->wxn, DD, m->tok_emb, m->tok_emb_s, DD, nb, c.vocab, nullptr, b->logits, c.vocab, st,
                       b->pgws, GEMM_WS_ELEMS));
    }
    CK(launch_argmax_batch(b->logits, nb, c.vocab, b->pval, b->pidx, b->palt, b->slots, TOKENS_CAP, slot_toklog(b->slots, b->rows),
                           m->tok_emb, m->tok_emb_s, DD, b->x, st));
    if (launches) CK(launch_gemmf_epoch_bump(b->wepoch, launches + 1, st));
    return 0;
}


// slot bucket of n streams: 1, 2, 4, 8, 16 or 32 slots (graph g of the bucket); past 32 the wide
// step's 64 or 128 (g = 6, 7)
static int slot_bucket(int n, int* g) {
    int k = 0;
    while ((1 << k) < n) k++;
    *g = k;
    return 1 << k;
}

// `steps` batched steps over slots 0..nb-1: replays of the bucket's step graph (captured the
// first time, and again only when the rope table moved), or eager launches
static int batch_run(vox_hip_batch_t* b, int nb, int gb, int gi, int splits, int kvt, int steps, int gemv, int mixed,
                     int ragged) {
    const int wmx4 = b->wmx4;  // fixed while a begun call is unfinished (vox_hip_batch_set_wmx4)
    const int gwmx4 = b->gemv_wmx4;  // likewise (vox_hip_batch_set_gemv_wmx4: on only with a plane to stream)
    const bool wide = nb > VOX_MAX_BATCH;  // buckets 64 and 128 (gemv == 0 there)
    auto step = [&]() {
        return wide ? batch_step_wide(b, nb, splits, kvt, mixed, ragged)
               : gemv ? batch_step_gemv(b, nb, splits, kvt, gwmx4) : batch_step(b, nb, splits, kvt, wmx4, mixed, ragged);
    };
    if (ragged) b->n_ragged_replays += steps;
    if (gemv) b->n_gemv_replays += steps;
    if (gemv && gwmx4) b->n_gemv_wmx4_replays += steps;
    if (!use_graphs()) {
        for (int k = 0; k < steps; k++)
            if (step()) return -1;
        b->n_replays += steps;
        return 0;
    }
    if (b->grope_gen != b->m->rope_gen) {
        batch_drop_graphs(b);
        b->grope_gen = b->m->rope_gen;
    }
    const int mr = mixed + 2 * ragged;
    hipGraphExec_t& ge = wide ? b->gwexec[mr][kvt][gb - 6][gi]
                         : gemv ? b->gvexec[3 * gwmx4 + kvt][gb][gi] : b->gexec[mr][3 * wmx4 + kvt][gb][gi];
    if (!ge) {
        hipGraph_t g = nullptr;
        CK(hipStreamBeginCapture(b->st, hipStreamCaptureModeThreadLocal));
        const int rc = step();
        hipError_t e = hipStreamEndCapture(b->st, &g);
        if (rc || e != hipSuccess) {
            if (g) hipGraphDestroy(g);
            return set_err("batch graph capture failed: %s", hipGetErrorString(e));
        }
        e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        if (e != hipSuccess) {
            ge = nullptr;
            return set_err("batch graph instantiate failed: %s", hipGetErrorString(e));
        }
        b->n_captures++;
        if (ragged) b->n_ragged_captures++;
        if (gemv) b->n_gemv_captures++;
    }
    for (int k = 0; k < steps; k++) CK(hipGraphLaunch(ge, b->st));
    if (wide) b->m->n_gemmf_q8 += (long long)steps * b->wide_q8;  // each replay, beside the capture's own count
    b->n_replays += steps;
    return 0;
}

// host mirror after `produced` device steps of stream s (as vox_hip_stream_decode)
static void stream_steps_done(vox_hip_stream_t* s, int produced, int last_token) {
    s->n_generated += produced;
    s->h_state[0] += produced;
    s->h_state[1] += produced;
    if (produced) s->h_state[2] = last_token;
    s->h_state[3] = s->n_generated;
}

// The prompts of several new streams in one stacked prefill pass on the batch queue (the
// decoder prefill of voxtral.c:1036-1057 per stream; rows [b np, (b + 1) np) = stream b):
// RMSNorm and the projections over all rows (every weight byte read once for the group),
// RoPE + K/V append and the causal attention per stream against its own ring (the batched
// encoder's row-offset kernels, at the ring element type of the streams: batch_begin refuses
// mixed types, so ss[0]->kvt speaks for the group), scratch of ss[0].  One stream takes the
// single-stream prefill.  The member queues must be idle.
// bounded (vox_hip_batch_decode_rows): a single new stream takes the stacked path too, on the
// batch queue -- its own queue may be busy with an encoder pass the steps overlap; only stacks
// past ENC_SUB rows (a prompt longer than one pass) still take the per-stream prefill on the
// member's own queue and wait there for any encoder pass queued on it.
// prefill_kv == 0 (vox_hip_batch_set_prefill_kv, A/B): streams with 16-bit or one-byte rings
// take that per-stream prefill as well (correct; the shared weight pass and the overlap are lost)
// The streams of one pass share a delay (batch_begin groups them): ss[0]'s prompt length and ada
// table speak for the group.
static int batch_prefill(vox_hip_batch_t* b, vox_hip_stream_t* const* ss, int B, bool bounded) {
    vox_hip_model_t* m = b->m;
    const vox_hip_config_t& c = m->c;
    const int np = 32 + stream_delay(ss[0]);
    // more prompts than one pass holds (ENC_SUB rows: 26 prompts of 39 rows): stacked passes of
    // as many as fit
    const int per = std::max(1, ENC_SUB / np);
    const int kvt = ss[0]->kvt;
    const bool one_by_one = kvt != KV_F32 && !b->prefill_kv;
    if (B > per && !one_by_one) {
        for (int i0 = 0; i0 < B; i0 += per)
            if (batch_prefill(b, ss + i0, std::min(per, B - i0), bounded)) return -1;
        return 0;
    }
    if ((B == 1 && !bounded) || one_by_one || B * np > ENC_SUB) {
        for (int i = 0; i < B; i++) {
            if (stream_prefill(ss[i])) return -1;
            CK(hipStreamSynchronize(ss[i]->st));
        }
        b->n_prefill_passes += B;
        b->n_prefilled += B;
        return 0;
    }
    const int DD = c.dec_dim, H = c.dec_heads, KVH = c.dec_kv_heads, hd = c.dec_head_dim;
    const int DQ = H * hd, DKV = KVH * hd;
    const float scale = 1.0f / sqrtf((float)hd);
    vox_hip_stream_t* lead = ss[0];
    const int N = B * np, cap = lead->dcap;
    hipStream_t st = b->st;
    if (stream_alloc_dec_rows(lead, N)) return -1;
    if (ensure_rope(lead, np + 2)) return -1;
    if (!b->pgws) CK(dalloc(&b->pgws, GEMM_WS_ELEMS));
    float* gws = b->pgws;
    const size_t gws_n = GEMM_WS_ELEMS;
    float* X = lead->xd;
    for (int i = 0; i < B; i++)
        CK(launch_embed_rows(ss[i]->adapter, m->tok_emb, m->tok_emb_s, 0, np, TOKEN_BOS, TOKEN_STREAMING_PAD, DD,
                             X + (size_t)i * np * DD, st));
    EncRows er;
    memset(&er, 0, sizeof er);
    er.B = B;
    for (int i = 0; i < B; i++) {
        er.off[i] = i * np;
        er.nr[i] = np;
        er.pos0[i] = 0;
    }
    // the layers with the lead's scratch and planes on the batch queue (its own flags and epoch)
    const bool gf = dec_gemmf_ok(m, N);
    if (gf) {
        if (!b->gflags) CK(dalloc(&b->gflags, gemmf_flag_ints()));
        if (model_frag(m) || stream_dec_planes(lead, N)) return -1;
    }
    if (rows_layers(m, dec_rows_stack(c), dec_rows_scratch(lead, X),
                    GemmfQ{st, gws, gws_n, b->gflags, &b->gepoch, &m->n_gemmf_q8, nullptr, nullptr}, gf, N,
                    [&](int l, uint16_t* planes) -> int {
                        for (int i = 0; i < B; i++) {
                            er.Kc[i] = dec_ring(ss[i], ss[i]->dk, l);
                            er.Vc[i] = dec_ring(ss[i], ss[i]->dv, l);
                        }
                        CK(launch_rope_kv_rows(lead->qkvd, N, DQ, DKV, hd, m->rope_dec, er, lead->qd_, cap, st, kvt));
                        CK(launch_attn_rows(hd, lead->qd_, er, N, cap, lead->attd, H, KVH, c.dec_window, scale, gws, gws_n, st,
                                            planes, kvt));
                        return 0;
                    }, RowsAda{lead->delay < 0 ? nullptr : stream_ada(lead), nullptr}))
        return -1;
    for (int i = 0; i < B; i++)
        if (stream_prefilled(ss[i], st)) return -1;
    b->n_prefill_passes++;
    b->n_prefilled += B;
    return 0;
}

// rows == null: every stream's adapter rows, its queue synchronised first (an async encoder
// pass finishes before the steps read its rows); rows[i]: only stream i's first rows[i] rows,
// which the caller guarantees complete, and the members' queues are left running (an encoder
// pass enqueued on them after those rows overlaps the steps)
// batch_begin enqueues the call's prefills, slot table and first chunk of steps and returns
// without waiting (0: steps in flight, 1: nothing to run); batch_finish waits for them, runs
// the remaining chunks and fills the outputs.  batch_decode = both.
static int batch_begin(vox_hip_batch_t* b, vox_hip_stream_t** streams, int n, const int* rows, int max_steps,
                       int stop_at_eos, int* tokens_out, int* counts_out) {
    if (!b || n < 1 || n > b->cap || n > VOX_MAX_SLOTS || max_steps < 0) return set_err("bad batch arguments");
    if (b->call.active) return set_err("batch: a begun call was not finished");
    vox_hip_model_t* m = b->m;
    const vox_hip_config_t& c = m->c;
    // a call in which no stream carries a delay of its own is plain: the shared-row kernels and their graphs
    int mixed = 0;
    for (int i = 0; i < n; i++) {
        if (!streams[i] || streams[i]->m != m) return set_err("batch streams must share the batch's model");
        if (streams[i]->held) return set_err("batch streams[%d]: %s", i, HELD_MSG);
        mixed |= streams[i]->delay >= 0;
        if (streams[i]->kvt != streams[0]->kvt)
            return set_err("batch streams must share the decoder KV element type (vox_hip_model_set_kv_dtype)");
        for (int j = 0; j < i; j++)
            if (streams[j] == streams[i]) return set_err("stream listed twice in a batch");
        counts_out[i] = 0;
    }
    const int kvt = streams[0]->kvt;
    b->n_calls++;
    b->lnb = 0;
    // every member's queue is idle before the batch queue touches its buffers (adapter rows
    // of an async encoder pass, a realloc'ed adapter buffer) -- unless the caller bounded the
    // rows each stream may read
    int avail[VOX_MAX_SLOTS];
    for (int i = 0; i < n; i++) {
        if (rows) {
            if (rows[i] < 0 || rows[i] > streams[i]->total_adapter) return set_err("batch rows[%d] out of range", i);
            avail[i] = rows[i];
        } else {
            CK(hipStreamSynchronize(streams[i]->st));
            avail[i] = streams[i]->total_adapter;
        }
    }
    if (max_steps == 0) return 1;
    // 0. growing rings (vox_hip_model_set_kv_grow): every listed stream's rings hold the whole
    //    call before the prefills are queued and the slot table names them -- its position, the
    //    prompt if it joins, and the steps its budget allows.  All the new rings are allocated
    //    before a copy is enqueued: a failure returns with nothing enqueued and every stream as it
    //    was.  The copies go on the batch queue (with rows[] the members' queues are not waited
    //    for: no encoder pass touches a decoder ring).  Nothing moves again until the call ends.
    int ragged = 0;
    {
        bool grows = false;
        for (int i = 0; i < n; i++) grows = grows || streams[i]->dslots0;
        if (grows) {
            std::vector<DecGrow> gr(n);
            for (int i = 0; i < n; i++) {
                vox_hip_stream_t* s = streams[i];
                const int np = 32 + stream_delay(s);
                const bool joins = !s->started && !s->eos_seen && avail[i] >= 1 + np;
                int need = 0;
                if (s->started && !s->eos_seen) need = s->h_state[0] + std::max(0, std::min(avail[i] - s->h_state[1], max_steps));
                else if (joins) need = np + std::max(0, std::min(avail[i] - np, max_steps));
                if (dec_grow_alloc(s, need, true, &gr[i])) {
                    dec_grow_drop(gr.data(), i);
                    return -1;
                }
            }
            // the capacities the call will run on: ragged if one of them is below the full size
            for (int i = 0; i < n; i++) ragged |= (gr[i].cap ? gr[i].cap : streams[i]->dcap) != dec_ring_full(streams[i]);
            if (ragged && !b->hcaps) {
                // the per-slot capacity table of the ragged instances, on the first call that needs
                // it -- before the growths are committed, so that a failure here too leaves every
                // stream as it was
                hipError_t e = b->dcaps ? hipSuccess : dalloc(&b->dcaps, (size_t)b->rows);
                if (e == hipSuccess) e = hipHostMalloc((void**)&b->hcaps, sizeof(int) * b->rows, hipHostMallocDefault);
                if (e != hipSuccess) {
                    b->hcaps = nullptr;
                    dec_grow_drop(gr.data(), n);
                    return set_err("batch: per-slot ring capacity table: %s", hipGetErrorString(e));
                }
            }
            if (dec_grow_commit(gr.data(), n, b->st)) return -1;
        }
        b->n_ragged_calls += ragged;
    }
    // 1. streams whose prompt is complete and whose decoder has not started: their prefills
    //    in one stacked pass; they take their first token in the batched steps below
    {
        //    (one pass per distinct delay, each with that delay's prompt length and ada table)
        vox_hip_stream_t* pre[VOX_MAX_SLOTS];
        int np = 0, longest_delay = 0;
        for (int i = 0; i < n; i++) {
            vox_hip_stream_t* s = streams[i];
            if (!s->started && !s->eos_seen && avail[i] >= 1 + 32 + stream_delay(s)) {
                pre[np++] = s;
                longest_delay = std::max(longest_delay, stream_delay(s));
            }
        }
        if (np && mixed) {
            // the rope table covers the longest prompt before the first pass is queued
            if (ensure_rope(pre[0], 32 + longest_delay + 2)) return -1;
            // stable grouping by delay: the streams of a delay keep the call's order
            std::stable_sort(pre, pre + np, [](const vox_hip_stream_t* a, const vox_hip_stream_t* c2) {
                return stream_delay(a) < stream_delay(c2);
            });
        }
        for (int i0 = 0; i0 < np;) {
            int i1 = i0 + 1;
            while (i1 < np && stream_delay(pre[i1]) == stream_delay(pre[i0])) i1++;
            if (batch_prefill(b, pre + i0, i1 - i0, rows != nullptr)) return -1;
            i0 = i1;
        }
    }
    // 2. the slot table: slot i = streams[i], a step budget per slot, empty slots up to the
    //    bucket stopped
    int gb = 0;
    const int nb = slot_bucket(n, &gb);
    BatchSlot* hs = b->hslots;
    int K = 0, longest = 0;
    for (int i = 0; i < nb; i++) {
        memset(&hs[i], 0, sizeof hs[i]);
        hs[i].stop_tok = -1;
        hs[i].ada = m->ada_scale;  // (a row past the call's streams rides through the norms on the model's table)
        if (ragged) b->hcaps[i] = i < n ? streams[i]->dcap : c.dec_window + DEC_SLACK;
        if (i >= n) continue;
        vox_hip_stream_t* s = streams[i];
        int lim = 0;
        if (s->started && !s->eos_seen) lim = std::max(0, std::min(avail[i] - s->h_state[1], max_steps));
        hs[i].state = s->state;
        hs[i].tokens = s->tokens;
        hs[i].adapter = s->adapter;
        hs[i].Kc = reinterpret_cast<char*>(s->dk);
        hs[i].Vc = reinterpret_cast<char*>(s->dv);
        hs[i].alts = s->n_alt > 1 ? s->alts : nullptr;
        hs[i].adapter_rows = avail[i];
        hs[i].left = lim;
        hs[i].stop_tok = stop_at_eos ? TOKEN_EOS : -1;
        hs[i].live = lim > 0;
        hs[i].pos = s->h_state[0];
        hs[i].produced = 0;
        hs[i].ada = stream_ada(s);
        if (lim > 0) {
            K = std::max(K, lim);
            longest = std::max(longest, s->h_state[0] + lim);
            if (ensure_rope(s, (long long)s->h_state[0] + lim + 1)) return -1;
        }
    }
    if (K == 0) {
        CK(hipStreamSynchronize(b->st));
        return 1;
    }
    const int gi = graph_index(streams[0], std::min(longest, c.dec_window));
    const int splits = graph_splits(streams[0], gi);
    CK(hipMemcpyAsync(b->slots, hs, sizeof(BatchSlot) * nb, hipMemcpyHostToDevice, b->st));
    if (ragged) CK(hipMemcpyAsync(b->dcaps, b->hcaps, sizeof(int) * nb, hipMemcpyHostToDevice, b->st));
    CK(launch_embed_batch(b->slots, nb, m->tok_emb, m->tok_emb_s, c.dec_dim, b->x, b->st));
    // 3. the steps, in chunks of STEP_BATCH replays: after each chunk one copy of the slot
    //    table + token log comes back; the call ends when no slot is live.  The first chunk
    //    goes out here, the rest in batch_finish.
    const int k = std::min(STEP_BATCH, K);
    // buckets of up to gemv_rows slots take the R-row GEMV step (vox_hip_batch_set_gemv_rows)
    // (a mixed call takes the MFMA step: k_gemvr has no per-slot prologue)
    // (a ragged call too: k_gemvr's QKV epilogue takes one ring geometry for all rows)
    const int gemv = b->gemv_rows && nb <= b->gemv_rows && !mixed && !ragged;
    if (batch_run(b, nb, gb, gi, splits, kvt, k, gemv, mixed, ragged)) return -1;
    CK(hipMemcpyAsync(hs, b->slots, slot_bytes(b->rows), hipMemcpyDeviceToHost, b->st));
    auto& cl = b->call;
    cl.active = 1;
    cl.gemv = gemv;
    cl.mixed = mixed;
    cl.ragged = ragged;
    cl.n = n;
    for (int i = 0; i < n; i++) cl.streams[i] = streams[i];
    cl.max_steps = max_steps;
    cl.stop_at_eos = stop_at_eos;
    cl.K = K;
    cl.nb = nb;
    cl.gb = gb;
    cl.gi = gi;
    cl.splits = splits;
    cl.kvt = kvt;
    cl.done = 0;
    cl.k = k;
    cl.tokens_out = tokens_out;
    cl.counts_out = counts_out;
    batch_hold(b);
    return 0;
}

static int batch_finish_steps(vox_hip_batch_t* b);

static int batch_finish(vox_hip_batch_t* b) {
    if (!b->call.active) return set_err("batch_finish: no begun call");
    b->call.active = 0;
    const int r = batch_finish_steps(b);
    // every step of the call has been waited for (on an error the queue is waited for here):
    // the members may move their buffers again, the adapter buffers they outgrew are freed
    if (r < 0) (void)hipStreamSynchronize(b->st);
    batch_release(b);
    return r;
}

static int batch_finish_steps(vox_hip_batch_t* b) {
    auto& cl = b->call;
    const int n = cl.n, max_steps = cl.max_steps, K = cl.K;
    vox_hip_stream_t** streams = cl.streams;
    int* tokens_out = cl.tokens_out;
    int* counts_out = cl.counts_out;
    if (K == 0) {
        // a begun call with nothing to run (vox_hip_batch_begin_rows)
        for (int i = 0; i < n; i++) counts_out[i] = 0;
        b->lnb = 0;
        return 0;
    }
    BatchSlot* hs = b->hslots;
    int* htok = slot_toklog(hs, b->rows);
    int got[VOX_MAX_SLOTS] = {0};
    int done = 0, k = cl.k;
    for (;;) {
        // the chunk of k steps in flight (its slot table + token log copy queued behind it)
        CK(hipStreamSynchronize(b->st));
        done += k;
        bool any = false;
        for (int i = 0; i < n; i++) {
            const int p = hs[i].produced;
            for (int j = got[i]; j < p; j++) tokens_out[(size_t)i * max_steps + j] = htok[i * BATCH_TOKLOG + j % BATCH_TOKLOG];
            got[i] = p;
            any = any || hs[i].live;
        }
        if (!any || done >= K) break;
        k = std::min(STEP_BATCH, K - done);
        if (batch_run(b, cl.nb, cl.gb, cl.gi, cl.splits, cl.kvt, k, cl.gemv, cl.mixed, cl.ragged)) return -1;
        CK(hipMemcpyAsync(hs, b->slots, slot_bytes(b->rows), hipMemcpyDeviceToHost, b->st));
    }
    // 4. host mirrors
    int total = 0;
    const int stop_at_eos = cl.stop_at_eos;
    for (int i = 0; i < n; i++) {
        vox_hip_stream_t* s = streams[i];
        const int p = got[i];
        counts_out[i] = p;
        total += p;
        b->luid[i] = s->uid;
        b->llive[i] = p > 0 && p == done;
        if (!p) continue;
        const int last = tokens_out[(size_t)i * max_steps + p - 1];
        stream_steps_done(s, p, last);
        if (stop_at_eos && last == TOKEN_EOS) s->eos_seen = 1;
    }
    b->lnb = n;
    b->n_rows += total;
    if (cl.gemv) b->n_gemv_rows += total;
    return total;
}

static int batch_decode(vox_hip_batch_t* b, vox_hip_stream_t** streams, int n, const int* rows, int max_steps,
                        int stop_at_eos, int* tokens_out, int* counts_out) {
    const int r = batch_begin(b, streams, n, rows, max_steps, stop_at_eos, tokens_out, counts_out);
    if (r < 0) return -1;
    return r ? 0 : batch_finish(b);
}

extern "C" int vox_hip_batch_decode(vox_hip_batch_t* b, vox_hip_stream_t** streams, int n, int max_steps,
                                    int stop_at_eos, int* tokens_out, int* counts_out) {
    return batch_decode(b, streams, n, nullptr, max_steps, stop_at_eos, tokens_out, counts_out);
}

extern "C" int vox_hip_batch_begin_rows(vox_hip_batch_t* b, vox_hip_stream_t** streams, int n, const int* rows,
                                        int max_steps, int stop_at_eos, int* tokens_out, int* counts_out) {
    if (!rows) return set_err("batch_begin_rows: null rows");
    const int r = batch_begin(b, streams, n, rows, max_steps, stop_at_eos, tokens_out, counts_out);
    if (r < 0) return -1;
    if (r) {
        // nothing to run: an empty call that batch_finish completes
        b->call = {};
        b->call.active = 1;
        b->call.n = n;
        for (int i = 0; i < n; i++) b->call.streams[i] = streams[i];
        b->call.max_steps = max_steps;
        b->call.tokens_out = tokens_out;
        b->call.counts_out = counts_out;
        b->call.K = 0;
        b->call.k = 0;
        batch_hold(b);
    }
    return 0;
}

extern "C" int vox_hip_batch_finish(vox_hip_batch_t* b) {
    if (!b) return set_err("batch_finish: null batch");
    return batch_finish(b);
}

extern "C" int vox_hip_batch_decode_rows(vox_hip_batch_t* b, vox_hip_stream_t** streams, int n, const int* rows,
                                         int max_steps, int stop_at_eos, int* tokens_out, int* counts_out) {
    if (!rows) return set_err("batch_decode_rows: null rows");
    return batch_decode(b, streams, n, rows, max_steps, stop_at_eos, tokens_out, counts_out);
}

extern "C" int vox_hip_batch_read_logits(vox_hip_batch_t* b, vox_hip_stream_t* s, float* out) {
    if (!b || !s || !out) return set_err("batch_read_logits: null argument");
    const int V = b->m->c.vocab;
    for (int i = 0; i < b->lnb; i++)
        if (b->luid[i] == s->uid && b->llive[i]) {
            CK(hipMemcpyAsync(out, b->logits + (size_t)i * V, (size_t)V * 4, hipMemcpyDeviceToHost, b->st));
            CK(hipStreamSynchronize(b->st));
            return 0;
        }
    return set_err("batch_read_logits: the stream was not advanced by the last batched step");
}

// ragged calls (a listed stream's decoder rings shorter than the full size), their step replays
// and their graph captures, since creation
extern "C" int vox_hip_batch_kv_grow_stats(const vox_hip_batch_t* b, long long out3[3]) {
    if (!b || !out3) return set_err("batch_kv_grow_stats: null argument");
    out3[0] = b->n_ragged_calls;
    out3[1] = b->n_ragged_replays;
    out3[2] = b->n_ragged_captures;
    return 0;
}

extern "C" int vox_hip_batch_stats(const vox_hip_batch_t* b, long long* out6) {
    if (!b || !out6) return set_err("batch_stats: null argument");
    out6[0] = b->n_calls;
    out6[1] = b->n_replays;
    out6[2] = b->n_rows;
    out6[3] = b->n_captures;
    out6[4] = b->n_prefill_passes;
    out6[5] = b->n_prefilled;
    return 0;
}
