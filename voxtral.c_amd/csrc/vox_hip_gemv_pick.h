// vox_hip_gemv_pick.h -- which k_gemv / k_gemvr instances exist, and the instance pickers that each
// weight format's object exports.  One format per object: vox_hip_gemv_<format>.hip holds one line,
// VOX_GEMV_FORMAT(WF, name), which instantiates that format's instances of both kernels and defines
// gemv_pick_<name> / gemvr_pick_<name>; vox_hip_gemv.hip (host code only) calls the picker of a
// launch's format and launches the pointer it returns.
#pragma once
#include "vox_hip_gemv.h"

namespace vox {

// the wpack13 and wmx4 instances: the decoder step's GEMVs (and STORE for a single packed GEMV);
// the encoder's single-row chunks stay bf16
template <int P, int E>
constexpr bool gemv_p13 = (P == PRO_NONE && (E == EPI_STORE || E == EPI_RESID)) || (P == PRO_NORM && E == EPI_QKV) ||
                          (P == PRO_NORM_ADA && E == EPI_SWIGLU) ||
                          (P == PRO_NORM && (E == EPI_LOGITS || E == EPI_LOGITS_ALT));

template <int P, int E, int RB, int WF>
static const void* gemv_fn(int kq) {
    if constexpr (WF == WF_BF16 || WF == WF_Q8 || gemv_p13<P, E>) {
        switch (kq) {
            case 1: return reinterpret_cast<const void*>(&k_gemv<P, E, RB, 1, WF>);
            case 2: return reinterpret_cast<const void*>(&k_gemv<P, E, RB, 2, WF>);
            case 3: return reinterpret_cast<const void*>(&k_gemv<P, E, RB, 3, WF>);
            case 4: return reinterpret_cast<const void*>(&k_gemv<P, E, RB, 4, WF>);
            case 5: return reinterpret_cast<const void*>(&k_gemv<P, E, RB, 5, WF>);
        }
    }
    return nullptr;
}

// k_gemv<pro, epi, rb, kq, WF>, or null: rb = rows per group, kq = K rounds of 256 chunks
template <int WF>
static const void* gemv_pick(int pro, int epi, int rb, int kq) {
#define GEMV_FN(P, E)         \
    if (pro == P && epi == E) \
        return rb == 8 ? gemv_fn<P, E, 8, WF>(kq) : rb == 2 ? gemv_fn<P, E, 2, WF>(kq) : gemv_fn<P, E, 4, WF>(kq);
    GEMV_FN(PRO_NONE, EPI_STORE) GEMV_FN(PRO_NONE, EPI_RESID) GEMV_FN(PRO_NORM, EPI_QKV)
    GEMV_FN(PRO_NORM_ADA, EPI_SWIGLU) GEMV_FN(PRO_NORM, EPI_LOGITS) GEMV_FN(PRO_NORM, EPI_LOGITS_ALT)
    // the encoder's single-row chunks (run_encoder_rows_gemv)
    GEMV_FN(PRO_NORM, EPI_QKV_BIAS) GEMV_FN(PRO_NORM, EPI_SWIGLU)
#undef GEMV_FN
    return nullptr;
}

// k_gemvr instances: 8-row groups only where the LM head has them (STORE), and more than two
// K rounds only where the input is not a dec_dim row (wo and W2: PRO_NONE) and the group is
// not the LM head's.  The MX4 instances exist for the 4- and 8-row groups of the wmx4 plane
// (gemv_rb_mx4 of a row count that is a multiple of 4); a 2-row wmx4 plane has none.  The Q8
// instances: K rounds of 256 16-weight chunks, 1..3 of them (K <= 12,288)
template <int P, int E, int RB, int KQ, int WF>
constexpr bool gemvr_inst = (RB < 8 || E == EPI_STORE) && (KQ <= 2 || (P == PRO_NONE && RB < 8)) &&
                            (WF != WF_MX4 || RB >= 4) && (WF != WF_Q8 || KQ <= 3);

template <int P, int E, int RB, int KQ, int WF>
static const void* gemvr_fn_r(int R) {
    if constexpr (gemvr_inst<P, E, RB, KQ, WF>) {
        switch (R) {
            case 1: return reinterpret_cast<const void*>(&k_gemvr<P, E, RB, KQ, WF, 1>);
            case 2: return reinterpret_cast<const void*>(&k_gemvr<P, E, RB, KQ, WF, 2>);
            case 4: return reinterpret_cast<const void*>(&k_gemvr<P, E, RB, KQ, WF, 4>);
            case 8: return reinterpret_cast<const void*>(&k_gemvr<P, E, RB, KQ, WF, 8>);
        }
    }
    return nullptr;
}
template <int P, int E, int RB, int WF>
static const void* gemvr_fn_kq(int kq, int R) {
    switch (kq) {
        case 1: return gemvr_fn_r<P, E, RB, 1, WF>(R);
        case 2: return gemvr_fn_r<P, E, RB, 2, WF>(R);
        case 3: return gemvr_fn_r<P, E, RB, 3, WF>(R);
        case 4: return gemvr_fn_r<P, E, RB, 4, WF>(R);
        case 5: return gemvr_fn_r<P, E, RB, 5, WF>(R);
        default: return nullptr;
    }
}

// k_gemvr<pro, epi, rb, kq, WF, R>, or null
template <int WF>
static const void* gemvr_pick(int pro, int epi, int rb, int kq, int R) {
#define GEMVR_FN(P, E)                                       \
    if (pro == P && epi == E)                                \
        return rb == 2   ? gemvr_fn_kq<P, E, 2, WF>(kq, R)   \
               : rb == 4 ? gemvr_fn_kq<P, E, 4, WF>(kq, R)   \
               : rb == 8 ? gemvr_fn_kq<P, E, 8, WF>(kq, R)   \
                         : nullptr;
    GEMVR_FN(PRO_NORM, EPI_QKV) GEMVR_FN(PRO_NONE, EPI_RESID) GEMVR_FN(PRO_NORM_ADA, EPI_SWIGLU)
    GEMVR_FN(PRO_NORM, EPI_STORE) GEMVR_FN(PRO_NONE, EPI_STORE)
#undef GEMVR_FN
    return nullptr;
}

#ifdef VOX_GEMV_STAMPS
#define VOX_GEMV_FORMAT_STAMPS(name)                                  \
    hipError_t gemv_set_stamps_##name(unsigned long long* p) {        \
        return hipMemcpyToSymbol(HIP_SYMBOL(g_gemv_stamps), &p, sizeof p); \
    }
#else
#define VOX_GEMV_FORMAT_STAMPS(name)
#endif

// the whole of a format's .hip file
#define VOX_GEMV_FORMAT(WF, name)                                                                                 \
    namespace vox {                                                                                               \
    const void* gemv_pick_##name(int pro, int epi, int rb, int kq) { return gemv_pick<WF>(pro, epi, rb, kq); }     \
    const void* gemvr_pick_##name(int pro, int epi, int rb, int kq, int R) {                                      \
        return gemvr_pick<WF>(pro, epi, rb, kq, R);                                                               \
    }                                                                                                             \
    VOX_GEMV_FORMAT_STAMPS(name)                                                                                  \
    }

}  // namespace vox
