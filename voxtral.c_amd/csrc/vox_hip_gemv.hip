// vox_hip_gemv.hip -- host side of the weight-streaming GEMVs: shapes, row groups, grids and the
// launches of k_gemv / k_gemvr.  No kernel lives here: the instances are in one object per weight
// format (vox_hip_gemv_bf16 / _p13 / _mx4 / _q8.hip), each behind its instance picker.
#include "vox_hip_internal.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

namespace vox {

#define GEMV_FORMATS(X) X(WF_BF16, bf16) X(WF_P13, p13) X(WF_MX4, mx4) X(WF_Q8, q8)
// k_gemv<pro, epi, rb, kq, WF> / k_gemvr<pro, epi, rb, kq, WF, R> of each format, or null (vox_hip_gemv_pick.h)
#define GEMV_PICK_DECL(WF, name)                                   \
    const void* gemv_pick_##name(int pro, int epi, int rb, int kq); \
    const void* gemvr_pick_##name(int pro, int epi, int rb, int kq, int R);
GEMV_FORMATS(GEMV_PICK_DECL)
#undef GEMV_PICK_DECL

#ifdef VOX_GEMV_STAMPS
// diagnostic build only (tools/kbench_stamps): where k_gemv's per-block stamps go (null: off)
#define GEMV_STAMPS_DECL(WF, name) hipError_t gemv_set_stamps_##name(unsigned long long* p);
GEMV_FORMATS(GEMV_STAMPS_DECL)
#undef GEMV_STAMPS_DECL
hipError_t gemv_set_stamps(unsigned long long* p) {
#define GEMV_STAMPS_SET(WF, name) \
    if (hipError_t e = gemv_set_stamps_##name(p); e != hipSuccess) return e;
    GEMV_FORMATS(GEMV_STAMPS_SET)
#undef GEMV_STAMPS_SET
    return hipSuccess;
}
#endif
VOX_KB_KNOB(g_gemv_rb, 0);  // tools/kbench knob: force 4- or 8-row groups (0 = automatic)
// Rows per group: each block should stream at least two groups, so that the next group's
// loads overlap this group's reduction and epilogue (one group per block left every block
// idle at its tail).  tools/kbench, bf16 / 768 blocks: QKV 10.2 -> 8.5 us with 4-row
// groups, W1|W3 20.5 -> 20.0, W2 12.1 -> 11.4 and wo 6.7 -> 6.4 with 2-row groups; the LM
// head (16 groups per block at 8 rows) keeps 8.
static int gemv_rb(int rows) {
    if (g_gemv_rb && rows % g_gemv_rb == 0) return g_gemv_rb;
    if (rows >= 65536 && rows % 8 == 0) return 8;
    if (rows >= 6144 && rows % 4 == 0) return 4;
    return 2;
}

int gemv_rowgroup(int rows) { return gemv_rb(rows); }
// wmx4 instances: a 2-row group's record would carry half a dword of padding (6 bits per
// weight instead of 5) and a quarter of a bf16 group's bytes, so they take at least 4 rows
// where the row count allows it; each row's bits do not depend on the group size
static int gemv_rb_mx4(int rows) {
    const int rb = gemv_rb(rows);
    return rb < 4 && rows % 4 == 0 ? 4 : rb;
}
int gemv_rowgroup_mx4(int rows) { return gemv_rb_mx4(rows); }

VOX_KB_KNOB(g_gemv_maxb, 0);  // tools/kbench knob: grid cap other than GEMV_MAX_BLOCKS (no LM head)
static int gemv_grid_rb(int rows, int rb) {
    // the largest divisor of the group count that fits 4 blocks per CU: every block then
    // runs the same number of groups (no tail); tools/kbench VOX_KB_ONLY=grid: 1536-2304
    // blocks were slower on every decode shape, bf16 and Q8 (profiles/r3_kbench_gemv_grid.txt)
    const int ng = rows / rb, maxb = g_gemv_maxb ? g_gemv_maxb : GEMV_MAX_BLOCKS;
    int best = 1;
    for (int gsz = 1; gsz <= maxb && gsz <= ng; gsz++)
        if (ng % gsz == 0) best = gsz;
    if (best < 256 && ng > maxb) best = maxb;  // no good divisor: accept a tail
    return best;
}
int gemv_grid(int rows) { return gemv_grid_rb(rows, gemv_rb(rows)); }
int gemv_grid_mx4(int rows) { return gemv_grid_rb(rows, gemv_rb_mx4(rows)); }

int gemv_occupancy(const void* fn) {
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 256, 0) != hipSuccess) occ = 0;
    return occ;
}

// the shapes launch_gemv accepts: whole 16-B chunks per row, whole row groups, and at most
// 5 rounds of 256 chunks per row (the instantiated KQ)
bool gemv_ok(int rows, int K, int q8) {
    const int kc = q8 ? K >> 4 : K >> 3;
    return rows > 0 && K > 0 && K % (q8 ? 16 : 8) == 0 && rows % gemv_rb(rows) == 0 && (kc + 255) / 256 <= 5;
}

// the shapes the wmx4 instances accept: gemv_ok's, whole 32-weight blocks, whole wmx4 row
// groups, and a plane that a 32-bit buffer offset reaches
bool gemv_ok_mx4(int rows, int K) {
    if (!gemv_ok(rows, K, 0) || K % 32 || rows % gemv_rb_mx4(rows)) return false;
    const int rb = gemv_rb_mx4(rows);
    return (long long)rows / rb * (K / 8) * (rb + (rb + 3) / 4) * 4 < (1LL << 31);
}

// weight source of a launch: Q8 rows (wscale), the wmx4 plane, the wpack13 planes, the raw rows
static int gemv_wf(const GemvArgs& a) { return a.wscale ? WF_Q8 : a.wm_plane ? WF_MX4 : a.wp_main ? WF_P13 : WF_BF16; }
// row group, grid and K rounds of a launch: the wmx4 plane has its own group size, Q8 rows 16-weight chunks
static int gemv_rb_wf(int rows, int wf) { return wf == WF_MX4 ? gemv_rb_mx4(rows) : gemv_rb(rows); }
static int gemv_grid_wf(int rows, int wf) { return gemv_grid_rb(rows, gemv_rb_wf(rows, wf)); }
static int gemv_kq(int K, int wf) { return ((wf == WF_Q8 ? K >> 4 : K >> 3) + 255) / 256; }

// kernel instance launch_gemv uses (also tools, occupancy queries)
const void* gemv_kernel(int pro, int epi, const GemvArgs& a) {
    const int wf = gemv_wf(a), rb = gemv_rb_wf(a.rows, wf), kq = gemv_kq(a.K, wf);
#define GEMV_PICK(WF, name) \
    if (wf == WF) return gemv_pick_##name(pro, epi, rb, kq);
    GEMV_FORMATS(GEMV_PICK)
#undef GEMV_PICK
    return nullptr;
}

// The same launch with HIP events recorded by the kernel's own dispatch packet
// (hipExtLaunchKernel): they bracket the kernel itself, not the marker packets an
// event-record node adds.  Eager launches only (not capturable into a graph).
hipError_t launch_gemv_timed(int pro, int epi, const GemvArgs& a, hipEvent_t start, hipEvent_t stop,
                             hipStream_t st) {
    const void* fn = gemv_kernel(pro, epi, a);
    if (!fn) return hipErrorInvalidValue;
    GemvArgs args = a;
    void* kargs[] = {&args};
    return hipExtLaunchKernel(fn, dim3(gemv_grid_wf(a.rows, gemv_wf(a))), dim3(256), kargs, 0, st, start, stop, 0);
}

hipError_t launch_gemv(int pro, int epi, const GemvArgs& a, hipStream_t st) {
    if (!gemv_ok(a.rows, a.K, a.wscale != nullptr)) return hipErrorInvalidValue;
    if (gemv_wf(a) == WF_MX4 && !gemv_ok_mx4(a.rows, a.K)) return hipErrorInvalidValue;
    if (epi == EPI_QKV_BIAS && !a.bias) return hipErrorInvalidValue;
    const void* fn = gemv_kernel(pro, epi, a);
    if (!fn) return hipErrorInvalidValue;
    GemvArgs args = a;
    void* kargs[] = {&args};
    return hipLaunchKernel(fn, dim3(gemv_grid_wf(a.rows, gemv_wf(a))), dim3(256), kargs, 0, st);
}

static const void* gemvr_pick(int pro, int epi, int rows, int K, int wf, int R) {
    if (!gemv_ok(rows, K, wf == WF_Q8)) return nullptr;
    if (wf == WF_MX4 && !gemv_ok_mx4(rows, K)) return nullptr;
    const int rb = gemv_rb_wf(rows, wf), kq = gemv_kq(K, wf);
#define GEMVR_PICK(WF, name) \
    if (wf == WF) return gemvr_pick_##name(pro, epi, rb, kq, R);
    GEMV_FORMATS(GEMVR_PICK)
#undef GEMVR_PICK
    return nullptr;
}

bool gemvr_ok(int pro, int epi, int rows, int K) { return gemvr_pick(pro, epi, rows, K, WF_BF16, 1) != nullptr; }
bool gemvr_ok_mx4(int pro, int epi, int rows, int K) { return gemvr_pick(pro, epi, rows, K, WF_MX4, 1) != nullptr; }
bool gemvr_ok_q8(int pro, int epi, int rows, int K) { return gemvr_pick(pro, epi, rows, K, WF_Q8, 1) != nullptr; }

// kernel instance launch_gemvr uses (also tools, occupancy queries)
const void* gemvr_kernel(int pro, int epi, int R, const GemvRArgs& a) {
    return gemvr_pick(pro, epi, a.g.rows, a.g.K, gemv_wf(a.g), R);
}

hipError_t launch_gemvr(int pro, int epi, int R, const GemvRArgs& a, hipStream_t st) {
    if (a.g.bias || (epi == EPI_QKV && !a.slots)) return hipErrorInvalidValue;
    const void* fn = gemvr_kernel(pro, epi, R, a);
    if (!fn) return hipErrorInvalidValue;
    GemvRArgs args = a;
    void* kargs[] = {&args};
    return hipLaunchKernel(fn, dim3(gemv_grid_wf(a.g.rows, gemv_wf(a.g))), dim3(256), kargs, 0, st);
}

}  // namespace vox
