// fa_moe_gemm.h - the host side that fa_moe_gemm.hip and the entry points (fa_api.hip) share: the limits of fa_moe_gemm and its
// launch plan.  Everything here is a function of the shapes alone: no device data, no synchronisation.
#pragma once
#include <cstdint>
#include "fa_mi355.h"
#include "fa_moe.h"
#include <hip/hip_runtime.h>

namespace fa {

constexpr int MOE_GEMM_MAX_K = 32768;
constexpr int MOE_GEMM_MAX_N = 65536;
constexpr int64_t MOE_GEMM_MAX_ROW_STRIDE = (int64_t)1 << 22;   // elements: a tile's 128 rows stay inside a 31-bit byte offset
constexpr int MOE_GEMM_BN = 128;                          // output columns of a tile, every plan
constexpr int MOE_GEMM_BK = 64;                           // contraction elements staged per step: four MFMA k-steps of 16
constexpr int MOE_GEMM_BM_WIDE = 128;                     // prefill: 2 x 2 waves of 64 x 64
constexpr int MOE_GEMM_BM_DECODE = 32;                    // decode: an expert sees a handful of rows, 4 waves of 32 rows x 32 columns

// Segment lengths are device data.  E segments and the +0 tail behind expert_offsets[E] cut M_max rows into E + 1 pieces, which
// need at most floor(M_max / BM) + E + 1 tiles of BM rows; the grid is that bound and a workgroup without a tile leaves at once.
// The decode shape is taken where a segment has 32 rows or fewer on average.
struct MoeGemmPlan { int bm, bn, bk; int64_t grid_m; int grid_n; };
static inline MoeGemmPlan moe_gemm_plan(int64_t m_max, int n, int k, int E, int layout, int dtype) {
    (void)k; (void)layout; (void)dtype;
    MoeGemmPlan pl;
    pl.bm = m_max <= (int64_t)MOE_GEMM_BM_DECODE * E ? MOE_GEMM_BM_DECODE : MOE_GEMM_BM_WIDE;
    pl.bn = MOE_GEMM_BN;
    pl.bk = MOE_GEMM_BK;
    pl.grid_m = m_max > 0 ? m_max / pl.bm + E + 1 : 0;
    pl.grid_n = (n + MOE_GEMM_BN - 1) / MOE_GEMM_BN;
    return pl;
}

void launch_moe_gemm(const fa_moe_gemm_params& s, hipStream_t stream);

// fa_moe_gemm_wgrad (fa_moe_gemm_wgrad.hip): one workgroup per 128 x 128 tile of one expert's dW, the segment's rows staged 64 a
// step.  dW is dense, so the grid is (ceil(n / 128), ceil(k / 128), E) whatever the segments hold.
constexpr int MOE_WGRAD_BN = 128;                         // tile extent along n (the columns of dy)
constexpr int MOE_WGRAD_BK = 128;                         // tile extent along k (the columns of x)
constexpr int MOE_WGRAD_BR = 64;                          // segment rows staged per step: four MFMA steps of 16
struct MoeWgradPlan { int bn, bk, br; int64_t grid_n, grid_k, grid_e; };
static inline MoeWgradPlan moe_gemm_wgrad_plan(int n, int k, int E, int layout, int dtype) {
    (void)layout; (void)dtype;
    MoeWgradPlan pl;
    pl.bn = MOE_WGRAD_BN;
    pl.bk = MOE_WGRAD_BK;
    pl.br = MOE_WGRAD_BR;
    pl.grid_n = (n + MOE_WGRAD_BN - 1) / MOE_WGRAD_BN;
    pl.grid_k = (k + MOE_WGRAD_BK - 1) / MOE_WGRAD_BK;
    pl.grid_e = E;
    return pl;
}

void launch_moe_gemm_wgrad(const fa_moe_gemm_wgrad_params& s, hipStream_t stream);

}  // namespace fa
