// fa_add_norm.h - the forward of the fused norm from the loads to the fp32 value of `out`, ONCE: fa_add_norm (fa_add_norm.hip)
// and fa_add_norm_quant (fa_quant.hip) are this body with two epilogues, so add_norm_quant(..) == quant_fp8(add_norm(..)) bit for
// bit by construction.  The formulas and the two forms (n <= 256, n > 256) are in fa_add_norm.hip's header; the row sums, mean and
// rstd are fa_rowsum.h's.  An epilogue has
//     piece(a, p, row, d, y)  the lane's piece p (column d) of `out` in fp32, called for the pieces the lane owns; it rounds ONCE
//                             to the 16-bit type (row_store8, or Elem<T>::pack2 - the same rounding);
//     row(..)                 called by EVERY lane after its pieces, outside every lane-dependent branch: the quantising epilogue
//                             has cross-lane reads and a barrier in it.
// A lane issues every load of x and residual that it owns before its first store, and it stores only columns it loaded.
// The bodies take AnArgs BY VALUE and hand it to piece(): hipcc optimises a body before it inlines it into the kernel, and behind a
// reference every store might change the arguments - the LayerNorm kernels at 4096 < n came out 0.7 % slower that way
// (profiles/add_norm.txt).
#pragma once
#include <cstdint>
#include "fa_rowsum.h"

namespace fa {

struct AnArgs {
    const uint16_t* x;
    const void* res;                                      // nullptr: no residual
    uint16_t* out;                                        // (fa_add_norm_quant: nullptr, out_rs 0)
    void* res_out;                                        // nullptr: not written
    const void* w;
    const void* b;                                        // nullptr: no bias
    int64_t x_rs, res_rs, out_rs, ro_rs;                  // row strides, elements
    int64_t rows;
    int n, group_log2;
    int res_fp32, ro_fp32, w_fp32;
    float eps, w_offset;
};

static inline AnArgs an_args(const fa_add_norm_params& s, const RowShape& sh) {
    AnArgs a;
    a.x = static_cast<const uint16_t*>(s.x);
    a.res = s.residual;
    a.out = static_cast<uint16_t*>(s.out);
    a.res_out = s.residual_out;
    a.w = s.weight;
    a.b = s.bias;
    a.x_rs = s.x_row_stride; a.res_rs = s.residual_row_stride; a.out_rs = s.out_row_stride; a.ro_rs = s.residual_out_row_stride;
    a.rows = s.rows;
    a.n = s.n; a.group_log2 = sh.group_log2;
    a.res_fp32 = s.residual_dtype == FA_FP32;
    a.ro_fp32 = s.residual_out_dtype == FA_FP32;
    a.w_fp32 = s.weight_dtype == FA_FP32;
    a.eps = s.eps; a.w_offset = s.weight_offset;
    return a;
}

// z of one piece: the loads, the add and the rounding to residual_out's type
template <typename T>
__device__ __forceinline__ void an_z8(const AnArgs& a, int64_t row, int d, float (&z)[8]) {
    row_load8<T>(a.x, row * a.x_rs + d, false, z);
    if (a.res) {
        float r[8];
        row_load8<T>(a.res, row * a.res_rs + d, a.res_fp32 != 0, r);
#pragma unroll
        for (int i = 0; i < 8; ++i) z[i] += r[i];
        if (!a.ro_fp32) row_round8<T>(z);
    }
}

// the fp32 value `out` is rounded from, of one piece, from xhat's two factors: v = z (RMSNorm) or z - mean
template <typename T>
__device__ __forceinline__ void an_y8(const AnArgs& a, int d, const float (&v)[8], float rstd, float (&y)[8]) {
    float g[8];
    rms_gains<T>(a.w, d, a.w_fp32 != 0, a.w_offset, g);
    if (a.b) {
        float b[8];
        row_load8<T>(a.b, d, a.w_fp32 != 0, b);
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = fmaf(v[i] * rstd, g[i], b[i]);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = (v[i] * rstd) * g[i];
    }
}

// n <= 256: a lane owns one piece of one row; lanes past the row or past the last row load a valid piece, hand in +0 and store
// nothing
template <typename T, bool LN, typename Epi>
__device__ __forceinline__ void an_small_body(const AnArgs a, Epi& epi) {
    const int lanes = 1 << a.group_log2;
    const int j = (int)threadIdx.x & (lanes - 1);
    const bool piece = 8 * j < a.n;
    const int d = piece ? 8 * j : 0;                      // (clamped: the loads stay inside the row)
    const int64_t r = (int64_t)blockIdx.x * (ROW_THREADS >> a.group_log2) + ((int)threadIdx.x >> a.group_log2);
    const bool act = piece && r < a.rows;
    const int64_t row = r < a.rows ? r : 0;               // (a slot past the last row: row 0)
    float z[8];
    an_z8<T>(a, row, d, z);
    if (act && a.res_out) row_store8<T>(a.res_out, row * a.ro_rs + d, a.ro_fp32 != 0, z);
    if (!act) {
#pragma unroll
        for (int i = 0; i < 8; ++i) z[i] = 0.f;
    }
    const float rstd = row_small_stats<LN>(z, act, lanes, a.n, a.eps);
    if (act) {
        float y[8];
        an_y8<T>(a, d, z, rstd, y);
        epi.piece(a, 0, row, d, y);
    }
    epi.row(row, act, d, lanes);
}

// n > 256: one workgroup per row, lane t owns the pieces t, t + threads, ..; red: the LDS slots of the two row sums
template <typename T, bool LN, int NP, typename Epi>
__device__ __forceinline__ void an_wide_body(const AnArgs a, float (&red)[2][ROW_WAVES], Epi& epi) {
    const int threads = (int)blockDim.x;
    const int64_t row = blockIdx.x;
    float z[NP][8];
    int d[NP];
    bool on[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int c = 8 * ((int)threadIdx.x + p * threads);
        on[p] = c < a.n;
        d[p] = on[p] ? c : 0;
        an_z8<T>(a, row, d[p], z[p]);
    }
    if (a.res_out) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
            if (on[p]) row_store8<T>(a.res_out, row * a.ro_rs + d[p], a.ro_fp32 != 0, z[p]);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if (!on[p]) {
#pragma unroll
            for (int i = 0; i < 8; ++i) z[p][i] = 0.f;
        }
    }
    const float rstd = row_wide_stats<LN, NP>(z, on, red[0], red[1], threads >> 6, (int)threadIdx.x >> 6, a.n, a.eps);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if (on[p]) {
            float y[8];
            an_y8<T>(a, d[p], z[p], rstd, y);
            epi.piece(a, p, row, d[p], y);
        }
    }
    epi.row(row, on, d);
}

}  // namespace fa
