// fa_add_norm.hip - residual add + RMSNorm / LayerNorm over the whole hidden size, one launch (fa_add_norm, include/fa_mi355.h):
//     z = x, or round_res(float(x) + float(residual)) - ONE fp32 add, ONE rounding to residual_out's type;   residual_out = z
//     RMSNorm:   rstd = 1 / sqrt(sum z^2 / n + eps),  xhat = z rstd
//     LayerNorm: mean = sum z / n,  rstd = 1 / sqrt(sum (z - mean)^2 / n + eps),  xhat = (z - mean) rstd     (two passes in registers)
//     out = round16(xhat g),  with a bias round16(fmaf(xhat, g, b));   g = weight_offset + w
// The norm reads the STORED z: add_norm(x, residual) leaves the bits of add_norm(residual_out).  The row sums have fa_rowsum.h's
// fixed order, a function of n alone.  Two forms, chosen by n alone (row_shape):
//   n <= 256: fa_rmsnorm.h's ownership - a lane owns one 16-byte piece (8 columns) of one row, a row is owned by G adjacent lanes
//     of a wave, a workgroup takes 256 / G consecutive rows; no LDS.  Every cross-lane read sits outside every lane-dependent
//     branch: lanes past the row or past the last row load a valid piece, hand in +0 and store nothing.
//   n > 256: one workgroup per row, lane t owns the pieces t, t + threads, ..; the whole row stays in registers (64 fp32 values
//     per lane at n = 16384); the waves meet through LDS.
// A lane issues every load of x and residual that it owns before its first store, and it stores only columns it loaded: out == x
// and residual_out == residual are legal.  Ordinary 16-byte loads and stores.
#include <cstdint>
#include "fa_rowsum.h"

namespace fa {

struct AnArgs {
    const uint16_t* x;
    const void* res;                                      // nullptr: no residual
    uint16_t* out;
    void* res_out;                                        // nullptr: not written
    const void* w;
    const void* b;                                        // nullptr: no bias
    int64_t x_rs, res_rs, out_rs, ro_rs;                  // row strides, elements
    int64_t rows;
    int n, group_log2;
    int res_fp32, ro_fp32, w_fp32;
    float eps, w_offset;
};

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

// out of one piece from xhat's two factors: v = z (RMSNorm) or z - mean
template <typename T>
__device__ __forceinline__ void an_out8(const AnArgs& a, int64_t row, int d, const float (&v)[8], float rstd) {
    float g[8], y[8];
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
    row_store8<T>(a.out, row * a.out_rs + d, false, y);
}

template <typename T, bool LN>
__global__ void __launch_bounds__(ROW_THREADS) add_norm_small_kernel(const AnArgs a) {
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
    if constexpr (LN) {
        const float mean = rms_group_sum(row_piece_sum(z), lanes) / (float)a.n;
#pragma unroll
        for (int i = 0; i < 8; ++i) z[i] = act ? z[i] - mean : 0.f;
    }
    const float rstd = rms_rstd(rms_group_sum(row_piece_ss(z), lanes), a.n, a.eps);
    if (act) an_out8<T>(a, row, d, z, rstd);
}

template <typename T, bool LN, int NP>
__global__ void __launch_bounds__(ROW_THREADS) add_norm_wide_kernel(const AnArgs a) {
    __shared__ float red[2][ROW_WAVES];
    const int threads = (int)blockDim.x, nwaves = threads >> 6;
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
    if constexpr (LN) {
        float s = row_piece_sum(z[0]);
#pragma unroll
        for (int p = 1; p < NP; ++p) s += row_piece_sum(z[p]);
        const float mean = row_block_sum(s, red[0], nwaves, (int)threadIdx.x >> 6) / (float)a.n;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int i = 0; i < 8; ++i) z[p][i] = on[p] ? z[p][i] - mean : 0.f;
        }
    }
    float ss = row_piece_ss(z[0]);
#pragma unroll
    for (int p = 1; p < NP; ++p) ss += row_piece_ss(z[p]);
    const float rstd = rms_rstd(row_block_sum(ss, red[1], nwaves, (int)threadIdx.x >> 6), a.n, a.eps);
#pragma unroll
    for (int p = 0; p < NP; ++p)
        if (on[p]) an_out8<T>(a, row, d[p], z[p], rstd);
}

template <typename T, bool LN>
static void launch_an(const AnArgs& a, const RowShape& sh, hipStream_t stream) {
    if (a.n <= ROW_SMALL_MAX) {
        const int per = ROW_THREADS >> sh.group_log2;
        const dim3 g((unsigned)((a.rows + per - 1) / per)), b(ROW_THREADS);
        hipLaunchKernelGGL((add_norm_small_kernel<T, LN>), g, b, 0, stream, a);
        return;
    }
    const dim3 g((unsigned)a.rows), b(sh.threads);
    switch (sh.pieces) {
    case 1:  hipLaunchKernelGGL((add_norm_wide_kernel<T, LN, 1>), g, b, 0, stream, a); break;
    case 2:  hipLaunchKernelGGL((add_norm_wide_kernel<T, LN, 2>), g, b, 0, stream, a); break;
    case 4:  hipLaunchKernelGGL((add_norm_wide_kernel<T, LN, 4>), g, b, 0, stream, a); break;
    default: hipLaunchKernelGGL((add_norm_wide_kernel<T, LN, 8>), g, b, 0, stream, a); break;
    }
}

// The caller (fa_api.hip) has validated the block; rows > 0
void launch_add_norm(const fa_add_norm_params& s, hipStream_t stream) {
    const RowShape sh = row_shape(s.n);
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
    const bool ln = !s.is_rms_norm;
    if (s.dtype == FA_BF16) {
        if (ln) launch_an<bf16_tag, true>(a, sh, stream);
        else    launch_an<bf16_tag, false>(a, sh, stream);
    } else {
        if (ln) launch_an<fp16_tag, true>(a, sh, stream);
        else    launch_an<fp16_tag, false>(a, sh, stream);
    }
}

}  // namespace fa
