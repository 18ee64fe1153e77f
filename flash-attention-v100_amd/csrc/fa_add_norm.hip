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
// The two forms are fa_add_norm.h's bodies, which fa_add_norm_quant (fa_quant.hip) shares; this source adds the epilogue that
// stores `out`, and the launch.
#include <cstdint>
#include "fa_add_norm.h"

namespace fa {

// the epilogue of fa_add_norm: a piece of `out` is rounded and stored; nothing is left to do for the row
template <typename T>
struct AnStore {
    __device__ __forceinline__ void piece(const AnArgs& a, int, int64_t row, int d, const float (&y)[8]) const {
        row_store8<T>(a.out, row * a.out_rs + d, false, y);
    }
    template <typename... Row>
    __device__ __forceinline__ void row(const Row&...) const {}
};

template <typename T, bool LN>
__global__ void __launch_bounds__(ROW_THREADS) add_norm_small_kernel(const AnArgs a) {
    AnStore<T> epi;
    an_small_body<T, LN>(a, epi);
}

template <typename T, bool LN, int NP>
__global__ void __launch_bounds__(ROW_THREADS) add_norm_wide_kernel(const AnArgs a) {
    __shared__ float red[2][ROW_WAVES];
    AnStore<T> epi;
    an_wide_body<T, LN, NP>(a, red, epi);
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
    const AnArgs a = an_args(s, sh);
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
