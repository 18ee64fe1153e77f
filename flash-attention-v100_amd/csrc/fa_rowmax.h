// fa_rowmax.h - the cross-lane maxima of the quantising row ops (fa_quant.hip), beside fa_rowsum.h's sums and with their lane
// ownership.  a = fmaxf(+0, |y_0|, |y_1|, ..) is exact and does not depend on the order, so - unlike a sum - nothing here fixes
// one; fmaxf skips a NaN, and a set of NaNs alone gives +0.  Lanes past the row hand in +0.
#pragma once
#include "fa_common.h"

namespace fa {

// the lane's part: the 8 columns of one piece of 16-bit values
template <typename T>
__device__ __forceinline__ float row_piece_amax(const u32x4& y) {
    using E = Elem<T>;
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) a = fmaxf(a, fmaxf(fabsf(E::lo(y[i])), fabsf(E::hi(y[i]))));
    return a;
}

// the maximum over `lanes` adjacent lanes (a power of two <= 64, uniform over the wave): EVERY lane of the wave must call this
__device__ __forceinline__ float row_group_max(float a, int lanes) {
    for (int m = 1; m < lanes; m <<= 1) a = fmaxf(a, __shfl_xor(a, m));
    return a;
}

// the maximum over a row owned by `nwaves` whole waves; slot: nwaves floats of LDS that nothing else in flight uses.  EVERY lane
// of the workgroup must call this.  One wave: no LDS, no barrier
__device__ __forceinline__ float row_block_max(float a, float* slot, int nwaves, int wave) {
    a = row_group_max(a, 64);
    if (nwaves == 1) return a;
    if ((threadIdx.x & 63) == 0) slot[wave] = a;
    __syncthreads();
    float t = slot[0];
    for (int w = 1; w < nwaves; ++w) t = fmaxf(t, slot[w]);
    return t;
}

}  // namespace fa
