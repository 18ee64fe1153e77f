// fa_lse.h - the fixed-order running (max, sum-exp) of fa_cross_entropy (fa_cross_entropy.hip), beside fa_rowsum.h's sums: the state
// of a set of columns is (m, s) with  sum_j exp(l_j) = s exp(m),  m the largest l_j that is not a NaN (-inf: none yet).
//   - a piece of 8 columns enters in column order (lse_piece): mn = max(m, max_i l_i);  ps = e(l_0 - b), ps += e(l_i - b) for
//     i = 1 .. 7;  s = fma(s, e(m - b), ps);  m = mn - where b = mn, or 0 while mn is still -inf, so that -inf - (-inf) never
//     reaches an exp: a column of -inf adds exactly 0, a NaN or a +inf column makes s a NaN (the maximum skips NaNs, the sum
//     does not);
//   - two states meet in lse_merge: mn = max(a.m, b.m), s = a.s e(a.m - b) + b.s e(b.m - b) - two products and ONE addition, never
//     contracted into a fused multiply-add, so both lanes of a butterfly pair compute the same bits;
//   - over a wave: the xor butterfly m = 1, 2, 4, .. 32 (lse_wave); over the workgroup: lane 0 of every wave writes its state to
//     LDS and the waves are merged in index order (lse_block); over the chunks of a row: in chunk order (the merge kernel).
// e(t) = exp2(t log2(e)): one product, one v_exp_f32 (lse_exp).  The order depends on the columns' positions alone.
// This header switches fused contraction OFF for the translation unit that includes it: every fma in it is written out.
#pragma once
#include "fa_rowsum.h"

#pragma clang fp contract(off)

namespace fa {

struct LseState { float m, s; };

__device__ __forceinline__ float lse_exp(float t) { return fast_exp2(t * kLog2e); }

// the value the differences are taken against: the maximum, or 0 while there is none
__device__ __forceinline__ float lse_base(float m) { return m == -INFINITY ? 0.f : m; }

__device__ __forceinline__ void lse_piece(LseState& st, const float (&l)[8]) {
    float pm = l[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) pm = fmaxf(pm, l[i]);
    const float mn = fmaxf(st.m, pm);
    const float b = lse_base(mn);
    float ps = lse_exp(l[0] - b);
#pragma unroll
    for (int i = 1; i < 8; ++i) ps += lse_exp(l[i] - b);
    st.s = fmaf(st.s, lse_exp(st.m - b), ps);
    st.m = mn;
}

__device__ __forceinline__ LseState lse_merge(const LseState& a, const LseState& b) {
    const float mn = fmaxf(a.m, b.m);
    const float base = lse_base(mn);
    const float ta = a.s * lse_exp(a.m - base);
    const float tb = b.s * lse_exp(b.m - base);
    return LseState{mn, ta + tb};
}

// EVERY lane of the wave must call this; afterwards every lane holds the same state
__device__ __forceinline__ LseState lse_wave(LseState st) {
    for (int m = 1; m < 64; m <<= 1) {
        const LseState o = {__shfl_xor(st.m, m), __shfl_xor(st.s, m)};
        st = lse_merge(st, o);
    }
    return st;
}

// the state of the workgroup's columns from every wave's (lse_wave); slots: 2 * ROW_WAVES floats of LDS.  EVERY lane of the
// workgroup must call this (it holds the barrier)
__device__ __forceinline__ LseState lse_block(LseState st, float* slots, int nwaves, int wave) {
    if (nwaves == 1) return st;
    if ((threadIdx.x & 63) == 0) { slots[wave] = st.m; slots[ROW_WAVES + wave] = st.s; }
    __syncthreads();
    LseState t = {slots[0], slots[ROW_WAVES]};
    for (int w = 1; w < nwaves; ++w) t = lse_merge(t, LseState{slots[w], slots[ROW_WAVES + w]});
    return t;
}

}  // namespace fa
