// fa_rmsnorm.h - RMSNorm of one head whose columns lie 8 per lane (one 16-byte piece) in G adjacent lanes of a wave, G a power of
// two.  Every form of fa_qk_norm_rope_store (fa_qk_norm_rope_store.hip) goes through these functions, so a head has the same bits
// in all of them:
//     ss   = sum_d x[d]^2                                  fp32
//     rstd = 1 / sqrt(ss / head_dim + eps)                 fp32: an IEEE division, a correctly rounded root, an IEEE division
//     y[d] = round16((x[d] * rstd) * (offset + w[d]))      fp32: one sum and two products, then ONE rounding to the io type
// The order of the sum is fixed:
//   - in a lane: s = x0 * x0, then s = fmaf(xi, xi, s) for i = 1 .. 7, in column order;
//   - across the G lanes: a xor butterfly, s += s of lane ^ m for m = 1, 2, 4, .. G / 2.  Both lanes of a pair add the same two
//     numbers, so after the last stage every lane of the group holds the same bits;
//   - lanes of the group past the head hand in +0.
// Nothing but the head's own columns enters, whatever other rows or heads the batch holds.  No LDS, no atomics, no workspace.
#pragma once
#include "fa_common.h"

namespace fa {

// the lane's part of the sum: its 8 columns in column order
template <typename T>
__device__ __forceinline__ float rms_piece_ss(const u32x4& x) {
    using E = Elem<T>;
    const float x0 = E::lo(x[0]);
    float s = x0 * x0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float lo = E::lo(x[i]), hi = E::hi(x[i]);
        if (i > 0) s = fmaf(lo, lo, s);
        s = fmaf(hi, hi, s);
    }
    return s;
}

// the sum over the group of `lanes` adjacent lanes (a power of two, uniform over the wave): EVERY lane of the wave must call this
__device__ __forceinline__ float rms_group_sum(float s, int lanes) {
    for (int m = 1; m < lanes; m <<= 1) s += __shfl_xor(s, m);
    return s;
}

__device__ __forceinline__ float rms_rstd(float ss, int head_dim, float eps) { return 1.0f / sqrtf(ss / (float)head_dim + eps); }

// g[i] = offset + w[i], computed once by the caller (rms_gains below)
template <typename T>
__device__ __forceinline__ u32x4 rms_scale(const u32x4& x, float rstd, const float (&g)[8]) {
    using E = Elem<T>;
    u32x4 y;
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = E::pack2((E::lo(x[i]) * rstd) * g[2 * i], (E::hi(x[i]) * rstd) * g[2 * i + 1]);
    return y;
}

// the 8 gains of a piece from a weight of the io type (one 16-byte load) or of fp32 (two)
template <typename T>
__device__ __forceinline__ void rms_gains(const void* w, int d, bool w_fp32, float offset, float (&g)[8]) {
    using E = Elem<T>;
    if (w_fp32) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(static_cast<const float*>(w) + d);
        const f32x4 b = *reinterpret_cast<const f32x4*>(static_cast<const float*>(w) + d + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { g[i] = offset + a[i]; g[4 + i] = offset + b[i]; }
    } else {
        const u32x4 a = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(w) + d);
#pragma unroll
        for (int i = 0; i < 4; ++i) { g[2 * i] = offset + E::lo(a[i]); g[2 * i + 1] = offset + E::hi(a[i]); }
    }
}

// the lane's part of sum_d a[d] b[d] (the backward, fa_qk_norm_rope_bwd.hip): its 8 columns in column order, as rms_piece_ss -
// s = a0 * b0, then s = fmaf(ai, bi, s) for i = 1 .. 7; rms_group_sum adds the lanes
__device__ __forceinline__ float rms_piece_dot(const float (&a)[8], const float (&b)[8]) {
    float s = a[0] * b[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s = fmaf(a[i], b[i], s);
    return s;
}

}  // namespace fa
