// fa_rowsum.h - the fixed-order sums over one row of N columns (N % 8 == 0, 8 <= N <= 16384) that fa_add_norm, fa_add_norm_quant
// (fa_add_norm.h) and fa_add_norm_bwd (fa_add_norm_bwd.hip) share: sum z, sum z^2 (or sum (z - mean)^2), sum a, sum a xhat.  The
// order of every sum depends on N ALONE - never on the number of rows, the row's index or the device - so a row's bits do not
// depend on what else is in the batch.  mean / rstd are row_small_stats / row_wide_stats in the forward and in the backward: the
// backward recomputes them with the forward's bits because it calls the forward's function.
//   N <= 256 (row_small): fa_rmsnorm.h's ownership - a row lies 8 columns per lane (one piece) in G adjacent lanes of a wave, G the
//     smallest power of two with 8 G >= N, several rows per wave:
//       - in a lane: the 8 columns in column order, s = v0 * v0 then s = fmaf(vi, vi, s) (row_piece_ss: the operations of
//         rms_piece_ss), s = a0 * b0 then fmaf (rms_piece_dot), s = v0 then s += vi (row_piece_sum);
//       - across the G lanes: fa_rmsnorm.h's xor butterfly (rms_group_sum); lanes past the row hand in +0.
//     No LDS.  An RMSNorm without bias has the bits of fa_qk_norm_rope_store's norm of a head of N columns.
//   N > 256 (row_wide): one workgroup of `threads` = 64 ceil(N / 512) <= 256 lanes per row; lane t owns the pieces t, t + threads,
//     t + 2 threads, .. (at most 8: 64 fp32 values at N = 16384):
//       - in a lane: every piece as above, then the lane's pieces added in ascending order, s = s0 + s1 + ..; a piece past the
//         row hands in +0;
//       - over the wave: the xor butterfly over all 64 lanes, m = 1, 2, 4, .. 32 (after it every lane holds the same bits);
//       - over the workgroup: lane 0 of every wave writes its sum to LDS, and every lane adds the waves in index order,
//         t = w0 + w1 + .. (row_block_sum).  One wave: no LDS, no barrier.
//     (The backward's weight-gradient kernels keep several rows in flight in one larger workgroup: each row is still owned by
//     `threads` lanes - whole waves - with LDS slots of their own, so its sums have this order there too.)
// mean = sum / N and rstd = 1 / sqrt(ss / N + eps) are IEEE divisions and a correctly rounded root (rms_rstd).
#pragma once
#include "fa_rmsnorm.h"

namespace fa {

constexpr int ROW_SMALL_MAX = 256;                        // N up to here: row_small
constexpr int ROW_THREADS = 256;                          // the most lanes that own one row
constexpr int ROW_WAVES = ROW_THREADS / 64;
constexpr int ROW_MAX_PIECES = 8;                         // pieces per lane at N = 16384

// the host side of the ownership: a function of N alone
struct RowShape { int group_log2, threads, pieces; };     // small: G = 1 << group_log2, pieces 1; wide: threads per row, pieces per lane
static inline RowShape row_shape(int n) {
    RowShape s = {0, ROW_THREADS, 1};
    if (n <= ROW_SMALL_MAX) {
        while ((8 << s.group_log2) < n) ++s.group_log2;
        return s;
    }
    const int np = n / 8;
    s.threads = np >= ROW_THREADS ? ROW_THREADS : (np + 63) / 64 * 64;
    const int per = (np + s.threads - 1) / s.threads;
    s.pieces = per <= 1 ? 1 : (per <= 2 ? 2 : (per <= 4 ? 4 : 8));   // the kernels are built for 1, 2, 4, 8 (absent pieces: +0)
    return s;
}

__device__ __forceinline__ float row_piece_ss(const float (&v)[8]) {
    float s = v[0] * v[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s = fmaf(v[i], v[i], s);
    return s;
}

__device__ __forceinline__ float row_piece_sum(const float (&v)[8]) {
    float s = v[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s += v[i];
    return s;
}

// the sum over a row owned by `nwaves` whole waves from every lane's own sum; wave: the lane's wave among them; slot: ROW_WAVES
// floats of LDS that no other sum in flight uses.  EVERY lane of the workgroup must call this (several rows in flight in one
// workgroup: each with its own slot)
__device__ __forceinline__ float row_block_sum(float s, float* slot, int nwaves, int wave) {
    s = rms_group_sum(s, 64);
    if (nwaves == 1) return s;
    if ((threadIdx.x & 63) == 0) slot[wave] = s;
    __syncthreads();
    float t = slot[0];
    for (int w = 1; w < nwaves; ++w) t += slot[w];
    return t;
}

// mean and rstd of a row that lies one piece per lane in `lanes` adjacent lanes of a wave (act: the lane has a piece of a row; a
// lane without one hands in z = +0): z is centred in place for LN, an absent piece stays +0; returns rstd.  EVERY lane of the wave
// must call this
template <bool LN>
__device__ __forceinline__ float row_small_stats(float (&z)[8], bool act, int lanes, int n, float eps) {
    if constexpr (LN) {
        const float mean = rms_group_sum(row_piece_sum(z), lanes) / (float)n;
#pragma unroll
        for (int i = 0; i < 8; ++i) z[i] = act ? z[i] - mean : 0.f;
    }
    return rms_rstd(rms_group_sum(row_piece_ss(z), lanes), n, eps);
}

// .. and of a row owned by `nwaves` whole waves, lane t the pieces t, t + threads, .. (on: the piece is inside the row; a piece
// past it comes in as +0 and stays +0); sum_slot, ss_slot: row_block_sum's LDS for the two sums.  EVERY lane of the workgroup must
// call this
template <bool LN, int NP>
__device__ __forceinline__ float row_wide_stats(float (&z)[NP][8], const bool (&on)[NP], float* sum_slot, float* ss_slot,
                                                int nwaves, int wave, int n, float eps) {
    if constexpr (LN) {
        float s = row_piece_sum(z[0]);
#pragma unroll
        for (int p = 1; p < NP; ++p) s += row_piece_sum(z[p]);
        const float mean = row_block_sum(s, sum_slot, nwaves, wave) / (float)n;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int i = 0; i < 8; ++i) z[p][i] = on[p] ? z[p][i] - mean : 0.f;
        }
    }
    float ss = row_piece_ss(z[0]);
#pragma unroll
    for (int p = 1; p < NP; ++p) ss += row_piece_ss(z[p]);
    return rms_rstd(row_block_sum(ss, ss_slot, nwaves, wave), n, eps);
}

// 8 columns of a 16-bit (one 16-byte load) or fp32 (two) tensor as fp32
template <typename T>
__device__ __forceinline__ void row_load8(const void* base, int64_t at, bool fp32, float (&v)[8]) {
    using E = Elem<T>;
    if (fp32) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(static_cast<const float*>(base) + at);
        const f32x4 b = *reinterpret_cast<const f32x4*>(static_cast<const float*>(base) + at + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
    } else {
        const u32x4 a = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(base) + at);
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = E::lo(a[i]); v[2 * i + 1] = E::hi(a[i]); }
    }
}

// .. and back: ONE rounding to the 16-bit type, none to fp32
template <typename T>
__device__ __forceinline__ void row_store8(void* base, int64_t at, bool fp32, const float (&v)[8]) {
    using E = Elem<T>;
    if (fp32) {
        *reinterpret_cast<f32x4*>(static_cast<float*>(base) + at) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(static_cast<float*>(base) + at + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else {
        u32x4 y;
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = E::pack2(v[2 * i], v[2 * i + 1]);
        *reinterpret_cast<u32x4*>(static_cast<uint16_t*>(base) + at) = y;
    }
}

// one element / one whole piece of a row of type T (fp32: fp32_tag): the accessor of fa_cross_entropy, fa_sample and fa_spec_accept
// (fa_moe.hip keeps a loader of its own on purpose: it tests the alignment per piece and fills with 0)
struct fp32_tag {};
template <typename T> struct RowIo {
    static constexpr int ESIZE = 2;
    static __device__ __forceinline__ float load1(const void* p, int64_t at) {
        return Elem<T>::lo((uint32_t) static_cast<const uint16_t*>(p)[at]);
    }
    static __device__ __forceinline__ void store1(void* p, int64_t at, float v) {
        static_cast<uint16_t*>(p)[at] = (uint16_t)Elem<T>::pack2(v, 0.f);
    }
    static __device__ __forceinline__ void load8(const void* p, int64_t at, float (&v)[8]) { row_load8<T>(p, at, false, v); }
    static __device__ __forceinline__ void store8(void* p, int64_t at, const float (&v)[8]) { row_store8<T>(p, at, false, v); }
};
template <> struct RowIo<fp32_tag> {
    static constexpr int ESIZE = 4;
    static __device__ __forceinline__ float load1(const void* p, int64_t at) { return static_cast<const float*>(p)[at]; }
    static __device__ __forceinline__ void store1(void* p, int64_t at, float v) { static_cast<float*>(p)[at] = v; }
    static __device__ __forceinline__ void load8(const void* p, int64_t at, float (&v)[8]) { row_load8<bf16_tag>(p, at, true, v); }
    static __device__ __forceinline__ void store8(void* p, int64_t at, const float (&v)[8]) { row_store8<bf16_tag>(p, at, true, v); }
};

// v rounded to the 16-bit type and widened again: the value a 16-bit store of v leaves
template <typename T>
__device__ __forceinline__ void row_round8(float (&v)[8]) {
    using E = Elem<T>;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t p = E::pack2(v[2 * i], v[2 * i + 1]);
        v[2 * i] = E::lo(p);
        v[2 * i + 1] = E::hi(p);
    }
}

}  // namespace fa
