// fa_mass.h - the integer-mass arithmetic over one row of logits: everything on which fa_sample (fa_sample.hip) and fa_spec_accept
// (fa_spec_verify.hip) must agree bit for bit - speculative decoding is lossless only if fa_spec_accept's masses ARE fa_sample's.
// With v_j the raw values of the row (a NaN counts as -inf, -0 as +0: mass_canon) in the order "larger value, then lower index":
//     x_j = v_j * inv_t (one rounding),  m = x_{j*},  e_j = e(x_j - m) (fa_lse.h's e),  q_j = floor(e_j * 2^40)  (uint64)
// inv_t = 1 / T, or 1 for a cold row (!(T > 0)); every decision behind the q_j is INTEGER arithmetic, so a sum of them does not
// depend on the order of addition.  The float part - (m, s), the first maximum j*, n0 = the number of values above -inf - has one
// fixed order: a piece is 8 columns counted from column 0 of the row, a run is ITERS x 64 pieces owned by one wave (lane l the
// pieces l, l + 64, ..), runs follow each other in index order; a lane folds its pieces in that order, the lanes meet in the xor
// butterfly, the 16 waves of a workgroup and then the chunks of a row are merged in index order (fa_lse.h's merge).  Two plans cut
// a row into runs: the whole row in one workgroup (ITERS from vocab) and chunks of MASS_CHUNK columns (ITERS = 2) - a row's bits
// depend on the plan and on its values alone.  A piece is one 16-byte load (fp32: two) where the row starts on a 16-byte boundary
// and the piece lies inside the row, element by element otherwise: the same values, never a column >= vocab.
// What only one of the two ops uses (the radix select, the residual of (p_j, q_j), the records) stays in its own file.
#pragma once
#include <cmath>
#include <cstdint>
#include "fa_lse.h"                                       // (first: its `fp contract(off)` covers x_j * inv_t - m below)

namespace fa {

constexpr int MASS_THREADS = 1024;                        // lanes of a workgroup
constexpr int MASS_WAVES = MASS_THREADS / 64;
constexpr int MASS_CHUNK = 16384;                         // columns per workgroup of the chunk plan
constexpr int MASS_CHUNK_ITERS = MASS_CHUNK / 8 / MASS_THREADS;   // pieces per lane per chunk
constexpr int MASS_NONE = 0x7fffffff;                     // no column: behind every index

__device__ __forceinline__ float mass_canon(float v) { return v != v ? -INFINITY : (v == 0.f ? 0.f : v); }

// e_j and q_j
__device__ __forceinline__ float mass_e(float v, float inv_t, float m) { return lse_exp(v * inv_t - m); }
__device__ __forceinline__ uint64_t mass_q(float e) { return e > 0.f ? (uint64_t)(e * 1099511627776.0f) : 0ull; }

// a cold row (T = 0, negative or a NaN) is greedy, and its x_j are its v_j
__device__ __forceinline__ bool mass_cold(float temp) { return !(temp > 0.f); }
__device__ __forceinline__ float mass_inv_t(float temp) { return mass_cold(temp) ? 1.0f : 1.0f / temp; }

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int off) {
    const uint32_t lo = __shfl_up((uint32_t)v, off), hi = __shfl_up((uint32_t)(v >> 32), off);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int lane) {
    const uint32_t lo = __shfl((uint32_t)v, lane), hi = __shfl((uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}
// the inclusive sum over the lanes 0 .. own of the wave
__device__ __forceinline__ uint64_t wave_scan64(uint64_t v, int lane) {
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t t = shfl_up64(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

// the row at element offset `rowoff` starts on a 16-byte boundary: its whole pieces are taken with vector accesses
template <typename T>
__device__ __forceinline__ bool mass_row_vec(const void* base, int64_t rowoff) {
    return ((reinterpret_cast<uintptr_t>(base) + (uint64_t)rowoff * RowIo<T>::ESIZE) & 15) == 0;
}

// a row as a lane sees it
template <typename T> struct MassRow {
    const void* p;
    int64_t rowoff;                                       // in elements
    int V, iters, wave, lane;
    int run;                                              // the wave's run among all runs of the row
    bool vec;                                             // the row starts on a 16-byte boundary
    __device__ __forceinline__ int col(int i) const { return 8 * ((run * iters + i) * 64 + lane); }
    // the raw values of the piece at column c (c < V); columns >= V: fill
    __device__ __forceinline__ void raw(int c, float fill, float (&r)[8]) const {
        if (vec && c + 8 <= V) {
            RowIo<T>::load8(p, rowoff + c, r);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = c + i < V ? RowIo<T>::load1(p, rowoff + c + i) : fill;
        }
    }
    // the canonical logits
    __device__ __forceinline__ void values(int c, float (&v)[8]) const {
        raw(c, -INFINITY, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = mass_canon(v[i]);
    }
};
// the view of the lane's wave on a row cut into runs of `iters` x 64 pieces: wave w of the workgroup owns run first_run + w
template <typename T>
__device__ __forceinline__ MassRow<T> mass_row(const void* base, int64_t rowoff, int V, int iters, int first_run) {
    MassRow<T> r;
    r.p = base;
    r.rowoff = rowoff;
    r.V = V;
    r.iters = iters;
    r.wave = (int)threadIdx.x >> 6;
    r.lane = (int)threadIdx.x & 63;
    r.run = first_run + r.wave;
    r.vec = mass_row_vec<T>(base, rowoff);
    return r;
}
// the whole row in one workgroup (iters: a function of vocab alone)
template <typename T>
__device__ __forceinline__ MassRow<T> mass_row_whole(const void* base, int64_t rowoff, int V, int iters) {
    return mass_row<T>(base, rowoff, V, iters, 0);
}
// chunk `chunk` of the row: the index order of the runs is the one-workgroup plan's
template <typename T>
__device__ __forceinline__ MassRow<T> mass_row_chunk(const void* base, int64_t rowoff, int V, int chunk) {
    return mass_row<T>(base, rowoff, V, MASS_CHUNK_ITERS, chunk * MASS_WAVES);
}

// the statistics of a set of columns - a workgroup's, then a row's: the workspace partial of both ops
struct MassStat { float m, s, bv; int bi; uint32_t n0, pad[3]; };   // (m, s) over x, the first maximum (bv, bi) of v, n0
static_assert(sizeof(MassStat) == 32, "the workspace layout");

__device__ __forceinline__ void mass_first_max(float& bv, int& bi, float ov, int oi) {
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
}

// the statistics of the workgroup's columns; slotf: 3 * MASS_WAVES floats, slot32: 2 * MASS_WAVES words of LDS.  EVERY lane of
// the workgroup calls it (it holds ONE barrier, behind the slots' stores); `merge`: the lane merges the waves in index order and
// gets the workgroup's statistics (a lane that does not gets its wave's - the chunk kernels leave with them)
template <typename T>
__device__ __forceinline__ MassStat mass_stats(const MassRow<T>& r, float inv_t, float* slotf, uint32_t* slot32, bool merge) {
    LseState st = {-INFINITY, 0.f};
    float bv = -INFINITY;
    int bi = MASS_NONE;
    uint32_t n0 = 0;
    for (int i = 0; i < r.iters; ++i) {
        const int c = r.col(i);
        if (c >= r.V) continue;
        float v[8], x[8];
        r.values(c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            x[e] = v[e] * inv_t;
            if (v[e] > bv) { bv = v[e]; bi = c + e; }
            n0 += v[e] > -INFINITY ? 1u : 0u;
        }
        lse_piece(st, x);
    }
    st = lse_wave(st);
    for (int m = 1; m < 64; m <<= 1) {
        mass_first_max(bv, bi, __shfl_xor(bv, m), __shfl_xor(bi, m));
        n0 += __shfl_xor(n0, m);
    }
    if (r.lane == 0) {
        slotf[r.wave] = st.m;
        slotf[MASS_WAVES + r.wave] = st.s;
        slotf[2 * MASS_WAVES + r.wave] = bv;
        slot32[r.wave] = (uint32_t)bi;
        slot32[MASS_WAVES + r.wave] = n0;
    }
    __syncthreads();
    if (merge) {
        st = LseState{slotf[0], slotf[MASS_WAVES]};
        bv = slotf[2 * MASS_WAVES];
        bi = (int)slot32[0];
        n0 = slot32[MASS_WAVES];
        for (int w = 1; w < MASS_WAVES; ++w) {
            st = lse_merge(st, LseState{slotf[w], slotf[MASS_WAVES + w]});
            mass_first_max(bv, bi, slotf[2 * MASS_WAVES + w], (int)slot32[w]);
            n0 += slot32[MASS_WAVES + w];
        }
    }
    return MassStat{st.m, st.s, bv, bi, n0, {0, 0, 0}};
}

// a row's C chunk partials merged in chunk order: the same bits in every workgroup that asks
__device__ __forceinline__ MassStat mass_merge(const MassStat* sp, int C) {
    MassStat o = sp[0];
    LseState st = {o.m, o.s};
    float bv = o.bv;
    int bi = o.bi;
    uint32_t n0 = o.n0;
    for (int c = 1; c < C; ++c) {
        o = sp[c];
        st = lse_merge(st, LseState{o.m, o.s});
        mass_first_max(bv, bi, o.bv, o.bi);
        n0 += o.n0;
    }
    return MassStat{st.m, st.s, bv, bi, n0, {0, 0, 0}};
}

// what a row's statistics and its temperature say
struct MassNode {
    LseState st;                                          // the row's (m, s): lse = st.m + log(st.s)
    float m, inv_t, bv;                                   // m = x_{j*}, the value the e_j are taken against
    int bi;                                               // j*
    uint32_t n0;
    bool empty, greedy;
};
__device__ __forceinline__ MassNode mass_node(const MassStat& o, float temp) {
    MassNode n;
    n.inv_t = mass_inv_t(temp);
    n.st = LseState{o.m, o.s};
    n.m = o.bv * n.inv_t;                                 // x_{j*}: the maximum of the running pair (the product is monotone)
    n.bv = o.bv;
    n.bi = o.bi;
    n.n0 = o.n0;
    n.empty = o.n0 == 0;
    n.greedy = mass_cold(temp) || !(fabsf(n.m) < INFINITY);         // (+inf in the row, or 1 / T overflows the product)
    return n;
}

// the draw: min(floor(u total), total - 1) for total >= 1; u <= 0 or NaN: 0
__device__ __forceinline__ uint64_t mass_draw_target(float u, uint64_t total) {
    const double uu = u > 0.f ? (double)u : 0.0;
    const double d = floor(uu * (double)total);
    uint64_t rr = d >= 18446744073709551615.0 ? total : (uint64_t)d;
    if (rr > total - 1) rr = total - 1;
    return rr;
}

// one step of the index walk of a wave over its run: the lane's piece starts at column c and has the weights wv (their sum ls),
// `running` is the weight in front of the wave's pieces of this step.  The one lane whose piece holds the index-order running
// weight `at` writes the column to `found`; `running` moves behind the step's pieces.  EVERY lane of the wave calls it
__device__ __forceinline__ void mass_walk_step(const uint64_t (&wv)[8], uint64_t ls, uint64_t& running, uint64_t at, int c, int lane,
                                               int& found) {
    const uint64_t incl = wave_scan64(ls, lane);
    uint64_t a = running + (incl - ls);
    if (a <= at && at < a + ls) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (a <= at && at < a + wv[e]) found = c + e;
            a += wv[e];
        }
    }
    running += shfl64(incl, 63);
}

}  // namespace fa
