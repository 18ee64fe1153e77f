// fa_moe.hip - what surrounds the expert GEMMs of a mixture-of-experts block (fa_moe_*, include/fa_mi355.h): top-k routing and
// its gradient, the stable counting sort of the (token, k) slots by expert, the permutation into per-expert segments and the
// weighted combine with its backward.  Memory-bound row ops: no host synchronisation, no ordering that depends on an atomic.
//
// fa_moe_route / fa_moe_route_bwd.  A row of E <= 512 logits lies 8 columns per lane in G adjacent lanes of a wave (G the smallest
// power of two with 8 G >= E, moe_group_log2: fa_rmsnorm.h's ownership), 256 / G rows per workgroup of 256 lanes; columns >= E
// are absent: never read, never selected.  fp32 throughout, every operation rounding once:
//     softmax   z_j = float(logit_j), NaN -> -inf;  c_j = z_j
//     sigmoid   s_j = act_sig(float(logit_j)) (fa_act.h: rcp(1 + exp2(-l * log2e)));  c_j = s_j + bias_j, NaN -> -inf
//     select    K rounds.  In a lane: its free columns in column order, a later one wins only where it is strictly greater.  Across
//               the G lanes: a xor butterfly on (c, index), the other side wins where c is greater, or equal with the lower index
//               (a total order: every lane of the group ends with the same pair).  The owner marks the column taken.  Absent and
//               taken columns carry the index INT_MAX, so a real -inf beats them: K <= E distinct ids inside [0, E), whatever
//               the row holds.
//     weights   softmax, renormalize:   m = c_{id_0};  e_k = exp2((c_{id_k} - m) * log2e);  S = e_0 + e_1 + ..;  w_k = e_k / S
//               softmax, all E:         e_j = exp2((z_j - m) * log2e);  Z: the lane's columns added in column order (absent: +0),
//                                       then rms_group_sum over the G lanes;  w_k = e_{id_k} / Z
//               sigmoid:                w_k = s_{id_k};  renormalize: S = w_0 + w_1 + ..;  w_k = w_k / S
//               last:                   w_k = w_k * scale                              (IEEE divisions; sums in ascending k)
// The order is a function of (E, K, dtype) alone.  The backward recomputes m, e_k, S / Z, w_k with exactly these lines - every lane
// of the group for itself, from logits[id_k] (an id outside [0, E) is not dereferenced: its logit counts as -inf) - and writes
// every column of the row once: the formulas are in the header.
//
// fa_moe_sort.  Slots s = t * K + k are cut into `chunks` runs of `chunk` slots (moe_sort_plan, a function of (T K, E)); a run is
// ONE wave.  (1) count: the wave's histogram of its run in LDS (integer adds of pure counts) -> counts[chunk][E]; the same
// launch fills sorted_slot with -1.  (2) scan: one workgroup; lane e walks counts[.][e] in chunk order (exclusive prefix, in
// place), then the align-padded totals are scanned over e (Hillis-Steele in LDS) -> expert_offsets.  (3) place: the wave walks its
// run 64 slots at a time; lanes with the same id find each other with 9 ballots (one per bit of the id), a slot's rank is the
// number of such lanes below it, its row is run[id] + rank, and the highest lane of each id adds the count to run[id].  Slots of
// an expert therefore ascend.  An id outside [0, E) is only compared: pos = -1.
//
// fa_moe_permute / fa_moe_combine / fa_moe_combine_bwd.  A lane owns one 16-byte piece (8 columns) of one output row; 256
// consecutive pieces are an item, a workgroup strides over items with four in flight.  Loads and stores are 16 bytes, every
// offset 64-bit; an index read from memory (sorted_slot, pos) is compared against its range before it addresses anything.  dw is
// the row sum of fa_rowsum.h (row_shape: n <= 256 in G lanes, above in `threads` lanes of one workgroup per slot).
#include <climits>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include "fa_common.h"
#include "fa_act.h"
#include "fa_rowsum.h"
#include "fa_moe.h"

namespace fa {

struct f32_tag {};

constexpr int MOE_THREADS = 256;
constexpr int MOE_GRID_CAP = 16384;                        // workgroups of the piece kernels; the rest by stride
constexpr int MOE_UNROLL = 4;                              // items a workgroup has in flight

// ---- a router row: 8 columns as fp32.  vec: the piece lies inside the row and starts on a 16-byte boundary
template <typename T>
__device__ __forceinline__ void moe_load8(const void* base, int64_t off, int col, int E, float (&v)[8]) {
    if constexpr (std::is_same<T, f32_tag>::value) {
        const float* p = static_cast<const float*>(base) + off + col;
        if (col + 8 <= E && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = col + i < E ? p[i] : 0.f;
        }
    } else {
        using El = Elem<T>;
        const uint16_t* p = static_cast<const uint16_t*>(base) + off + col;
        if (col + 8 <= E && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const u32x4 a = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
            for (int i = 0; i < 4; ++i) { v[2 * i] = El::lo(a[i]); v[2 * i + 1] = El::hi(a[i]); }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = col + i < E ? El::lo((uint32_t)p[i]) : 0.f;
        }
    }
}

template <typename T>
__device__ __forceinline__ float moe_load1(const void* base, int64_t at) {
    if constexpr (std::is_same<T, f32_tag>::value) return static_cast<const float*>(base)[at];
    else return Elem<T>::lo((uint32_t)static_cast<const uint16_t*>(base)[at]);
}

// .. and back, ONE rounding to the io type; columns >= E are not written
template <typename T>
__device__ __forceinline__ void moe_store8(void* base, int64_t off, int col, int E, const float (&v)[8]) {
    if constexpr (std::is_same<T, f32_tag>::value) {
        float* p = static_cast<float*>(base) + off + col;
        if (col + 8 <= E && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (col + i < E) p[i] = v[i];
        }
    } else {
        using El = Elem<T>;
        uint16_t* p = static_cast<uint16_t*>(base) + off + col;
        if (col + 8 <= E && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            u32x4 y;
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = El::pack2(v[2 * i], v[2 * i + 1]);
            *reinterpret_cast<u32x4*>(p) = y;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (col + i < E) p[i] = (uint16_t)El::pack2(v[i], 0.f);
        }
    }
}

__device__ __forceinline__ float moe_nan_to_ninf(float x) { return x != x ? -INFINITY : x; }
__device__ __forceinline__ float moe_exp(float t) { return fast_exp2(t * kLog2e); }

struct MoeRouteArgs {
    const void* logits; const float* bias; float* weights; int* ids;
    const float* dweights; void* dlogits;                   // the backward's
    int64_t rs, drs, tokens;
    int E, K, glog2, renorm;
    float scale;
};

// Z of the softmax over all E: the lane's columns in column order (absent: +0), then the butterfly
__device__ __forceinline__ float moe_row_z(const float (&z)[8], float m, int col0, int E, int G, float (&e)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = col0 + i < E ? moe_exp(z[i] - m) : 0.f;
    float s = e[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s += e[i];
    return rms_group_sum(s, G);
}

template <typename T, int SCORING>
__global__ void __launch_bounds__(MOE_THREADS) moe_route_kernel(const MoeRouteArgs a) {
    const int G = 1 << a.glog2;
    const int gl = (int)threadIdx.x & (G - 1);               // the lane inside its group
    const int64_t row = (int64_t)blockIdx.x * (MOE_THREADS >> a.glog2) + ((int)threadIdx.x >> a.glog2);
    const bool live = row < a.tokens;                        // (a dead row's lanes still take part in the shuffles)
    const int col0 = gl * 8;
    const int E = live ? a.E : 0;
    float z[8], c[8], s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = 0.f;
    if (live) moe_load8<T>(a.logits, row * a.rs, col0, E, z);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if constexpr (SCORING == FA_MOE_SOFTMAX) {
            z[i] = moe_nan_to_ninf(z[i]);
            c[i] = z[i];
            s[i] = 0.f;
        } else {
            s[i] = act_sig(z[i]);
            const float b = (a.bias && col0 + i < E) ? a.bias[col0 + i] : 0.f;
            c[i] = moe_nan_to_ninf(a.bias ? s[i] + b : s[i]);
        }
    }
    uint32_t taken = 0;
    float wv[MOE_MAX_TOPK];
    int id[MOE_MAX_TOPK];
#pragma unroll
    for (int k = 0; k < MOE_MAX_TOPK; ++k) {
        wv[k] = 0.f;
        id[k] = 0;
        if (k < a.K) {
            float bv = -INFINITY;
            int bi = INT_MAX;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bool free_col = col0 + i < E && !((taken >> i) & 1u);
                if (free_col && (bi == INT_MAX || c[i] > bv)) { bv = c[i]; bi = col0 + i; }
            }
            for (int m = 1; m < G; m <<= 1) {
                const float ov = __shfl_xor(bv, m);
                const int oi = __shfl_xor(bi, m);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if ((bi >> 3) == gl) taken |= 1u << (bi & 7);
            id[k] = bi;
            if constexpr (SCORING == FA_MOE_SOFTMAX) {
                wv[k] = bv;
            } else {
                float mine = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) mine = col0 + i == bi ? s[i] : mine;
                wv[k] = __shfl(mine, (((int)threadIdx.x & 63) & ~(G - 1)) + ((bi >> 3) & (G - 1)));
            }
        }
    }
    if constexpr (SCORING == FA_MOE_SOFTMAX) {
        const float m = wv[0];
        float den = 0.f;
        if (a.renorm) {
#pragma unroll
            for (int k = 0; k < MOE_MAX_TOPK; ++k)
                if (k < a.K) { wv[k] = moe_exp(wv[k] - m); den = k == 0 ? wv[0] : den + wv[k]; }
        } else {
            float e[8];
            den = moe_row_z(z, m, col0, E, G, e);
#pragma unroll
            for (int k = 0; k < MOE_MAX_TOPK; ++k)
                if (k < a.K) wv[k] = moe_exp(wv[k] - m);
        }
#pragma unroll
        for (int k = 0; k < MOE_MAX_TOPK; ++k)
            if (k < a.K) wv[k] = wv[k] / den;
    } else if (a.renorm) {
        float den = 0.f;
#pragma unroll
        for (int k = 0; k < MOE_MAX_TOPK; ++k)
            if (k < a.K) den = k == 0 ? wv[0] : den + wv[k];
#pragma unroll
        for (int k = 0; k < MOE_MAX_TOPK; ++k)
            if (k < a.K) wv[k] = wv[k] / den;
    }
#pragma unroll
    for (int k = 0; k < MOE_MAX_TOPK; ++k) {
        if (k < a.K && live && gl == (k & (G - 1))) {
            a.weights[row * a.K + k] = wv[k] * a.scale;
            a.ids[row * a.K + k] = id[k];
        }
    }
}

template <typename T, int SCORING>
__global__ void __launch_bounds__(MOE_THREADS) moe_route_bwd_kernel(const MoeRouteArgs a) {
    const int G = 1 << a.glog2;
    const int gl = (int)threadIdx.x & (G - 1);
    const int64_t row = (int64_t)blockIdx.x * (MOE_THREADS >> a.glog2) + ((int)threadIdx.x >> a.glog2);
    const bool live = row < a.tokens;
    const int col0 = gl * 8;
    const int E = live ? a.E : 0;
    const bool dense = SCORING == FA_MOE_SOFTMAX && !a.renorm;
    // the K selected columns, every lane of the group for itself: id, the recomputed score, the incoming gradient
    int id[MOE_MAX_TOPK];
    float v[MOE_MAX_TOPK], dw[MOE_MAX_TOPK];
#pragma unroll
    for (int k = 0; k < MOE_MAX_TOPK; ++k) {
        id[k] = -1; v[k] = 0.f; dw[k] = 0.f;
        if (k < a.K && live) {
            id[k] = a.ids[row * a.K + k];
            dw[k] = a.dweights[row * a.K + k];
            const float l = (uint32_t)id[k] < (uint32_t)E ? moe_load1<T>(a.logits, row * a.rs + id[k]) : -INFINITY;
            if (!((uint32_t)id[k] < (uint32_t)E)) id[k] = -1;
            v[k] = SCORING == FA_MOE_SOFTMAX ? moe_nan_to_ninf(l) : act_sig(l);
        }
    }
    float out[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = 0.f;
    if constexpr (SCORING == FA_MOE_SOFTMAX) {
        const float m = v[0];
        float z[8], e[8], den = 0.f;
        if (dense) {                                          // (uniform over the launch)
#pragma unroll
            for (int i = 0; i < 8; ++i) z[i] = 0.f;
            if (live) moe_load8<T>(a.logits, row * a.rs, col0, E, z);
#pragma unroll
            for (int i = 0; i < 8; ++i) z[i] = moe_nan_to_ninf(z[i]);
            den = moe_row_z(z, m, col0, E, G, e);
        }
#pragma unroll
        for (int k = 0; k < MOE_MAX_TOPK; ++k)
            if (k < a.K) { v[k] = moe_exp(v[k] - m); if (!dense) den = k == 0 ? v[0] : den + v[k]; }
        float D = 0.f;
#pragma unroll
        for (int k = 0; k < MOE_MAX_TOPK; ++k)
            if (k < a.K) { v[k] = v[k] / den; dw[k] = dw[k] * a.scale; D = fmaf(dw[k], v[k], D); }
        if (dense) {
            float g[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) g[i] = 0.f;
#pragma unroll
            for (int k = 0; k < MOE_MAX_TOPK; ++k)
                if (k < a.K) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) g[i] = col0 + i == id[k] ? dw[k] : g[i];
                }
#pragma unroll
            for (int i = 0; i < 8; ++i) out[i] = (e[i] / den) * (g[i] - D);
        } else {
#pragma unroll
            for (int k = 0; k < MOE_MAX_TOPK; ++k)
                if (k < a.K) {
                    const float dl = v[k] * (dw[k] - D);
#pragma unroll
                    for (int i = 0; i < 8; ++i) out[i] = col0 + i == id[k] ? dl : out[i];
                }
        }
    } else {
        float den = 1.f, D = 0.f;
        if (a.renorm) {
#pragma unroll
            for (int k = 0; k < MOE_MAX_TOPK; ++k)
                if (k < a.K) den = k == 0 ? v[0] : den + v[k];
#pragma unroll
            for (int k = 0; k < MOE_MAX_TOPK; ++k)
                if (k < a.K) D = fmaf(dw[k], v[k] / den, D);
        }
#pragma unroll
        for (int k = 0; k < MOE_MAX_TOPK; ++k)
            if (k < a.K) {
                const float ds = a.renorm ? ((dw[k] - D) * a.scale) / den : dw[k] * a.scale;
                const float dl = (ds * v[k]) * (1.0f - v[k]);
#pragma unroll
                for (int i = 0; i < 8; ++i) out[i] = col0 + i == id[k] ? dl : out[i];
            }
    }
    if (live && col0 < E) moe_store8<T>(a.dlogits, row * a.drs, col0, E, out);
}

// ---- fa_moe_sort
struct MoeSortArgs {
    const int* ids; int* sorted_slot; int* pos; int* offsets; int* counts;
    int64_t slots, mmax, chunk, chunks;
    int E, align;
};

__global__ void __launch_bounds__(64) moe_sort_count_kernel(const MoeSortArgs a) {
    __shared__ int hist[MOE_MAX_EXPERTS];
    const int lane = (int)threadIdx.x;
    for (int e = lane; e < a.E; e += 64) hist[e] = 0;
    __syncthreads();
    const int64_t s0 = (int64_t)blockIdx.x * a.chunk;
    const int64_t s1 = s0 + a.chunk < a.slots ? s0 + a.chunk : a.slots;
    for (int64_t s = s0 + lane; s < s1; s += 64) {
        const int id = a.ids[s];
        if ((uint32_t)id < (uint32_t)a.E) atomicAdd(&hist[id], 1);          // (a pure count: its value has no order)
    }
    __syncthreads();
    for (int e = lane; e < a.E; e += 64) a.counts[(int64_t)blockIdx.x * a.E + e] = hist[e];
    for (int64_t i = (int64_t)blockIdx.x * 64 + lane; i < a.mmax; i += a.chunks * 64) a.sorted_slot[i] = -1;
}

__global__ void __launch_bounds__(MOE_MAX_EXPERTS) moe_sort_scan_kernel(const MoeSortArgs a) {
    __shared__ int buf[2][MOE_MAX_EXPERTS];
    const int e = (int)threadIdx.x;
    int padded = 0;
    if (e < a.E) {
        int run = 0;
        for (int64_t b = 0; b < a.chunks; ++b) {
            const int c = a.counts[b * a.E + e];
            a.counts[b * a.E + e] = run;
            run += c;
        }
        padded = (run + a.align - 1) / a.align * a.align;
    }
    buf[0][e] = padded;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < MOE_MAX_EXPERTS; d <<= 1) {          // inclusive scan over the experts
        const int t = buf[cur][e] + (e >= d ? buf[cur][e - d] : 0);
        buf[cur ^ 1][e] = t;
        cur ^= 1;
        __syncthreads();
    }
    if (e < a.E) a.offsets[e] = buf[cur][e] - padded;
    if (e == a.E - 1) a.offsets[a.E] = buf[cur][e];
}

__global__ void __launch_bounds__(64) moe_sort_place_kernel(const MoeSortArgs a) {
    __shared__ int run[MOE_MAX_EXPERTS];
    const int lane = (int)threadIdx.x;
    for (int e = lane; e < a.E; e += 64) run[e] = a.offsets[e] + a.counts[(int64_t)blockIdx.x * a.E + e];
    __syncthreads();
    const int64_t s0 = (int64_t)blockIdx.x * a.chunk;
    const int64_t s1 = s0 + a.chunk < a.slots ? s0 + a.chunk : a.slots;
    for (int64_t base = s0; base < s1; base += 64) {          // (uniform: every lane takes part in the ballots)
        const int64_t s = base + lane;
        const int id = s < s1 ? a.ids[s] : -1;
        const bool ok = (uint32_t)id < (uint32_t)a.E;
        unsigned long long same = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 9; ++b) {
            const bool bit = (id >> b) & 1;
            const unsigned long long with = __ballot(ok && bit);
            same &= bit ? with : ~with;
        }
        if (ok) {
            const int rank = __popcll(same & ((1ull << lane) - 1ull));
            const int p = run[id] + rank;
            a.sorted_slot[p] = (int)s;
            a.pos[s] = p;
        } else if (s < s1) {
            a.pos[s] = -1;
        }
        __syncthreads();
        if (ok && lane == 63 - __clzll(same)) run[id] += __popcll(same);
        __syncthreads();
    }
}

// ---- the piece kernels: permute, combine, the dy of combine's backward
struct MoePieceArgs {
    const uint16_t* src; const int* index; const float* scale; uint16_t* dst;
    int64_t src_rs, dst_rs, rows, slots, total, items;        // total: pieces in all; items: runs of 256 pieces
    int K, P;                                                 // P: pieces per row
};

// the piece `item * 256 + lane`: its row and its column.  One 64-bit division per workgroup (uniform), 32-bit ones per lane
__device__ __forceinline__ bool moe_piece(const MoePieceArgs& a, int64_t item, int64_t& r, int& col) {
    const int64_t base = item * MOE_THREADS;
    const int64_t r0 = base / a.P;
    const uint32_t o = (uint32_t)(base - r0 * a.P) + threadIdx.x;
    const uint32_t q = o / (uint32_t)a.P;
    r = r0 + q;
    col = 8 * (int)(o - q * (uint32_t)a.P);
    return item < a.items && base + threadIdx.x < a.total;
}

template <typename T>
__device__ __forceinline__ u32x4 moe_scale8(const u32x4& x, float w) {
    using El = Elem<T>;
    u32x4 y;
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = El::pack2(w * El::lo(x[i]), w * El::hi(x[i]));
    return y;
}

// out[r] = x[index[r] / K] (x scale[index[r]]); an index outside [0, slots) - and every row where index is NULL: +0
template <typename T, bool SCALED>
__global__ void __launch_bounds__(MOE_THREADS) moe_permute_kernel(const MoePieceArgs a) {
    for (int64_t item0 = blockIdx.x; item0 < a.items; item0 += (int64_t)MOE_UNROLL * gridDim.x) {
        u32x4 v[MOE_UNROLL];
        float w[MOE_UNROLL];
        int64_t r[MOE_UNROLL];
        int col[MOE_UNROLL];
        bool in[MOE_UNROLL];
#pragma unroll
        for (int u = 0; u < MOE_UNROLL; ++u) {
            in[u] = moe_piece(a, item0 + (int64_t)u * gridDim.x, r[u], col[u]);
            v[u] = u32x4{0, 0, 0, 0};
            w[u] = 0.f;
            if (in[u]) {
                const int s = a.index ? a.index[r[u]] : -1;
                if ((uint64_t)(int64_t)s < (uint64_t)a.slots) {
                    v[u] = *reinterpret_cast<const u32x4*>(a.src + (int64_t)(s / a.K) * a.src_rs + col[u]);
                    if constexpr (SCALED) w[u] = a.scale[s];
                } else if constexpr (SCALED) {
                    w[u] = 1.f;                               // (padding: +0 itself, not scale x +0)
                }
            }
        }
#pragma unroll
        for (int u = 0; u < MOE_UNROLL; ++u) {
            if (in[u]) {
                if constexpr (SCALED) v[u] = moe_scale8<T>(v[u], w[u]);
                *reinterpret_cast<u32x4*>(a.dst + r[u] * a.dst_rs + col[u]) = v[u];
            }
        }
    }
}

// dst[index[s]] = scale[s] x src[s / K] for every slot s whose index lies inside [0, rows): the dy of the combine's backward
template <typename T>
__global__ void __launch_bounds__(MOE_THREADS) moe_scatter_kernel(const MoePieceArgs a) {
    for (int64_t item0 = blockIdx.x; item0 < a.items; item0 += (int64_t)MOE_UNROLL * gridDim.x) {
        u32x4 v[MOE_UNROLL];
        float w[MOE_UNROLL];
        int64_t p[MOE_UNROLL];
        int col[MOE_UNROLL];
        bool in[MOE_UNROLL];
#pragma unroll
        for (int u = 0; u < MOE_UNROLL; ++u) {
            int64_t s;
            in[u] = moe_piece(a, item0 + (int64_t)u * gridDim.x, s, col[u]);
            if (in[u]) {
                p[u] = a.index[s];
                in[u] = (uint64_t)p[u] < (uint64_t)a.rows;
            }
            if (in[u]) {
                v[u] = *reinterpret_cast<const u32x4*>(a.src + (s / a.K) * a.src_rs + col[u]);
                w[u] = a.scale[s];
            }
        }
#pragma unroll
        for (int u = 0; u < MOE_UNROLL; ++u)
            if (in[u]) *reinterpret_cast<u32x4*>(a.dst + p[u] * a.dst_rs + col[u]) = moe_scale8<T>(v[u], w[u]);
    }
}

// out[t] = round16(sum_k w[t, k] * y[pos[t, k]]): fma in ascending k from +0; scale NULL: ones
template <typename T>
__global__ void __launch_bounds__(MOE_THREADS) moe_combine_kernel(const MoePieceArgs a) {
    using El = Elem<T>;
    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        int64_t t;
        int col;
        if (!moe_piece(a, item, t, col)) continue;
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        for (int k0 = 0; k0 < a.K; k0 += MOE_UNROLL) {
            u32x4 v[MOE_UNROLL];
            float w[MOE_UNROLL];
            bool on[MOE_UNROLL];
#pragma unroll
            for (int u = 0; u < MOE_UNROLL; ++u) {
                on[u] = false;
                if (k0 + u < a.K) {
                    const int64_t p = a.index[t * a.K + k0 + u];
                    on[u] = (uint64_t)p < (uint64_t)a.rows;
                    if (on[u]) {
                        v[u] = *reinterpret_cast<const u32x4*>(a.src + p * a.src_rs + col);
                        w[u] = a.scale ? a.scale[t * a.K + k0 + u] : 1.f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < MOE_UNROLL; ++u) {
                if (on[u]) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        acc[2 * i] = fmaf(w[u], El::lo(v[u][i]), acc[2 * i]);
                        acc[2 * i + 1] = fmaf(w[u], El::hi(v[u][i]), acc[2 * i + 1]);
                    }
                }
            }
        }
        u32x4 y;
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = El::pack2(acc[2 * i], acc[2 * i + 1]);
        *reinterpret_cast<u32x4*>(a.dst + t * a.dst_rs + col) = y;
    }
}

// ---- dw[s] = sum_n dout[s / K, n] * y[pos[s], n] in fa_rowsum.h's order
struct MoeDwArgs {
    const uint16_t* dout; const uint16_t* y; const int* pos; float* dw;
    int64_t dout_rs, y_rs, rows, slots;
    int K, n, glog2, threads, pieces;
};

template <typename T>
__device__ __forceinline__ float moe_piece_dot(const uint16_t* a, const uint16_t* b) {
    float x[8], y[8];
    row_load8<T>(a, 0, false, x);
    row_load8<T>(b, 0, false, y);
    return rms_piece_dot(x, y);
}

template <typename T>
__global__ void __launch_bounds__(MOE_THREADS) moe_dw_small_kernel(const MoeDwArgs a) {
    const int G = 1 << a.glog2;
    const int gl = (int)threadIdx.x & (G - 1);
    const int64_t s = (int64_t)blockIdx.x * (MOE_THREADS >> a.glog2) + ((int)threadIdx.x >> a.glog2);
    const int64_t p = s < a.slots ? (int64_t)a.pos[s] : -1;
    const bool on = (uint64_t)p < (uint64_t)a.rows;
    float part = 0.f;
    if (on && gl * 8 < a.n) part = moe_piece_dot<T>(a.dout + (s / a.K) * a.dout_rs + gl * 8, a.y + p * a.y_rs + gl * 8);
    part = rms_group_sum(part, G);
    if (s < a.slots && gl == 0) a.dw[s] = on ? part : 0.f;
}

template <typename T>
__global__ void __launch_bounds__(ROW_THREADS) moe_dw_wide_kernel(const MoeDwArgs a) {
    __shared__ float slot[ROW_WAVES];
    const int64_t s = blockIdx.x;
    const int64_t p = a.pos[s];
    if (!((uint64_t)p < (uint64_t)a.rows)) {                  // (uniform over the workgroup)
        if (threadIdx.x == 0) a.dw[s] = 0.f;
        return;
    }
    const uint16_t* d = a.dout + (s / a.K) * a.dout_rs;
    const uint16_t* y = a.y + p * a.y_rs;
    float sum = 0.f;
    for (int j = 0; j < a.pieces; ++j) {
        const int col = 8 * ((int)threadIdx.x + j * a.threads);
        const float part = col < a.n ? moe_piece_dot<T>(d + col, y + col) : 0.f;
        sum = j == 0 ? part : sum + part;
    }
    sum = row_block_sum(sum, slot, a.threads / 64, (int)threadIdx.x >> 6);
    if (threadIdx.x == 0) a.dw[s] = sum;
}

// ---- the host side.  The caller (fa_api.hip) has validated every block
template <typename T>
static void launch_route_scoring(const MoeRouteArgs& a, int scoring, bool bwd, hipStream_t stream) {
    const int64_t per = MOE_THREADS >> a.glog2;
    const dim3 g((unsigned)((a.tokens + per - 1) / per)), b(MOE_THREADS);
    if (bwd) {
        if (scoring == FA_MOE_SOFTMAX) hipLaunchKernelGGL((moe_route_bwd_kernel<T, FA_MOE_SOFTMAX>), g, b, 0, stream, a);
        else                           hipLaunchKernelGGL((moe_route_bwd_kernel<T, FA_MOE_SIGMOID>), g, b, 0, stream, a);
    } else {
        if (scoring == FA_MOE_SOFTMAX) hipLaunchKernelGGL((moe_route_kernel<T, FA_MOE_SOFTMAX>), g, b, 0, stream, a);
        else                           hipLaunchKernelGGL((moe_route_kernel<T, FA_MOE_SIGMOID>), g, b, 0, stream, a);
    }
}

static void launch_route_dtype(const MoeRouteArgs& a, int dtype, int scoring, bool bwd, hipStream_t stream) {
    if (dtype == FA_BF16)      launch_route_scoring<bf16_tag>(a, scoring, bwd, stream);
    else if (dtype == FA_FP16) launch_route_scoring<fp16_tag>(a, scoring, bwd, stream);
    else                       launch_route_scoring<f32_tag>(a, scoring, bwd, stream);
}

void launch_moe_route(const fa_moe_route_params& s, hipStream_t stream) {
    MoeRouteArgs a = {};
    a.logits = s.logits; a.bias = s.scoring == FA_MOE_SIGMOID ? static_cast<const float*>(s.bias) : nullptr;
    a.weights = static_cast<float*>(s.weights); a.ids = static_cast<int*>(s.ids);
    a.rs = s.logits_row_stride; a.tokens = s.tokens;
    a.E = s.num_experts; a.K = s.top_k; a.glog2 = moe_group_log2(s.num_experts); a.renorm = s.renormalize; a.scale = s.scale;
    launch_route_dtype(a, s.dtype, s.scoring, false, stream);
}

void launch_moe_route_bwd(const fa_moe_route_bwd_params& s, hipStream_t stream) {
    MoeRouteArgs a = {};
    a.logits = s.logits; a.ids = const_cast<int*>(static_cast<const int*>(s.ids));
    a.dweights = static_cast<const float*>(s.dweights); a.dlogits = s.dlogits;
    a.rs = s.logits_row_stride; a.drs = s.dlogits_row_stride; a.tokens = s.tokens;
    a.E = s.num_experts; a.K = s.top_k; a.glog2 = moe_group_log2(s.num_experts); a.renorm = s.renormalize; a.scale = s.scale;
    launch_route_dtype(a, s.dtype, s.scoring, true, stream);
}

void launch_moe_sort(const fa_moe_sort_params& s, hipStream_t stream) {
    MoeSortArgs a = {};
    a.ids = static_cast<const int*>(s.ids); a.sorted_slot = static_cast<int*>(s.sorted_slot); a.pos = static_cast<int*>(s.pos);
    a.offsets = static_cast<int*>(s.expert_offsets); a.counts = static_cast<int*>(s.workspace);
    a.slots = s.tokens * s.top_k;
    a.mmax = a.slots + (int64_t)s.num_experts * (s.align - 1);
    const MoeSortPlan pl = moe_sort_plan(a.slots, s.num_experts);
    a.chunk = pl.chunk; a.chunks = pl.chunks; a.E = s.num_experts; a.align = s.align;
    hipLaunchKernelGGL(moe_sort_count_kernel, dim3((unsigned)pl.chunks), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(moe_sort_scan_kernel, dim3(1), dim3(MOE_MAX_EXPERTS), 0, stream, a);
    if (a.slots > 0) hipLaunchKernelGGL(moe_sort_place_kernel, dim3((unsigned)pl.chunks), dim3(64), 0, stream, a);
}

static void piece_plan(MoePieceArgs& a, int64_t out_rows, int n, unsigned* grid) {
    a.P = n / 8;
    a.total = out_rows * a.P;
    a.items = (a.total + MOE_THREADS - 1) / MOE_THREADS;
    *grid = (unsigned)(a.items < MOE_GRID_CAP ? a.items : MOE_GRID_CAP);
}

static void launch_permute(MoePieceArgs& a, int64_t out_rows, int n, int dtype, hipStream_t stream) {
    unsigned grid;
    piece_plan(a, out_rows, n, &grid);
    if (grid == 0) return;
    const dim3 g(grid), b(MOE_THREADS);
    if (dtype == FA_BF16) {
        if (a.scale) hipLaunchKernelGGL((moe_permute_kernel<bf16_tag, true>), g, b, 0, stream, a);
        else         hipLaunchKernelGGL((moe_permute_kernel<bf16_tag, false>), g, b, 0, stream, a);
    } else {
        if (a.scale) hipLaunchKernelGGL((moe_permute_kernel<fp16_tag, true>), g, b, 0, stream, a);
        else         hipLaunchKernelGGL((moe_permute_kernel<fp16_tag, false>), g, b, 0, stream, a);
    }
}

void launch_moe_permute(const fa_moe_permute_params& s, hipStream_t stream) {
    MoePieceArgs a = {};
    a.src = static_cast<const uint16_t*>(s.x); a.index = static_cast<const int*>(s.sorted_slot);
    a.scale = static_cast<const float*>(s.slot_scale); a.dst = static_cast<uint16_t*>(s.out);
    a.src_rs = s.x_row_stride; a.dst_rs = s.out_row_stride; a.rows = s.rows; a.slots = s.tokens * s.top_k; a.K = s.top_k;
    launch_permute(a, s.rows, s.n, s.dtype, stream);
}

void launch_moe_combine(const fa_moe_combine_params& s, hipStream_t stream) {
    MoePieceArgs a = {};
    a.src = static_cast<const uint16_t*>(s.y); a.index = static_cast<const int*>(s.pos);
    a.scale = static_cast<const float*>(s.weights); a.dst = static_cast<uint16_t*>(s.out);
    a.src_rs = s.y_row_stride; a.dst_rs = s.out_row_stride; a.rows = s.rows; a.slots = s.tokens * s.top_k; a.K = s.top_k;
    unsigned grid;
    piece_plan(a, s.tokens, s.n, &grid);
    if (grid == 0) return;
    if (s.dtype == FA_BF16) hipLaunchKernelGGL(moe_combine_kernel<bf16_tag>, dim3(grid), dim3(MOE_THREADS), 0, stream, a);
    else                    hipLaunchKernelGGL(moe_combine_kernel<fp16_tag>, dim3(grid), dim3(MOE_THREADS), 0, stream, a);
}

void launch_moe_combine_bwd(const fa_moe_combine_bwd_params& s, hipStream_t stream) {
    const int64_t slots = s.tokens * s.top_k;
    if (s.dy) {
        MoePieceArgs z = {};                                 // dy = +0 ..
        z.dst = static_cast<uint16_t*>(s.dy); z.dst_rs = s.dy_row_stride; z.rows = s.rows; z.K = s.top_k;
        launch_permute(z, s.rows, s.n, s.dtype, stream);
        MoePieceArgs a = {};                                 // .. then the live rows
        a.src = static_cast<const uint16_t*>(s.dout); a.index = static_cast<const int*>(s.pos);
        a.scale = static_cast<const float*>(s.weights); a.dst = static_cast<uint16_t*>(s.dy);
        a.src_rs = s.dout_row_stride; a.dst_rs = s.dy_row_stride; a.rows = s.rows; a.slots = slots; a.K = s.top_k;
        unsigned grid;
        piece_plan(a, slots, s.n, &grid);
        if (grid) {
            if (s.dtype == FA_BF16) hipLaunchKernelGGL(moe_scatter_kernel<bf16_tag>, dim3(grid), dim3(MOE_THREADS), 0, stream, a);
            else                    hipLaunchKernelGGL(moe_scatter_kernel<fp16_tag>, dim3(grid), dim3(MOE_THREADS), 0, stream, a);
        }
    }
    if (s.dw && slots > 0) {
        MoeDwArgs a = {};
        a.dout = static_cast<const uint16_t*>(s.dout); a.y = static_cast<const uint16_t*>(s.y);
        a.pos = static_cast<const int*>(s.pos); a.dw = static_cast<float*>(s.dw);
        a.dout_rs = s.dout_row_stride; a.y_rs = s.y_row_stride; a.rows = s.rows; a.slots = slots; a.K = s.top_k; a.n = s.n;
        const RowShape sh = row_shape(s.n);
        a.glog2 = sh.group_log2; a.threads = sh.threads; a.pieces = sh.pieces;
        if (s.n <= ROW_SMALL_MAX) {
            const int64_t per = MOE_THREADS >> a.glog2;
            const dim3 g((unsigned)((slots + per - 1) / per)), b(MOE_THREADS);
            if (s.dtype == FA_BF16) hipLaunchKernelGGL(moe_dw_small_kernel<bf16_tag>, g, b, 0, stream, a);
            else                    hipLaunchKernelGGL(moe_dw_small_kernel<fp16_tag>, g, b, 0, stream, a);
        } else {
            const dim3 g((unsigned)slots), b((unsigned)sh.threads);
            if (s.dtype == FA_BF16) hipLaunchKernelGGL(moe_dw_wide_kernel<bf16_tag>, g, b, 0, stream, a);
            else                    hipLaunchKernelGGL(moe_dw_wide_kernel<fp16_tag>, g, b, 0, stream, a);
        }
    }
}

}  // namespace fa
