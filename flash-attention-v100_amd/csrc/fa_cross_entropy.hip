// fa_cross_entropy.hip - softmax cross-entropy over the vocabulary and its backward (fa_cross_entropy / fa_cross_entropy_bwd,
// include/fa_mi355.h).  logits x: [rows, V] fp16 / bf16 / fp32, labels int64 [rows]; all arithmetic fp32:
//     l_j  = logit_scale * float(x_j)                                     one rounding
//     lse  = m + log(s),  (m, s) the fixed-order running maximum and sum of exp(l_j - m) of fa_lse.h;  NaN where m = -inf
//     loss = fma(-(1 - ls), l_label, lse);  with smoothing ls > 0:  loss = fma(-(ls / V), sum_j l_j, loss)
//     z    = (lse_square_scale * lse) * lse;   loss = loss + z
//     dx_j = round_x(g * (((p_j * F) - (1 - ls) [j == label]) - ls / V)),   p_j = e(l_j - lse),  g = dloss * logit_scale,
//            F = fma(2 lse_square_scale, lse, 1)
// 1 - ls and ls / V are formed on the host in fp32.  sum_j l_j skips columns of -inf (they contribute 0 everywhere) and is not
// formed at ls = 0.  label == ignore_index: loss = z = +0 and a dx row of +0; a label outside [0, V): NaN - it is only ever
// COMPARED with column numbers, no address is formed from it.
// Forward: a row is cut into nchunks = ceil(V / CHUNK) column chunks (CHUNK: a function of the dtype alone, ce_chunk) and the grid
// is rows x nchunks workgroups of 256 lanes.  Lane t owns the pieces (8 columns, counted from column 0 of the row) t, t + 256, ..
// of its chunk and folds them into its state in that order; the lanes, the waves and - in ce_merge_kernel, from one 16-byte
// partial (m, s, sum l) per workgroup - the chunks meet in fa_lse.h's order.  With nchunks == 1 the workgroup writes the results
// itself: one launch, no workspace.  A piece is one 16-byte load (fp32: two) where the row starts on a 16-byte boundary and the
// piece lies inside the row, and is taken element by element otherwise: the same values either way, and never a column >= V.
// Backward: rows x ceil(V / 8192) workgroups; a lane loads its 4 pieces, then stores them: dx == x is legal.
// No atomics, LDS only for the wave slots, every offset 64-bit.
#include <cmath>
#include <cstdint>
#include "fa_lse.h"

#ifndef FA_CE_CHUNK16
#define FA_CE_CHUNK16 32768       // columns per forward workgroup, 16-bit logits (profiles/cross_entropy.txt: the sweep)
#endif
#ifndef FA_CE_CHUNK32
#define FA_CE_CHUNK32 (FA_CE_CHUNK16 / 2)   // fp32 logits: the same bytes per workgroup
#endif

namespace fa {

constexpr int CE_THREADS = ROW_THREADS;
constexpr int CE_STEP = 8 * CE_THREADS;                   // columns the workgroup takes side by side
constexpr int CE_UNROLL = 4;                              // pieces a lane has in flight
constexpr int CE_BWD_CHUNK = CE_UNROLL * CE_STEP;         // columns per backward workgroup
static_assert(FA_CE_CHUNK16 % CE_STEP == 0 && FA_CE_CHUNK32 % CE_STEP == 0 && FA_CE_CHUNK16 > 0 && FA_CE_CHUNK32 > 0,
              "a chunk is whole steps of the workgroup");

// the row starts on a 16-byte boundary: its whole pieces are taken with vector accesses
template <typename T>
__device__ __forceinline__ bool ce_row_vec(const void* base, int64_t rowoff) {
    return ((reinterpret_cast<uintptr_t>(base) + (uint64_t)rowoff * RowIo<T>::ESIZE) & 15) == 0;
}

// l of the piece at column `col` of the row at element offset `rowoff`; columns >= V: -inf
template <typename T>
__device__ __forceinline__ void ce_load_piece(const void* x, int64_t rowoff, int64_t col, int V, bool vec, float scale, float (&l)[8]) {
    if (vec && col + 8 <= V) {
        RowIo<T>::load8(x, rowoff + col, l);
#pragma unroll
        for (int i = 0; i < 8; ++i) l[i] = scale * l[i];
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) l[i] = col + i < V ? scale * RowIo<T>::load1(x, rowoff + col + i) : -INFINITY;
    }
}

// the piece's part of sum_j l_j in column order; a column of -inf hands in +0
__device__ __forceinline__ float ce_piece_sum(const float (&l)[8]) {
    float s = l[0] == -INFINITY ? 0.f : l[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s += l[i] == -INFINITY ? 0.f : l[i];
    return s;
}

struct CeArgs {
    const void* x;
    const int64_t* labels;
    float* losses;
    float* z_losses;
    float* lse;
    f32x4* ws;                                            // [rows, nchunks] partials (m, s, sum l, 0); nchunks == 1: unused
    int64_t x_rs, rows, ignore_index;
    int V, chunk, nchunks, smooth;
    float scale, one_minus_ls, ls_over_v, zscale;
};

// lse, loss and z_loss of one row from its whole state: one lane
template <typename T>
__device__ __forceinline__ void ce_finish(const CeArgs& a, int64_t row, const LseState& st, float sum_l) {
    const float lse = st.m == -INFINITY ? NAN : st.m + logf(st.s);
    a.lse[row] = lse;
    const int64_t lab = a.labels[row];
    float loss = 0.f, z = 0.f;
    if (lab != a.ignore_index) {
        if (lab < 0 || lab >= a.V) {
            loss = z = NAN;
        } else {
            const float ll = a.scale * RowIo<T>::load1(a.x, row * a.x_rs + lab);
            loss = fmaf(-a.one_minus_ls, ll, lse);
            if (a.smooth) loss = fmaf(-a.ls_over_v, sum_l, loss);
            z = (a.zscale * lse) * lse;
            loss = loss + z;
        }
    }
    a.losses[row] = loss;
    a.z_losses[row] = z;
}

template <typename T, bool SMOOTH>
__global__ void __launch_bounds__(CE_THREADS) ce_fwd_kernel(const CeArgs a) {
    __shared__ float red[3 * ROW_WAVES];
    const int64_t row = (int64_t)blockIdx.x / a.nchunks;
    const int chunk = (int)((int64_t)blockIdx.x - row * a.nchunks);
    const int64_t rowoff = row * a.x_rs;
    const bool vec = ce_row_vec<T>(a.x, rowoff);
    const int64_t c0 = (int64_t)chunk * a.chunk;
    const int64_t c1 = c0 + a.chunk < a.V ? c0 + a.chunk : a.V;
    LseState st = {-INFINITY, 0.f};
    float sum_l = 0.f;
    for (int64_t base = c0 + 8 * (int)threadIdx.x; base < c1; base += (int64_t)CE_UNROLL * CE_STEP) {
        float l[CE_UNROLL][8];
#pragma unroll
        for (int u = 0; u < CE_UNROLL; ++u) {
            const int64_t col = base + (int64_t)u * CE_STEP;
            if (col < c1) ce_load_piece<T>(a.x, rowoff, col, a.V, vec, a.scale, l[u]);
        }
#pragma unroll
        for (int u = 0; u < CE_UNROLL; ++u) {
            if (base + (int64_t)u * CE_STEP < c1) {
                lse_piece(st, l[u]);
                if constexpr (SMOOTH) sum_l += ce_piece_sum(l[u]);
            }
        }
    }
    const int wave = (int)threadIdx.x >> 6;
    st = lse_block(lse_wave(st), red, ROW_WAVES, wave);
    if constexpr (SMOOTH) sum_l = row_block_sum(sum_l, red + 2 * ROW_WAVES, ROW_WAVES, wave);
    if (threadIdx.x != 0) return;
    if (a.nchunks == 1) ce_finish<T>(a, row, st, sum_l);
    else a.ws[row * a.nchunks + chunk] = f32x4{st.m, st.s, sum_l, 0.f};
}

// one lane per row: the chunks in index order
template <typename T>
__global__ void __launch_bounds__(64) ce_merge_kernel(const CeArgs a) {
    const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (row >= a.rows) return;
    const f32x4* p = a.ws + row * a.nchunks;
    f32x4 v = p[0];
    LseState st = {v[0], v[1]};
    float sum_l = v[2];
    for (int c = 1; c < a.nchunks; ++c) {
        v = p[c];
        st = lse_merge(st, LseState{v[0], v[1]});
        sum_l += v[2];
    }
    ce_finish<T>(a, row, st, sum_l);
}

struct CeBwdArgs {
    const float* dlosses;
    const void* x;
    const int64_t* labels;
    const float* lse;
    void* dx;
    int64_t dl_stride, x_rs, dx_rs, rows, ignore_index;
    int V, nchunks;
    float scale, one_minus_ls, ls_over_v, two_z;
};

template <typename T>
__global__ void __launch_bounds__(CE_THREADS) ce_bwd_kernel(const CeBwdArgs a) {
    const int64_t row = (int64_t)blockIdx.x / a.nchunks;
    const int chunk = (int)((int64_t)blockIdx.x - row * a.nchunks);
    const int64_t xoff = row * a.x_rs, doff = row * a.dx_rs;
    const bool vec_in = ce_row_vec<T>(a.x, xoff), vec_out = ce_row_vec<T>(a.dx, doff);
    const int64_t lab = a.labels[row];
    const bool ignored = lab == a.ignore_index;
    const bool bad = !ignored && (lab < 0 || lab >= a.V);
    const int64_t base = (int64_t)chunk * CE_BWD_CHUNK + 8 * (int)threadIdx.x;
    float v[CE_UNROLL][8];
    if (ignored || bad) {
        const float fill = bad ? NAN : 0.f;
#pragma unroll
        for (int u = 0; u < CE_UNROLL; ++u) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[u][i] = fill;
        }
    } else {
        const float lse = a.lse[row];
        const float g = a.dlosses[row * a.dl_stride] * a.scale;
        const float F = fmaf(a.two_z, lse, 1.0f);
#pragma unroll
        for (int u = 0; u < CE_UNROLL; ++u) {
            const int64_t col = base + (int64_t)u * CE_STEP;
            if (col < a.V) ce_load_piece<T>(a.x, xoff, col, a.V, vec_in, a.scale, v[u]);
        }
#pragma unroll
        for (int u = 0; u < CE_UNROLL; ++u) {
            const int64_t col = base + (int64_t)u * CE_STEP;
            if (col < a.V) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float t = lse_exp(v[u][i] - lse) * F;
                    t = t - (col + i == lab ? a.one_minus_ls : 0.f);
                    t = t - a.ls_over_v;
                    v[u][i] = g * t;
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < CE_UNROLL; ++u) {
        const int64_t col = base + (int64_t)u * CE_STEP;
        if (col >= a.V) continue;
        if (vec_out && col + 8 <= a.V) {
            RowIo<T>::store8(a.dx, doff + col, v[u]);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (col + i < a.V) RowIo<T>::store1(a.dx, doff + col + i, v[u][i]);
        }
    }
}

// ---- the host side: the launch plan is a function of (rows, V, dtype) alone
int ce_chunk(int dtype) { return dtype == FA_FP32 ? FA_CE_CHUNK32 : FA_CE_CHUNK16; }
int64_t ce_nchunks(int V, int dtype) { return ((int64_t)V + ce_chunk(dtype) - 1) / ce_chunk(dtype); }
int64_t ce_bwd_nchunks(int V) { return ((int64_t)V + CE_BWD_CHUNK - 1) / CE_BWD_CHUNK; }
size_t cross_entropy_workspace_bytes(int64_t rows, int V, int dtype) {
    const int64_t nc = ce_nchunks(V, dtype);
    return nc <= 1 ? 0 : (size_t)rows * (size_t)nc * sizeof(f32x4);
}

template <typename T>
static void launch_ce(const CeArgs& a, hipStream_t stream) {
    const dim3 g((unsigned)(a.rows * a.nchunks)), b(CE_THREADS);
    if (a.smooth) hipLaunchKernelGGL((ce_fwd_kernel<T, true>), g, b, 0, stream, a);
    else          hipLaunchKernelGGL((ce_fwd_kernel<T, false>), g, b, 0, stream, a);
    if (a.nchunks > 1) hipLaunchKernelGGL((ce_merge_kernel<T>), dim3((unsigned)((a.rows + 63) / 64)), dim3(64), 0, stream, a);
}

// The caller (fa_api.hip) has validated the block; rows > 0
void launch_cross_entropy(const fa_cross_entropy_params& s, hipStream_t stream) {
    CeArgs a;
    a.x = s.logits; a.labels = s.labels;
    a.losses = s.losses; a.z_losses = s.z_losses; a.lse = s.lse;
    a.ws = static_cast<f32x4*>(s.workspace);
    a.x_rs = s.logits_row_stride; a.rows = s.rows; a.ignore_index = s.ignore_index;
    a.V = s.vocab; a.chunk = ce_chunk(s.dtype); a.nchunks = (int)ce_nchunks(s.vocab, s.dtype);
    a.smooth = s.label_smoothing > 0.f;
    a.scale = s.logit_scale;
    a.one_minus_ls = 1.0f - s.label_smoothing;
    a.ls_over_v = s.label_smoothing / (float)s.vocab;
    a.zscale = s.lse_square_scale;
    if (s.dtype == FA_BF16) launch_ce<bf16_tag>(a, stream);
    else if (s.dtype == FA_FP16) launch_ce<fp16_tag>(a, stream);
    else launch_ce<fp32_tag>(a, stream);
}

void launch_cross_entropy_bwd(const fa_cross_entropy_bwd_params& s, hipStream_t stream) {
    CeBwdArgs a;
    a.dlosses = s.dlosses; a.x = s.logits; a.labels = s.labels; a.lse = s.lse; a.dx = s.dlogits;
    a.dl_stride = s.dlosses_stride; a.x_rs = s.logits_row_stride; a.dx_rs = s.dlogits_row_stride;
    a.rows = s.rows; a.ignore_index = s.ignore_index;
    a.V = s.vocab; a.nchunks = (int)ce_bwd_nchunks(s.vocab);
    a.scale = s.logit_scale;
    a.one_minus_ls = 1.0f - s.label_smoothing;
    a.ls_over_v = s.label_smoothing / (float)s.vocab;
    a.two_z = 2.0f * s.lse_square_scale;
    const dim3 g((unsigned)(a.rows * a.nchunks)), b(CE_THREADS);
    if (s.dtype == FA_BF16) hipLaunchKernelGGL((ce_bwd_kernel<bf16_tag>), g, b, 0, stream, a);
    else if (s.dtype == FA_FP16) hipLaunchKernelGGL((ce_bwd_kernel<fp16_tag>), g, b, 0, stream, a);
    else hipLaunchKernelGGL((ce_bwd_kernel<fp32_tag>), g, b, 0, stream, a);
}

}  // namespace fa
