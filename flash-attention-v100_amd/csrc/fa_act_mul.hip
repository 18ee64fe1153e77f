// fa_act_mul.hip - the gated activation of the MLP and its backward (fa_act_mul / fa_act_mul_bwd, include/fa_mi355.h): SwiGLU,
// GeGLU and their ungated forms.  gate, up, out, dout, dgate, dup: [rows, N] fp16 / bf16, last dimension contiguous, each with a
// row stride of its own.  All arithmetic fp32, ONE rounding to the io type per result:
//     g = float(gate_j), u = float(up_j), d = float(dout_j)
//     out_j   = round16(act(g) * u)                 up == NULL: round16(act(g))
//     dgate_j = round16((d * u) * act'(g))          up == NULL: round16(d * act'(g))
//     dup_j   = round16(d * act(g))
// with act / act' in exactly this fp32 order (every operation rounds once; fma is one rounding):
//     e(t) = exp2(t * log2e) on v_exp_f32, log2e rounded to fp32;  sig(t) = rcp(1 + e(-t)) on v_rcp_f32
//     SILU       s = sig(g);  act = g * s;  act' = s * fma(g, 1 - s, 1)
//     GELU_TANH  q = g * g;  w = (K2 * g) * fma(C3, q, 1);  s = sig(w);  act = g * s            [0.5 (1 + tanh z) = sig(2 z), w = 2 z]
//                act' = s * fma(g * (1 - s), K2 * fma(3 C3, q, 1), 1)     K2 = 2 sqrt(2 / pi), C3 = 0.044715, 3 C3 = 0.134145
//     GELU       ph = fma(0.5, erff(g * sqrt(1/2)), 0.5);  act = g * ph;  act' = fma(g, e((g * g) * -0.5) * sqrt(1 / (2 pi)), ph)
//     RELU       act = g <= 0 ? +0 : g  (a NaN stays);  act' = g <= 0 ? 0 : (g > 0 ? 1 : g)
//     RELU2      r = relu(g);  act = r * r;  act' = r + r
// Special values are what these lines give literally (flash_attn_mi355/act_mul.py lists them); silu(-100) = -0, never NaN.
// Plan (a function of (rows, N) alone, act_plan): a row has P = ceil(N / 8) pieces of 8 columns counted from column 0; it is cut
// into nchunks = ceil(P / 1024) runs of the SAME length - chunk = ceil(P / nchunks) pieces rounded up to whole waves (64) - so no
// workgroup of a row is a quarter empty at N = 14336 (2 x 896 pieces instead of 1024 + 768) or 11008 (704 + 672).  An item is one
// run of one row; a workgroup of 256 lanes takes the items blockIdx.x, blockIdx.x + gridDim.x, .. (grid = min(items,
// FA_ACT_GRID_CAP)).  Lane t owns the pieces t, t + 256, t + 512, t + 768 of the run and no other lane touches them: the forward
// loads all four from every input before its first store, the backward - three inputs - two and then the other two, each pair
// loaded before it is stored, so out == gate, out == up, dgate == gate and dup == up are legal.  A piece is one nontemporal 16-byte
// load per input and one ordinary 16-byte store per output where that tensor's row starts on a 16-byte boundary and the piece
// lies inside the row, and is taken element by element otherwise: the same bits either way, never a column >= N.  Every
// element's bits depend on its own operands alone.  No LDS, no atomics, no workspace, every offset 64-bit.
#include <cmath>
#include <cstdint>
#include "fa_common.h"
#include "fa_act.h"
#include "fa_rowops.h"

#ifndef FA_ACT_GRID_CAP
#define FA_ACT_GRID_CAP 65536         // workgroups (profiles/act_mul.txt: 1024 and 2048 - about what is resident at once - lose 10 - 30 %)
#endif
#ifndef FA_ACT_NT_LOADS
#define FA_ACT_NT_LOADS 1             // 0: ordinary loads (profiles/act_mul.txt)
#endif

namespace fa {

constexpr int ACT_THREADS = 256;
constexpr int ACT_UNROLL = 4;                               // pieces a lane has in flight per input
constexpr int ACT_MAX_PIECES = ACT_UNROLL * ACT_THREADS;    // pieces per item at most (8192 columns)

struct ActPlan { int chunk_pieces; int64_t nchunks, items; int grid; };
ActPlan act_plan(int64_t rows, int n) {
    ActPlan pl;
    const int64_t P = ((int64_t)n + 7) / 8;
    pl.nchunks = (P + ACT_MAX_PIECES - 1) / ACT_MAX_PIECES;
    const int64_t per = (P + pl.nchunks - 1) / pl.nchunks;
    pl.chunk_pieces = (int)((per + 63) / 64 * 64);           // (<= ACT_MAX_PIECES: that is a multiple of 64)
    pl.nchunks = (P + pl.chunk_pieces - 1) / pl.chunk_pieces;
    pl.items = rows * pl.nchunks;                            // the caller has checked rows <= (2^31 - 1) / nchunks
    pl.grid = (int)(pl.items < FA_ACT_GRID_CAP ? pl.items : FA_ACT_GRID_CAP);
    return pl;
}

// (act_eval - act(g) and act'(g) - is fa_act.h's: fa_act_mul_quant, fa_quant.hip, rounds the same values)

// the row at element offset `off` starts on a 16-byte boundary: its whole pieces are taken with vector accesses
__device__ __forceinline__ bool act_row_vec(const uint16_t* base, int64_t off) {
    return ((reinterpret_cast<uintptr_t>(base) + (uint64_t)off * 2) & 15) == 0;
}

// the piece at column `col` of the row at `off`; columns >= n: +0, never read
template <typename T>
__device__ __forceinline__ void act_load(const uint16_t* p, int64_t off, int64_t col, int n, bool vec, float (&v)[8]) {
    using E = Elem<T>;
    if (vec && col + 8 <= n) {
#if FA_ACT_NT_LOADS
        const u32x4 a = ld_nt16(p + off + col);
#else
        const u32x4 a = *reinterpret_cast<const u32x4*>(p + off + col);
#endif
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = E::lo(a[i]); v[2 * i + 1] = E::hi(a[i]); }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = col + i < n ? E::lo((uint32_t)p[off + col + i]) : 0.f;
    }
}

template <typename T>
__device__ __forceinline__ void act_store(uint16_t* p, int64_t off, int64_t col, int n, bool vec, const float (&v)[8]) {
    using E = Elem<T>;
    if (vec && col + 8 <= n) {
        u32x4 y;
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = E::pack2(v[2 * i], v[2 * i + 1]);
        *reinterpret_cast<u32x4*>(p + off + col) = y;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (col + i < n) p[off + col + i] = (uint16_t)E::pack2(v[i], 0.f);
    }
}

struct ActArgs {
    const uint16_t *gate, *up, *dout;                       // forward: dout unused
    uint16_t *out, *dup;                                    // forward: out; backward: out = dgate
    int64_t gate_rs, up_rs, dout_rs, out_rs, dup_rs;
    int64_t items, nchunks;
    int n, chunk;                                           // chunk: columns per run
};

template <typename T, int ACT, bool GATED>
__global__ void __launch_bounds__(ACT_THREADS) act_mul_kernel(const ActArgs a) {
    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int64_t row = item / a.nchunks;
        const int64_t c0 = (item - row * a.nchunks) * a.chunk;
        const int64_t c1 = c0 + a.chunk < a.n ? c0 + a.chunk : a.n;
        const int64_t goff = row * a.gate_rs, uoff = row * a.up_rs, ooff = row * a.out_rs;
        const bool gvec = act_row_vec(a.gate, goff), ovec = act_row_vec(a.out, ooff);
        const bool uvec = GATED && act_row_vec(a.up, uoff);
        const int64_t base = c0 + 8 * (int)threadIdx.x;
        float g[ACT_UNROLL][8], u[ACT_UNROLL][8];
#pragma unroll
        for (int k = 0; k < ACT_UNROLL; ++k) {
            const int64_t col = base + (int64_t)k * 8 * ACT_THREADS;
            if (col < c1) {
                act_load<T>(a.gate, goff, col, a.n, gvec, g[k]);
                if constexpr (GATED) act_load<T>(a.up, uoff, col, a.n, uvec, u[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < ACT_UNROLL; ++k) {
            const int64_t col = base + (int64_t)k * 8 * ACT_THREADS;
            if (col < c1) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float av, dv;
                    act_eval<ACT, false>(g[k][i], av, dv);
                    g[k][i] = GATED ? av * u[k][i] : av;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < ACT_UNROLL; ++k) {
            const int64_t col = base + (int64_t)k * 8 * ACT_THREADS;
            if (col < c1) act_store<T>(a.out, ooff, col, a.n, ovec, g[k]);
        }
    }
}

// the backward holds three inputs per piece: two pieces in flight per half of the lane's four, each half loaded before it is stored
// - a lane's pieces are its own, so in place stays legal
template <typename T, int ACT, bool GATED>
__global__ void __launch_bounds__(ACT_THREADS) act_mul_bwd_kernel(const ActArgs a) {
    constexpr int HALF = ACT_UNROLL / 2;
    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int64_t row = item / a.nchunks;
        const int64_t c0 = (item - row * a.nchunks) * a.chunk;
        const int64_t c1 = c0 + a.chunk < a.n ? c0 + a.chunk : a.n;
        const int64_t goff = row * a.gate_rs, uoff = row * a.up_rs, doff = row * a.dout_rs, ooff = row * a.out_rs,
                      poff = row * a.dup_rs;
        const bool gvec = act_row_vec(a.gate, goff), dvec = act_row_vec(a.dout, doff), ovec = act_row_vec(a.out, ooff);
        const bool uvec = GATED && act_row_vec(a.up, uoff), pvec = GATED && act_row_vec(a.dup, poff);
#pragma unroll
        for (int h = 0; h < ACT_UNROLL; h += HALF) {
            const int64_t base = c0 + 8 * (int)threadIdx.x + (int64_t)h * 8 * ACT_THREADS;
            float g[HALF][8], u[HALF][8], d[HALF][8];
#pragma unroll
            for (int k = 0; k < HALF; ++k) {
                const int64_t col = base + (int64_t)k * 8 * ACT_THREADS;
                if (col < c1) {
                    act_load<T>(a.dout, doff, col, a.n, dvec, d[k]);
                    act_load<T>(a.gate, goff, col, a.n, gvec, g[k]);
                    if constexpr (GATED) act_load<T>(a.up, uoff, col, a.n, uvec, u[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < HALF; ++k) {
                const int64_t col = base + (int64_t)k * 8 * ACT_THREADS;
                if (col < c1) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        float av, dv;
                        act_eval<ACT, true>(g[k][i], av, dv);
                        if constexpr (GATED) {
                            g[k][i] = (d[k][i] * u[k][i]) * dv;
                            u[k][i] = d[k][i] * av;
                        } else {
                            g[k][i] = d[k][i] * dv;
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < HALF; ++k) {
                const int64_t col = base + (int64_t)k * 8 * ACT_THREADS;
                if (col < c1) {
                    act_store<T>(a.out, ooff, col, a.n, ovec, g[k]);
                    if constexpr (GATED) act_store<T>(a.dup, poff, col, a.n, pvec, u[k]);
                }
            }
        }
    }
}

// ---- the host side
template <typename T, int ACT, bool BWD>
static void launch_act_gated(const ActArgs& a, int grid, hipStream_t stream) {
    const dim3 g((unsigned)grid), b(ACT_THREADS);
    if constexpr (BWD) {
        if (a.up) hipLaunchKernelGGL((act_mul_bwd_kernel<T, ACT, true>), g, b, 0, stream, a);
        else      hipLaunchKernelGGL((act_mul_bwd_kernel<T, ACT, false>), g, b, 0, stream, a);
    } else {
        if (a.up) hipLaunchKernelGGL((act_mul_kernel<T, ACT, true>), g, b, 0, stream, a);
        else      hipLaunchKernelGGL((act_mul_kernel<T, ACT, false>), g, b, 0, stream, a);
    }
}

template <typename T, bool BWD>
static void launch_act_kind(const ActArgs& a, int act, int grid, hipStream_t stream) {
    switch (act) {
        case FA_ACT_SILU:      launch_act_gated<T, FA_ACT_SILU, BWD>(a, grid, stream); break;
        case FA_ACT_GELU:      launch_act_gated<T, FA_ACT_GELU, BWD>(a, grid, stream); break;
        case FA_ACT_GELU_TANH: launch_act_gated<T, FA_ACT_GELU_TANH, BWD>(a, grid, stream); break;
        case FA_ACT_RELU:      launch_act_gated<T, FA_ACT_RELU, BWD>(a, grid, stream); break;
        default:               launch_act_gated<T, FA_ACT_RELU2, BWD>(a, grid, stream); break;
    }
}

static void act_fill_plan(ActArgs& a, int64_t rows, int n, int* grid) {
    const ActPlan pl = act_plan(rows, n);
    a.items = pl.items; a.nchunks = pl.nchunks;
    a.n = n; a.chunk = 8 * pl.chunk_pieces;
    *grid = pl.grid;
}

// The caller (fa_api.hip) has validated the block; rows > 0
void launch_act_mul(const fa_act_mul_params& s, hipStream_t stream) {
    ActArgs a = {};
    a.gate = static_cast<const uint16_t*>(s.gate); a.up = static_cast<const uint16_t*>(s.up);
    a.out = static_cast<uint16_t*>(s.out);
    a.gate_rs = s.gate_row_stride; a.up_rs = s.up_row_stride; a.out_rs = s.out_row_stride;
    int grid;
    act_fill_plan(a, s.rows, s.n, &grid);
    if (s.dtype == FA_BF16) launch_act_kind<bf16_tag, false>(a, s.activation, grid, stream);
    else                    launch_act_kind<fp16_tag, false>(a, s.activation, grid, stream);
}

void launch_act_mul_bwd(const fa_act_mul_bwd_params& s, hipStream_t stream) {
    ActArgs a = {};
    a.dout = static_cast<const uint16_t*>(s.dout);
    a.gate = static_cast<const uint16_t*>(s.gate); a.up = static_cast<const uint16_t*>(s.up);
    a.out = static_cast<uint16_t*>(s.dgate); a.dup = static_cast<uint16_t*>(s.dup);
    a.dout_rs = s.dout_row_stride; a.gate_rs = s.gate_row_stride; a.up_rs = s.up_row_stride;
    a.out_rs = s.dgate_row_stride; a.dup_rs = s.dup_row_stride;
    int grid;
    act_fill_plan(a, s.rows, s.n, &grid);
    if (s.dtype == FA_BF16) launch_act_kind<bf16_tag, true>(a, s.activation, grid, stream);
    else                    launch_act_kind<fp16_tag, true>(a, s.activation, grid, stream);
}

}  // namespace fa
