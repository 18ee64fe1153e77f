// fa_add_norm_bwd.hip - the backward of fa_add_norm (fa_add_norm_bwd, include/fa_mi355.h): from dy (the gradient of out), the saved
// z (residual_out, or x) and an optional dres_out (the gradient of residual_out) to dx / dres and to dweight / dbias.  Both
// roundings of the forward are treated as the identity (straight-through); mean and rstd are RECOMPUTED from z with fa_rowsum.h's
// fixed-order sums, so they have the forward's bits and the forward saves nothing.
//     a = dy g,  xhat = z rstd  (LayerNorm: (z - mean) rstd)
//     RMSNorm:   c = (sum_d a xhat) / n,                          dz = rstd fmaf(-xhat, c, a)          (the QK-norm backward's form)
//     LayerNorm: c1 = (sum_d a) / n,  c2 = (sum_d a xhat) / n,    dz = rstd fmaf(-xhat, c2, a - c1)
//     with dres_out: dz = fmaf(rstd, that, dres_out);    dx = round16(dz),  dres = round_res(dz)
// The sums for c, c1, c2 have the forward's order (fa_rowsum.h), and the ownership is the forward's (fa_add_norm.hip): n <= 256 a
// group of G adjacent lanes per row, n > 256 a workgroup per row with the row in registers.  A lane issues all loads of a row
// before its stores and stores only columns it loaded: dx == dy is legal.
// dweight[d] = sum_rows dy xhat, dbias[d] = sum_rows dy - deterministic, no atomics (the QK-norm backward's pattern):
//   - workgroup b of P walks the consecutive rows (n <= 256: passes of 256 / G rows) of run b; a lane's columns are the same in
//     every row it meets, so it keeps its partial sums in registers and adds the rows with fmaf (dbias: +) in the order it meets them;
//   - n > 256: P <= 256 workgroups of 4 waves would leave the part nearly empty, so a workgroup keeps RW = 4, 2 or 1 rows in flight
//     (RW x threads lanes; a function of n and of whether dbias is wanted - what the register file takes without a spill): group g
//     walks the rows g, g + RW, .. of the run, and at the end group 0 adds the sums of groups 1, 2, .. to its own through LDS, in
//     that order.  A row's own sums do not change: its owner is still `threads` lanes with their own LDS slots;
//   - n <= 256: at the end the 256 / G lanes that own the same piece are added through LDS in the order of their thread index;
//   - the workgroup writes ONE fp32 partial row [1 or 2][n] into the workspace (2: dbias is wanted);
//   - a second kernel on the same stream adds the P partial rows - ANB_FIN_SEGS contiguous runs of them in row order side by side,
//     then the runs in order - and writes dweight / dbias with one rounding.
// P <= 256 and the run length depend on (rows, n, dbias wanted) alone (anb_plan: the workspace query and the launch share it), so
// the bits are the same on every card.  Without dweight and dbias: one row per workgroup / group, no workspace, no second launch.
#include <cstdint>
#include "fa_rowsum.h"

namespace fa {

constexpr int ANB_MAX_PARTS = 256;                        // partial rows: one per CU of the part
constexpr int ANB_FIN_COLS = 16;                          // the second kernel: columns per workgroup (64 bytes of a partial row) ...
constexpr int ANB_FIN_SEGS = ROW_THREADS / ANB_FIN_COLS;  // ... and runs of partial rows that are added side by side
constexpr int ANB_FIN_BATCH = 8;                          // partial rows whose loads are in flight together

struct AnbArgs {
    const uint16_t* dy;
    const void* z;
    const void* dro;                                      // nullptr: no dres_out
    uint16_t* dx;                                         // nullptr: not written
    void* dres;
    const void* w;
    float* partial;                                       // [parts][slots][n] fp32 (DW kernels)
    int64_t dy_rs, z_rs, dro_rs, dx_rs, dres_rs;          // row strides, elements
    int64_t rows, run;                                    // run: rows (n > 256) or passes (n <= 256) per workgroup
    int n, group_log2;
    int z_fp32, dres_fp32, w_fp32;
    float eps, w_offset;
};

struct AnbFinArgs {
    const float* partial;                                 // [n_parts][slots][n]
    void* dw;                                             // [n] of the weight's type, or nullptr
    void* db;
    int n_parts, n, slots, w_fp32;
};

enum { ANB_NONE = 0, ANB_DW = 1, ANB_DW_DB = 2 };         // DW: no weight gradient / dweight / dweight and dbias

// dz of one piece, stored to dx and dres
template <typename T>
__device__ __forceinline__ void anb_store8(const AnbArgs& a, int64_t row, int d, const float (&dz)[8]) {
    if (a.dx) row_store8<T>(a.dx, row * a.dx_rs + d, false, dz);
    if (a.dres) row_store8<T>(a.dres, row * a.dres_rs + d, a.dres_fp32 != 0, dz);
}

// the sums of one piece over the RW groups of a workgroup, through LDS: group 0 adds groups 1, 2, .. to its own, in that order.
// t: the lane's index in its group.  EVERY lane of the workgroup must call this
template <int RW>
__device__ __forceinline__ void anb_fold_groups(float (&mine)[8], float (*comb)[9], int grp, int t) {
    for (int g = 1; g < RW; ++g) {
        if (grp == g) {
#pragma unroll
            for (int i = 0; i < 8; ++i) comb[t][i] = mine[i];
        }
        __syncthreads();
        if (grp == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) mine[i] += comb[t][i];
        }
        __syncthreads();
    }
}

template <typename T, bool LN, int DW>
__global__ void __launch_bounds__(ROW_THREADS) add_norm_bwd_small_kernel(const AnbArgs a) {
    const int lanes = 1 << a.group_log2;
    const int j = (int)threadIdx.x & (lanes - 1);
    const bool piece = 8 * j < a.n;
    const int d = piece ? 8 * j : 0;                      // (clamped: the loads stay inside the row)
    const int slot = (int)threadIdx.x >> a.group_log2;
    const int spp = ROW_THREADS >> a.group_log2;          // rows per pass of the workgroup
    float g[8], dw[8], db[8];
    rms_gains<T>(a.w, d, a.w_fp32 != 0, a.w_offset, g);
#pragma unroll
    for (int i = 0; i < 8; ++i) dw[i] = db[i] = 0.f;
    const int64_t passes = (a.rows + spp - 1) / spp;
    const int64_t q0 = (int64_t)blockIdx.x * a.run;
    const int64_t q1 = q0 + a.run < passes ? q0 + a.run : passes;
    // (the trip count is workgroup-uniform: every lane of every wave takes part in the cross-lane reads below)
    for (int64_t q = q0; q < q1; ++q) {
        const int64_t r = q * spp + slot;
        const bool act = piece && r < a.rows;
        const int64_t row = r < a.rows ? r : 0;           // (a slot past the last row: row 0)
        float dy[8], z[8], dro[8];
        row_load8<T>(a.dy, row * a.dy_rs + d, false, dy);
        row_load8<T>(a.z, row * a.z_rs + d, a.z_fp32 != 0, z);
        if (a.dro) row_load8<T>(a.dro, row * a.dro_rs + d, a.z_fp32 != 0, dro);
        if (!act) {
#pragma unroll
            for (int i = 0; i < 8; ++i) z[i] = 0.f;
        }
        const float rstd = row_small_stats<LN>(z, act, lanes, a.n, a.eps);
        float xh[8], av[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { xh[i] = z[i] * rstd; av[i] = dy[i] * g[i]; }
        float c1 = 0.f;
        if constexpr (LN) c1 = rms_group_sum(act ? row_piece_sum(av) : 0.f, lanes) / (float)a.n;
        const float c = rms_group_sum(act ? rms_piece_dot(av, xh) : 0.f, lanes) / (float)a.n;
        float dz[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float t = fmaf(-xh[i], c, LN ? av[i] - c1 : av[i]);
            dz[i] = a.dro ? fmaf(rstd, t, dro[i]) : rstd * t;
        }
        if constexpr (DW != ANB_NONE) {
            if (act) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    dw[i] = fmaf(dy[i], xh[i], dw[i]);
                    if constexpr (DW == ANB_DW_DB) db[i] += dy[i];
                }
            }
        }
        if (act) anb_store8<T>(a, row, d, dz);
    }
    if constexpr (DW != ANB_NONE) {
        // the lanes that own the same piece, added in the order of their thread index; one partial row per workgroup
        constexpr int SLOTS = DW == ANB_DW_DB ? 2 : 1;
        __shared__ float red[ROW_THREADS][8 * SLOTS + 1]; // (+ 1: the lanes of a wave write their rows to different banks)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            red[threadIdx.x][i] = dw[i];
            if constexpr (DW == ANB_DW_DB) red[threadIdx.x][8 + i] = db[i];
        }
        __syncthreads();
        float* prow = a.partial + (int64_t)blockIdx.x * SLOTS * a.n;
        for (int w = (int)threadIdx.x; w < SLOTS * a.n; w += ROW_THREADS) {
            const int k = w >= a.n ? 1 : 0, col = w - k * a.n;
            const int pj = col >> 3, pi = (col & 7) + 8 * k;
            float s = red[pj][pi];
            for (int t = 1; t < spp; ++t) s += red[t * lanes + pj][pi];
            prow[w] = s;
        }
    }
}

// RW: rows in flight per workgroup (DW kernels: 1, 2 or 4 - the P <= 256 workgroups would otherwise keep 4 waves a CU busy); the
// workgroup has RW x `threads` lanes, group g = thread / threads walks the rows r0 + g, r0 + g + RW, .. of the run
template <typename T, bool LN, int NP, int DW, int RW>
__global__ void __launch_bounds__(ROW_THREADS * RW) add_norm_bwd_wide_kernel(const AnbArgs a) {
    __shared__ float red[4][RW][ROW_WAVES];
    const int threads = (int)blockDim.x / RW, nwaves = threads >> 6;
    const int grp = RW == 1 ? 0 : (int)threadIdx.x / threads, t = (int)threadIdx.x - grp * threads, wave = t >> 6;
    constexpr int NDW = DW != ANB_NONE ? NP : 1, NDB = DW == ANB_DW_DB ? NP : 1;
    float dw[NDW][8], db[NDB][8];
    int d[NP];
    bool on[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int c = 8 * (t + p * threads);
        on[p] = c < a.n;
        d[p] = on[p] ? c : 0;
    }
#pragma unroll
    for (int p = 0; p < NDW; ++p) {
#pragma unroll
        for (int i = 0; i < 8; ++i) dw[p][i] = 0.f;
    }
#pragma unroll
    for (int p = 0; p < NDB; ++p) {
#pragma unroll
        for (int i = 0; i < 8; ++i) db[p][i] = 0.f;
    }
    const int64_t r0 = (int64_t)blockIdx.x * a.run;
    const int64_t r1 = r0 + a.run < a.rows ? r0 + a.run : a.rows;
    // (the trip count is workgroup-uniform: every group takes part in the barriers of the row sums; a group past the run's last
    //  row works on that last row again and neither stores nor accumulates)
    for (int64_t rb = r0; rb < r1; rb += RW) {
        const bool live = rb + grp < r1;
        const int64_t row = live ? rb + grp : r1 - 1;
        float dy[NP][8], z[NP][8];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            row_load8<T>(a.dy, row * a.dy_rs + d[p], false, dy[p]);
            row_load8<T>(a.z, row * a.z_rs + d[p], a.z_fp32 != 0, z[p]);
            if (!on[p]) {
#pragma unroll
                for (int i = 0; i < 8; ++i) z[p][i] = 0.f;
            }
        }
        const float rstd = row_wide_stats<LN, NP>(z, on, red[0][grp], red[1][grp], nwaves, wave, a.n, a.eps);
        // z becomes xhat, dy stays (dweight / dbias), av = dy g
        float av[NP][8];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            float g[8];
            rms_gains<T>(a.w, d[p], a.w_fp32 != 0, a.w_offset, g);
#pragma unroll
            for (int i = 0; i < 8; ++i) { z[p][i] *= rstd; av[p][i] = dy[p][i] * g[i]; }
        }
        float c1 = 0.f;
        if constexpr (LN) {
            float s = on[0] ? row_piece_sum(av[0]) : 0.f;
#pragma unroll
            for (int p = 1; p < NP; ++p) s += on[p] ? row_piece_sum(av[p]) : 0.f;
            c1 = row_block_sum(s, red[2][grp], nwaves, wave) / (float)a.n;
        }
        float dot = on[0] ? rms_piece_dot(av[0], z[0]) : 0.f;
#pragma unroll
        for (int p = 1; p < NP; ++p) dot += on[p] ? rms_piece_dot(av[p], z[p]) : 0.f;
        const float c = row_block_sum(dot, red[3][grp], nwaves, wave) / (float)a.n;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if constexpr (DW != ANB_NONE) {
                if (on[p] && live) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        dw[p][i] = fmaf(dy[p][i], z[p][i], dw[p][i]);
                        if constexpr (DW == ANB_DW_DB) db[p][i] += dy[p][i];
                    }
                }
            }
            float dz[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) dz[i] = fmaf(-z[p][i], c, LN ? av[p][i] - c1 : av[p][i]);
            if (a.dro) {
                float dro[8];
                row_load8<T>(a.dro, row * a.dro_rs + d[p], a.z_fp32 != 0, dro);
#pragma unroll
                for (int i = 0; i < 8; ++i) dz[i] = fmaf(rstd, dz[i], dro[i]);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) dz[i] = rstd * dz[i];
            }
            if (on[p] && live) anb_store8<T>(a, row, d[p], dz);
        }
    }
    if constexpr (DW != ANB_NONE) {
        constexpr int SLOTS = DW == ANB_DW_DB ? 2 : 1;
        if constexpr (RW > 1) {
            __shared__ float comb[ROW_THREADS][9];        // (9: the lanes of a wave write their rows to different banks)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                anb_fold_groups<RW>(dw[p], comb, grp, t);
                if constexpr (DW == ANB_DW_DB) anb_fold_groups<RW>(db[p], comb, grp, t);
            }
        }
        // every column has one owner in group 0: the lane writes its sums into the workgroup's partial row
        float* prow = a.partial + (int64_t)blockIdx.x * SLOTS * a.n;
        if (grp == 0) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if (on[p]) {
                    row_store8<T>(prow, d[p], true, dw[p]);
                    if constexpr (DW == ANB_DW_DB) row_store8<T>(prow, a.n + d[p], true, db[p]);
                }
            }
        }
    }
}

// dweight / dbias from the partial rows: workgroup b owns ANB_FIN_COLS columns of the [slots][n] row, thread (seg, col) adds its
// run of partial rows in row order (the loads of ANB_FIN_BATCH rows are issued together, the additions keep the order), the runs
// are added in order, one rounding to the weight's type
template <typename T>
__global__ void __launch_bounds__(ROW_THREADS) add_norm_bwd_finish_kernel(const AnbFinArgs a) {
    using E = Elem<T>;
    __shared__ float red[ANB_FIN_SEGS][ANB_FIN_COLS];
    const int col = (int)threadIdx.x & (ANB_FIN_COLS - 1), seg = (int)threadIdx.x / ANB_FIN_COLS;
    const int w = (int)blockIdx.x * ANB_FIN_COLS + col;
    const bool ok = w < a.slots * a.n;
    const int per = (a.n_parts + ANB_FIN_SEGS - 1) / ANB_FIN_SEGS;
    const int p0 = seg * per < a.n_parts ? seg * per : a.n_parts, p1 = p0 + per < a.n_parts ? p0 + per : a.n_parts;
    const int64_t stride = (int64_t)a.slots * a.n;
    float s = 0.f;
    if (ok) {
        int p = p0;
        for (; p + ANB_FIN_BATCH <= p1; p += ANB_FIN_BATCH) {
            float v[ANB_FIN_BATCH];
#pragma unroll
            for (int i = 0; i < ANB_FIN_BATCH; ++i) v[i] = a.partial[(p + i) * stride + w];
#pragma unroll
            for (int i = 0; i < ANB_FIN_BATCH; ++i) s += v[i];
        }
        for (; p < p1; ++p) s += a.partial[p * stride + w];
    }
    red[seg][col] = s;
    __syncthreads();
    if (seg != 0 || !ok) return;
#pragma unroll
    for (int t = 1; t < ANB_FIN_SEGS; ++t) s += red[t][col];
    const int k = w >= a.n ? 1 : 0, c = w - k * a.n;
    void* dst = k ? a.db : a.dw;
    if (!dst) return;
    if (a.w_fp32) static_cast<float*>(dst)[c] = s;
    else          static_cast<uint16_t*>(dst)[c] = (uint16_t)(E::pack2(s, 0.f) & 0xffffu);
}

// The launch plan: a function of (rows, n, dweight / dbias wanted) alone (never of the device), shared by the workspace query and
// the launch.  The caller has validated the sizes.
struct AnbPlan {
    RowShape shape;
    int rows_in_flight;                                   // RW of the wide DW kernels, by what fits the register file without a spill:
                                                          // 1 piece a lane 4; 2 pieces 4 (with dbias 2); 4 pieces 2; 8 pieces 1
    int mode;                                             // ANB_NONE / ANB_DW / ANB_DW_DB
    int slots;                                            // fp32 rows per partial row: 1, or 2 with dbias
    int parts;                                            // P: workgroups of the DW kernels = partial rows
    int64_t run;                                          // rows (n > 256) or passes (n <= 256) per workgroup
    int64_t grid;
    size_t bytes;
};

static AnbPlan anb_plan(const fa_add_norm_bwd_params& s) {
    AnbPlan pl = {};
    pl.shape = row_shape(s.n);
    pl.mode = s.dbias ? ANB_DW_DB : (s.dweight ? ANB_DW : ANB_NONE);
    pl.slots = s.dbias ? 2 : 1;
    pl.rows_in_flight = 1;
    if (pl.mode != ANB_NONE && s.n > ROW_SMALL_MAX)
        pl.rows_in_flight = pl.shape.pieces == 1 ? 4 : (pl.shape.pieces == 2 ? (pl.mode == ANB_DW_DB ? 2 : 4) : (pl.shape.pieces == 4 ? 2 : 1));
    if (s.rows <= 0) return pl;
    const bool small = s.n <= ROW_SMALL_MAX;
    const int64_t units = small ? (s.rows + (ROW_THREADS >> pl.shape.group_log2) - 1) / (ROW_THREADS >> pl.shape.group_log2) : s.rows;
    if (pl.mode == ANB_NONE) {
        pl.run = 1;
        pl.grid = units;
        return pl;
    }
    pl.run = (units + ANB_MAX_PARTS - 1) / ANB_MAX_PARTS;
    pl.parts = (int)((units + pl.run - 1) / pl.run);
    pl.grid = pl.parts;
    pl.bytes = (size_t)pl.parts * pl.slots * (size_t)s.n * sizeof(float);
    return pl;
}

size_t add_norm_bwd_workspace_bytes(const fa_add_norm_bwd_params& s) { return anb_plan(s).bytes; }

template <typename T, bool LN, int DW>
static void launch_anb_np(const AnbArgs& a, const AnbPlan& pl, hipStream_t stream) {
    const dim3 g((unsigned)pl.grid);
    if (a.n <= ROW_SMALL_MAX) {
        hipLaunchKernelGGL((add_norm_bwd_small_kernel<T, LN, DW>), g, dim3(ROW_THREADS), 0, stream, a);
        return;
    }
    constexpr int RW1 = DW == ANB_NONE ? 1 : 4, RW2 = DW == ANB_NONE ? 1 : (DW == ANB_DW_DB ? 2 : 4), RW4 = DW == ANB_NONE ? 1 : 2;   // anb_plan's rows_in_flight
    const dim3 b(pl.shape.threads * pl.rows_in_flight);
    switch (pl.shape.pieces) {
    case 1:  hipLaunchKernelGGL((add_norm_bwd_wide_kernel<T, LN, 1, DW, RW1>), g, b, 0, stream, a); break;
    case 2:  hipLaunchKernelGGL((add_norm_bwd_wide_kernel<T, LN, 2, DW, RW2>), g, b, 0, stream, a); break;
    case 4:  hipLaunchKernelGGL((add_norm_bwd_wide_kernel<T, LN, 4, DW, RW4>), g, b, 0, stream, a); break;
    default: hipLaunchKernelGGL((add_norm_bwd_wide_kernel<T, LN, 8, DW, 1>), g, b, 0, stream, a); break;
    }
}

template <typename T, bool LN>
static void launch_anb(const AnbArgs& a, const AnbPlan& pl, hipStream_t stream) {
    if (pl.mode == ANB_NONE)    launch_anb_np<T, LN, ANB_NONE>(a, pl, stream);
    else if (pl.mode == ANB_DW) launch_anb_np<T, LN, ANB_DW>(a, pl, stream);
    else                        launch_anb_np<T, LN, ANB_DW_DB>(a, pl, stream);
}

// one launch, two with a wanted dweight / dbias; rows == 0: none, and a wanted dweight / dbias is set to zero.  The caller
// (fa_api.hip) has validated the block: the workspace holds add_norm_bwd_workspace_bytes()
void launch_add_norm_bwd(const fa_add_norm_bwd_params& s, hipStream_t stream) {
    const AnbPlan pl = anb_plan(s);
    if (pl.grid == 0) {
        const size_t wbytes = (size_t)s.n * (s.weight_dtype == FA_FP32 ? 4 : 2);
        if (s.dweight) (void)hipMemsetAsync(s.dweight, 0, wbytes, stream);
        if (s.dbias) (void)hipMemsetAsync(s.dbias, 0, wbytes, stream);
        return;
    }
    AnbArgs a;
    a.dy = static_cast<const uint16_t*>(s.dy);
    a.z = s.z;
    a.dro = s.dres_out;
    a.dx = static_cast<uint16_t*>(s.dx);
    a.dres = s.dres;
    a.w = s.weight;
    a.partial = static_cast<float*>(s.workspace);
    a.dy_rs = s.dy_row_stride; a.z_rs = s.z_row_stride; a.dro_rs = s.dres_out_row_stride;
    a.dx_rs = s.dx_row_stride; a.dres_rs = s.dres_row_stride;
    a.rows = s.rows; a.run = pl.run;
    a.n = s.n; a.group_log2 = pl.shape.group_log2;
    a.z_fp32 = s.z_dtype == FA_FP32;
    a.dres_fp32 = s.dres_dtype == FA_FP32;
    a.w_fp32 = s.weight_dtype == FA_FP32;
    a.eps = s.eps; a.w_offset = s.weight_offset;
    const bool ln = !s.is_rms_norm;
    if (s.dtype == FA_BF16) {
        if (ln) launch_anb<bf16_tag, true>(a, pl, stream);
        else    launch_anb<bf16_tag, false>(a, pl, stream);
    } else {
        if (ln) launch_anb<fp16_tag, true>(a, pl, stream);
        else    launch_anb<fp16_tag, false>(a, pl, stream);
    }
    if (pl.mode == ANB_NONE) return;
    AnbFinArgs f;
    f.partial = a.partial;
    f.dw = s.dweight; f.db = s.dbias;
    f.n_parts = pl.parts; f.n = s.n; f.slots = pl.slots; f.w_fp32 = a.w_fp32;
    const dim3 g((pl.slots * s.n + ANB_FIN_COLS - 1) / ANB_FIN_COLS), b(ROW_THREADS);
    if (s.dtype == FA_BF16) hipLaunchKernelGGL((add_norm_bwd_finish_kernel<bf16_tag>), g, b, 0, stream, f);
    else                    hipLaunchKernelGGL((add_norm_bwd_finish_kernel<fp16_tag>), g, b, 0, stream, f);
}

}  // namespace fa
