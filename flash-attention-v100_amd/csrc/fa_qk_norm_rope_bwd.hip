// fa_qk_norm_rope_bwd.hip - the backward of fa_qk_norm_rope_store's norm + rotation (fa_qk_norm_rope_bwd, include/fa_mi355.h): from
// dz (the gradient of q_out / k_out) and the saved pre-norm x to dx and, per weight, dw[d] = sum over rows and heads of dy xhat.
// Both 16-bit roundings of the forward are treated as the identity (straight-through); rstd is RECOMPUTED from x with fa_rmsnorm.h's
// fixed-order sum, so it has the forward's bits and the forward saves nothing.
//     dy   = conj_rope(dz)                    fp32, NOT rounded: fa_rope.h's rope_y0 / rope_y1 with the sign of sin flipped exactly
//     no weight:  dx = round16(dy)            (fa_rotary's bits with `conjugate`)
//     weight:     xhat = x rstd,  a = dy g,  c = (sum_d a xhat) / head_dim,  dx = round16(rstd fmaf(-xhat, c, a)),  dw += dy xhat
// The ownership is the forward's (fa_qk_norm_rope_store.hip): a lane owns one 16-byte piece (8 columns) of one head, a head is
// owned by G adjacent lanes of one wave, the NeoX partner piece of dz comes from the partner lane's registers, every cross-lane read
// sits outside every lane-dependent branch with workgroup-uniform trip counts, and a lane issues all loads of its QNB_U items
// before its first store: dq == dq_out and dk == dk_out are legal.  x and dz are read once (nontemporal loads); dx gets ordinary
// vector stores.
// The sum for c has ss's fixed order: the products in column order with fmaf inside the lane (rms_piece_dot), then the xor
// butterfly over the group - a head's dx bits do not depend on what else is in the batch.
// dw, deterministic, no atomics:
//   - a lane's columns are the same for every head it meets: it keeps its partial dw (8 fp32 for q, 8 for k) in registers over the
//     whole grid-stride loop and adds rows with fmaf in the order it meets them;
//   - at the end the workgroup adds the QNB_THREADS / G lanes that own the same piece through LDS, in the order of their thread
//     index, and writes ONE fp32 partial row [2][head_dim] into the workspace (zeros for a tensor without a wanted dw);
//   - a second kernel on the same stream adds the partial rows - QNB_FIN_SEGS contiguous runs of them in row order, then the runs in
//     order - and writes dq_weight / dk_weight with one rounding.
// The grid, the rows per step and the cap depend on the parameter block alone (qnb_plan: the workspace query and the launch share
// it), so the bits are the same on every card.  Without a wanted dw: no accumulation, no LDS, no second launch, no workspace.
#include <cstdint>
#include "fa_rowops.h"
#include "fa_rmsnorm.h"

namespace fa {

constexpr int QNB_THREADS = 256;
constexpr int QNB_U = 2;                                  // items in flight per lane: loads first, then stores
constexpr int QNB_STEP_LANES = 2048;                      // lanes of work a workgroup step aims for
constexpr int QNB_MAX_GROUP_ROWS = 64;
constexpr int QNB_GRID_CAP = 256 * 4;                     // 4 workgroups per CU, then grid-stride: the partial slab is <= 2 MB
constexpr int QNB_FIN_COLS = 16;                          // the second kernel: columns per workgroup (64 bytes of a partial row) ...
constexpr int QNB_FIN_SEGS = QNB_THREADS / QNB_FIN_COLS;  // ... and runs of partial rows that are added side by side
constexpr int QNB_FIN_BATCH = 8;                          // partial rows whose loads are in flight together

struct QnbArgs {
    const uint16_t* dzq;                                  // the gradients of q_out / k_out
    const uint16_t* dzk;
    const uint16_t* xq;                                   // the saved inputs (read where the tensor has a weight)
    const uint16_t* xk;
    uint16_t* dxq;                                        // nullptr: not written
    uint16_t* dxk;
    int64_t dzq_row_stride, dzq_head_stride, dzk_row_stride, dzk_head_stride;     // elements
    int64_t xq_row_stride, xq_head_stride, xk_row_stride, xk_head_stride;
    int64_t dxq_row_stride, dxq_head_stride, dxk_row_stride, dxk_head_stride;
    const int64_t* positions;                             // read where there is a rotation
    int64_t n_rows;
    const uint16_t* cos;
    const uint16_t* sin;
    const void* wq;                                       // nullptr: q has no weight
    const void* wk;
    float* partial;                                       // [grid][2][head_dim] fp32 (DW kernels)
    int nheads_q, nheads_k, head_dim, rotary_dim, seqlen_ro, group_rows;
    int group_log2;                                       // G = 1 << group_log2 lanes per head
    int q_inplace, k_inplace, w_fp32, dw_q, dw_k;         // dw_q / dw_k: that tensor's dw is wanted
    float eps, w_offset;
};

struct QnbFinArgs {
    const float* partial;                                 // [n_parts][2][head_dim]
    void* dwq;                                            // [head_dim] of the weight's type, or nullptr
    void* dwk;
    int n_parts, head_dim, w_fp32;
};

// T: the 16-bit io type; ROPE: the pair rule; DW: a weight gradient is wanted
template <typename T, int ROPE, bool DW>
__global__ void __launch_bounds__(QNB_THREADS) qk_norm_rope_bwd_kernel(const QnbArgs a) {
    typedef typename RopeTable<ROPE>::type CS;
    using E = Elem<T>;
    constexpr bool NEOX = ROPE == ROPE_NEOX;
    const int lanes = 1 << a.group_log2;                  // G
    const int lane = threadIdx.x & 63;
    const int j = (int)threadIdx.x & (lanes - 1);         // the lane's piece of its head ...
    const bool piece = 8 * j < a.head_dim;                // ... if the head has one there
    const int d = piece ? 8 * j : 0;                      // its first column (clamped: the loads stay inside the head)
    const int slot0 = (int)threadIdx.x >> a.group_log2;   // the lane's head slot within a pass
    const int spp = QNB_THREADS >> a.group_log2;          // head slots per pass of the workgroup
    const int rd = ROPE == ROPE_NONE ? 0 : a.rotary_dim;
    const int half = rd >> 1;
    const bool inside = piece && d < rd;                  // the piece is rotated (where its row is)
    const bool first = d < half;                          // NeoX: a piece of the first half
    const int partner = NEOX && inside ? (first ? lane + (half >> 3) : lane - (half >> 3)) : lane;   // inside the group
    const int tcol = !inside ? 0 : (NEOX ? (first ? d : d - half) : d >> 1);                         // its place in a table row
    const int nq = a.nheads_q, hpr = nq + a.nheads_k;     // head slots per row (the host launches nothing where this is 0)
    const bool norm_q = a.wq != nullptr, norm_k = a.wk != nullptr;
    float gq[8], gk[8], dwq[8], dwk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { gq[i] = gk[i] = 1.f; dwq[i] = dwk[i] = 0.f; }
    if (norm_q) rms_gains<T>(a.wq, d, a.w_fp32 != 0, a.w_offset, gq);
    if (norm_k) rms_gains<T>(a.wk, d, a.w_fp32 != 0, a.w_offset, gk);
    for (int64_t r0 = (int64_t)blockIdx.x * a.group_rows; r0 < a.n_rows; r0 += (int64_t)gridDim.x * a.group_rows) {
        const int64_t left = a.n_rows - r0;
        const int n = (int)(left < a.group_rows ? left : a.group_rows) * hpr;     // head slots of the step
        // (the trip count is workgroup-uniform: every lane of every wave takes part in the cross-lane reads below)
        for (int base = 0; base < n; base += spp * QNB_U) {
            u32x4 x[QNB_U], dz[QNB_U];
            CS cw[QNB_U], sw[QNB_U];
            uint16_t* op[QNB_U];                          // the piece in dq / dk
            int kind[QNB_U];
            bool act[QNB_U], rot[QNB_U];
#pragma unroll
            for (int u = 0; u < QNB_U; ++u) {
                const int s = base + u * spp + slot0;
                const bool in = s < n;
                const uint32_t sc = in ? (uint32_t)s : 0u;                        // (a slot past the step's last: its first one)
                const uint32_t kr = sc / (uint32_t)hpr, c = sc - kr * (uint32_t)hpr;
                kind[u] = (int)c < nq ? ROW_Q : ROW_K;
                const bool isq = kind[u] == ROW_Q;
                const int64_t h = (int64_t)c - (isq ? 0 : nq);
                const int64_t r = r0 + kr;
                act[u] = in && piece;
                dz[u] = ld_nt16((isq ? a.dzq + r * a.dzq_row_stride + h * a.dzq_head_stride
                                    : a.dzk + r * a.dzk_row_stride + h * a.dzk_head_stride) + d);
                x[u] = u32x4{0, 0, 0, 0};
                if (isq ? norm_q : norm_k)
                    x[u] = ld_nt16((isq ? a.xq + r * a.xq_row_stride + h * a.xq_head_stride
                                       : a.xk + r * a.xk_row_stride + h * a.xk_head_stride) + d);
                op[u] = (isq ? a.dxq + r * a.dxq_row_stride + h * a.dxq_head_stride
                             : a.dxk + r * a.dxk_row_stride + h * a.dxk_head_stride) + d;
                rot[u] = false;
                if constexpr (ROPE != ROPE_NONE) {
                    const int64_t p = a.positions[r];
                    const bool at = p >= 0 && p < a.seqlen_ro;
                    rot[u] = act[u] && inside && at;
                    const int64_t trow = (at ? p : 0) * half;                     // (a row that is not rotated: the table's row 0)
                    cw[u] = *reinterpret_cast<const CS*>(a.cos + trow + tcol);
                    sw[u] = *reinterpret_cast<const CS*>(a.sin + trow + tcol);
                }
            }
#pragma unroll
            for (int u = 0; u < QNB_U; ++u) {
                const bool isq = kind[u] == ROW_Q;
                const bool norm = isq ? norm_q : norm_k;
                const u32x4 zero = {0, 0, 0, 0};
                const float ss = rms_group_sum(rms_piece_ss<T>(act[u] ? x[u] : zero), lanes);
                const float rstd = rms_rstd(ss, a.head_dim, a.eps);
                float dy[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) { dy[2 * i] = E::lo(dz[u][i]); dy[2 * i + 1] = E::hi(dz[u][i]); }
                if constexpr (ROPE != ROPE_NONE) {
                    // the conjugate rotation: sin -> -sin exactly, as fa_rotary.hip does, then fa_rope.h's pair rule in fp32.  Both
                    // halves' formulas are evaluated and one is kept (NeoX), so that the table values stay in registers
                    u32x4 dp = dz[u];                     // the partner's piece of dz (NeoX)
                    if constexpr (NEOX) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) dp[i] = (uint32_t)__shfl((int)dz[u][i], partner);
                    }
                    float ry[8];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if constexpr (NEOX) {
                            const float a0 = dy[2 * i], a1 = dy[2 * i + 1];
                            const float b0 = E::lo(dp[i]), b1 = E::hi(dp[i]);
                            const float c0 = E::lo(cw[u][i]), c1 = E::hi(cw[u][i]);
                            const float s0 = E::lo(sw[u][i] ^ 0x80008000u), s1 = E::hi(sw[u][i] ^ 0x80008000u);
                            ry[2 * i] = first ? rope_y0(a0, b0, c0, s0) : rope_y1(b0, a0, c0, s0);
                            ry[2 * i + 1] = first ? rope_y0(a1, b1, c1, s1) : rope_y1(b1, a1, c1, s1);
                        } else {
                            const float x0 = dy[2 * i], x1 = dy[2 * i + 1];
                            const uint32_t cword = cw[u][i >> 1], sword = sw[u][i >> 1] ^ 0x80008000u;
                            const float c = (i & 1) ? E::hi(cword) : E::lo(cword);
                            const float s = (i & 1) ? E::hi(sword) : E::lo(sword);
                            ry[2 * i] = rope_y0(x0, x1, c, s);
                            ry[2 * i + 1] = rope_y1(x0, x1, c, s);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) dy[i] = rot[u] ? ry[i] : dy[i];
                }
                float xh[8], av[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    xh[2 * i] = E::lo(x[u][i]) * rstd;
                    xh[2 * i + 1] = E::hi(x[u][i]) * rstd;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) av[i] = dy[i] * (isq ? gq[i] : gk[i]);
                // (lanes past the head, slots past the step and tensors without a weight hand in +0)
                const float dot = rms_group_sum(act[u] && norm ? rms_piece_dot(av, xh) : 0.f, lanes);
                const float c = dot / (float)a.head_dim;
                u32x4 out;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    out[i] = norm ? E::pack2(rstd * fmaf(-xh[2 * i], c, av[2 * i]), rstd * fmaf(-xh[2 * i + 1], c, av[2 * i + 1]))
                                  : E::pack2(dy[2 * i], dy[2 * i + 1]);
                }
                if constexpr (DW) {
                    if (act[u] && norm) {
                        if (isq) {
                            if (a.dw_q) {
#pragma unroll
                                for (int i = 0; i < 8; ++i) dwq[i] = fmaf(dy[i], xh[i], dwq[i]);
                            }
                        } else if (a.dw_k) {
#pragma unroll
                            for (int i = 0; i < 8; ++i) dwk[i] = fmaf(dy[i], xh[i], dwk[i]);
                        }
                    }
                }
                if (act[u]) {
                    const bool inplace = isq ? a.q_inplace != 0 : a.k_inplace != 0;
                    const bool wanted = isq ? a.dxq != nullptr : a.dxk != nullptr;
                    if (wanted && (!inplace || norm || rot[u])) *reinterpret_cast<u32x4*>(op[u]) = out;
                }
            }
        }
    }
    if constexpr (DW) {
        // the lanes that own the same piece, added in the order of their thread index; one partial row per workgroup
        __shared__ float red[QNB_THREADS][17];            // (17: the lanes of a wave write their rows to different banks)
#pragma unroll
        for (int i = 0; i < 8; ++i) { red[threadIdx.x][i] = dwq[i]; red[threadIdx.x][8 + i] = dwk[i]; }
        __syncthreads();
        float* row = a.partial + (int64_t)blockIdx.x * 2 * a.head_dim;
        for (int w = (int)threadIdx.x; w < 2 * a.head_dim; w += QNB_THREADS) {
            const int k = w >= a.head_dim ? 1 : 0, col = w - k * a.head_dim;
            const int pj = col >> 3, pi = (col & 7) + 8 * k;
            float s = red[pj][pi];
            for (int t = 1; t < spp; ++t) s += red[t * lanes + pj][pi];
            row[w] = s;
        }
    }
}

// dq_weight / dk_weight from the partial rows: workgroup b owns QNB_FIN_COLS columns of the [2][head_dim] row, thread (seg, col)
// adds its run of partial rows in row order (the loads of QNB_FIN_BATCH rows are issued together, the additions keep the order),
// the runs are added in order, one rounding to the weight's type
template <typename T>
__global__ void __launch_bounds__(QNB_THREADS) qk_norm_rope_bwd_finish_kernel(const QnbFinArgs a) {
    using E = Elem<T>;
    __shared__ float red[QNB_FIN_SEGS][QNB_FIN_COLS];
    const int col = (int)threadIdx.x & (QNB_FIN_COLS - 1), seg = (int)threadIdx.x / QNB_FIN_COLS;
    const int w = (int)blockIdx.x * QNB_FIN_COLS + col;
    const bool ok = w < 2 * a.head_dim;
    const int per = (a.n_parts + QNB_FIN_SEGS - 1) / QNB_FIN_SEGS;
    const int p0 = seg * per, p1 = p0 + per < a.n_parts ? p0 + per : a.n_parts;
    const int64_t stride = 2 * (int64_t)a.head_dim;
    float s = 0.f;
    if (ok) {
        int p = p0;
        for (; p + QNB_FIN_BATCH <= p1; p += QNB_FIN_BATCH) {
            float v[QNB_FIN_BATCH];
#pragma unroll
            for (int i = 0; i < QNB_FIN_BATCH; ++i) v[i] = a.partial[(p + i) * stride + w];
#pragma unroll
            for (int i = 0; i < QNB_FIN_BATCH; ++i) s += v[i];
        }
        for (; p < p1; ++p) s += a.partial[p * stride + w];
    }
    red[seg][col] = s;
    __syncthreads();
    if (seg != 0 || !ok) return;
#pragma unroll
    for (int t = 1; t < QNB_FIN_SEGS; ++t) s += red[t][col];
    const int k = w >= a.head_dim ? 1 : 0, c = w - k * a.head_dim;
    void* dst = k ? a.dwk : a.dwq;
    if (!dst) return;
    if (a.w_fp32) static_cast<float*>(dst)[c] = s;
    else          static_cast<uint16_t*>(dst)[c] = (uint16_t)(E::pack2(s, 0.f) & 0xffffu);
}

// The launch plan: a function of the parameter block alone (never of the device), shared by the workspace query and the launch.
// The caller has validated the sizes.
struct QnbPlan {
    int nheads_q, nheads_k;                               // heads that are worked on (0: that tensor is skipped)
    int group_log2, group_rows, grid;
    bool dw_q, dw_k;
    size_t bytes;                                         // the partial slab: grid x [2][head_dim] fp32, 0 without a wanted dw
};

static QnbPlan qnb_plan(const fa_qk_norm_rope_bwd_params& s) {
    QnbPlan pl = {};
    const bool has_q = s.q != nullptr;
    pl.dw_q = has_q && s.q_weight && s.dq_weight && s.nheads_q > 0;
    pl.dw_k = s.k_weight && s.dk_weight && s.nheads_k > 0;
    pl.nheads_q = has_q && (s.dq || pl.dw_q) ? s.nheads_q : 0;
    pl.nheads_k = (s.dk || pl.dw_k) ? s.nheads_k : 0;
    const int64_t hpr = (int64_t)pl.nheads_q + pl.nheads_k;
    if (hpr == 0 || s.total_rows <= 0 || s.head_dim <= 0) return pl;
    while ((8 << pl.group_log2) < s.head_dim) ++pl.group_log2;
    const RowPlan rp = row_plan(s.total_rows, hpr << pl.group_log2, QNB_STEP_LANES, QNB_MAX_GROUP_ROWS, QNB_GRID_CAP);
    pl.group_rows = rp.group_rows; pl.grid = rp.grid;
    // (a dw whose tensor is not worked on - a NULL q - still goes through the partial rows: they hold zeros for it)
    if (s.dq_weight || s.dk_weight) pl.bytes = (size_t)pl.grid * 2 * (size_t)s.head_dim * sizeof(float);
    return pl;
}

size_t qk_norm_rope_bwd_workspace_bytes(const fa_qk_norm_rope_bwd_params& s) { return qnb_plan(s).bytes; }

template <typename T, bool DW>
static void launch_qnb_w(const QnbArgs& a, int rope, int grid, hipStream_t stream) {
    const dim3 g(grid), b(QNB_THREADS);
    if (rope == ROPE_NONE)             hipLaunchKernelGGL((qk_norm_rope_bwd_kernel<T, ROPE_NONE, DW>), g, b, 0, stream, a);
    else if (rope == ROPE_INTERLEAVED) hipLaunchKernelGGL((qk_norm_rope_bwd_kernel<T, ROPE_INTERLEAVED, DW>), g, b, 0, stream, a);
    else                                   hipLaunchKernelGGL((qk_norm_rope_bwd_kernel<T, ROPE_NEOX, DW>), g, b, 0, stream, a);
}

// one launch, two with a wanted dw; where no head is worked on (no rows, no heads, no output that needs them) none, and a wanted
// dw is set to zero.  The caller (fa_api.hip) has validated the block: the workspace holds qk_norm_rope_bwd_workspace_bytes()
void launch_qk_norm_rope_bwd(const fa_qk_norm_rope_bwd_params& s, hipStream_t stream) {
    const QnbPlan pl = qnb_plan(s);
    if (pl.grid == 0) {
        const size_t wbytes = (size_t)(s.head_dim > 0 ? s.head_dim : 0) * (s.weight_dtype == FA_FP32 ? 4 : 2);
        if (s.dq_weight && wbytes) (void)hipMemsetAsync(s.dq_weight, 0, wbytes, stream);
        if (s.dk_weight && wbytes) (void)hipMemsetAsync(s.dk_weight, 0, wbytes, stream);
        return;
    }
    QnbArgs a;
    a.dzq = static_cast<const uint16_t*>(s.dq_out);
    a.dzk = static_cast<const uint16_t*>(s.dk_out);
    a.xq = static_cast<const uint16_t*>(s.q);
    a.xk = static_cast<const uint16_t*>(s.k);
    a.dxq = static_cast<uint16_t*>(s.dq);
    a.dxk = static_cast<uint16_t*>(s.dk);
    a.dzq_row_stride = s.dqo_row_stride; a.dzq_head_stride = s.dqo_head_stride;
    a.dzk_row_stride = s.dko_row_stride; a.dzk_head_stride = s.dko_head_stride;
    a.xq_row_stride = s.q_row_stride; a.xq_head_stride = s.q_head_stride;
    a.xk_row_stride = s.k_row_stride; a.xk_head_stride = s.k_head_stride;
    a.dxq_row_stride = s.dq_row_stride; a.dxq_head_stride = s.dq_head_stride;
    a.dxk_row_stride = s.dk_row_stride; a.dxk_head_stride = s.dk_head_stride;
    a.positions = s.positions;
    a.n_rows = s.total_rows;
    a.cos = static_cast<const uint16_t*>(s.rotary_cos);
    a.sin = static_cast<const uint16_t*>(s.rotary_sin);
    a.wq = s.q ? s.q_weight : nullptr;
    a.wk = s.k_weight;
    a.partial = static_cast<float*>(s.workspace);
    a.nheads_q = pl.nheads_q; a.nheads_k = pl.nheads_k; a.head_dim = s.head_dim;
    a.rotary_dim = s.rotary_dim; a.seqlen_ro = s.seqlen_ro;
    a.group_rows = pl.group_rows; a.group_log2 = pl.group_log2;
    a.q_inplace = s.dq == s.dq_out; a.k_inplace = s.dk == s.dk_out;
    a.w_fp32 = s.weight_dtype == FA_FP32;
    a.dw_q = pl.dw_q; a.dw_k = pl.dw_k;
    a.eps = s.eps; a.w_offset = s.weight_offset;
    const int rope = s.seqlen_ro <= 0 ? ROPE_NONE : (s.rotary_interleaved ? ROPE_INTERLEAVED : ROPE_NEOX);
    const bool dw = pl.bytes != 0;
    if (s.dtype == FA_BF16) {
        if (dw) launch_qnb_w<bf16_tag, true>(a, rope, pl.grid, stream);
        else    launch_qnb_w<bf16_tag, false>(a, rope, pl.grid, stream);
    } else {
        if (dw) launch_qnb_w<fp16_tag, true>(a, rope, pl.grid, stream);
        else    launch_qnb_w<fp16_tag, false>(a, rope, pl.grid, stream);
    }
    if (!dw) return;
    QnbFinArgs f;
    f.partial = a.partial;
    f.dwq = s.dq_weight; f.dwk = s.dk_weight;
    f.n_parts = pl.grid; f.head_dim = s.head_dim; f.w_fp32 = a.w_fp32;
    const dim3 g((2 * s.head_dim + QNB_FIN_COLS - 1) / QNB_FIN_COLS), b(QNB_THREADS);
    if (s.dtype == FA_BF16) hipLaunchKernelGGL((qk_norm_rope_bwd_finish_kernel<bf16_tag>), g, b, 0, stream, f);
    else                    hipLaunchKernelGGL((qk_norm_rope_bwd_finish_kernel<fp16_tag>), g, b, 0, stream, f);
}

}  // namespace fa
