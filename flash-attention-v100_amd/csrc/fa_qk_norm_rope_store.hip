// fa_qk_norm_rope_store.hip - fa_rope_store with a per-head RMSNorm of q and k in front of the rotation, one launch
// (fa_qk_norm_rope_store, include/fa_mi355.h): the prologue of a serving step for models with QK-norm.  The statistics are
// fa_rmsnorm.h's, the rotation fa_rope.h's rope_chunk on the normalised values ROUNDED to the io type, the slot addressing and
// the fp8 rounding fa_rope_store.hip's (fa_fp8_cvt.h's to_fp8x8): the call leaves the bits of "norm only, then fa_rope_store".
// Byte movement plus one row sum per head: no LDS, no atomics, no workspace.
//   - a lane owns one 16-byte piece: 8 consecutive columns of one head.  A head is owned by a GROUP of G adjacent lanes of one
//     wave, G = the smallest power of two >= head_dim / 8 (1 .. 32); the lanes of a group past the head hand +0 to the sum and
//     store nothing.  fa_rope_store's flat item list does not carry over: the row sum needs a head's lanes side by side;
//   - a lane's columns are the same for every head it meets, so it reads its 8 q gains and 8 k gains (weight_offset + w) once,
//     before the row loop;
//   - a row has nheads_q + nheads_k head slots, and nheads_k more for v with caches (plain copies into the cache by lanes of the
//     same launch).  A workgroup step owns a run of consecutive rows (QkNormArgs::group_rows, chosen by the host so that a step
//     has about QN_STEP_LANES lanes of work: a decode batch does not run one nearly empty wave per row); the grid is capped at
//     QN_GRID_CAP steps and strides over the rest;
//   - the row sum and the GPT-NeoX partner piece travel between lanes (rotary_dim % 16 == 0: the partner is rotary_dim / 16 lanes
//     away inside the group, and what is fetched is its normalised, rounded piece).  Every cross-lane read sits outside every
//     lane-dependent branch, and the trip counts are workgroup-uniform;
//   - a lane issues all loads of its QN_U items - x, position, slot, cos / sin - unconditionally and from clamped valid addresses,
//     then computes, then stores.  It only ever loads its own columns, so in place nothing is read after it was written;
//   - q / k / v are read once: nontemporal loads.  q_out / k_out and the cache lines are read by the attention call that follows:
//     ordinary stores (the choices profiles/rope_store.txt measured).  Vector stores only; fp8 caches get 8-byte stores.
#include <cstdint>
#include "fa_rowops.h"
#include "fa_rmsnorm.h"
#include "fa_fp8_cvt.h"

namespace fa {

constexpr int QN_THREADS = 256;
constexpr int QN_U = 2;                                   // items in flight per lane: loads first, then stores
constexpr int QN_STEP_LANES = 2048;                       // lanes of work a workgroup step aims for
constexpr int QN_MAX_GROUP_ROWS = 64;
constexpr int QN_GRID_CAP = 256 * 16;                     // as fa_rope_store.hip: 16 workgroups per CU in flight, then grid-stride

struct QkNormArgs {
    const uint16_t* q;                                    // nheads_q == 0 where there is no q
    const uint16_t* k;
    const uint16_t* v;                                    // read with caches only
    uint16_t* qo;
    uint16_t* ko;                                         // nullptr: K is not written back
    int64_t q_row_stride, q_head_stride, k_row_stride, k_head_stride, v_row_stride, v_head_stride;   // elements
    int64_t qo_row_stride, qo_head_stride, ko_row_stride, ko_head_stride;
    void* kc;                                             // nullptr (both): no cache
    void* vc;
    int64_t kc_batch_stride, kc_row_stride, kc_head_stride;                       // elements of the cache type
    int64_t vc_batch_stride, vc_row_stride, vc_head_stride;
    const int64_t* positions;                             // read where there is a rotation
    const int64_t* slot_mapping;
    int64_t n_rows, n_slots;                              // rows of q / k / v; num_blocks x page_block_size
    const uint16_t* cos;
    const uint16_t* sin;
    const void* wq;                                       // nullptr: q is not normalised
    const void* wk;
    int nheads_q, nheads_k, head_dim, page, rotary_dim, seqlen_ro, group_rows;
    int group_log2;                                       // G = 1 << group_log2 lanes per head
    int q_inplace, k_inplace, w_fp32;
    float k_descale, v_descale, eps, w_offset;
};

// where slot `s` lies in a cache with the given strides (the caller knows 0 <= s < n_slots)
__device__ __forceinline__ int64_t qn_cache_row(int64_t s, int64_t n_slots, int page, int64_t batch_stride, int64_t row_stride) {
    int64_t blk, row;
    if (n_slots <= 0x7fffffffll) {                        // (uniform: the 32-bit division is a fraction of the 64-bit one)
        const uint32_t b = (uint32_t)s / (uint32_t)page;
        blk = b; row = (uint32_t)s - b * (uint32_t)page;
    } else {
        blk = s / page; row = s - blk * page;
    }
    return blk * batch_stride + row * row_stride;
}

// T: the 16-bit io type; KV8: fp8-e4m3 cache; ROPE: the pair rule
template <typename T, bool KV8, int ROPE>
__global__ void __launch_bounds__(QN_THREADS) qk_norm_rope_store_kernel(const QkNormArgs a) {
    typedef typename RopeTable<ROPE>::type CS;
    constexpr bool NEOX = ROPE == ROPE_NEOX;
    const int lanes = 1 << a.group_log2;                  // G
    const int lane = threadIdx.x & 63;
    const int j = (int)threadIdx.x & (lanes - 1);         // the lane's piece of its head ...
    const bool piece = 8 * j < a.head_dim;                // ... if the head has one there
    const int d = piece ? 8 * j : 0;                      // its first column (clamped: the loads stay inside the head)
    const int slot0 = (int)threadIdx.x >> a.group_log2;   // the lane's head slot within a pass
    const int spp = QN_THREADS >> a.group_log2;           // head slots per pass of the workgroup
    const int rd = ROPE == ROPE_NONE ? 0 : a.rotary_dim;
    const int half = rd >> 1;
    const bool inside = piece && d < rd;                  // the piece is rotated (where its row is)
    const bool first = d < half;                          // NeoX: a piece of the first half
    const int partner = NEOX && inside ? (first ? lane + (half >> 3) : lane - (half >> 3)) : lane;   // inside the group
    const int tcol = !inside ? 0 : (NEOX ? (first ? d : d - half) : d >> 1);                         // its place in a table row
    const bool cached = a.kc != nullptr;
    const int nq = a.nheads_q, nqk = nq + a.nheads_k;
    const int hpr = nqk + (cached ? a.nheads_k : 0);      // head slots per row (the host launches nothing where this is 0)
    const bool norm_q = a.wq != nullptr, norm_k = a.wk != nullptr;
    float gq[8], gk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) gq[i] = gk[i] = 1.f;
    if (norm_q) rms_gains<T>(a.wq, d, a.w_fp32 != 0, a.w_offset, gq);
    if (norm_k) rms_gains<T>(a.wk, d, a.w_fp32 != 0, a.w_offset, gk);
    float kinv = 1.f, vinv = 1.f;
    if (KV8) {
        kinv = fp8_inv_descale(a.k_descale);
        vinv = fp8_inv_descale(a.v_descale);
    }
    for (int64_t r0 = (int64_t)blockIdx.x * a.group_rows; r0 < a.n_rows; r0 += (int64_t)gridDim.x * a.group_rows) {
        const int64_t left = a.n_rows - r0;
        const int n = (int)(left < a.group_rows ? left : a.group_rows) * hpr;     // head slots of the step
        // (the trip count is workgroup-uniform: every lane of every wave takes part in the cross-lane reads below)
        for (int base = 0; base < n; base += spp * QN_U) {
            u32x4 x[QN_U];
            CS cw[QN_U], sw[QN_U];
            uint16_t* op[QN_U];                           // the piece in q_out / k_out
            int64_t co[QN_U];                             // the piece in k_cache / v_cache, < 0: not cached
            int kind[QN_U];
            bool act[QN_U], rot[QN_U];
#pragma unroll
            for (int u = 0; u < QN_U; ++u) {
                const int s = base + u * spp + slot0;
                const bool in = s < n;
                const uint32_t sc = in ? (uint32_t)s : 0u;                        // (a slot past the step's last: its first one)
                const uint32_t kr = sc / (uint32_t)hpr, c = sc - kr * (uint32_t)hpr;
                kind[u] = (int)c < nq ? ROW_Q : ((int)c < nqk ? ROW_K : ROW_V);
                const int64_t h = (int64_t)c - (kind[u] == ROW_Q ? 0 : (kind[u] == ROW_K ? nq : nqk));
                const int64_t r = r0 + kr;
                act[u] = in && piece;
                const uint16_t* src = kind[u] == ROW_Q ? a.q + r * a.q_row_stride + h * a.q_head_stride
                                    : kind[u] == ROW_K ? a.k + r * a.k_row_stride + h * a.k_head_stride
                                                       : a.v + r * a.v_row_stride + h * a.v_head_stride;
                x[u] = ld_nt16(src + d);
                op[u] = (kind[u] == ROW_Q ? a.qo + r * a.qo_row_stride + h * a.qo_head_stride
                                          : a.ko + r * a.ko_row_stride + h * a.ko_head_stride) + d;
                co[u] = -1;
                if (cached) {
                    const int64_t slot = a.slot_mapping[r];
                    if (kind[u] != ROW_Q && slot >= 0 && slot < a.n_slots) {
                        const bool isv = kind[u] == ROW_V;
                        co[u] = qn_cache_row(slot, a.n_slots, a.page, isv ? a.vc_batch_stride : a.kc_batch_stride,
                                             isv ? a.vc_row_stride : a.kc_row_stride) +
                                h * (isv ? a.vc_head_stride : a.kc_head_stride) + d;
                    }
                }
                rot[u] = false;
                if constexpr (ROPE != ROPE_NONE) {
                    const int64_t p = a.positions[r];
                    const bool at = p >= 0 && p < a.seqlen_ro;
                    rot[u] = act[u] && inside && at && kind[u] != ROW_V;
                    const int64_t trow = (at ? p : 0) * half;                     // (a row that is not rotated: the table's row 0)
                    cw[u] = *reinterpret_cast<const CS*>(a.cos + trow + tcol);
                    sw[u] = *reinterpret_cast<const CS*>(a.sin + trow + tcol);
                }
            }
#pragma unroll
            for (int u = 0; u < QN_U; ++u) {
                const bool norm = kind[u] == ROW_Q ? norm_q : (kind[u] == ROW_K && norm_k);
                const u32x4 zero = {0, 0, 0, 0};
                const float ss = rms_group_sum(rms_piece_ss<T>(act[u] ? x[u] : zero), lanes);
                const float rstd = rms_rstd(ss, a.head_dim, a.eps);
                float g[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) g[i] = kind[u] == ROW_Q ? gq[i] : gk[i];
                u32x4 y = norm ? rms_scale<T>(x[u], rstd, g) : x[u];
                if constexpr (ROPE != ROPE_NONE) {
                    u32x4 yp = y;                         // the partner's normalised, rounded piece (NeoX)
                    if constexpr (NEOX) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) yp[i] = (uint32_t)__shfl((int)y[i], partner);
                    }
                    // rope_chunk reads its cos / sin through pointers: hand it the piece's values (registers after inlining;
                    // d_base 0 / half = "a piece of the first / second half", table index 0), as fa_rope_store.hip does.  Both
                    // halves' formulas are evaluated with a constant d_base and one is kept: a lane-dependent d_base would make
                    // the table index dynamic, and hipcc would move the two table pieces into LDS
                    const CS cl = cw[u], sl = sw[u];
                    const uint16_t* cosp = reinterpret_cast<const uint16_t*>(&cl);
                    const uint16_t* sinp = reinterpret_cast<const uint16_t*>(&sl);
                    u32x4 z = y;
                    rope_chunk<T>(z, yp, cosp, sinp, 0, rd, !NEOX);
                    if constexpr (NEOX) {
                        u32x4 zb = y;
                        rope_chunk<T>(zb, yp, cosp, sinp, half, rd, false);
                        z = first ? z : zb;
                    }
                    y = rot[u] ? z : y;
                }
                if (act[u] && kind[u] != ROW_V) {
                    const bool inplace = kind[u] == ROW_Q ? a.q_inplace != 0 : a.k_inplace != 0;
                    const bool wanted = kind[u] == ROW_Q || a.ko != nullptr;
                    if (wanted && (!inplace || norm || rot[u])) *reinterpret_cast<u32x4*>(op[u]) = y;
                }
                if (act[u] && co[u] >= 0) {
                    if (KV8) {
                        uint8_t* p = static_cast<uint8_t*>(kind[u] == ROW_V ? a.vc : a.kc) + co[u];
                        *reinterpret_cast<u32x2*>(p) = to_fp8x8<T>(y, kind[u] == ROW_V ? vinv : kinv);
                    } else {
                        *reinterpret_cast<u32x4*>(static_cast<uint16_t*>(kind[u] == ROW_V ? a.vc : a.kc) + co[u]) = y;
                    }
                }
            }
        }
    }
}

template <typename T, bool KV8>
static void launch_qk_norm_w(const QkNormArgs& a, int rope, int grid, hipStream_t stream) {
    const dim3 g(grid), b(QN_THREADS);
    if (rope == ROPE_NONE)             hipLaunchKernelGGL((qk_norm_rope_store_kernel<T, KV8, ROPE_NONE>), g, b, 0, stream, a);
    else if (rope == ROPE_INTERLEAVED) hipLaunchKernelGGL((qk_norm_rope_store_kernel<T, KV8, ROPE_INTERLEAVED>), g, b, 0, stream, a);
    else                                  hipLaunchKernelGGL((qk_norm_rope_store_kernel<T, KV8, ROPE_NEOX>), g, b, 0, stream, a);
}

// one launch (none where a row has no head); the caller (fa_api.hip) has validated the block, replaced descales of 0 by 1.0, set
// nheads_q to 0 where q is NULL and knows that total_rows and head_dim are positive
void launch_qk_norm_rope_store(const fa_qk_norm_rope_store_params& s, hipStream_t stream) {
    QkNormArgs a;
    fill_rope_store_args(a, s);
    a.wq = s.q ? s.q_weight : nullptr;
    a.wk = s.k_weight;
    a.w_fp32 = s.weight_dtype == FA_FP32;
    a.eps = s.eps; a.w_offset = s.weight_offset;
    const bool cached = s.k_cache != nullptr;
    const bool kv8 = cached && s.cache_dtype == FA_FP8_E4M3;
    const int rope = s.seqlen_ro <= 0 ? ROPE_NONE : (s.rotary_interleaved ? ROPE_INTERLEAVED : ROPE_NEOX);
    a.group_log2 = 0;
    while ((8 << a.group_log2) < s.head_dim) ++a.group_log2;
    const int64_t hpr = a.nheads_q + a.nheads_k * (cached ? 2 : 1);
    if (hpr == 0) return;
    const RowPlan pl = row_plan(a.n_rows, hpr << a.group_log2, QN_STEP_LANES, QN_MAX_GROUP_ROWS, QN_GRID_CAP);
    a.group_rows = pl.group_rows;
    if (s.dtype == FA_BF16) {
        if (kv8) launch_qk_norm_w<bf16_tag, true>(a, rope, pl.grid, stream);
        else     launch_qk_norm_w<bf16_tag, false>(a, rope, pl.grid, stream);
    } else {
        if (kv8) launch_qk_norm_w<fp16_tag, true>(a, rope, pl.grid, stream);
        else     launch_qk_norm_w<fp16_tag, false>(a, rope, pl.grid, stream);
    }
}

}  // namespace fa
