// fa_rowops.h - what the row ops around attention share (fa_rotary.hip, fa_kv_store.hip, fa_kv_gather.hip, fa_rope_store.hip,
// fa_qk_norm_rope_store.hip, fa_qk_norm_rope_bwd.hip): the streaming load, the names of the rotation kinds and of the q / k / v
// items, the host's group_rows / grid plan and the argument fill of the two rope-store kernels.  Definitions only: each kernel
// keeps its own tuning constants and its own body.
#pragma once
#include <cstdint>
#include "fa_rope.h"

namespace fa {

// q / k / v and the gradients are read once: a nontemporal 16-byte load
__device__ __forceinline__ u32x4 ld_nt16(const uint16_t* p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }

enum { ROPE_NONE = 0, ROPE_INTERLEAVED = 1, ROPE_NEOX = 2 };          // NONE: no table (or an empty one), no row is rotated
enum { ROW_Q = 0, ROW_K = 1, ROW_V = 2 };                             // what an item or a head slot of a row belongs to

template <int ROPE> struct RopeTable { typedef u32x2 type; };         // the cos / sin values of one piece: 4 pairs (interleaved)
template <> struct RopeTable<ROPE_NEOX> { typedef u32x4 type; };      // 8 pairs

// A workgroup step owns group_rows consecutive rows - as many as bring it to about `step_target` units of work (items or lanes;
// a row has `per_row` > 0 of them), at least 1 and at most `max_group_rows` - and the grid is capped at `grid_cap` steps (the
// kernels stride over the rest).
struct RowPlan { int group_rows, grid; };
inline RowPlan row_plan(int64_t n_rows, int64_t per_row, int step_target, int max_group_rows, int grid_cap) {
    const int64_t rows = (step_target + per_row - 1) / per_row;
    RowPlan pl;
    pl.group_rows = (int)(rows < 1 ? 1 : (rows > max_group_rows ? max_group_rows : rows));
    const int64_t groups = (n_rows + pl.group_rows - 1) / pl.group_rows;
    pl.grid = (int)(groups < grid_cap ? groups : grid_cap);
    return pl;
}

// The fields that RopeStoreArgs (fa_rope_store.hip) and QkNormArgs (fa_qk_norm_rope_store.hip) have in common, from the fields
// that fa_rope_store_params and fa_qk_norm_rope_store_params have in common (the caller has validated the block)
template <typename Args, typename Params>
inline void fill_rope_store_args(Args& a, const Params& s) {
    a.q = static_cast<const uint16_t*>(s.q);
    a.k = static_cast<const uint16_t*>(s.k);
    a.v = static_cast<const uint16_t*>(s.v);
    a.qo = static_cast<uint16_t*>(s.q_out);
    a.ko = static_cast<uint16_t*>(s.k_out);
    a.q_row_stride = s.q_row_stride; a.q_head_stride = s.q_head_stride;
    a.k_row_stride = s.k_row_stride; a.k_head_stride = s.k_head_stride;
    a.v_row_stride = s.v_row_stride; a.v_head_stride = s.v_head_stride;
    a.qo_row_stride = s.qo_row_stride; a.qo_head_stride = s.qo_head_stride;
    a.ko_row_stride = s.ko_row_stride; a.ko_head_stride = s.ko_head_stride;
    a.kc = s.k_cache; a.vc = s.v_cache;
    a.kc_batch_stride = s.kc_batch_stride; a.kc_row_stride = s.kc_row_stride; a.kc_head_stride = s.kc_head_stride;
    a.vc_batch_stride = s.vc_batch_stride; a.vc_row_stride = s.vc_row_stride; a.vc_head_stride = s.vc_head_stride;
    a.positions = s.positions;
    a.slot_mapping = s.k_cache ? s.slot_mapping : nullptr;
    a.n_rows = s.total_rows;
    a.n_slots = s.k_cache ? (int64_t)s.num_blocks * s.page_block_size : 0;
    a.cos = static_cast<const uint16_t*>(s.rotary_cos);
    a.sin = static_cast<const uint16_t*>(s.rotary_sin);
    a.nheads_q = s.q ? s.nheads_q : 0; a.nheads_k = s.nheads_k; a.head_dim = s.head_dim;
    a.page = s.k_cache ? s.page_block_size : 1;
    a.rotary_dim = s.rotary_dim; a.seqlen_ro = s.seqlen_ro;
    a.q_inplace = s.q_out == s.q; a.k_inplace = s.k_out == s.k;
    a.k_descale = s.k_descale; a.v_descale = s.v_descale;
}

}  // namespace fa
