// fa_moe.h - the host side that fa_moe.hip and the entry points (fa_api.hip) share: the limits of the fa_moe_* ops, the lane
// ownership of a router row and the launch plan of fa_moe_sort.  Everything here is a function of the shapes alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include "fa_mi355.h"
#include <hip/hip_runtime.h>

namespace fa {

constexpr int MOE_MAX_EXPERTS = 512;
constexpr int MOE_MAX_TOPK = 16;
constexpr int MOE_MAX_ALIGN = 256;
constexpr int MOE_MAX_N = 16384;
constexpr int MOE_SORT_MAX_CHUNKS = 1024;                 // waves that count and place: one per SIMD of the chip
constexpr int MOE_SORT_MIN_CHUNK = 256;                   // slots a wave takes at the least

// a router row of E columns lies 8 per lane in G = 1 << moe_group_log2(E) adjacent lanes (E <= 512: G <= 64)
static inline int moe_group_log2(int E) {
    int g = 0;
    while ((8 << g) < E) ++g;
    return g;
}

// fa_moe_sort: `chunks` waves, each counting and placing `chunk` consecutive slots; the workspace holds chunks x E counts
struct MoeSortPlan { int64_t chunk, chunks; size_t workspace_bytes; };
static inline MoeSortPlan moe_sort_plan(int64_t slots, int E) {
    MoeSortPlan pl;
    const int64_t per = (slots + MOE_SORT_MAX_CHUNKS - 1) / MOE_SORT_MAX_CHUNKS;
    pl.chunk = (per + 63) / 64 * 64;
    if (pl.chunk < MOE_SORT_MIN_CHUNK) pl.chunk = MOE_SORT_MIN_CHUNK;
    pl.chunks = (slots + pl.chunk - 1) / pl.chunk;
    if (pl.chunks < 1) pl.chunks = 1;                     // (no slots: one wave still writes the offsets and the padding)
    pl.workspace_bytes = (size_t)pl.chunks * (size_t)E * sizeof(int32_t);
    return pl;
}

void launch_moe_route(const fa_moe_route_params& s, hipStream_t stream);
void launch_moe_route_bwd(const fa_moe_route_bwd_params& s, hipStream_t stream);
void launch_moe_sort(const fa_moe_sort_params& s, hipStream_t stream);
void launch_moe_permute(const fa_moe_permute_params& s, hipStream_t stream);
void launch_moe_combine(const fa_moe_combine_params& s, hipStream_t stream);
void launch_moe_combine_bwd(const fa_moe_combine_bwd_params& s, hipStream_t stream);

}  // namespace fa
