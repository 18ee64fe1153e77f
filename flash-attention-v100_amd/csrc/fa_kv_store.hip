// fa_kv_store.hip - store a ragged packed batch of K / V rows into a KV cache (fa_kv_store, include/fa_mi355.h): the step between
// a ragged prefill and everything that reads a cache.  One launch writes K and V; paged or contiguous caches of the input's
// 16-bit type or fp8-e4m3; rows addressed by a slot mapping, or by (cu_seqlens, cache_seqlens, block_table / cache_batch_idx)
// with fa_fwd_kvcache's append rule; optional RoPE on K at the row's cache position.  The rotation is fa_rope.h's rope_chunk and
// the quantisation fa_fp8_cvt.h's to_fp8x8 - the append kernel's own (fa_kvcache.hip), so both write the same bits.
// Pure byte movement, HBM-bound like fa_rows.hip / fa_rotary.hip: no LDS, no atomics, no workspace, one launch.
//   - a workgroup step owns a GROUP of consecutive source rows (KvStoreArgs::group_rows <= KVS_MAX_GROUP_ROWS, chosen by the host
//     so that a step has about KVS_STEP_ITEMS items); the grid is capped at KVS_GRID_CAP groups and strides over the rest;
//   - lane l of every wave works out row l of the group once per step: where it goes in k_cache / v_cache (or that it is dropped)
//     and its rotary position (slot mode: one 8-byte load and one division; sequence mode: ONE wave-uniform binary search in
//     cu_seqlens for the group's first row, then the lanes walk on - empty sequences included - and a stored row reads its
//     block-table entry); the items fetch their row's triple with a cross-lane read;
//   - an ITEM is what one lane owns: W 16-byte pieces (8 W consecutive columns of one head) of K and the same of V.  W = 1 for
//     16-bit caches (16-byte stores); fp8 caches take W = 2 where head_dim % 16 == 0 and the cache is 16-byte aligned (16 source
//     elements, 16-byte stores) and W = 1 otherwise (8-byte stores).  A NeoX pair needs the partner piece of K as well: the lane
//     loads it too (the cache is never the source, so nothing is read after it was written);
//   - a lane loads everything of its items - K, V, partner, cos / sin - then computes, then stores.  The loads are unconditional
//     and branch-free (clamped to addresses inside k / v and the tables), so hipcc keeps all of them in flight; only the
//     rotation and the stores depend on what the row turned out to be;
//   - k / v are read once: nontemporal loads.  The cache lines are re-read by the attention call that follows: ordinary stores
//     (FA_KV_STORE_NT_STORES=1 builds the nontemporal-store variant; profiles/kv_store.txt has both).
#include <cstdint>
#include "fa_rowops.h"
#include "fa_fp8_cvt.h"

#ifndef FA_KV_STORE_NT_STORES
#define FA_KV_STORE_NT_STORES 0
#endif

namespace fa {

constexpr int KVS_THREADS = 256;
constexpr int KVS_MAX_GROUP_ROWS = 16;                    // rows per workgroup step at most (one lane each: <= 64)
constexpr int KVS_STEP_ITEMS = 2048;                      // items a workgroup step aims for
constexpr int KVS_GRID_CAP = 256 * 16;                    // as fa_rows.hip: 16 workgroups per CU in flight, then grid-stride

struct KvStoreArgs {
    const uint16_t* k;
    const uint16_t* v;
    int64_t k_row_stride, k_head_stride, v_row_stride, v_head_stride;             // elements
    void* kc;
    void* vc;
    int64_t kc_batch_stride, kc_row_stride, kc_head_stride;                       // elements of the cache type
    int64_t vc_batch_stride, vc_row_stride, vc_head_stride;
    const int64_t* slot_mapping;
    const int32_t* cu_seqlens;
    const int32_t* cache_seqlens;
    const int32_t* block_table;
    const int32_t* cache_batch_idx;
    int64_t block_table_batch_stride;
    int64_t n_rows, n_slots;                              // rows of k / v; num_blocks x page_block_size
    const uint16_t* cos;
    const uint16_t* sin;
    int batch, nheads, head_dim, page, capacity;          // capacity: positions a sequence can hold (sequence mode)
    int rotary_dim, seqlen_ro, group_rows;
    float k_descale, v_descale;
};

struct KvsRow {
    int64_t ko, vo;                                       // element offsets of the row in k_cache / v_cache, ko < 0: the row is dropped
    int pos;                                              // its position in the cos / sin tables, -1: store it unrotated
};

// row r0 + lane of the group (only lanes < group_rows are ever asked)
__device__ __forceinline__ KvsRow kvs_row(const KvStoreArgs& a, int64_t r0, int lane) {
    const int64_t r = r0 + lane;
    KvsRow w;
    w.ko = -1; w.vo = 0; w.pos = -1;
    if (a.slot_mapping) {
        if (r >= a.n_rows) return w;
        const int64_t slot = a.slot_mapping[r];
        if (slot < 0 || slot >= a.n_slots) return w;
        const int64_t blk = slot / a.page, row = slot - blk * a.page;
        w.ko = blk * a.kc_batch_stride + row * a.kc_row_stride;
        w.vo = blk * a.vc_batch_stride + row * a.vc_row_stride;
        return w;
    }
    int lo = 0, hi = a.batch;                             // wave-uniform: the first sequence that ends behind r0 (batch: none)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.cu_seqlens[mid + 1] <= r0) lo = mid + 1; else hi = mid;
    }
    int b = lo;
    while (b < a.batch && a.cu_seqlens[b + 1] <= r) ++b;  // the lane's own row: a few sequences further at most
    if (b >= a.batch || r >= a.n_rows) return w;          // behind cu_seqlens[batch]: no sequence
    const int64_t pos = (int64_t)(a.cache_seqlens ? a.cache_seqlens[b] : 0) + (r - a.cu_seqlens[b]);
    if (pos < 0 || pos >= a.capacity) return w;           // beyond the capacity: dropped, as in the append
    if (a.block_table) {
        const int64_t pg = pos / a.page, pr = pos - pg * a.page;
        const int64_t phys = a.block_table[(int64_t)b * a.block_table_batch_stride + pg];
        w.ko = phys * a.kc_batch_stride + pr * a.kc_row_stride;
        w.vo = phys * a.vc_batch_stride + pr * a.vc_row_stride;
    } else {
        const int64_t cb = a.cache_batch_idx ? a.cache_batch_idx[b] : b;
        w.ko = cb * a.kc_batch_stride + pos * a.kc_row_stride;
        w.vo = cb * a.vc_batch_stride + pos * a.vc_row_stride;
    }
    w.pos = pos < a.seqlen_ro ? (int)pos : -1;
    return w;
}

template <typename V>
__device__ __forceinline__ void kvs_st(V* p, V v) {
#if FA_KV_STORE_NT_STORES
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// T: the 16-bit input type; KV8: fp8-e4m3 cache; W: 16-byte source pieces per item; ROPE: rotation of K
template <typename T, bool KV8, int W, int ROPE>
__global__ void __launch_bounds__(KVS_THREADS) kv_store_kernel(const KvStoreArgs a) {
    typedef typename RopeTable<ROPE>::type CS;
    constexpr int U = 2;                                  // items in flight per lane: loads first, then stores
    const int lane = threadIdx.x & 63;
    const int half = a.rotary_dim >> 1;
    const int iph = a.head_dim / (8 * W);                 // items per head
    const int ipr = a.nheads * iph;                       // items per row
    float kinv = 1.f, vinv = 1.f;
    if (KV8) {
        kinv = fp8_inv_descale(a.k_descale);
        vinv = fp8_inv_descale(a.v_descale);
    }
    for (int64_t r0 = (int64_t)blockIdx.x * a.group_rows; r0 < a.n_rows; r0 += (int64_t)gridDim.x * a.group_rows) {
        const KvsRow mine = kvs_row(a, r0, lane);
        const int64_t left = a.n_rows - r0;
        const int n = (int)(left < a.group_rows ? left : a.group_rows) * ipr;
        // (the trip count is workgroup-uniform and the cross-lane reads sit outside every lane-dependent branch: the lanes that
        //  hold the rows are active whenever they are read)
        for (int base = 0; base < n; base += KVS_THREADS * U) {
            u32x4 kx[U][W], vx[U][W], kp[U][W];
            CS cw[U][W], sw[U][W];
            int64_t ko[U], vo[U];
            bool ok[U], rot[U][W], first[U][W];                   // first: the piece lies in the first half of a NeoX rotation
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int w = base + u * KVS_THREADS + (int)threadIdx.x;
                const bool in = w < n;
                const uint32_t wc = in ? (uint32_t)w : 0u;
                const uint32_t kr = wc / (uint32_t)ipr, c = wc - kr * (uint32_t)ipr;
                const uint32_t h = c / (uint32_t)iph, j = c - h * (uint32_t)iph;
                const int64_t rko = __shfl(mine.ko, (int)kr), rvo = __shfl(mine.vo, (int)kr);
                const int pos = __shfl(mine.pos, (int)kr);
                ok[u] = in && rko >= 0;
                const int d = (int)j * 8 * W;             // first column of the item
                const uint16_t* khead = a.k + (r0 + kr) * a.k_row_stride + (int64_t)h * a.k_head_stride;
                const uint16_t* vhead = a.v + (r0 + kr) * a.v_row_stride + (int64_t)h * a.v_head_stride;
                ko[u] = rko + (int64_t)h * a.kc_head_stride + d;
                vo[u] = rvo + (int64_t)h * a.vc_head_stride + d;
                const int64_t trow = (int64_t)(pos >= 0 ? pos : 0) * half;
                // every load is unconditional, from an address that is valid whatever the lane's item is (an item past the step's
                // last one reads the step's first piece, a dropped row its own source row, a piece that is not rotated the
                // partner and table entries of a piece that is): no branch sits between the loads, so all of them are in flight
                // before the first use.  What is stored, and whether, is decided afterwards.
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    const int dq = d + 8 * q;
                    const bool inside = ROPE != ROPE_NONE && dq < a.rotary_dim;
                    rot[u][q] = inside && ok[u] && pos >= 0;
                    first[u][q] = dq < half;
                    kx[u][q] = ld_nt16(khead + dq);
                    vx[u][q] = ld_nt16(vhead + dq);
                    if (ROPE != ROPE_NONE) {
                        const int ds = inside ? dq : 0;
                        int t = ds >> 1;                  // interleaved: pairs ds / 2 .. ds / 2 + 3
                        if (ROPE == ROPE_NEOX) {
                            const bool f = ds < half;
                            kp[u][q] = ld_nt16(khead + ds + (f ? half : -half));
                            t = f ? ds : ds - half;
                        }
                        cw[u][q] = *reinterpret_cast<const CS*>(a.cos + trow + t);
                        sw[u][q] = *reinterpret_cast<const CS*>(a.sin + trow + t);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                if (ROPE != ROPE_NONE) {
#pragma unroll
                    for (int q = 0; q < W; ++q) {
                        // rope_chunk reads its cos / sin through pointers: hand it the piece's values (registers after inlining:
                        // d_base is a literal 0 or `half`, "a piece of the first / second half", table index 0).  Every piece is
                        // rotated and the result kept where the piece is to be rotated: a branch around the arithmetic would let
                        // hipcc sink the partner and table loads into it, behind the first wait.
                        const CS cl = cw[u][q], sl = sw[u][q];
                        const uint16_t* cp = reinterpret_cast<const uint16_t*>(&cl);
                        const uint16_t* sp = reinterpret_cast<const uint16_t*>(&sl);
                        u32x4 y = kx[u][q];
                        if (ROPE == ROPE_INTERLEAVED) {
                            rope_chunk<T>(y, y, cp, sp, 0, a.rotary_dim, true);
                        } else {
                            u32x4 y2 = y;
                            rope_chunk<T>(y, kp[u][q], cp, sp, 0, a.rotary_dim, false);
                            rope_chunk<T>(y2, kp[u][q], cp, sp, half, a.rotary_dim, false);
                            if (!first[u][q]) y = y2;
                        }
                        if (rot[u][q]) kx[u][q] = y;
                    }
                }
                if (KV8) {
                    uint8_t* kd = static_cast<uint8_t*>(a.kc) + ko[u];
                    uint8_t* vd = static_cast<uint8_t*>(a.vc) + vo[u];
                    if (W == 2) {
                        const u32x2 k0 = to_fp8x8<T>(kx[u][0], kinv), k1 = to_fp8x8<T>(kx[u][W - 1], kinv);
                        const u32x2 v0 = to_fp8x8<T>(vx[u][0], vinv), v1 = to_fp8x8<T>(vx[u][W - 1], vinv);
                        kvs_st(reinterpret_cast<u32x4*>(kd), u32x4{k0[0], k0[1], k1[0], k1[1]});
                        kvs_st(reinterpret_cast<u32x4*>(vd), u32x4{v0[0], v0[1], v1[0], v1[1]});
                    } else {
                        kvs_st(reinterpret_cast<u32x2*>(kd), to_fp8x8<T>(kx[u][0], kinv));
                        kvs_st(reinterpret_cast<u32x2*>(vd), to_fp8x8<T>(vx[u][0], vinv));
                    }
                } else {
                    kvs_st(reinterpret_cast<u32x4*>(static_cast<uint16_t*>(a.kc) + ko[u]), kx[u][0]);
                    kvs_st(reinterpret_cast<u32x4*>(static_cast<uint16_t*>(a.vc) + vo[u]), vx[u][0]);
                }
            }
        }
    }
}

// fp8 caches: 16 source elements and one 16-byte store per lane where the cache allows it (the header's contract)
static bool kvs_wide_ok(const fa_kv_store_params& s) {
    if (s.cache_dtype != FA_FP8_E4M3 || s.head_dim % 16 != 0) return false;
    const uint64_t bits = (uint64_t)reinterpret_cast<uintptr_t>(s.k_cache) | (uint64_t)reinterpret_cast<uintptr_t>(s.v_cache) |
                          (uint64_t)s.kc_batch_stride | (uint64_t)s.kc_row_stride | (uint64_t)s.kc_head_stride |
                          (uint64_t)s.vc_batch_stride | (uint64_t)s.vc_row_stride | (uint64_t)s.vc_head_stride;
    return (bits & 15) == 0;
}

template <typename T, bool KV8, int W>
static void launch_kv_store_w(const KvStoreArgs& a, int rope, int grid, hipStream_t stream) {
    const dim3 g(grid), b(KVS_THREADS);
    if (rope == ROPE_NONE)             hipLaunchKernelGGL((kv_store_kernel<T, KV8, W, ROPE_NONE>), g, b, 0, stream, a);
    else if (rope == ROPE_INTERLEAVED) hipLaunchKernelGGL((kv_store_kernel<T, KV8, W, ROPE_INTERLEAVED>), g, b, 0, stream, a);
    else                                   hipLaunchKernelGGL((kv_store_kernel<T, KV8, W, ROPE_NEOX>), g, b, 0, stream, a);
}

template <typename T>
static void launch_kv_store_t(const KvStoreArgs& a, bool kv8, int w, int rope, int grid, hipStream_t stream) {
    if (!kv8)        launch_kv_store_w<T, false, 1>(a, rope, grid, stream);
    else if (w == 2) launch_kv_store_w<T, true, 2>(a, rope, grid, stream);
    else             launch_kv_store_w<T, true, 1>(a, rope, grid, stream);
}

// one launch; the caller (fa_api.hip) has validated the block, replaced descales of 0 by 1.0 and knows the problem is not empty
void launch_kv_store(const fa_kv_store_params& s, hipStream_t stream) {
    KvStoreArgs a;
    a.k = static_cast<const uint16_t*>(s.k);
    a.v = static_cast<const uint16_t*>(s.v);
    a.k_row_stride = s.k_row_stride; a.k_head_stride = s.k_head_stride;
    a.v_row_stride = s.v_row_stride; a.v_head_stride = s.v_head_stride;
    a.kc = s.k_cache; a.vc = s.v_cache;
    a.kc_batch_stride = s.kc_batch_stride; a.kc_row_stride = s.kc_row_stride; a.kc_head_stride = s.kc_head_stride;
    a.vc_batch_stride = s.vc_batch_stride; a.vc_row_stride = s.vc_row_stride; a.vc_head_stride = s.vc_head_stride;
    a.slot_mapping = s.slot_mapping;
    a.cu_seqlens = s.cu_seqlens; a.cache_seqlens = s.cache_seqlens;
    a.block_table = s.block_table; a.cache_batch_idx = s.cache_batch_idx;
    a.block_table_batch_stride = s.block_table_batch_stride;
    a.n_rows = s.total_rows;
    a.n_slots = (int64_t)s.num_blocks * s.page_block_size;
    a.cos = static_cast<const uint16_t*>(s.rotary_cos);
    a.sin = static_cast<const uint16_t*>(s.rotary_sin);
    a.batch = s.batch; a.nheads = s.nheads; a.head_dim = s.head_dim; a.page = s.page_block_size;
    const int64_t cap = s.block_table ? (int64_t)s.max_blocks * s.page_block_size : (int64_t)s.page_block_size;
    a.capacity = (int)(cap < INT32_MAX ? cap : INT32_MAX);                        // (positions are sums of two int32: < 2^32)
    a.rotary_dim = s.rotary_dim; a.seqlen_ro = s.rotary_dim > 0 ? s.seqlen_ro : 0;
    a.k_descale = s.k_descale; a.v_descale = s.v_descale;
    const bool kv8 = s.cache_dtype == FA_FP8_E4M3;
    const int w = kvs_wide_ok(s) ? 2 : 1;
    const int rope = (s.rotary_dim <= 0 || s.seqlen_ro <= 0) ? ROPE_NONE : (s.rotary_interleaved ? ROPE_INTERLEAVED : ROPE_NEOX);
    const int64_t ipr = (int64_t)s.nheads * (s.head_dim / (8 * w));
    const RowPlan pl = row_plan(a.n_rows, ipr, KVS_STEP_ITEMS, KVS_MAX_GROUP_ROWS, KVS_GRID_CAP);
    a.group_rows = pl.group_rows;
    if (s.dtype == FA_BF16) launch_kv_store_t<bf16_tag>(a, kv8, w, rope, pl.grid, stream);
    else                    launch_kv_store_t<fp16_tag>(a, kv8, w, rope, pl.grid, stream);
}

}  // namespace fa
