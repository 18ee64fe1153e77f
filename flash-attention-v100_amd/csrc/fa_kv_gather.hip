// fa_kv_gather.hip - read ragged K / V rows out of a KV cache into a packed [total_rows, nheads, head_dim] pair (fa_kv_gather,
// include/fa_mi355.h): fa_kv_store.hip read backwards.  One launch reads K and V; paged or contiguous caches of the output's
// 16-bit type (copied bit for bit) or fp8-e4m3 (fa_fp8_cvt.h's from_fp8x8: fp32(code) * descale, one rounding); rows addressed by
// a slot mapping, or by (cu_seqlens, seq_offsets, block_table / cache_batch_idx).  EVERY output row is written exactly once: a row
// that names nothing (slot or position out of range, behind cu_seqlens[batch]) becomes +0 in K and V.
// Pure byte movement, HBM-bound like fa_kv_store.hip / fa_rows.hip: no LDS, no atomics, no workspace, one launch.
//   - a workgroup step owns a GROUP of consecutive OUTPUT rows (KvGatherArgs::group_rows <= KVG_MAX_GROUP_ROWS, chosen by the
//     host so that a step has about KVG_STEP_ITEMS items); the grid is capped at KVG_GRID_CAP groups and strides over the rest;
//   - lane l of every wave works out row l of the group once per step: where it lies in k_cache / v_cache, or that it is a zero
//     row (slot mode: one 8-byte load and one division; sequence mode: ONE wave-uniform binary search in cu_seqlens for the
//     group's first row, then the lanes walk on - empty sequences included - and a gathered row reads its block-table entry);
//     the items fetch their row's offsets with a cross-lane read;
//   - an ITEM is what one lane owns: 8 W consecutive columns of one head of K and the same of V.  W = 1 for 16-bit caches (16-byte
//     load, 16-byte store); fp8 caches take W = 2 where head_dim % 16 == 0 and the cache is 16-byte aligned (16 codes in one
//     16-byte load, two 16-byte stores) and W = 1 otherwise (8 codes in one 8-byte load, one 16-byte store).  Both widths run the
//     same conversion on the same codes: the same bits;
//   - a lane loads everything of its items, then converts, then stores.  The loads are unconditional and branch-free: an item
//     past the step's last one and a zero row read the cache's first row instead (an address inside the cache), so hipcc keeps
//     all of them in flight; what is stored - the row or zeros - is decided afterwards.  (A cache without a single slot has no
//     such address: one kernel-uniform test keeps every load away from it, and every row is a zero row.)
//   - the output is read by the next op: ordinary stores.  The cache rows cross once: nontemporal loads, decided by the
//     measurement (profiles/kv_gather.txt has both builds: at 65536 rows 83.4 against 109.8 us from a bf16 cache, 69.8 against
//     85.3 us from an fp8 one; 2 - 3 us slower at 8192 rows, where the cache sits in the last-level cache between the sweep's calls).
//     FA_KV_GATHER_NT_LOADS=0 builds the ordinary-load variant.
#include <cstdint>
#include "fa_rowops.h"
#include "fa_fp8_cvt.h"

#ifndef FA_KV_GATHER_NT_LOADS
#define FA_KV_GATHER_NT_LOADS 1
#endif

namespace fa {

constexpr int KVG_THREADS = 256;
constexpr int KVG_MAX_GROUP_ROWS = 16;                    // rows per workgroup step at most (one lane each: <= 64)
constexpr int KVG_STEP_ITEMS = 2048;                      // items a workgroup step aims for
constexpr int KVG_GRID_CAP = 256 * 16;                    // as fa_kv_store.hip: 16 workgroups per CU in flight, then grid-stride

struct KvGatherArgs {
    const void* kc;
    const void* vc;
    int64_t kc_batch_stride, kc_row_stride, kc_head_stride;                       // elements of the cache type
    int64_t vc_batch_stride, vc_row_stride, vc_head_stride;
    uint16_t* k;
    uint16_t* v;
    int64_t k_row_stride, k_head_stride, v_row_stride, v_head_stride;             // elements
    const int64_t* slot_mapping;
    const int32_t* cu_seqlens;
    const int32_t* seq_offsets;
    const int32_t* block_table;
    const int32_t* cache_batch_idx;
    int64_t block_table_batch_stride;
    int64_t n_rows, n_slots;                              // rows of k / v; num_blocks x page_block_size
    int batch, nheads, head_dim, page, capacity;          // capacity: positions a sequence can hold (sequence mode)
    int group_rows;
    float k_descale, v_descale;
};

struct KvgRow {
    int64_t ko, vo;                                       // element offsets of the row in k_cache / v_cache, ko < 0: a zero row
};

// row r0 + lane of the group (only lanes < group_rows are ever asked)
__device__ __forceinline__ KvgRow kvg_row(const KvGatherArgs& a, int64_t r0, int lane) {
    const int64_t r = r0 + lane;
    KvgRow w;
    w.ko = -1; w.vo = 0;
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
    const int64_t pos = (int64_t)(a.seq_offsets ? a.seq_offsets[b] : 0) + (r - a.cu_seqlens[b]);
    if (pos < 0 || pos >= a.capacity) return w;           // outside the sequence's capacity: nothing to read
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
    return w;
}

template <typename V>
__device__ __forceinline__ V kvg_ld(const V* p) {
#if FA_KV_GATHER_NT_LOADS
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

template <bool KV8, int W> struct KvgPiece { typedef u32x4 type; };   // what one lane loads of K (and of V): 16 bytes
template <> struct KvgPiece<true, 1> { typedef u32x2 type; };         // 8 codes

// T: the 16-bit output type; KV8: fp8-e4m3 cache; W: 16-byte output pieces per item
template <typename T, bool KV8, int W>
__global__ void __launch_bounds__(KVG_THREADS) kv_gather_kernel(const KvGatherArgs a) {
    typedef typename KvgPiece<KV8, W>::type P;
    constexpr int U = 2;                                  // items in flight per lane: loads first, then stores
    const int lane = threadIdx.x & 63;
    const int iph = a.head_dim / (8 * W);                 // items per head
    const int ipr = a.nheads * iph;                       // items per row
    const bool any_slot = a.n_slots > 0;                  // kernel-uniform: the cache has a first row to clamp to
    for (int64_t r0 = (int64_t)blockIdx.x * a.group_rows; r0 < a.n_rows; r0 += (int64_t)gridDim.x * a.group_rows) {
        const KvgRow mine = kvg_row(a, r0, lane);
        const int64_t left = a.n_rows - r0;
        const int n = (int)(left < a.group_rows ? left : a.group_rows) * ipr;
        // (the trip count is workgroup-uniform and the cross-lane reads sit outside every lane-dependent branch: the lanes that
        //  hold the rows are active whenever they are read)
        for (int base = 0; base < n; base += KVG_THREADS * U) {
            P kx[U], vx[U];
            uint16_t* kd[U];
            uint16_t* vd[U];
            int64_t ko[U], vo[U];
            bool in[U], ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int w = base + u * KVG_THREADS + (int)threadIdx.x;
                in[u] = w < n;
                const uint32_t wc = in[u] ? (uint32_t)w : 0u;
                const uint32_t kr = wc / (uint32_t)ipr, c = wc - kr * (uint32_t)ipr;
                const uint32_t h = c / (uint32_t)iph, j = c - h * (uint32_t)iph;
                const int64_t rko = __shfl(mine.ko, (int)kr), rvo = __shfl(mine.vo, (int)kr);
                ok[u] = in[u] && rko >= 0;
                const int d = (int)j * 8 * W;             // first column of the item
                kd[u] = a.k + (r0 + kr) * a.k_row_stride + (int64_t)h * a.k_head_stride + d;
                vd[u] = a.v + (r0 + kr) * a.v_row_stride + (int64_t)h * a.v_head_stride + d;
                // a zero row (and an item past the step's last one, which is row 0 of the group) loads from the cache's first row
                ko[u] = (rko >= 0 ? rko : 0) + (int64_t)h * a.kc_head_stride + d;
                vo[u] = (rko >= 0 ? rvo : 0) + (int64_t)h * a.vc_head_stride + d;
                kx[u] = P{};
                vx[u] = P{};
            }
            if (any_slot) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if constexpr (KV8) {
                        kx[u] = kvg_ld(reinterpret_cast<const P*>(static_cast<const uint8_t*>(a.kc) + ko[u]));
                        vx[u] = kvg_ld(reinterpret_cast<const P*>(static_cast<const uint8_t*>(a.vc) + vo[u]));
                    } else {
                        kx[u] = kvg_ld(reinterpret_cast<const P*>(static_cast<const uint16_t*>(a.kc) + ko[u]));
                        vx[u] = kvg_ld(reinterpret_cast<const P*>(static_cast<const uint16_t*>(a.vc) + vo[u]));
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!in[u]) continue;
                const u32x4 zero = {0, 0, 0, 0};
                if constexpr (KV8) {
#pragma unroll
                    for (int q = 0; q < W; ++q) {
                        const u32x2 kc8 = {kx[u][2 * q], kx[u][2 * q + 1]}, vc8 = {vx[u][2 * q], vx[u][2 * q + 1]};
                        const u32x4 ky = from_fp8x8<T>(kc8, a.k_descale), vy = from_fp8x8<T>(vc8, a.v_descale);
                        *reinterpret_cast<u32x4*>(kd[u] + 8 * q) = ok[u] ? ky : zero;
                        *reinterpret_cast<u32x4*>(vd[u] + 8 * q) = ok[u] ? vy : zero;
                    }
                } else {
                    *reinterpret_cast<u32x4*>(kd[u]) = ok[u] ? kx[u] : zero;          // bit for bit
                    *reinterpret_cast<u32x4*>(vd[u]) = ok[u] ? vx[u] : zero;
                }
            }
        }
    }
}

// fp8 caches: 16 codes per load where the cache allows it (the header's contract)
static bool kvg_wide_ok(const fa_kv_gather_params& s) {
    if (s.cache_dtype != FA_FP8_E4M3 || s.head_dim % 16 != 0) return false;
    const uint64_t bits = (uint64_t)reinterpret_cast<uintptr_t>(s.k_cache) | (uint64_t)reinterpret_cast<uintptr_t>(s.v_cache) |
                          (uint64_t)s.kc_batch_stride | (uint64_t)s.kc_row_stride | (uint64_t)s.kc_head_stride |
                          (uint64_t)s.vc_batch_stride | (uint64_t)s.vc_row_stride | (uint64_t)s.vc_head_stride;
    return (bits & 15) == 0;
}

template <typename T>
static void launch_kv_gather_fp8(const KvGatherArgs& a, int w, int grid, hipStream_t stream) {
    const dim3 g(grid), b(KVG_THREADS);
    if (w == 2) hipLaunchKernelGGL((kv_gather_kernel<T, true, 2>), g, b, 0, stream, a);
    else        hipLaunchKernelGGL((kv_gather_kernel<T, true, 1>), g, b, 0, stream, a);
}

// one launch; the caller (fa_api.hip) has validated the block, replaced descales of 0 by 1.0 and knows the problem is not empty
void launch_kv_gather(const fa_kv_gather_params& s, hipStream_t stream) {
    KvGatherArgs a;
    a.kc = s.k_cache; a.vc = s.v_cache;
    a.kc_batch_stride = s.kc_batch_stride; a.kc_row_stride = s.kc_row_stride; a.kc_head_stride = s.kc_head_stride;
    a.vc_batch_stride = s.vc_batch_stride; a.vc_row_stride = s.vc_row_stride; a.vc_head_stride = s.vc_head_stride;
    a.k = static_cast<uint16_t*>(s.k);
    a.v = static_cast<uint16_t*>(s.v);
    a.k_row_stride = s.k_row_stride; a.k_head_stride = s.k_head_stride;
    a.v_row_stride = s.v_row_stride; a.v_head_stride = s.v_head_stride;
    a.slot_mapping = s.slot_mapping;
    a.cu_seqlens = s.cu_seqlens; a.seq_offsets = s.seq_offsets;
    a.block_table = s.block_table; a.cache_batch_idx = s.cache_batch_idx;
    a.block_table_batch_stride = s.block_table_batch_stride;
    a.n_rows = s.total_rows;
    a.n_slots = (int64_t)s.num_blocks * s.page_block_size;
    a.batch = s.batch; a.nheads = s.nheads; a.head_dim = s.head_dim; a.page = s.page_block_size;
    const int64_t cap = s.block_table ? (int64_t)s.max_blocks * s.page_block_size : (int64_t)s.page_block_size;
    a.capacity = (int)(cap < INT32_MAX ? cap : INT32_MAX);                        // (positions are sums of two int32: < 2^32)
    a.k_descale = s.k_descale; a.v_descale = s.v_descale;
    const bool kv8 = s.cache_dtype == FA_FP8_E4M3;
    const int w = kvg_wide_ok(s) ? 2 : 1;
    const int64_t ipr = (int64_t)s.nheads * (s.head_dim / (8 * w));
    const RowPlan pl = row_plan(a.n_rows, ipr, KVG_STEP_ITEMS, KVG_MAX_GROUP_ROWS, KVG_GRID_CAP);
    a.group_rows = pl.group_rows;
    // (a 16-bit cache is copied bit for bit: one kernel serves fp16 and bf16)
    if (!kv8)                    hipLaunchKernelGGL((kv_gather_kernel<bf16_tag, false, 1>), dim3(pl.grid), dim3(KVG_THREADS), 0, stream, a);
    else if (s.dtype == FA_BF16) launch_kv_gather_fp8<bf16_tag>(a, w, pl.grid, stream);
    else                         launch_kv_gather_fp8<fp16_tag>(a, w, pl.grid, stream);
}

}  // namespace fa
