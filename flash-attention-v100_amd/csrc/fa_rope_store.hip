// fa_rope_store.hip - the prologue of a serving step in one launch (fa_rope_store, include/fa_mi355.h): rotate q and k at per-token
// positions, write them back (in place or out of place) and store the rotated K and V into a KV cache by slot.  fa_rotary's
// rotation (fa_rope.h's rope_chunk / rope_y0 / rope_y1) and fa_kv_store's slot addressing and quantisation (fa_fp8_cvt.h's
// to_fp8x8), so q_out / k_out carry fa_rotary's bits and the cache the bits fa_rotary + fa_kv_store by slot would leave.
// Pure byte movement, HBM-bound like fa_rotary.hip / fa_kv_store.hip: no LDS, no atomics, no workspace, one launch.
//   - a workgroup step owns a GROUP of consecutive rows (RopeStoreArgs::group_rows <= RS_MAX_GROUP_ROWS, chosen by the host so
//     that a step has about RS_STEP_ITEMS items); the grid is capped at RS_GRID_CAP groups and strides over the rest;
//   - lane l of every wave reads positions[] and slot_mapping[] of row l of the group once per step (two 8-byte loads and one
//     division) and works out where the row goes in k_cache / v_cache (or that it is not cached) and its place in the cos / sin
//     tables (or that it is not rotated); the items fetch their row's triple with a cross-lane read;
//   - an ITEM is what one lane owns: a RUN of W 16-byte pieces (8 W consecutive columns of one head of q, k or v), and - inside
//     rotary_dim of a NeoX rotation - the partner run `rotary_dim / 2` columns on as well, fa_rotary's fast form.  W = 1 but for
//     fp8 caches that take 16-byte stores (16 columns: W = 2, the host's rs_wide_ok).  A row's items: the q heads, the k heads,
//     the v heads; q and k items behind rotary_dim exist only where those columns are copied (out != in, or into the cache);
//   - a lane loads everything of its items - both runs, cos / sin - then computes, then stores: in place no element is read after
//     its partner was written, and no two items share an element.  The loads are unconditional and branch-free (clamped to
//     addresses inside q / k / v and the tables), so hipcc keeps all of them in flight; only the stores depend on what the row
//     turned out to be;
//   - q / k / v are read once: nontemporal loads.  The cache lines and q_out / k_out are read by the attention call that follows:
//     ordinary stores (FA_ROPE_STORE_NT_OUT=1 builds the variant with nontemporal q_out / k_out stores; profiles/rope_store.txt
//     has both);
//   - two items are in flight per lane, also in the W = 2 form (FA_ROPE_STORE_WIDE_U=1 builds that form with one: fewer registers,
//     no faster - the same profile).
#include <cstdint>
#include "fa_rowops.h"
#include "fa_fp8_cvt.h"

#ifndef FA_ROPE_STORE_NT_OUT
#define FA_ROPE_STORE_NT_OUT 0
#endif
#ifndef FA_ROPE_STORE_WIDE_U
#define FA_ROPE_STORE_WIDE_U 2
#endif

namespace fa {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_GROUP_ROWS = 16;                     // rows per workgroup step at most (one lane each: <= 64)
constexpr int RS_STEP_ITEMS = 2048;                       // items a workgroup step aims for
constexpr int RS_GRID_CAP = 256 * 16;                     // as fa_rows.hip: 16 workgroups per CU in flight, then grid-stride

struct RopeStoreArgs {
    const uint16_t* q;                                    // nheads_q == 0 where there is no q
    const uint16_t* k;
    const uint16_t* v;                                    // read with caches only
    uint16_t* qo;
    uint16_t* ko;                                         // nullptr: K is not written back
    int64_t q_row_stride, q_head_stride, k_row_stride, k_head_stride, v_row_stride, v_head_stride;   // elements
    int64_t qo_row_stride, qo_head_stride, ko_row_stride, ko_head_stride;
    void* kc;                                             // nullptr (both): rotate only
    void* vc;
    int64_t kc_batch_stride, kc_row_stride, kc_head_stride;                       // elements of the cache type
    int64_t vc_batch_stride, vc_row_stride, vc_head_stride;
    const int64_t* positions;
    const int64_t* slot_mapping;
    int64_t n_rows, n_slots;                              // rows of q / k / v; num_blocks x page_block_size
    const uint16_t* cos;
    const uint16_t* sin;
    int nheads_q, nheads_k, head_dim, page, rotary_dim, seqlen_ro, group_rows;
    int q_inplace, k_inplace;
    float k_descale, v_descale;
};

struct RsRow {
    int64_t ko, vo;                                       // element offsets of the row in k_cache / v_cache, ko < 0: not cached
    int pos;                                              // its position in the cos / sin tables, -1: leave it unrotated
};

// row r0 + lane of the group (only lanes < group_rows are ever asked)
__device__ __forceinline__ RsRow rs_row(const RopeStoreArgs& a, int64_t r0, int lane) {
    const int64_t r = r0 + lane;
    RsRow w;
    w.ko = -1; w.vo = 0; w.pos = -1;
    if (r >= a.n_rows) return w;
    const int64_t p = a.positions[r];
    if (p >= 0 && p < a.seqlen_ro) w.pos = (int)p;
    if (a.slot_mapping) {
        const int64_t slot = a.slot_mapping[r];
        if (slot >= 0 && slot < a.n_slots) {
            const int64_t blk = slot / a.page, row = slot - blk * a.page;
            w.ko = blk * a.kc_batch_stride + row * a.kc_row_stride;
            w.vo = blk * a.vc_batch_stride + row * a.vc_row_stride;
        }
    }
    return w;
}

__device__ __forceinline__ void rs_st_out(uint16_t* p, u32x4 v) {
#if FA_ROPE_STORE_NT_OUT
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
#else
    *reinterpret_cast<u32x4*>(p) = v;
#endif
}

// one run of an item into the cache: W pieces at `off` (elements of the cache type)
template <typename T, bool KV8, int W>
__device__ __forceinline__ void rs_st_cache(void* cache, int64_t off, const u32x4 (&y)[W], float inv) {
    if (KV8) {
        uint8_t* p = static_cast<uint8_t*>(cache) + off;
        if (W == 2) {
            const u32x2 c0 = to_fp8x8<T>(y[0], inv), c1 = to_fp8x8<T>(y[W - 1], inv);
            *reinterpret_cast<u32x4*>(p) = u32x4{c0[0], c0[1], c1[0], c1[1]};
        } else {
            *reinterpret_cast<u32x2*>(p) = to_fp8x8<T>(y[0], inv);
        }
    } else {
        *reinterpret_cast<u32x4*>(static_cast<uint16_t*>(cache) + off) = y[0];
    }
}

// T: the 16-bit io type; KV8: fp8-e4m3 cache; W: 16-byte pieces per run (2: fp8 caches with 16-byte stores); ROPE: the pair rule
template <typename T, bool KV8, int W, int ROPE>
__global__ void __launch_bounds__(RS_THREADS) rope_store_kernel(const RopeStoreArgs a) {
    typedef typename RopeTable<ROPE>::type CS;
    constexpr bool NEOX = ROPE == ROPE_NEOX;
    constexpr int U = W == 2 ? FA_ROPE_STORE_WIDE_U : 2;  // items in flight per lane: loads first, then stores
    constexpr int RUN = 8 * W;                            // columns of a run
    const int lane = threadIdx.x & 63;
    const int rd = ROPE == ROPE_NONE ? 0 : a.rotary_dim;
    const int half = rd >> 1;
    const int n_rot = rd / (NEOX ? 2 * RUN : RUN);        // items of a head inside rotary_dim
    const int n_tail = (a.head_dim - rd) / RUN;           // and behind it
    const bool cached = a.kc != nullptr;
    const int iph_q = n_rot + (a.q_inplace ? 0 : n_tail);
    const int iph_k = n_rot + (cached || (a.ko && !a.k_inplace) ? n_tail : 0);
    const int iph_v = cached ? a.head_dim / RUN : 0;
    const int nq = a.nheads_q * iph_q, nk = a.nheads_k * iph_k;
    const int ipr = nq + nk + a.nheads_k * iph_v;         // items per row (the host launches nothing where this is 0)
    float kinv = 1.f, vinv = 1.f;
    if (KV8) {
        kinv = fp8_inv_descale(a.k_descale);
        vinv = fp8_inv_descale(a.v_descale);
    }
    for (int64_t r0 = (int64_t)blockIdx.x * a.group_rows; r0 < a.n_rows; r0 += (int64_t)gridDim.x * a.group_rows) {
        const RsRow mine = rs_row(a, r0, lane);
        const int64_t left = a.n_rows - r0;
        const int n = (int)(left < a.group_rows ? left : a.group_rows) * ipr;
        // (the trip count is workgroup-uniform and the cross-lane reads sit outside every lane-dependent branch: the lanes that
        //  hold the rows are active whenever they are read)
        for (int base = 0; base < n; base += RS_THREADS * U) {
            u32x4 xa[U][W], xb[U][W];                     // the run, and its partner run (NeoX, inside rotary_dim)
            CS cw[U][W], sw[U][W];
            uint16_t* op[U];                              // the run in q_out / k_out
            void* cp[U];                                  // k_cache / v_cache
            int64_t co[U];                                // the run in it
            float inv[U];
            bool st[U], cst[U], rot[U], two[U];           // st: written to q_out / k_out; cst: to the cache; two: has a partner run
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int w = base + u * RS_THREADS + (int)threadIdx.x;
                const bool in = w < n;
                const uint32_t wc = in ? (uint32_t)w : 0u;
                const uint32_t kr = wc / (uint32_t)ipr, c = wc - kr * (uint32_t)ipr;
                const int kind = (int)c < nq ? ROW_Q : ((int)c < nq + nk ? ROW_K : ROW_V);
                const uint32_t ck = c - (uint32_t)(kind == ROW_Q ? 0 : (kind == ROW_K ? nq : nq + nk));
                const uint32_t iph = (uint32_t)(kind == ROW_Q ? iph_q : (kind == ROW_K ? iph_k : iph_v));
                const uint32_t h = ck / iph, j = ck - h * iph;
                const int64_t rko = __shfl(mine.ko, (int)kr), rvo = __shfl(mine.vo, (int)kr);
                const int pos = __shfl(mine.pos, (int)kr);
                const int k_rot = kind == ROW_V ? 0 : n_rot, k_rd = kind == ROW_V ? 0 : rd;
                const bool inside = (int)j < k_rot;
                const int d = inside ? (int)j * RUN : k_rd + ((int)j - k_rot) * RUN;      // first column of the item
                const int64_t r = r0 + kr;
                const uint16_t* src = kind == ROW_Q ? a.q + r * a.q_row_stride + (int64_t)h * a.q_head_stride
                                    : kind == ROW_K ? a.k + r * a.k_row_stride + (int64_t)h * a.k_head_stride
                                                    : a.v + r * a.v_row_stride + (int64_t)h * a.v_head_stride;
                op[u] = (kind == ROW_Q ? a.qo + r * a.qo_row_stride + (int64_t)h * a.qo_head_stride
                                       : a.ko + r * a.ko_row_stride + (int64_t)h * a.ko_head_stride) + d;
                cp[u] = kind == ROW_V ? a.vc : a.kc;
                co[u] = (kind == ROW_V ? rvo + (int64_t)h * a.vc_head_stride : rko + (int64_t)h * a.kc_head_stride) + d;
                inv[u] = kind == ROW_V ? vinv : kinv;
                rot[u] = ROPE != ROPE_NONE && in && inside && pos >= 0;
                two[u] = NEOX && inside;
                st[u] = in && (kind == ROW_Q ? (rot[u] || !a.q_inplace) : (kind == ROW_K && a.ko && (rot[u] || !a.k_inplace)));
                cst[u] = in && kind != ROW_Q && cached && rko >= 0;
                const int64_t trow = (int64_t)(pos >= 0 ? pos : 0) * half;
                // every load is unconditional, from an address that is valid whatever the lane's item is (an item past the step's
                // last one reads the step's first run, a run without a partner itself, a run that is not rotated the first table
                // entries of its row or of row 0): no branch sits between the loads, so all of them are in flight before the first
                // use.  What is stored, and whether, is decided afterwards.
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    xa[u][q] = ld_nt16(src + d + 8 * q);
                    if constexpr (NEOX) xb[u][q] = ld_nt16(src + d + (inside ? half : 0) + 8 * q);
                    if constexpr (ROPE != ROPE_NONE) {
                        const int ds = inside ? d + 8 * q : 0;
                        const int t = NEOX ? ds : ds >> 1;                        // interleaved: pairs ds / 2 .. ds / 2 + 3
                        cw[u][q] = *reinterpret_cast<const CS*>(a.cos + trow + t);
                        sw[u][q] = *reinterpret_cast<const CS*>(a.sin + trow + t);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!st[u] && !cst[u]) continue;
                u32x4 ya[W], yb[W];
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    ya[q] = xa[u][q];
                    yb[q] = xa[u][q];
                    if constexpr (ROPE != ROPE_NONE) {
                        // rope_chunk reads its cos / sin through pointers: hand it the piece's values (registers after inlining;
                        // d_base 0 / half = "a piece of the first / second half", table index 0).  Every piece is rotated and the
                        // result kept where the row is to be rotated: a branch around the arithmetic would let hipcc sink the
                        // partner and table loads into it, behind the first wait.
                        const CS cl = cw[u][q], sl = sw[u][q];
                        const uint16_t* cosp = reinterpret_cast<const uint16_t*>(&cl);
                        const uint16_t* sinp = reinterpret_cast<const uint16_t*>(&sl);
                        u32x4 za = xa[u][q];
                        if constexpr (NEOX) {
                            u32x4 zb = xb[u][q];
                            rope_chunk<T>(za, xb[u][q], cosp, sinp, 0, rd, false);
                            rope_chunk<T>(zb, xa[u][q], cosp, sinp, half, rd, false);
                            yb[q] = rot[u] ? zb : xb[u][q];
                        } else {
                            rope_chunk<T>(za, za, cosp, sinp, 0, rd, true);
                        }
                        ya[q] = rot[u] ? za : xa[u][q];
                    }
                }
                if (st[u]) {
#pragma unroll
                    for (int q = 0; q < W; ++q) {
                        rs_st_out(op[u] + 8 * q, ya[q]);
                        if (NEOX && two[u]) rs_st_out(op[u] + half + 8 * q, yb[q]);
                    }
                }
                if (cst[u]) {
                    rs_st_cache<T, KV8, W>(cp[u], co[u], ya, inv[u]);
                    if (NEOX && two[u]) rs_st_cache<T, KV8, W>(cp[u], co[u] + half, yb, inv[u]);
                }
            }
        }
    }
}

// fp8 caches: 16 source columns and one 16-byte store per run where the cache and the rotation allow it (the header's contract)
static bool rs_wide_ok(const fa_rope_store_params& s) {
    if (!s.k_cache || s.cache_dtype != FA_FP8_E4M3 || s.head_dim % 16 != 0) return false;
    if (!s.rotary_interleaved && s.rotary_dim % 32 != 0) return false;            // a NeoX half must hold whole 16-column runs
    const uint64_t bits = (uint64_t)reinterpret_cast<uintptr_t>(s.k_cache) | (uint64_t)reinterpret_cast<uintptr_t>(s.v_cache) |
                          (uint64_t)s.kc_batch_stride | (uint64_t)s.kc_row_stride | (uint64_t)s.kc_head_stride |
                          (uint64_t)s.vc_batch_stride | (uint64_t)s.vc_row_stride | (uint64_t)s.vc_head_stride;
    return (bits & 15) == 0;
}

template <typename T, bool KV8, int W>
static void launch_rope_store_w(const RopeStoreArgs& a, int rope, int grid, hipStream_t stream) {
    const dim3 g(grid), b(RS_THREADS);
    if (rope == ROPE_NONE)             hipLaunchKernelGGL((rope_store_kernel<T, KV8, W, ROPE_NONE>), g, b, 0, stream, a);
    else if (rope == ROPE_INTERLEAVED) hipLaunchKernelGGL((rope_store_kernel<T, KV8, W, ROPE_INTERLEAVED>), g, b, 0, stream, a);
    else                                  hipLaunchKernelGGL((rope_store_kernel<T, KV8, W, ROPE_NEOX>), g, b, 0, stream, a);
}

template <typename T>
static void launch_rope_store_t(const RopeStoreArgs& a, bool kv8, int w, int rope, int grid, hipStream_t stream) {
    if (!kv8)        launch_rope_store_w<T, false, 1>(a, rope, grid, stream);
    else if (w == 2) launch_rope_store_w<T, true, 2>(a, rope, grid, stream);
    else             launch_rope_store_w<T, true, 1>(a, rope, grid, stream);
}

// one launch (none where no row has an item: in place with an empty table); the caller (fa_api.hip) has validated the block,
// replaced descales of 0 by 1.0 and knows that total_rows, head_dim and nheads_q + nheads_k are positive
void launch_rope_store(const fa_rope_store_params& s, hipStream_t stream) {
    RopeStoreArgs a;
    fill_rope_store_args(a, s);
    const bool cached = s.k_cache != nullptr;
    const bool kv8 = cached && s.cache_dtype == FA_FP8_E4M3;
    const int w = rs_wide_ok(s) ? 2 : 1;
    const int rope = s.seqlen_ro <= 0 ? ROPE_NONE : (s.rotary_interleaved ? ROPE_INTERLEAVED : ROPE_NEOX);
    // the kernel's own item count of a row
    const int run = 8 * w, rd = rope == ROPE_NONE ? 0 : s.rotary_dim;
    const int n_rot = rd / (rope == ROPE_NEOX ? 2 * run : run), n_tail = (s.head_dim - rd) / run;
    const int64_t iph_q = n_rot + (a.q_inplace ? 0 : n_tail);
    const int64_t iph_k = n_rot + (cached || (a.ko && !a.k_inplace) ? n_tail : 0);
    const int64_t iph_v = cached ? s.head_dim / run : 0;
    const int64_t ipr = a.nheads_q * iph_q + a.nheads_k * (iph_k + iph_v);
    if (ipr == 0) return;
    const RowPlan pl = row_plan(a.n_rows, ipr, RS_STEP_ITEMS, RS_MAX_GROUP_ROWS, RS_GRID_CAP);
    a.group_rows = pl.group_rows;
    if (s.dtype == FA_BF16) launch_rope_store_t<bf16_tag>(a, kv8, w, rope, pl.grid, stream);
    else                    launch_rope_store_t<fp16_tag>(a, kv8, w, rope, pl.grid, stream);
}

}  // namespace fa
