// fa_rotary.hip - standalone rotary embedding (fa_rotary, include/fa_mi355.h): y = rope(x, pos) for every (batch, row, head) of a
// [B, S, H, D] tensor (or a packed [T, H, D] one with cu_seqlens), out of place or in place, forward or - with `conjugate` -
// backward.  The pair rule and the arithmetic are fa_rope.h's (rope_chunk / rope_y0 / rope_y1): fp32 math, one rounding to the
// 16-bit io type, so a row rotated here carries the bits the kv-cache op's in-kernel RoPE gives it.
// Pure byte movement, HBM-bound like fa_rows.hip: no LDS, no atomics, no workspace, one launch.
//   - a workgroup step owns a GROUP of consecutive rows (RotaryArgs::group_rows <= ROT_MAX_GROUP_ROWS, chosen by the host so
//     that a step has about ROT_STEP_ITEMS items); the grid is capped at ROT_GRID_CAP groups and strides over the rest;
//   - lane l of every wave works out row l of the group once per step: its element offsets in x / out and its position
//     (dense: one division; packed: ONE wave-uniform binary search in cu_seqlens for the group's first row, then the lanes walk
//     on from there - empty sequences included); the items fetch their row's triple with a cross-lane read;
//   - an ITEM is what one lane owns: fast form - one 16-byte piece (interleaved), BOTH 16-byte partner pieces of a NeoX pair, or
//     one 16-byte piece of the columns behind rotary_dim (copied when out != x); general form - one pair, or one column behind
//     rotary_dim.  A lane loads everything of its items, computes, then stores: in place no element is read after its partner
//     was overwritten, and no two items share an element;
//   - a position outside [0, seqlen_ro) leaves the row unrotated (copied when out != x, untouched in place) and reads no
//     cos / sin; rows of a packed tensor behind cu_seqlens[batch] are treated the same way;
//   - x streams (nontemporal loads and stores: every byte crosses once), cos / sin use ordinary loads (reused across heads and
//     batch entries, they stay in L2).
#include <cstdint>
#include "fa_rowops.h"

namespace fa {

constexpr int ROT_THREADS = 256;
constexpr int ROT_MAX_GROUP_ROWS = 16;                    // rows per workgroup step at most (one lane each: <= 64)
constexpr int ROT_STEP_ITEMS = 2048;                      // items a workgroup step aims for
constexpr int ROT_GRID_CAP = 256 * 16;                    // as fa_rows.hip: 16 workgroups per CU in flight, then grid-stride

struct RotaryArgs {
    const uint16_t* x;
    uint16_t* out;
    int64_t x_batch_stride, x_row_stride, x_head_stride;  // elements
    int64_t o_batch_stride, o_row_stride, o_head_stride;
    const void* cos;
    const void* sin;
    const int32_t* seqlen_offsets;
    const int32_t* cu_seqlens;
    int64_t n_rows;                                       // batch x seqlen, or total_rows
    int batch, seqlen, nheads, head_dim, rotary_dim, seqlen_ro, seqlen_offset;
    int conjugate, inplace, group_rows;
};

struct RotRow {
    int64_t xo, oo;                                       // element offsets of the row in x / out
    int pos;                                              // its position in the cos / sin table, -1: leave the row unrotated
};

// row r0 + lane of the group (clamped to the last row; only lanes < group_rows are ever asked)
__device__ __forceinline__ RotRow rot_row(const RotaryArgs& a, int64_t r0, int lane) {
    int64_t r = r0 + lane;
    if (r >= a.n_rows) r = a.n_rows - 1;
    RotRow w;
    int64_t b, i;
    bool in_seq = true;
    if (a.cu_seqlens) {
        int lo = 0, hi = a.batch;                         // wave-uniform: the first sequence that ends behind r0 (batch: none)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.cu_seqlens[mid + 1] <= r0) lo = mid + 1; else hi = mid;
        }
        b = lo;
        while (b < a.batch && a.cu_seqlens[b + 1] <= r) ++b;      // the lane's own row: a few sequences further at most
        in_seq = b < a.batch;
        if (!in_seq) b = a.batch - 1;
        i = r - a.cu_seqlens[b];
        w.xo = r * a.x_row_stride;
        w.oo = r * a.o_row_stride;
    } else {
        b = r / a.seqlen;
        i = r - b * a.seqlen;
        w.xo = b * a.x_batch_stride + i * a.x_row_stride;
        w.oo = b * a.o_batch_stride + i * a.o_row_stride;
    }
    const int64_t p = i + a.seqlen_offset + (a.seqlen_offsets ? a.seqlen_offsets[b] : 0);
    w.pos = (in_seq && p >= 0 && p < a.seqlen_ro) ? (int)p : -1;
    return w;
}

__device__ __forceinline__ void rot_st(uint16_t* p, u32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p)); }

template <bool INTERLEAVED> struct RotTable;                          // the cos / sin values of one item
template <> struct RotTable<true> { typedef u32x2 type; };            // 4 pairs
template <> struct RotTable<false> { typedef u32x4 type; };           // 8 pairs

enum { ROT_NONE = 0, ROT_ROTATE = 1, ROT_COPY = 2 };

// Fast form: base addresses and strides of x / out multiples of 16 bytes, rotary_dim % 16 == 0 (NeoX) or % 8 == 0 (interleaved),
// cos / sin of the io type and 16-byte aligned, (head_dim - rotary_dim) % 8 == 0 when the columns behind rotary_dim are copied.
template <typename T, bool INTERLEAVED>
__global__ void __launch_bounds__(ROT_THREADS) rotary_fast_kernel(const RotaryArgs a) {
    typedef typename RotTable<INTERLEAVED>::type CS;
    constexpr int U = INTERLEAVED ? 4 : 2;                // items in flight per lane: loads first, then stores
    const int lane = threadIdx.x & 63;
    const int half = a.rotary_dim >> 1;
    const int n_rot = INTERLEAVED ? a.rotary_dim >> 3 : a.rotary_dim >> 4;
    const int iph = n_rot + (a.inplace ? 0 : (a.head_dim - a.rotary_dim) >> 3);       // items per head
    const int ipr = a.nheads * iph;                                                    // items per row
    const uint16_t* cosb = static_cast<const uint16_t*>(a.cos);
    const uint16_t* sinb = static_cast<const uint16_t*>(a.sin);
    const uint32_t sgn = a.conjugate ? 0x80008000u : 0u;  // sin -> -sin, exactly
    for (int64_t r0 = (int64_t)blockIdx.x * a.group_rows; r0 < a.n_rows; r0 += (int64_t)gridDim.x * a.group_rows) {
        const RotRow mine = rot_row(a, r0, lane);
        const int64_t left = a.n_rows - r0;
        const int n = (int)(left < a.group_rows ? left : a.group_rows) * ipr;
        // (the trip count is workgroup-uniform and the cross-lane reads sit outside every lane-dependent branch: the lanes that
        //  hold the rows are active whenever they are read)
        for (int base = 0; base < n; base += ROT_THREADS * U) {
            u32x4 va[U], vb[U];
            CS cw[U], sw[U];
            uint16_t* op[U];
            int kind[U];
            bool two[U];                                  // the item has a partner piece `half` columns on (NeoX, inside rotary_dim)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int w = base + u * ROT_THREADS + (int)threadIdx.x;
                const bool ok = w < n;
                const uint32_t wc = ok ? (uint32_t)w : 0u;
                const uint32_t k = wc / (uint32_t)ipr, c = wc - k * (uint32_t)ipr;
                const uint32_t h = c / (uint32_t)iph, j = c - h * (uint32_t)iph;
                const int64_t xo = __shfl(mine.xo, (int)k), oo = __shfl(mine.oo, (int)k);
                const int pos = __shfl(mine.pos, (int)k);
                const bool inside = (int)j < n_rot;
                const int d = inside ? (int)j * 8 : a.rotary_dim + ((int)j - n_rot) * 8;   // first column of the item
                const uint16_t* xp = a.x + xo + (int64_t)h * a.x_head_stride + d;
                op[u] = a.out + oo + (int64_t)h * a.o_head_stride + d;
                kind[u] = !ok ? ROT_NONE : (inside && pos >= 0) ? ROT_ROTATE : (a.inplace ? ROT_NONE : ROT_COPY);
                two[u] = !INTERLEAVED && inside;
                va[u] = vb[u] = u32x4{0, 0, 0, 0};
                cw[u] = sw[u] = CS{};
                if (kind[u] != ROT_NONE) {
                    va[u] = ld_nt16(xp);
                    if (two[u]) vb[u] = ld_nt16(xp + half);
                }
                if (kind[u] == ROT_ROTATE) {
                    const int64_t t = (int64_t)pos * half + (INTERLEAVED ? d >> 1 : d);
                    cw[u] = *reinterpret_cast<const CS*>(cosb + t);
                    sw[u] = *reinterpret_cast<const CS*>(sinb + t);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (kind[u] == ROT_NONE) continue;
                u32x4 ya = va[u], yb = vb[u];
                if (kind[u] == ROT_ROTATE) {
                    // rope_chunk reads its cos / sin through pointers: hand it the item's values (registers after inlining);
                    // d_base 0 / half = "the first piece of the first / second half", table index 0
                    const CS cl = cw[u];
                    CS sl = sw[u];
#pragma unroll
                    for (int q = 0; q < (int)(sizeof(CS) / 4); ++q) sl[q] ^= sgn;
                    const uint16_t* cp = reinterpret_cast<const uint16_t*>(&cl);
                    const uint16_t* sp = reinterpret_cast<const uint16_t*>(&sl);
                    if (INTERLEAVED) {
                        rope_chunk<T>(ya, ya, cp, sp, 0, a.rotary_dim, true);
                    } else {
                        rope_chunk<T>(ya, vb[u], cp, sp, 0, a.rotary_dim, false);
                        rope_chunk<T>(yb, va[u], cp, sp, half, a.rotary_dim, false);
                    }
                }
                rot_st(op[u], ya);
                if (two[u]) rot_st(op[u] + half, yb);
            }
        }
    }
}

// General form: any even rotary_dim, 2-byte aligned views, fp32 or 16-bit cos / sin.  One pair (or one column behind rotary_dim,
// copied when out != x) per lane, 2-byte accesses; the same rope_y0 / rope_y1 on the same fp32 values and the same rounding as
// the fast form, so the two forms give the same bits.
template <typename T, bool INTERLEAVED, typename CS>
__global__ void __launch_bounds__(ROT_THREADS) rotary_general_kernel(const RotaryArgs a) {
    using E = Elem<T>;
    const int lane = threadIdx.x & 63;
    const int half = a.rotary_dim >> 1;
    const int iph = half + (a.inplace ? 0 : a.head_dim - a.rotary_dim);
    const int ipr = a.nheads * iph;
    const CS* cosb = static_cast<const CS*>(a.cos);
    const CS* sinb = static_cast<const CS*>(a.sin);
    for (int64_t r0 = (int64_t)blockIdx.x * a.group_rows; r0 < a.n_rows; r0 += (int64_t)gridDim.x * a.group_rows) {
        const RotRow mine = rot_row(a, r0, lane);
        const int64_t left = a.n_rows - r0;
        const int n = (int)(left < a.group_rows ? left : a.group_rows) * ipr;
        for (int base = 0; base < n; base += ROT_THREADS) {
            const int w = base + (int)threadIdx.x;
            const bool ok = w < n;
            const uint32_t wc = ok ? (uint32_t)w : 0u;
            const uint32_t k = wc / (uint32_t)ipr, c = wc - k * (uint32_t)ipr;
            const uint32_t h = c / (uint32_t)iph, j = c - h * (uint32_t)iph;
            const int64_t xo = __shfl(mine.xo, (int)k), oo = __shfl(mine.oo, (int)k);
            const int pos = __shfl(mine.pos, (int)k);
            if (!ok) continue;
            const uint16_t* xp = a.x + xo + (int64_t)h * a.x_head_stride;
            uint16_t* op = a.out + oo + (int64_t)h * a.o_head_stride;
            if ((int)j >= half) {                         // a column behind rotary_dim (out != x only)
                const int d = a.rotary_dim + ((int)j - half);
                op[d] = xp[d];
                continue;
            }
            const int i0 = INTERLEAVED ? 2 * (int)j : (int)j, i1 = INTERLEAVED ? i0 + 1 : i0 + half;
            if (pos < 0) {
                if (!a.inplace) {
                    const uint16_t x0 = xp[i0], x1 = xp[i1];
                    op[i0] = x0;
                    op[i1] = x1;
                }
                continue;
            }
            const uint32_t x0 = xp[i0], x1 = xp[i1];
            const int64_t t = (int64_t)pos * half + (int)j;
            float cv, sv;
            if (sizeof(CS) == 4) {
                cv = (float)cosb[t];
                sv = (float)sinb[t];
            } else {
                cv = E::lo((uint32_t)cosb[t]);
                sv = E::lo((uint32_t)sinb[t]);
            }
            if (a.conjugate) sv = -sv;
            const float f0 = E::lo(x0), f1 = E::lo(x1);
            const uint32_t y = E::pack2(rope_y0(f0, f1, cv, sv), rope_y1(f0, f1, cv, sv));
            op[i0] = (uint16_t)(y & 0xffffu);
            op[i1] = (uint16_t)(y >> 16);
        }
    }
}

// the fast form's conditions (the header's contract); fa_api.hip has validated the block
static bool rotary_fast_ok(const fa_rotary_params& r, bool inplace) {
    if (r.cos_sin_fp32) return false;
    uint64_t bits = (uint64_t)reinterpret_cast<uintptr_t>(r.x) | (uint64_t)reinterpret_cast<uintptr_t>(r.out) |
                    (uint64_t)(r.x_row_stride * 2) | (uint64_t)(r.x_head_stride * 2) | (uint64_t)(r.o_row_stride * 2) |
                    (uint64_t)(r.o_head_stride * 2) | (uint64_t)reinterpret_cast<uintptr_t>(r.cos) |
                    (uint64_t)reinterpret_cast<uintptr_t>(r.sin);
    if (!r.cu_seqlens) bits |= (uint64_t)(r.x_batch_stride * 2) | (uint64_t)(r.o_batch_stride * 2);
    if (bits & 15) return false;
    if (r.rotary_dim % (r.interleaved ? 8 : 16) != 0) return false;
    return inplace || (r.head_dim - r.rotary_dim) % 8 == 0;
}

template <typename T>
static void launch_rotary_t(const RotaryArgs& a, bool fast, bool interleaved, bool cs32, int grid, hipStream_t stream) {
    const dim3 g(grid), b(ROT_THREADS);
    if (fast) {
        if (interleaved) hipLaunchKernelGGL((rotary_fast_kernel<T, true>), g, b, 0, stream, a);
        else             hipLaunchKernelGGL((rotary_fast_kernel<T, false>), g, b, 0, stream, a);
    } else if (cs32) {
        if (interleaved) hipLaunchKernelGGL((rotary_general_kernel<T, true, float>), g, b, 0, stream, a);
        else             hipLaunchKernelGGL((rotary_general_kernel<T, false, float>), g, b, 0, stream, a);
    } else {
        if (interleaved) hipLaunchKernelGGL((rotary_general_kernel<T, true, uint16_t>), g, b, 0, stream, a);
        else             hipLaunchKernelGGL((rotary_general_kernel<T, false, uint16_t>), g, b, 0, stream, a);
    }
}

// one launch; the caller (fa_api.hip) has validated the block and knows the problem is not empty
void launch_rotary(const fa_rotary_params& r, hipStream_t stream) {
    RotaryArgs a;
    a.x = static_cast<const uint16_t*>(r.x);
    a.out = static_cast<uint16_t*>(r.out);
    a.x_batch_stride = r.x_batch_stride; a.x_row_stride = r.x_row_stride; a.x_head_stride = r.x_head_stride;
    a.o_batch_stride = r.o_batch_stride; a.o_row_stride = r.o_row_stride; a.o_head_stride = r.o_head_stride;
    a.cos = r.cos; a.sin = r.sin;
    a.seqlen_offsets = r.seqlen_offsets; a.cu_seqlens = r.cu_seqlens;
    a.n_rows = r.cu_seqlens ? (int64_t)r.total_rows : (int64_t)r.batch * r.seqlen;
    a.batch = r.batch; a.seqlen = r.seqlen; a.nheads = r.nheads; a.head_dim = r.head_dim;
    a.rotary_dim = r.rotary_dim; a.seqlen_ro = r.seqlen_ro; a.seqlen_offset = r.seqlen_offset;
    a.conjugate = r.conjugate != 0;
    a.inplace = r.out == r.x;
    const bool fast = rotary_fast_ok(r, a.inplace != 0);
    const int half = r.rotary_dim / 2, tail = a.inplace ? 0 : r.head_dim - r.rotary_dim;
    const int64_t iph = fast ? (r.interleaved ? r.rotary_dim / 8 : r.rotary_dim / 16) + tail / 8 : half + tail;
    const int64_t ipr = iph * r.nheads;
    const RowPlan pl = row_plan(a.n_rows, ipr, ROT_STEP_ITEMS, ROT_MAX_GROUP_ROWS, ROT_GRID_CAP);
    a.group_rows = pl.group_rows;
    if (r.dtype == FA_BF16) launch_rotary_t<bf16_tag>(a, fast, r.interleaved != 0, r.cos_sin_fp32 != 0, pl.grid, stream);
    else                    launch_rotary_t<fp16_tag>(a, fast, r.interleaved != 0, r.cos_sin_fp32 != 0, pl.grid, stream);
}

}  // namespace fa
