// fa_merge.hip - merge of attention states computed over DISJOINT key sets (fa_merge_states, include/fa_mi355.h):
//   LSE = logsumexp_s(lse_s),   out = sum_s exp(lse_s - LSE) out_s        (fp32 arithmetic, 16-bit in and out)
// the device form of sharding.merge_attention_shards, used by the shared-prefix ("cascade") decode of cascade.py: the prefix
// pass and the per-sequence suffix pass each leave (out, lse), this kernel combines them.
// Pure byte movement, HBM-bound, no matrix work, no atomics, no workspace: n + 1 tensors of rows x heads x D 16-bit values cross
// the memory interface once.  One lane owns one 16-byte piece (8 values) of one (row, head) - 8 bytes where a base address or a
// stride is only 8-byte aligned -; the lanes of a (row, head) sit next to each other, so a wave-instruction covers whole
// contiguous rows of D values.  Every lane reads the n LSEs of its (row, head) itself (the same address across the D / 8 lanes
// of a row: one request) - no LDS, no cross-lane traffic.  All loads of an item are issued before the first use.
//   - a part with lse_s = -inf (or a weight that underflows to 0) is SKIPPED, never multiplied: NaN in its out_s stays out;
//   - every part -inf: out = 0, LSE = -inf;
//   - exactly one finite part: its weight is exp2(0) / 1 = 1 and the accumulator starts at -0.0, so fma(1, x, -0.0) = x for
//     every x (signed zeros included), a 16-bit value survives the fp32 round trip and LSE = m + log2(1) ln 2 = m: the row is that
//     part's row bit for bit.
#include <cstdint>
#include "fa_common.h"

namespace fa {

constexpr int MERGE_THREADS = 256;

struct MergeArgs {
    fa_merge_state parts[FA_MERGE_MAX_PARTS];
    fa_merge_state out;
    int seqlen, nheads, chunks;          // chunks: pieces of VEC values per (row, head)
    int64_t total;                       // batch x seqlen x nheads x chunks
};

template <int VEC> struct MergeVec;
template <> struct MergeVec<8> { typedef u32x4 type; };
template <> struct MergeVec<4> { typedef u32x2 type; };

// NMAX: the number of parts, a compile-time constant so that the part loop unrolls without branches and all loads are in flight
template <typename T, int VEC, int NMAX>
__global__ void __launch_bounds__(MERGE_THREADS) merge_states_kernel(const MergeArgs a) {
    using E = Elem<T>;
    typedef typename MergeVec<VEC>::type V;
    constexpr int W = VEC / 2;                                   // 32-bit words per piece
    const int64_t i = (int64_t)blockIdx.x * MERGE_THREADS + threadIdx.x;      // one item per lane, no loop: nothing to amortise
    if (i < a.total) {
        int64_t b;                                               // item -> (batch, row, head, piece), the piece fastest
        int s, h, c;
        if (a.total <= 0xffffffffll) {                           // (wave-uniform; 64-bit divisions cost ~10 x the 32-bit ones)
            const uint32_t u = (uint32_t)i / (uint32_t)a.chunks, r = u / (uint32_t)a.nheads, bb = r / (uint32_t)a.seqlen;
            c = (int)((uint32_t)i - u * (uint32_t)a.chunks);
            h = (int)(u - r * (uint32_t)a.nheads);
            s = (int)(r - bb * (uint32_t)a.seqlen);
            b = bb;
        } else {
            const int64_t u = i / a.chunks, r = u / a.nheads;
            b = r / a.seqlen;
            c = (int)(i - u * a.chunks);
            h = (int)(u - r * a.nheads);
            s = (int)(r - b * a.seqlen);
        }
        float l[NMAX];
        V v[NMAX];
#pragma unroll
        for (int p = 0; p < NMAX; ++p) {
            const fa_merge_state& t = a.parts[p];
            l[p] = t.lse[b * t.lse_batch_stride + h * t.lse_head_stride + s * t.lse_row_stride];
            v[p] = __builtin_nontemporal_load(reinterpret_cast<const V*>(
                static_cast<const uint16_t*>(t.o) + b * t.o_batch_stride + s * t.o_row_stride + h * t.o_head_stride + c * VEC));
        }
        float m = l[0];
#pragma unroll
        for (int p = 1; p < NMAX; ++p) m = fmaxf(m, l[p]);
        const float m_safe = m > -INFINITY ? m : 0.f;
        float w[NMAX], den = 0.f;
#pragma unroll
        for (int p = 0; p < NMAX; ++p) {
            w[p] = fast_exp2((l[p] - m_safe) * kLog2e);          // (-inf: 0)
            den += w[p];
        }
        const bool any = den > 0.f;
        const float inv = any ? 1.0f / den : 0.f;
        float acc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = -0.0f;
#pragma unroll
        for (int p = 0; p < NMAX; ++p) {
            const float wp = w[p] * inv;
            if (wp != 0.f) {
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    acc[2 * j] = fmaf(wp, E::lo(v[p][j]), acc[2 * j]);
                    acc[2 * j + 1] = fmaf(wp, E::hi(v[p][j]), acc[2 * j + 1]);
                }
            }
        }
        V o;
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = any ? E::pack2(acc[2 * j], acc[2 * j + 1]) : 0u;
        const fa_merge_state& t = a.out;
        __builtin_nontemporal_store(o, reinterpret_cast<V*>(
            static_cast<uint16_t*>(t.o) + b * t.o_batch_stride + s * t.o_row_stride + h * t.o_head_stride + c * VEC));
        if (c == 0)
            t.lse[b * t.lse_batch_stride + h * t.lse_head_stride + s * t.lse_row_stride] = any ? m + fast_log2(den) * kLn2 : -INFINITY;
    }
}

// widest piece every `o` of the call allows: 8 values (16 bytes), 4 values (8 bytes), or 0 (not even 8-byte aligned)
int merge_vec_width(const fa_merge_params& m) {
    uint64_t bits = 0;
    for (int p = 0; p <= m.n_parts; ++p) {
        const fa_merge_state& t = p < m.n_parts ? m.parts[p] : m.out;
        bits |= (uint64_t)reinterpret_cast<uintptr_t>(t.o) | (uint64_t)(t.o_batch_stride * 2) | (uint64_t)(t.o_row_stride * 2) |
                (uint64_t)(t.o_head_stride * 2);
    }
    return (bits & 15) == 0 ? 8 : ((bits & 7) == 0 ? 4 : 0);
}

template <typename T, int VEC>
static void launch_merge_n(const MergeArgs& a, int n, int grid, hipStream_t stream) {
#define FA_MERGE_CASE(N) \
    case N: hipLaunchKernelGGL((merge_states_kernel<T, VEC, N>), dim3(grid), dim3(MERGE_THREADS), 0, stream, a); break;
    switch (n) { FA_MERGE_CASE(2) FA_MERGE_CASE(3) FA_MERGE_CASE(4) FA_MERGE_CASE(5) FA_MERGE_CASE(6) FA_MERGE_CASE(7) FA_MERGE_CASE(8) }
#undef FA_MERGE_CASE
}

// one launch; the caller (fa_api.hip) has validated the block and knows merge_vec_width() != 0
void launch_merge_states(const fa_merge_params& m, hipStream_t stream) {
    MergeArgs a;
    for (int p = 0; p < FA_MERGE_MAX_PARTS; ++p) a.parts[p] = m.parts[p < m.n_parts ? p : 0];
    a.out = m.out;
    const int vec = merge_vec_width(m);
    a.seqlen = m.seqlen; a.nheads = m.nheads; a.chunks = m.head_dim / vec;
    a.total = (int64_t)m.batch * m.seqlen * m.nheads * a.chunks;
    // one item per lane: 256 / chunks (row, head) pairs per workgroup (16 at D = 128), so a few thousand pairs already give every
    // CU a workgroup (fa_api.hip has checked that the grid fits 31 bits)
    const int grid = (int)((a.total + MERGE_THREADS - 1) / MERGE_THREADS);
    const bool bf16 = m.dtype == FA_BF16;
    const int n = m.n_parts;
    if (vec == 8) { if (bf16) launch_merge_n<bf16_tag, 8>(a, n, grid, stream); else launch_merge_n<fp16_tag, 8>(a, n, grid, stream); }
    else          { if (bf16) launch_merge_n<bf16_tag, 4>(a, n, grid, stream); else launch_merge_n<fp16_tag, 4>(a, n, grid, stream); }
}

}  // namespace fa
