// fa_moe_tile.h - the device code that the grouped expert GEMMs (fa_moe_gemm.hip, fa_moe_gemm_mxfp4.hip, fa_moe_gemm_mxfp4_dgrad.hip) share: which tile of
// out a workgroup owns, found from expert_offsets on the device, and the bounded buffer descriptor their loads go through.
#pragma once
#include "fa_common.h"
#include "fa_moe.h"

namespace fa {

namespace {

constexpr int GEMM_THREADS = 256;
constexpr int SEG_PER_LANE = 9;                         // 64 x 9 >= 512 + 1 segments
static_assert(64 * SEG_PER_LANE >= MOE_MAX_EXPERTS + 1, "a wave covers every segment");

struct GemmTile { int seg, m0, m_end; bool valid; };

// the (segment, first row, segment end) of tile `mt`; every lane of every wave returns the same (wave-uniform) answer
template <int BM>
__device__ __forceinline__ GemmTile find_tile(const int32_t* offs, int E, int M, int mt, int lane) {
    int b[SEG_PER_LANE + 1];
#pragma unroll
    for (int i = 0; i <= SEG_PER_LANE; ++i) {
        const int idx = lane * SEG_PER_LANE + i;
        int v = M;                                       // (the boundary behind expert_offsets[E]: the tail segment ends at rows)
        if (idx <= E) {
            v = offs[idx];
            v = v < 0 ? 0 : (v > M ? M : v);
        }
        b[i] = v;
    }
    long long cnt = 0;
#pragma unroll
    for (int i = 0; i < SEG_PER_LANE; ++i) {
        const int len = b[i + 1] - b[i];
        cnt += len > 0 ? (len + BM - 1) / BM : 0;
    }
    long long incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    long long c = incl - cnt;
    int seg = -1, m0 = 0, m_end = 0;
#pragma unroll
    for (int i = 0; i < SEG_PER_LANE; ++i) {
        const int len = b[i + 1] - b[i];
        const long long nt = len > 0 ? (len + BM - 1) / BM : 0;
        if (mt >= c && mt < c + nt) {
            seg = lane * SEG_PER_LANE + i;
            m0 = b[i] + (int)(mt - c) * BM;
            m_end = b[i + 1];
        }
        c += nt;
    }
    const unsigned long long bal = __ballot(seg >= 0);
    GemmTile t = {0, 0, 0, false};
    if (bal == 0) return t;
    const int src = __ffsll(bal) - 1;
    t.seg = __builtin_amdgcn_readfirstlane(__shfl(seg, src));
    t.m0 = __builtin_amdgcn_readfirstlane(__shfl(m0, src));
    t.m_end = __builtin_amdgcn_readfirstlane(__shfl(m_end, src));
    t.valid = t.seg >= 0 && t.seg <= E && t.m0 >= 0 && t.m0 < t.m_end && t.m_end <= M;
    return t;
}

// a descriptor over `bytes` (clamped to 2^31 - 1: kOobVoff is then always out of range) behind a wave-uniform address
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_rsrc(uint64_t at, int64_t bytes) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)at);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(at >> 32));
    const int64_t cl = bytes < 0 ? 0 : (bytes > 0x7fffffffLL ? 0x7fffffffLL : bytes);
    const uint32_t n = __builtin_amdgcn_readfirstlane((uint32_t)cl);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, (int)n, 0x00020000);
}

}  // namespace

}  // namespace fa
