// fa_moe_gemm.hip - the grouped expert GEMM of a mixture-of-experts block (fa_moe_gemm, include/fa_mi355.h).
//
//   out[r, :] = round16(sum_k float(a_r[k]) * float(W_e[k, :]) (+ float(bias[e, :])))   for expert_offsets[e] <= r < expert_offsets[e + 1]
//   out[r, :] = +0                                                                       for expert_offsets[E] <= r < rows
//
// with a_r = x[r] (plain form: x is fa_moe_permute's output) or a_r = x[sorted_slot[r] / top_k] (fused gather; a slot outside
// [0, tokens * top_k) is a row of +0 and forms no address).
//
// One workgroup of four waves owns a BM x 128 tile of out, BM = 128 (2 x 2 waves of 64 rows x 64 columns) or 32 (four waves of
// 32 x 32 side by side).  The tile is computed TRANSPOSED: the MFMA's A operand is the weight (i = output column), its B operand
// the activation (n = row), so a lane ends up with groups of four consecutive output columns of one row and, after one
// v_permlane32_swap with its partner lane, stores 16 bytes.  Every output element has one accumulator chain of
// v_mfma_f32_32x32x16 over k ascending in steps of 16 from +0 - whatever the tile shape - so a row's bits are a function of its
// source row, W_e, bias[e] and K alone.  A K tail is zero-filled (adding +0 * +0 leaves the chain's bits), never padded on the host.
//
// Staging, BK = 64 contraction elements a step, two LDS stages:
//   x, plain     [BM][64]  swz_row_off<64>, LDS-DMA (rows at or behind the segment's end and columns >= K: the out-of-range offset)
//   x, gather    the same image, written with ds_write_b128 from ordinary 16-byte loads through sorted_slot
//   w, "nk"      [128 n][64 k]  swz_row_off<64>, LDS-DMA; read by rows (ds_read_b128) like x: the Q K^T shape
//   w, "kn"      [64 k][128 n]  swzt_row_off<128>, LDS-DMA; read transposed (ds_read_b64_tr_b16, the counted-wait asm form): the
//                P V shape.  The transposing read names the 16 k of a step in "slot order" (fa_common.h); x is then read as two
//                8-byte halves in the same order.
// A buffer descriptor never spans more than what is left of ONE expert's slab (or of x) behind the tile's first element and
// never more than 2^31 - 1 bytes, so the out-of-range offset 2^31 always reads zeros; an expert's base is a 64-bit pointer.
//
// Which tile: segment lengths are device data.  Every wave reads the E + 1 offsets (a lane the 10 boundaries of its 9 segments),
// clamps them to [0, rows], counts each segment's tiles, scans the counts over the wave and finds the (segment, tile) of
// blockIdx.x - or leaves: the grid is the host's bound (fa_moe_gemm.h).  Segment E is the +0 tail; rows below a positive
// expert_offsets[0] (fa_moe_sort writes 0) are in no segment and are not written.  Offsets are only compared and clamped: a
// malformed table gives wrong rows, never an address outside out, x or w.
#include "fa_common.h"
#include "fa_moe_gemm.h"
#include <type_traits>

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

template <typename T, int BM, bool KN, bool GATHER>
__global__ void __launch_bounds__(GEMM_THREADS) moe_gemm_kernel(const fa_moe_gemm_params s) {
    using E = Elem<T>;
    constexpr int BN = MOE_GEMM_BN, BK = MOE_GEMM_BK;
    constexpr int WM = BM == 128 ? 2 : 1, WN = 4 / WM;          // waves along the rows | the columns of the tile
    constexpr int MB = BM / (32 * WM), NB = BN / (32 * WN);      // 32 x 32 blocks a wave owns: 2 x 2 | 1 x 1
    constexpr int X_BYTES = BM * BK * 2, W_BYTES = BN * BK * 2, STAGE = X_BYTES + W_BYTES;
    constexpr int XCH = X_BYTES / 1024 / 4, WCH = W_BYTES / 1024 / 4;   // 1 KiB LDS-DMA instructions a wave issues per operand
    static_assert(XCH >= 1 && WCH == 4, "tile shapes");
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, g = lane >> 5;
    const int M = (int)s.rows, N = s.n, K = s.k, nE = s.num_experts;
    const GemmTile tl = find_tile<BM>(static_cast<const int32_t*>(s.expert_offsets), nE, M, (int)blockIdx.x, lane);
    if (!tl.valid) return;
    const int seg = tl.seg, m0 = tl.m0, m_end = tl.m_end;
    const int n0 = (int)blockIdx.y * BN;
    uint16_t* const outp = static_cast<uint16_t*>(s.out);

    if (seg == nE) {
        // rows behind every segment: +0, 16 bytes a thread
        for (int c = tid; c < BM * (BN / 8); c += GEMM_THREADS) {
            const int m = m0 + c / (BN / 8), n = n0 + (c % (BN / 8)) * 8;
            if (m < m_end && n < N) *reinterpret_cast<u32x4*>(outp + (int64_t)m * s.out_row_stride + n) = u32x4{0u, 0u, 0u, 0u};
        }
        return;
    }

    const int wm_base = (wave / WN) * (MB * 32), wn_base = (wave % WN) * (NB * 32);
    const uint64_t w_at = reinterpret_cast<uint64_t>(s.w) + (uint64_t)((int64_t)seg * s.w_expert_stride * 2);   // this expert's slab
    const int64_t w_bytes = (int64_t)N * K * 2;
    const uint64_t x_at = reinterpret_cast<uint64_t>(s.x);
    const int64_t x_bytes = GATHER ? 0 : ((int64_t)(M - 1) * s.x_row_stride + K) * 2;

    // ---- lane maps of the loads: instruction `inst` fills 1 KiB, lane-linear; the swizzle is applied to the SOURCE column ----
    uint32_t x_voff[XCH], w_voff[WCH];
    int x_col[XCH], w_key[WCH];                                  // x, "nk" w: the lane's first k in the step; "kn" w: its k row
    const uint16_t* x_row[GATHER ? XCH : 1];
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
        const int inst = wave * XCH + i, row = inst * 8 + lane / 8;
        const int cb = swz_row_off<BK>(row, (lane % 8) * 16) - row * BK * 2;          // logical byte column
        x_col[i] = cb / 2;
        const bool live = m0 + row < m_end;
        if constexpr (GATHER) {
            x_row[i] = nullptr;
            if (live) {
                const uint32_t slot = (uint32_t)static_cast<const int32_t*>(s.sorted_slot)[m0 + row];
                if (slot < (uint32_t)(s.tokens * s.top_k))
                    x_row[i] = static_cast<const uint16_t*>(s.x) + (int64_t)(slot / (uint32_t)s.top_k) * s.x_row_stride + cb / 2;
            }
            x_voff[i] = 0;
        } else {
            x_voff[i] = live ? (uint32_t)((int64_t)row * s.x_row_stride * 2 + cb) : kOobVoff;
        }
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
        const int inst = wave * WCH + i;
        if constexpr (KN) {
            const int row = inst * 4 + lane / 16;                                     // k within the step
            const int cb = swzt_row_off<BN>(row, (lane % 16) * 16) - row * BN * 2;    // logical byte column: n within the tile
            w_key[i] = row;
            w_voff[i] = n0 + cb / 2 < N ? (uint32_t)((int64_t)row * N * 2 + cb) : kOobVoff;
        } else {
            const int row = inst * 8 + lane / 8;                                      // n within the tile
            const int cb = swz_row_off<BK>(row, (lane % 8) * 16) - row * BK * 2;
            w_key[i] = cb / 2;
            w_voff[i] = n0 + row < N ? (uint32_t)((int64_t)row * K * 2 + cb) : kOobVoff;
        }
    }

    u32x4 xreg[GATHER ? XCH : 1];
    auto issue = [&](int k0, int stage) {
        char* base = smem + stage * STAGE;
        // w: "nk" from W_e[n0, k0], "kn" from W_e[k0, n0]
        const int64_t w_first = KN ? ((int64_t)k0 * N + n0) * 2 : ((int64_t)n0 * K + k0) * 2;
        const __amdgpu_buffer_rsrc_t wr = span_rsrc(w_at + (uint64_t)w_first, w_bytes - w_first);
#pragma unroll
        for (int i = 0; i < WCH; ++i)
            buf_load_lds_b128(wr, base + X_BYTES + (wave * WCH + i) * 1024, k0 + w_key[i] < K ? w_voff[i] : kOobVoff, 0);
        if constexpr (GATHER) {
#pragma unroll
            for (int i = 0; i < XCH; ++i) {
                xreg[i] = u32x4{0u, 0u, 0u, 0u};
                if (x_row[i] && k0 + x_col[i] < K) xreg[i] = *reinterpret_cast<const u32x4*>(x_row[i] + k0);
            }
        } else {
            const int64_t x_first = ((int64_t)m0 * s.x_row_stride + k0) * 2;
            const __amdgpu_buffer_rsrc_t xr = span_rsrc(x_at + (uint64_t)x_first, x_bytes - x_first);
#pragma unroll
            for (int i = 0; i < XCH; ++i)
                buf_load_lds_b128(xr, base + (wave * XCH + i) * 1024, k0 + x_col[i] < K ? x_voff[i] : kOobVoff, 0);
        }
    };
    auto land = [&](int stage) {                                 // gather: the rows fetched by `issue` go to their LDS-DMA places
        if constexpr (GATHER) {
#pragma unroll
            for (int i = 0; i < XCH; ++i) lds_write_b128(smem + stage * STAGE + (wave * XCH + i) * 1024 + lane * 16, xreg[i]);
        }
    };

    f32x16 acc[NB][MB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nb][mb][r] = 0.f;

    // lane-constant read addresses of the transposing read (fa_fwd.hip's V operand): row 4 g + (lane & 15) / 4 (+ 8), the lane's
    // 8-byte piece of the 64-byte column block
    const int t_rr = (lane & 15) >> 2, t_cb = (((lane >> 4) & 1) << 5) + ((lane & 3) << 3);
    const lds_char* w_tp[2][NB];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
            w_tp[h][nb] = lds_pin(smem + X_BYTES + (KN ? swzt_row_off<BN>(4 * g + t_rr + 8 * h, (wn_base + nb * 32) * 2 + t_cb) : 0));

    auto compute = [&](auto stage_c) {
        constexpr int stage = decltype(stage_c)::value;
        const char* sx = smem + stage * STAGE;
        const char* sw = sx + X_BYTES;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            u32x4 af[NB], bf[MB];
            if constexpr (KN) {
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    const int row = wm_base + mb * 32 + l31;
                    const u32x2 lo = *reinterpret_cast<const u32x2*>(sx + swz_row_off<BK>(row, 32 * ks) + 8 * g);
                    const u32x2 hi = *reinterpret_cast<const u32x2*>(sx + swz_row_off<BK>(row, 32 * ks + 16) + 8 * g);
                    bf[mb] = u32x4{lo[0], lo[1], hi[0], hi[1]};
                }
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const u32x2 v0 = lds_read_tr16_nw(w_tp[0][nb], stage * STAGE + 16 * ks * BN * 2);
                    const u32x2 v1 = lds_read_tr16_nw(w_tp[1][nb], stage * STAGE + 16 * ks * BN * 2);
                    af[nb] = u32x4{v0[0], v0[1], v1[0], v1[1]};
                }
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) lds_tr_wait(af[nb], 0);
            } else {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) af[nb] = lds_read_b128(sw + swz_row_off<BK>(wn_base + nb * 32 + l31, 32 * ks + 16 * g));
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) bf[mb] = lds_read_b128(sx + swz_row_off<BK>(wm_base + mb * 32 + l31, 32 * ks + 16 * g));
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = E::mfma(af[nb], bf[mb], acc[nb][mb]);
        }
    };

    // ---- the k loop: the loads of step t + 1 fly while step t is multiplied ----
    const int steps = (K + BK - 1) / BK;
    auto step = [&](auto stage_c, int t) {
        constexpr int stage = decltype(stage_c)::value;
        const bool more = t + 1 < steps;
        if (more) issue((t + 1) * BK, stage ^ 1);
        compute(stage_c);
        if (more) land(stage ^ 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the LDS-DMA of the next stage has landed
        __syncthreads();
    };
    issue(0, 0);
    land(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < steps; t += 2) {
        step(std::integral_constant<int, 0>{}, t);
        if (t + 1 < steps) step(std::integral_constant<int, 1>{}, t + 1);
    }

    // ---- epilogue: D[column (r & 3) + 8 (r >> 2) + 4 g][row l31]: + bias in fp32, one rounding, 16-byte stores ----
    const bool bias32 = s.bias_dtype == FA_FP32;
    auto bias_at = [&](int n) -> float {
        if (!s.bias || n >= N) return 0.f;
        const int64_t at = (int64_t)seg * N + n;
        if (bias32) return static_cast<const float*>(s.bias)[at];
        const uint32_t v = static_cast<const uint16_t*>(s.bias)[at];
        return E::lo(v);
    };
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int nb0 = n0 + wn_base + nb * 32;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float bv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) bv[j] = bias_at(nb0 + 16 * q + 8 * (j >> 2) + 4 * g + (j & 3));
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const f32x16& a = acc[nb][mb];
                const bool hb = s.bias != nullptr;
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = hb ? a[8 * q + j] + bv[j] : a[8 * q + j];
                // columns 16 q + 4 g + (0..3) in (a0, a1), 16 q + 8 + 4 g + (0..3) in (b0, b1); the swap with lane ^ 32 leaves
                // columns 16 q + 8 g + (0..7) in (a0, a1, b0, b1)
                uint32_t a0 = E::pack2(v[0], v[1]), a1 = E::pack2(v[2], v[3]), b0 = E::pack2(v[4], v[5]), b1 = E::pack2(v[6], v[7]);
                permlane32_swap(a0, b0);
                permlane32_swap(a1, b1);
                const int m = m0 + wm_base + mb * 32 + l31, n = nb0 + 16 * q + 8 * g;
                if (m < m_end && n < N) *reinterpret_cast<u32x4*>(outp + (int64_t)m * s.out_row_stride + n) = u32x4{a0, a1, b0, b1};
            }
        }
    }
}

template <typename T, int BM, bool KN>
void launch_g(const fa_moe_gemm_params& s, dim3 grid, hipStream_t stream) {
    if (s.sorted_slot) hipLaunchKernelGGL((moe_gemm_kernel<T, BM, KN, true>), grid, dim3(GEMM_THREADS), 0, stream, s);
    else hipLaunchKernelGGL((moe_gemm_kernel<T, BM, KN, false>), grid, dim3(GEMM_THREADS), 0, stream, s);
}
template <typename T, int BM>
void launch_l(const fa_moe_gemm_params& s, dim3 grid, hipStream_t stream) {
    if (s.layout == FA_MOE_W_KN) launch_g<T, BM, true>(s, grid, stream);
    else launch_g<T, BM, false>(s, grid, stream);
}
template <typename T>
void launch_t(const fa_moe_gemm_params& s, const MoeGemmPlan& pl, hipStream_t stream) {
    const dim3 grid((unsigned)pl.grid_m, (unsigned)pl.grid_n);
    if (pl.bm == MOE_GEMM_BM_DECODE) launch_l<T, MOE_GEMM_BM_DECODE>(s, grid, stream);
    else launch_l<T, MOE_GEMM_BM_WIDE>(s, grid, stream);
}

}  // namespace

void launch_moe_gemm(const fa_moe_gemm_params& s, hipStream_t stream) {
    const MoeGemmPlan pl = moe_gemm_plan(s.rows, s.n, s.k, s.num_experts, s.layout, s.dtype);
    if (s.dtype == FA_BF16) launch_t<bf16_tag>(s, pl, stream);
    else launch_t<fp16_tag>(s, pl, stream);
}

}  // namespace fa
