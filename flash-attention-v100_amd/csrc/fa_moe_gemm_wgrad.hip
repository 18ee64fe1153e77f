// fa_moe_gemm_wgrad.hip - the weight and bias gradients of the grouped expert GEMM (fa_moe_gemm_wgrad, include/fa_mi355.h).
//
//   dW_e[n, k] = round(sum_r float(dy[r, n]) * float(a_r[k]))  (+ the old dw with accumulate)   r in [expert_offsets[e], expert_offsets[e + 1])
//   dbias[e, n] = round(sum_r float(dy[r, n]))
//
// with a_r = x[r] or, with sorted_slot, x[sorted_slot[r] / top_k] (a slot outside [0, tokens * top_k): a row of +0, no address) -
// fa_moe_gemm's rule, so the gradient of a fused-gather layer needs no permuted copy of x.
//
// dW is dense: the grid is (ceil(n / 128), ceil(k / 128), E), known on the host.  One workgroup of four waves (2 x 2, 64 x 64
// each) owns one 128 x 128 tile of one expert's dW; the ragged dimension is the CONTRACTION, so there is no tile search and no
// straddling store.  A workgroup reads its two offsets, clamps them to [0, rows] and walks the segment from its first row in
// steps of 64 rows, two LDS stages:
//   dy   [64 r][128 n]  swzt_row_off<128>, LDS-DMA (rows at or behind the segment's end, columns >= n: the out-of-range offset)
//   x    [64 r][128 k]  the same image, LDS-DMA; gathered: ds_write_b128 from ordinary 16-byte loads through sorted_slot (the
//                       slots of the step after next are fetched one step ahead)
// Both are the forward's "kn" weight shape and both are read with the counted-wait transposing read, which names the 16 rows of
// an MFMA step in the same slot order for A and B.  The A operand's columns become the dimension a lane holds four consecutive
// elements of: x for "nk" (k contiguous in dw), dy for "kn" - the template parameter KN only swaps the two LDS regions.
// Every element is one chain of v_mfma_f32_32x32x16 from +0 over the segment's rows ascending; rows that are not the segment's
// are zero-filled by the loads, never loaded and masked.  An empty expert's workgroups store the +0 accumulators (accumulate:
// leave at once).  A buffer descriptor spans what is left of dy / x behind the step's first element, at most 2^31 - 1 bytes.
//
// dbias is a second, small launch (moe_dbias_kernel): a workgroup per (128 columns, expert); simpler than riding in the k-tile-0
// workgroups of the GEMM, whose LDS image is laid out for the transposing read.
#include "fa_common.h"
#include "fa_moe_gemm.h"
#include <type_traits>

namespace fa {

namespace {

constexpr int WGRAD_THREADS = 256;

// a descriptor over `bytes` (clamped to 2^31 - 1: kOobVoff is then always out of range) behind a wave-uniform address
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wgrad_span_rsrc(uint64_t at, int64_t bytes) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)at);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(at >> 32));
    const int64_t cl = bytes < 0 ? 0 : (bytes > 0x7fffffffLL ? 0x7fffffffLL : bytes);
    const uint32_t n = __builtin_amdgcn_readfirstlane((uint32_t)cl);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, (int)n, 0x00020000);
}

// the segment of expert e, clamped to [0, rows] (wave-uniform)
__device__ __forceinline__ void wgrad_segment(const void* offsets, int e, int M, int& lo, int& hi) {
    const int32_t* offs = static_cast<const int32_t*>(offsets);
    int a = offs[e], b = offs[e + 1];
    a = a < 0 ? 0 : (a > M ? M : a);
    b = b < 0 ? 0 : (b > M ? M : b);
    lo = __builtin_amdgcn_readfirstlane(a);
    hi = __builtin_amdgcn_readfirstlane(b);
}

template <typename T, bool KN, bool GATHER, bool OUT32>
__global__ void __launch_bounds__(WGRAD_THREADS) moe_gemm_wgrad_kernel(const fa_moe_gemm_wgrad_params s) {
    using E = Elem<T>;
    constexpr int BT = 128, BR = MOE_WGRAD_BR;                   // tile extent along n and along k | rows a step
    static_assert(MOE_WGRAD_BN == BT && MOE_WGRAD_BK == BT, "one LDS image for both operands");
    constexpr int OP_BYTES = BR * BT * 2, STAGE = 2 * OP_BYTES;  // dy at 0, x at OP_BYTES
    constexpr int CH = OP_BYTES / 1024 / 4;                      // 1 KiB LDS-DMA instructions a wave issues per operand
    constexpr int A_OP = KN ? 0 : 1, B_OP = 1 - A_OP;            // 0: dy, 1: x
    static_assert(CH == 4, "tile shapes");
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, g = lane >> 5;
    const int M = (int)s.rows, N = s.n, K = s.k;
    const int e = (int)blockIdx.z;
    int r_lo, r_hi;
    wgrad_segment(s.expert_offsets, e, M, r_lo, r_hi);
    const bool empty = r_hi <= r_lo;
    if (empty && s.accumulate) return;                           // (dw + 0 would turn a -0 into +0: left untouched)
    const int n0 = (int)blockIdx.x * BT, k0 = (int)blockIdx.y * BT;

    // ---- lane maps of the loads: instruction `inst` fills 1 KiB = 4 rows, lane-linear; the swizzle is applied to the SOURCE column ----
    uint32_t dy_voff[CH], x_voff[CH];
    int lrow[CH], lcol[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int inst = wave * CH + i, row = inst * 4 + lane / 16;
        const int cb = swzt_row_off<BT>(row, (lane % 16) * 16) - row * BT * 2;        // logical byte column
        lrow[i] = row;
        lcol[i] = cb / 2;
        dy_voff[i] = n0 + cb / 2 < N ? (uint32_t)((int64_t)row * s.dy_row_stride * 2 + cb) : kOobVoff;
        x_voff[i] = k0 + cb / 2 < K ? (uint32_t)((int64_t)row * s.x_row_stride * 2 + cb) : kOobVoff;
    }
    const uint64_t dy_at = reinterpret_cast<uint64_t>(s.dy), x_at = reinterpret_cast<uint64_t>(s.x);
    const int64_t dy_bytes = ((int64_t)(M - 1) * s.dy_row_stride + N) * 2;
    const int64_t x_bytes = GATHER ? 0 : ((int64_t)(M - 1) * s.x_row_stride + K) * 2;
    const uint32_t n_slots = (uint32_t)(s.tokens * s.top_k);

    uint32_t slot[GATHER ? CH : 1];
    auto fetch_slots = [&](int rs) {                             // the gather's slots of the step that begins at row rs
        if constexpr (GATHER) {
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int r = rs + lrow[i];
                slot[i] = r < r_hi ? (uint32_t)static_cast<const int32_t*>(s.sorted_slot)[r] : 0xffffffffu;
            }
        }
    };
    u32x4 xreg[GATHER ? CH : 1];
    auto issue = [&](int t, int stage) {
        char* base = smem + stage * STAGE;
        const int rs = r_lo + t * BR;
        const int64_t dy_first = ((int64_t)rs * s.dy_row_stride + n0) * 2;
        const __amdgpu_buffer_rsrc_t dr = wgrad_span_rsrc(dy_at + (uint64_t)dy_first, dy_bytes - dy_first);
#pragma unroll
        for (int i = 0; i < CH; ++i)
            buf_load_lds_b128(dr, base + (wave * CH + i) * 1024, rs + lrow[i] < r_hi ? dy_voff[i] : kOobVoff, 0);
        if constexpr (GATHER) {
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                xreg[i] = u32x4{0u, 0u, 0u, 0u};
                if (slot[i] < n_slots && k0 + lcol[i] < K)
                    xreg[i] = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(s.x) +
                                                              (int64_t)(slot[i] / (uint32_t)s.top_k) * s.x_row_stride + k0 + lcol[i]);
            }
            fetch_slots(rs + BR);
        } else {
            const int64_t x_first = ((int64_t)rs * s.x_row_stride + k0) * 2;
            const __amdgpu_buffer_rsrc_t xr = wgrad_span_rsrc(x_at + (uint64_t)x_first, x_bytes - x_first);
#pragma unroll
            for (int i = 0; i < CH; ++i)
                buf_load_lds_b128(xr, base + OP_BYTES + (wave * CH + i) * 1024, rs + lrow[i] < r_hi ? x_voff[i] : kOobVoff, 0);
        }
    };
    auto land = [&](int stage) {                                 // gather: the rows fetched by `issue` go to their LDS-DMA places
        if constexpr (GATHER) {
#pragma unroll
            for (int i = 0; i < CH; ++i) lds_write_b128(smem + stage * STAGE + OP_BYTES + (wave * CH + i) * 1024 + lane * 16, xreg[i]);
        }
    };

    f32x16 acc[2][2];                                            // [32 columns of the A operand][32 columns of the B operand]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    // lane-constant read addresses of the transposing read (fa_moe_gemm.hip's "kn" weight): row 4 g + (lane & 15) / 4 (+ 8), the
    // lane's 8-byte piece of the 64-byte column block.  The wave owns A columns wa .. wa + 63 and B columns wb .. wb + 63.
    const int wa = (wave & 1) * 64, wb = (wave >> 1) * 64;
    const int t_rr = (lane & 15) >> 2, t_cb = (((lane >> 4) & 1) << 5) + ((lane & 3) << 3);
    const lds_char* a_tp[2][2];
    const lds_char* b_tp[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            a_tp[h][blk] = lds_pin(smem + A_OP * OP_BYTES + swzt_row_off<BT>(4 * g + t_rr + 8 * h, (wa + blk * 32) * 2 + t_cb));
            b_tp[h][blk] = lds_pin(smem + B_OP * OP_BYTES + swzt_row_off<BT>(4 * g + t_rr + 8 * h, (wb + blk * 32) * 2 + t_cb));
        }

    auto compute = [&](auto stage_c) {
        constexpr int stage = decltype(stage_c)::value;
#pragma unroll
        for (int ks = 0; ks < BR / 16; ++ks) {
            const int off = stage * STAGE + 16 * ks * BT * 2;
            u32x4 af[2], bf[2];
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const u32x2 v0 = lds_read_tr16_nw(a_tp[0][blk], off);
                const u32x2 v1 = lds_read_tr16_nw(a_tp[1][blk], off);
                af[blk] = u32x4{v0[0], v0[1], v1[0], v1[1]};
            }
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const u32x2 v0 = lds_read_tr16_nw(b_tp[0][blk], off);
                const u32x2 v1 = lds_read_tr16_nw(b_tp[1][blk], off);
                bf[blk] = u32x4{v0[0], v0[1], v1[0], v1[1]};
            }
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) lds_tr_wait(af[blk], 0);
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) lds_tr_wait(bf[blk], 0);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = E::mfma(af[a], bf[b], acc[a][b]);
        }
    };

    // ---- the row loop: the loads of step t + 1 fly while step t is multiplied ----
    const int steps = empty ? 0 : (r_hi - r_lo + BR - 1) / BR;
    auto step = [&](auto stage_c, int t) {
        constexpr int stage = decltype(stage_c)::value;
        const bool more = t + 1 < steps;
        if (more) issue(t + 1, stage ^ 1);
        compute(stage_c);
        if (more) land(stage ^ 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the LDS-DMA of the next stage has landed
        __syncthreads();
    };
    if (steps > 0) {
        fetch_slots(r_lo);
        issue(0, 0);
        land(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int t = 0; t < steps; t += 2) {
            step(std::integral_constant<int, 0>{}, t);
            if (t + 1 < steps) step(std::integral_constant<int, 1>{}, t + 1);
        }
    }

    // ---- epilogue: D[A column (r & 3) + 8 (r >> 2) + 4 g][B column l31]; the A columns are contiguous in dw ----
    const int c_org = (KN ? n0 : k0) + wa, r_org = (KN ? k0 : n0) + wb;
    const int CN = KN ? N : K, RN = KN ? K : N;                  // dw_e is [RN][CN]
    const int64_t slab = (int64_t)e * s.dw_expert_stride;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const f32x16& d = acc[a][b];
            const int R = r_org + b * 32 + l31;
            if constexpr (OUT32) {
                float* const row = static_cast<float*>(s.dw) + slab + (int64_t)R * CN;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int C = c_org + a * 32 + 8 * p + 4 * g;
                    if (R < RN && C < CN) {
                        f32x4 v = {d[4 * p], d[4 * p + 1], d[4 * p + 2], d[4 * p + 3]};
                        if (s.accumulate) v = *reinterpret_cast<const f32x4*>(row + C) + v;
                        *reinterpret_cast<f32x4*>(row + C) = v;
                    }
                }
            } else {
                uint16_t* const row = static_cast<uint16_t*>(s.dw) + slab + (int64_t)R * CN;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    // columns 16 q + 4 g + (0..3) in (a0, a1), 16 q + 8 + 4 g + (0..3) in (b0, b1); the swap with lane ^ 32 leaves
                    // columns 16 q + 8 g + (0..7) in (a0, a1, b0, b1)
                    uint32_t a0 = E::pack2(d[8 * q], d[8 * q + 1]), a1 = E::pack2(d[8 * q + 2], d[8 * q + 3]);
                    uint32_t b0 = E::pack2(d[8 * q + 4], d[8 * q + 5]), b1 = E::pack2(d[8 * q + 6], d[8 * q + 7]);
                    permlane32_swap(a0, b0);
                    permlane32_swap(a1, b1);
                    const int C = c_org + a * 32 + 16 * q + 8 * g;
                    if (R < RN && C < CN) *reinterpret_cast<u32x4*>(row + C) = u32x4{a0, a1, b0, b1};
                }
            }
        }
    }
}

// dbias[e, n]: 16 row lanes x 16 column groups of 8.  Row lane j adds rows first + j, first + j + 16, .. in ascending order from
// +0; the 16 partial sums of a column are then added in ascending j from +0: an order that depends on the segment's length alone.
template <typename T>
__global__ void __launch_bounds__(WGRAD_THREADS) moe_dbias_kernel(const fa_moe_gemm_wgrad_params s) {
    using E = Elem<T>;
    __shared__ float part[16][128 + 4];
    const int tid = threadIdx.x, cg = tid & 15, rl = tid >> 4;
    const int M = (int)s.rows, N = s.n, e = (int)blockIdx.y;
    int r_lo, r_hi;
    wgrad_segment(s.expert_offsets, e, M, r_lo, r_hi);
    const int n = (int)blockIdx.x * 128 + cg * 8;
    float sum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sum[j] = 0.f;
    if (n < N) {
        const uint16_t* col = static_cast<const uint16_t*>(s.dy) + n;
        for (int r = r_lo + rl; r < r_hi; r += 16) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(col + (int64_t)r * s.dy_row_stride);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sum[2 * j] += E::lo(v[j]);
                sum[2 * j + 1] += E::hi(v[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) part[rl][cg * 8 + j] = sum[j];
    __syncthreads();
    const int c = (int)blockIdx.x * 128 + tid;
    if (tid < 128 && c < N) {
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) t += part[j][tid];
        const int64_t at = (int64_t)e * N + c;
        if (s.dbias_dtype == FA_FP32) static_cast<float*>(s.dbias)[at] = t;
        else static_cast<uint16_t*>(s.dbias)[at] = (uint16_t)E::pack2(t, 0.f);
    }
}

template <typename T, bool KN, bool GATHER>
void launch_o(const fa_moe_gemm_wgrad_params& s, dim3 grid, hipStream_t stream) {
    if (s.dw_dtype == FA_FP32) hipLaunchKernelGGL((moe_gemm_wgrad_kernel<T, KN, GATHER, true>), grid, dim3(WGRAD_THREADS), 0, stream, s);
    else hipLaunchKernelGGL((moe_gemm_wgrad_kernel<T, KN, GATHER, false>), grid, dim3(WGRAD_THREADS), 0, stream, s);
}
template <typename T, bool KN>
void launch_g(const fa_moe_gemm_wgrad_params& s, dim3 grid, hipStream_t stream) {
    if (s.sorted_slot) launch_o<T, KN, true>(s, grid, stream);
    else launch_o<T, KN, false>(s, grid, stream);
}
template <typename T>
void launch_t(const fa_moe_gemm_wgrad_params& s, hipStream_t stream) {
    if (s.dw) {
        const MoeWgradPlan pl = moe_gemm_wgrad_plan(s.n, s.k, s.num_experts, s.layout, s.dtype);
        const dim3 grid((unsigned)pl.grid_n, (unsigned)pl.grid_k, (unsigned)pl.grid_e);
        if (s.layout == FA_MOE_W_KN) launch_g<T, true>(s, grid, stream);
        else launch_g<T, false>(s, grid, stream);
    }
    if (s.dbias) {
        const dim3 grid((unsigned)((s.n + 127) / 128), (unsigned)s.num_experts);
        hipLaunchKernelGGL((moe_dbias_kernel<T>), grid, dim3(WGRAD_THREADS), 0, stream, s);
    }
}

}  // namespace

void launch_moe_gemm_wgrad(const fa_moe_gemm_wgrad_params& s, hipStream_t stream) {
    if (s.dtype == FA_BF16) launch_t<bf16_tag>(s, stream);
    else launch_t<fp16_tag>(s, stream);
}

}  // namespace fa
