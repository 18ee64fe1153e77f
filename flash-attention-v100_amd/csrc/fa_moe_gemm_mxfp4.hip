// fa_moe_gemm_mxfp4.hip - the grouped expert GEMM on MXFP4 weights and bf16 activations (fa_moe_gemm_mxfp4, include/fa_mi355.h).
//
//   out[r, :] = round_bf16(sum_k float(a_r[k]) * W_e[:, k] (+ float(bias[e, :])))   for expert_offsets[e] <= r < expert_offsets[e + 1]
//   out[r, :] = +0                                                                   for expert_offsets[E] <= r < rows
//   W_e[n, k] = e2m1(w_blocks[e, n, k / 2] >> 4 (k & 1)) * 2^(w_scales[e, n, k / 32] - 127)
//
// An e2m1 value times a power of two is exact in bf16 (scale bytes 2 ... 252), so this is fa_moe_gemm on the dequantised weights
// BIT FOR BIT as long as each MFMA sees the same operands in the same slots.  The tile shapes, the wave layout, the transposed
// product (A = weight, B = activation), the accumulator chain - v_mfma_f32_32x32x16 over k ascending in steps of 16 from +0 -,
// the epilogue, the tile search and the bounded descriptors are therefore those of fa_moe_gemm.hip ("nk" form); what differs is
// how the A operand gets into its registers.
//
// Staging, two LDS stages of BK contraction elements - 256 in the decode plan (BM 32), 128 in the prefill plan (BM 128), see
// fa_moe_gemm.h:
//   x        [BM][BK] bf16, swz_row_off<BK>, LDS-DMA (gather: ds_write_b128 from 16-byte loads through sorted_slot)
//   codes    [128 n][BK / 2 bytes], swz_row_off<BK / 4> (a row of BK / 2 bytes is a 16-bit row of BK / 4), LDS-DMA with the
//            swizzle applied to the source column.  At BK 256 this is byte for byte the 16-bit kernel's [128][64] image, four
//            times the k per byte.  K is a multiple of 32, so a 16-byte piece is wholly inside or outside K: the tail is the
//            out-of-range offset, zero codes, +0 whatever the scale.
//   scales   never staged: a lane loads the BK / 32 bytes of its weight row with byte loads (rows of K / 32 bytes have no
//            alignment) through a descriptor over what is left of the expert's scale slab, a step ahead, into registers.
//            Groups at or behind K and rows at or behind N take the out-of-range offset: byte 0, a finite scale.  (Byte 255 is
//            NaN even with a zero code - tools/probes/probe_cvt_fp4.hip - so a tail must never see another expert's bytes.)
//
// The A operand of MFMA step ks: lane (l31, g) holds the 8 weights k = 16 ks + 8 g ... + 7 of row l31: ONE dword of codes.  A
// lane reads 16 bytes of its row at byte 32 j + 16 g - the k 64 j + 32 g ... + 31, dwords d0 ... d3 - and two v_permlane32_swap
// with its partner lane (d0 <-> d1, d2 <-> d3) leave the dwords of steps 4 j + (0, 1, 2, 3) in (d0, d2, d1, d3) of both lanes:
// a quarter of the 16-bit kernel's LDS reads.  v_cvt_scalef32_pk_bf16_fp4 then turns byte b of the dword into operand dword b:
// the low nibble becomes the low bf16 and byte_sel counts bytes from bit 0 (probed, same file), which is the storage order, so
// four converts with the group's scale (scale_byte << 23 as fp32) build the operand of fa_moe_gemm.hip.
#include "fa_common.h"
#include "fa_moe_gemm.h"
#include "fa_moe_tile.h"
#include <type_traits>

namespace fa {

namespace {

__device__ __forceinline__ uint32_t cvt_fp4x2(uint32_t w, float scale, std::integral_constant<int, 0>) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0));
}
__device__ __forceinline__ uint32_t cvt_fp4x2(uint32_t w, float scale, std::integral_constant<int, 1>) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1));
}
__device__ __forceinline__ uint32_t cvt_fp4x2(uint32_t w, float scale, std::integral_constant<int, 2>) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2));
}
__device__ __forceinline__ uint32_t cvt_fp4x2(uint32_t w, float scale, std::integral_constant<int, 3>) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
}
// 8 codes (one dword, element i in nibble i) times 2^(scale_byte - 127) -> the 8 bf16 of an MFMA operand
__device__ __forceinline__ u32x4 dequant8(uint32_t w, uint32_t scale_byte) {
    const float sc = __builtin_bit_cast(float, scale_byte << 23);
    return u32x4{cvt_fp4x2(w, sc, std::integral_constant<int, 0>{}), cvt_fp4x2(w, sc, std::integral_constant<int, 1>{}),
                 cvt_fp4x2(w, sc, std::integral_constant<int, 2>{}), cvt_fp4x2(w, sc, std::integral_constant<int, 3>{})};
}

template <int BM, bool GATHER>
__global__ void __launch_bounds__(GEMM_THREADS) __attribute__((amdgpu_waves_per_eu(2))) moe_mxfp4_kernel(const fa_moe_gemm_mxfp4_params s) {
    using E = Elem<bf16_tag>;
    constexpr int BN = MOE_GEMM_BN, BK = BM == MOE_GEMM_BM_DECODE ? MOE_GEMM_MXFP4_BK : MOE_GEMM_MXFP4_BK_WIDE;
    constexpr int WM = BM == 128 ? 2 : 1, WN = 4 / WM;          // waves along the rows | the columns of the tile
    constexpr int MB = BM / (32 * WM), NB = BN / (32 * WN);      // 32 x 32 blocks a wave owns: 2 x 2 | 1 x 1
    constexpr int XROWB = BK * 2, WROWB = BK / 2;                // bytes of a staged row: bf16 x | e2m1 codes
    constexpr int X_BYTES = BM * XROWB, W_BYTES = BN * WROWB, STAGE = X_BYTES + W_BYTES;
    constexpr int XCH = X_BYTES / 1024 / 4, WCH = W_BYTES / 1024 / 4;   // 1 KiB LDS-DMA instructions a wave issues per operand
    constexpr int XLPR = XROWB / 16, WLPR = WROWB / 16;          // lanes (16-byte pieces) per staged row
    constexpr int NG = BK / 32;                                  // scale groups per step
    static_assert(XCH >= 1 && WCH >= 1 && 64 % XLPR == 0 && 64 % WLPR == 0 && BK % 64 == 0, "tile shapes");
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
    const int KB = K / 2, KG = K / 32;                           // bytes of a row of codes | of scales
    const uint64_t w_at = reinterpret_cast<uint64_t>(s.w_blocks) + (uint64_t)((int64_t)seg * s.w_blocks_expert_stride);
    const uint64_t c_at = reinterpret_cast<uint64_t>(s.w_scales) + (uint64_t)((int64_t)seg * s.w_scales_expert_stride);
    const int64_t w_bytes = (int64_t)N * KB, c_bytes = (int64_t)N * KG;          // this expert's slabs
    const uint64_t x_at = reinterpret_cast<uint64_t>(s.x);
    const int64_t x_bytes = GATHER ? 0 : ((int64_t)(M - 1) * s.x_row_stride + K) * 2;

    // ---- lane maps of the loads: instruction `inst` fills 1 KiB, lane-linear; the swizzle is applied to the SOURCE column ----
    uint32_t x_voff[XCH], w_voff[WCH], c_voff[NB];
    int w_key[WCH];                                              // the lane's first k in the step
    // x: the same for instruction i is x_col(i).  Rows of >= 256 bytes are swizzled with row & 15, instruction i holds the rows
    // (wave XCH + i) (64 / XLPR) + lane / XLPR, and i (64 / XLPR) never carries into the other two terms: one register, not XCH
    static_assert(XLPR >= 16 && (XCH * (64 / XLPR)) % 8 == 0 && XCH * (64 / XLPR) <= 32, "x_col's XOR form");
    int x_col0 = 0;
    auto x_col = [&](int i) { return x_col0 ^ (((i * (64 / XLPR)) & 15) * 8); };
    int x_tok[GATHER ? XCH : 1];                                 // gather: the lane's source row (token), -1: a row of +0
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
        const int inst = wave * XCH + i, row = inst * (64 / XLPR) + lane / XLPR;
        const int cb = swz_row_off<BK>(row, (lane % XLPR) * 16) - row * XROWB;        // logical byte column
        if (i == 0) x_col0 = cb / 2;
        const bool live = m0 + row < m_end;
        if constexpr (GATHER) {
            x_tok[i] = -1;
            if (live) {
                const uint32_t slot = (uint32_t)static_cast<const int32_t*>(s.sorted_slot)[m0 + row];
                if (slot < (uint32_t)(s.tokens * s.top_k)) x_tok[i] = (int)(slot / (uint32_t)s.top_k);
            }
            x_voff[i] = 0;
        } else {
            x_voff[i] = live ? (uint32_t)((int64_t)row * s.x_row_stride * 2 + cb) : kOobVoff;
        }
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
        const int inst = wave * WCH + i, row = inst * (64 / WLPR) + lane / WLPR;      // n within the tile
        const int cb = swz_row_off<BK / 4>(row, (lane % WLPR) * 16) - row * WROWB;    // logical byte column: 32 codes
        w_key[i] = cb * 2;
        w_voff[i] = n0 + row < N ? (uint32_t)((int64_t)row * KB + cb) : kOobVoff;
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {                            // the scale row of the lane's weight row in block nb
        const int row = wn_base + nb * 32 + l31;
        c_voff[nb] = n0 + row < N ? (uint32_t)((int64_t)row * KG) : kOobVoff;
    }

    u32x4 xreg[GATHER ? XCH : 1];
    uint32_t sc[2][NB][NG];                                      // scale bytes, [stage]
    auto issue = [&](int k0, auto stage_c) {
        constexpr int stage = decltype(stage_c)::value;
        char* base = smem + stage * STAGE;
        const int64_t w_first = (int64_t)n0 * KB + k0 / 2;
        const __amdgpu_buffer_rsrc_t wr = span_rsrc(w_at + (uint64_t)w_first, w_bytes - w_first);
#pragma unroll
        for (int i = 0; i < WCH; ++i)
            buf_load_lds_b128(wr, base + X_BYTES + (wave * WCH + i) * 1024, k0 + w_key[i] < K ? w_voff[i] : kOobVoff, 0);
        const int64_t c_first = (int64_t)n0 * KG + k0 / 32;
        const __amdgpu_buffer_rsrc_t cr = span_rsrc(c_at + (uint64_t)c_first, c_bytes - c_first);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int j = 0; j < NG; ++j)
                sc[stage][nb][j] = __builtin_amdgcn_raw_buffer_load_b8(cr, k0 + 32 * j < K ? c_voff[nb] + (uint32_t)j : kOobVoff, 0, 0);
        if constexpr (GATHER) {
#pragma unroll
            for (int i = 0; i < XCH; ++i) {
                xreg[i] = u32x4{0u, 0u, 0u, 0u};
                if (x_tok[i] >= 0 && k0 + x_col(i) < K)
                    xreg[i] = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(s.x) + (int64_t)x_tok[i] * s.x_row_stride + k0 + x_col(i));
            }
        } else {
            const int64_t x_first = ((int64_t)m0 * s.x_row_stride + k0) * 2;
            const __amdgpu_buffer_rsrc_t xr = span_rsrc(x_at + (uint64_t)x_first, x_bytes - x_first);
#pragma unroll
            for (int i = 0; i < XCH; ++i)
                buf_load_lds_b128(xr, base + (wave * XCH + i) * 1024, k0 + x_col(i) < K ? x_voff[i] : kOobVoff, 0);
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

    auto compute = [&](auto stage_c) {
        constexpr int stage = decltype(stage_c)::value;
        const char* sx = smem + stage * STAGE;
        const char* sw = sx + X_BYTES;
#pragma unroll
        for (int j = 0; j < BK / 64; ++j) {
            // 64 k: the lane's 16 bytes of codes per block, exchanged so that (d0, d2, d1, d3) are its dwords of steps 4 j + 0 ... 3
            uint32_t wd[NB][4];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const u32x4 q = lds_read_b128(sw + swz_row_off<BK / 4>(wn_base + nb * 32 + l31, 32 * j + 16 * g));
                uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3];
                permlane32_swap(d0, d1);
                permlane32_swap(d2, d3);
                wd[nb][0] = d0, wd[nb][1] = d2, wd[nb][2] = d1, wd[nb][3] = d3;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ks = 4 * j + q;
                u32x4 af[NB], bf[MB];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) af[nb] = dequant8(wd[nb][q], sc[stage][nb][ks / 2]);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) bf[mb] = lds_read_b128(sx + swz_row_off<BK>(wm_base + mb * 32 + l31, 32 * ks + 16 * g));
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = E::mfma(af[nb], bf[mb], acc[nb][mb]);
            }
        }
    };

    // ---- the k loop: the loads of step t + 1 fly while step t is multiplied ----
    const int steps = (K + BK - 1) / BK;
    auto step = [&](auto stage_c, int t) {
        constexpr int stage = decltype(stage_c)::value;
        const bool more = t + 1 < steps;
        if (more) issue((t + 1) * BK, std::integral_constant<int, stage ^ 1>{});
        compute(stage_c);
        if (more) land(stage ^ 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the LDS-DMA of the next stage has landed
        __syncthreads();
    };
    issue(0, std::integral_constant<int, 0>{});
    land(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < steps; t += 2) {
        step(std::integral_constant<int, 0>{}, t);
        if (t + 1 < steps) step(std::integral_constant<int, 1>{}, t + 1);
    }

    // ---- epilogue (fa_moe_gemm.hip's): D[column (r & 3) + 8 (r >> 2) + 4 g][row l31]: + bias in fp32, one rounding, 16-byte stores ----
    const bool bias32 = s.bias_dtype == FA_FP32, hb = s.bias != nullptr;
    auto bias_at = [&](int n) -> float {
        if (!hb || n >= N) return 0.f;
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

template <int BM>
void launch_g(const fa_moe_gemm_mxfp4_params& s, dim3 grid, hipStream_t stream) {
    if (s.sorted_slot) hipLaunchKernelGGL((moe_mxfp4_kernel<BM, true>), grid, dim3(GEMM_THREADS), 0, stream, s);
    else hipLaunchKernelGGL((moe_mxfp4_kernel<BM, false>), grid, dim3(GEMM_THREADS), 0, stream, s);
}

}  // namespace

void launch_moe_gemm_mxfp4(const fa_moe_gemm_mxfp4_params& s, hipStream_t stream) {
    const MoeGemmPlan pl = moe_gemm_mxfp4_plan(s.rows, s.n, s.k, s.num_experts);
    const dim3 grid((unsigned)pl.grid_m, (unsigned)pl.grid_n);
    if (pl.bm == MOE_GEMM_BM_DECODE) launch_g<MOE_GEMM_BM_DECODE>(s, grid, stream);
    else launch_g<MOE_GEMM_BM_WIDE>(s, grid, stream);
}

}  // namespace fa
