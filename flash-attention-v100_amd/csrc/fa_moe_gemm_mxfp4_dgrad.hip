// fa_moe_gemm_mxfp4_dgrad.hip - the data gradient of the grouped expert GEMM on MXFP4 weights (fa_moe_gemm_mxfp4_dgrad,
// include/fa_mi355.h): the contraction runs over the ROWS of an "nk" MXFP4 weight.
//
//   dx[r, k] = round_bf16(sum_n float(dy[r, n]) * W_e[n, k])      for expert_offsets[e] <= r < expert_offsets[e + 1]
//   dx[r, :] = +0                                                  for expert_offsets[E] <= r < rows
//   W_e[n, k] = e2m1(w_blocks[e, n, k / 2] >> 4 (k & 1)) * 2^(w_scales[e, n, k / 32] - 127)
//
// An e2m1 value times a power of two is exact in bf16 (scale bytes 2 ... 252), so this is fa_moe_gemm's "kn" form on the
// dequantised [n][k] weights BIT FOR BIT as long as each MFMA sees the same operands in the same slots.  The tile shapes, the
// wave layout, the transposed product (A = weight, B = activation), the accumulator chain - v_mfma_f32_32x32x16 over n ascending
// in steps of 16 from +0 -, the transposing read and its slot order, the epilogue, the tile search and the bounded descriptors
// are therefore those of fa_moe_gemm.hip ("kn" form, plain); what differs is how the weight image gets into LDS.  The forward's
// way (fa_moe_gemm_mxfp4.hip: codes in LDS, converted in the operand registers) does not carry over: codes are packed two to a
// byte along k and a scale covers 32 k, and k is the OUTPUT dimension here - a transposing read of nibbles does not exist.
//
// Staging, BK = 64 contraction elements (weight rows n) a step, two LDS stages:
//   dy       [BM][64] bf16, swz_row_off<64>, LDS-DMA (rows at or behind the segment's end and columns >= n: the out-of-range
//            offset) - as fa_moe_gemm.hip stages x
//   weight   [64 n][128 k] bf16, swzt_row_off<128>: the very image the "kn" kernel's ds_read_b64_tr_b16 reads, built by
//            dequantising on the way in.  The step's codes are 64 rows of 64 bytes = 4 KiB: ONE 16-byte piece per lane - lane
//            (row = tid / 4, piece = tid % 4) holds the 32 k of one row that share ONE scale byte.  A lane issues its 16-byte
//            code load and its scale byte load for step t + 1 before step t's MFMAs and, behind them, turns each code dword into
//            8 bf16 (4 x v_cvt_scalef32_pk_bf16_fp4, byte b of the dword -> operand dword b: the storage order) and writes its
//            64 bytes with four ds_write_b128.  Global weight traffic stays at 17 / 32 byte a weight; the bf16 image exists in
//            LDS only.
// Tails: rows n >= N and pieces k >= K take the out-of-range offset in both loads - zero codes and scale byte 0, a finite scale
// (2^-127), give +0.  A descriptor never spans more than what is left of ONE expert's code or scale slab behind the step's first
// element (byte 255 is NaN even with a zero code, so a tail must never see another expert's scales) and never more than
// 2^31 - 1 bytes; an expert's base is a 64-bit pointer.
#include "fa_common.h"
#include "fa_moe_gemm.h"
#include "fa_moe_tile.h"
#include "fa_mx_cvt.h"
#include <type_traits>

namespace fa {

namespace {

template <int BM>
__device__ __forceinline__ void moe_mxfp4_dgrad_body(const fa_moe_gemm_mxfp4_dgrad_params& s) {
    using E = Elem<bf16_tag>;
    constexpr int BN = MOE_GEMM_BN, BK = MOE_GEMM_BK;            // output columns (k) of a tile | contraction elements (n) a step
    constexpr int WM = BM == 128 ? 2 : 1, WN = 4 / WM;          // waves along the rows | the columns of the tile
    constexpr int MB = BM / (32 * WM), NB = BN / (32 * WN);      // 32 x 32 blocks a wave owns: 2 x 2 | 1 x 1
    constexpr int X_BYTES = BM * BK * 2, W_BYTES = BN * BK * 2, STAGE = X_BYTES + W_BYTES;
    constexpr int XCH = X_BYTES / 1024 / 4;                      // 1 KiB LDS-DMA instructions a wave issues for dy
    static_assert(XCH >= 1 && BK * (BN / 32) == GEMM_THREADS, "tile shapes: one 32-k piece of the step's codes per lane");
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, g = lane >> 5;
    const int M = (int)s.rows, N = s.n, K = s.k, nE = s.num_experts;
    const GemmTile tl = find_tile<BM>(static_cast<const int32_t*>(s.expert_offsets), nE, M, (int)blockIdx.x, lane);
    if (!tl.valid) return;
    const int seg = tl.seg, m0 = tl.m0, m_end = tl.m_end;
    const int k0 = (int)blockIdx.y * BN;
    uint16_t* const outp = static_cast<uint16_t*>(s.dx);

    if (seg == nE) {
        // rows behind every segment: +0, 16 bytes a thread
        for (int c = tid; c < BM * (BN / 8); c += GEMM_THREADS) {
            const int m = m0 + c / (BN / 8), k = k0 + (c % (BN / 8)) * 8;
            if (m < m_end && k < K) *reinterpret_cast<u32x4*>(outp + (int64_t)m * s.dx_row_stride + k) = u32x4{0u, 0u, 0u, 0u};
        }
        return;
    }

    const int wm_base = (wave / WN) * (MB * 32), wn_base = (wave % WN) * (NB * 32);
    const int KB = K / 2, KG = K / 32;                           // bytes of a row of codes | of scales
    const uint64_t w_at = reinterpret_cast<uint64_t>(s.w_blocks) + (uint64_t)((int64_t)seg * s.w_blocks_expert_stride);
    const uint64_t c_at = reinterpret_cast<uint64_t>(s.w_scales) + (uint64_t)((int64_t)seg * s.w_scales_expert_stride);
    const int64_t w_bytes = (int64_t)N * KB, c_bytes = (int64_t)N * KG;          // this expert's slabs
    const uint64_t x_at = reinterpret_cast<uint64_t>(s.dy);
    const int64_t x_bytes = ((int64_t)(M - 1) * s.dy_row_stride + N) * 2;

    // ---- lane maps of the loads.  dy: instruction `inst` fills 1 KiB, lane-linear; the swizzle is applied to the SOURCE column ----
    uint32_t x_voff[XCH];
    int x_col[XCH];                                              // the lane's first n in the step
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
        const int inst = wave * XCH + i, row = inst * 8 + lane / 8;
        const int cb = swz_row_off<BK>(row, (lane % 8) * 16) - row * BK * 2;          // logical byte column
        x_col[i] = cb / 2;
        x_voff[i] = m0 + row < m_end ? (uint32_t)((int64_t)row * s.dy_row_stride * 2 + cb) : kOobVoff;
    }
    // the weight: row w_row of the step, the 32 k from k0 + 32 w_pc on; behind K: out of range in every step
    const int w_row = tid >> 2, w_pc = tid & 3;
    const bool w_live = k0 + 32 * w_pc < K;
    const uint32_t w_voff = w_live ? (uint32_t)(w_row * KB + 16 * w_pc) : kOobVoff;
    const uint32_t c_voff = w_live ? (uint32_t)(w_row * KG + w_pc) : kOobVoff;
    char* const w_dst = smem + X_BYTES + w_row * BN * 2;         // the lane's image row; its four 16-byte slots: w_slot ^ (i << 4)
    const int w_slot = swzt_row_off<BN>(w_row, 64 * w_pc) - w_row * BN * 2;

    u32x4 wq;                                                    // the lane's 32 codes of the step in flight
    uint32_t wsc;                                                // and their scale byte
    auto issue = [&](int n0, int stage) {
        char* base = smem + stage * STAGE;
        // codes and scales from W_e[n0, k0] to the end of the expert's slab
        const int64_t w_first = (int64_t)n0 * KB + k0 / 2, c_first = (int64_t)n0 * KG + k0 / 32;
        const __amdgpu_buffer_rsrc_t wr = span_rsrc(w_at + (uint64_t)w_first, w_bytes - w_first);
        const __amdgpu_buffer_rsrc_t cr = span_rsrc(c_at + (uint64_t)c_first, c_bytes - c_first);
        const bool live = n0 + w_row < N;
        wq = buf_load_b128(wr, live ? w_voff : kOobVoff, 0);
        wsc = __builtin_amdgcn_raw_buffer_load_b8(cr, live ? c_voff : kOobVoff, 0, 0);
        const int64_t x_first = ((int64_t)m0 * s.dy_row_stride + n0) * 2;
        const __amdgpu_buffer_rsrc_t xr = span_rsrc(x_at + (uint64_t)x_first, x_bytes - x_first);
#pragma unroll
        for (int i = 0; i < XCH; ++i)
            buf_load_lds_b128(xr, base + (wave * XCH + i) * 1024, n0 + x_col[i] < N ? x_voff[i] : kOobVoff, 0);
    };
    auto land = [&](int stage) {                                 // the codes fetched by `issue` become the lane's 64 bytes of the image
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_write_b128(w_dst + stage * STAGE + (w_slot ^ (i << 4)), dequant8(wq[i], wsc & 0xffu));
    };

    f32x16 acc[NB][MB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nb][mb][r] = 0.f;

    // lane-constant read addresses of the transposing read (fa_moe_gemm.hip's): row 4 g + (lane & 15) / 4 (+ 8), the lane's
    // 8-byte piece of the 64-byte column block
    const int t_rr = (lane & 15) >> 2, t_cb = (((lane >> 4) & 1) << 5) + ((lane & 3) << 3);
    const lds_char* w_tp[2][NB];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
            w_tp[h][nb] = lds_pin(smem + X_BYTES + swzt_row_off<BN>(4 * g + t_rr + 8 * h, (wn_base + nb * 32) * 2 + t_cb));

    auto compute = [&](auto stage_c) {
        constexpr int stage = decltype(stage_c)::value;
        const char* sx = smem + stage * STAGE;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            u32x4 af[NB], bf[MB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {                    // dy in the slot order of the transposing read: two 8-byte halves
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
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = E::mfma(af[nb], bf[mb], acc[nb][mb]);
        }
    };

    // ---- the n loop: the loads of step t + 1 fly while step t is multiplied ----
    const int steps = (N + BK - 1) / BK;
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

    // ---- epilogue (fa_moe_gemm.hip's, no bias): D[column (r & 3) + 8 (r >> 2) + 4 g][row l31]: one rounding, 16-byte stores ----
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int nb0 = k0 + wn_base + nb * 32;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const f32x16& a = acc[nb][mb];
                // columns 16 q + 4 g + (0..3) in (a0, a1), 16 q + 8 + 4 g + (0..3) in (b0, b1); the swap with lane ^ 32 leaves
                // columns 16 q + 8 g + (0..7) in (a0, a1, b0, b1)
                uint32_t a0 = E::pack2(a[8 * q], a[8 * q + 1]), a1 = E::pack2(a[8 * q + 2], a[8 * q + 3]);
                uint32_t b0 = E::pack2(a[8 * q + 4], a[8 * q + 5]), b1 = E::pack2(a[8 * q + 6], a[8 * q + 7]);
                permlane32_swap(a0, b0);
                permlane32_swap(a1, b1);
                const int m = m0 + wm_base + mb * 32 + l31, k = nb0 + 16 * q + 8 * g;
                if (m < m_end && k < K) *reinterpret_cast<u32x4*>(outp + (int64_t)m * s.dx_row_stride + k) = u32x4{a0, a1, b0, b1};
            }
        }
    }
}

template <int BM>
__global__ void __launch_bounds__(GEMM_THREADS) moe_mxfp4_dgrad_kernel(const fa_moe_gemm_mxfp4_dgrad_params s) {
    moe_mxfp4_dgrad_body<BM>(s);
}

}  // namespace

void launch_moe_gemm_mxfp4_dgrad(const fa_moe_gemm_mxfp4_dgrad_params& s, hipStream_t stream) {
    const MoeGemmPlan pl = moe_gemm_mxfp4_dgrad_plan(s.rows, s.n, s.k, s.num_experts);
    const dim3 grid((unsigned)pl.grid_m, (unsigned)pl.grid_n);
    if (pl.bm == MOE_GEMM_BM_DECODE)
        hipLaunchKernelGGL((moe_mxfp4_dgrad_kernel<MOE_GEMM_BM_DECODE>), grid, dim3(GEMM_THREADS), 0, stream, s);
    else
        hipLaunchKernelGGL((moe_mxfp4_dgrad_kernel<MOE_GEMM_BM_WIDE>), grid, dim3(GEMM_THREADS), 0, stream, s);
}

}  // namespace fa
