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
//
// fa_moe_gemm_mxfp4_glu (GLU 1, 2): the same body over a gate-up weight of 2 n rows, writing out[r, j] = round_bf16(act(g, u)) with
// g, u = the gate and up elements of output column j exactly as fa_moe_gemm_mxfp4 would have stored them - the same chains, the
// bias, ONE rounding to bf16 - widened again (include/fa_mi355.h has the arithmetic, fa_act.h its one definition).  A tile is
// BM x 64 OUTPUT columns over a 128-row weight image; the k loop is untouched.  What GLU changes is which weight row an MFMA
// operand row is, and the epilogue:
//   operand rows   operand row c of the tile (c = 32 B + l31, B the 32-row block) is the GATE of output column n0 + (c >> 1) for
//                  even c and its UP for odd c, in both forms.  In D[column (r & 3) + 8 (r >> 2) + 4 g][row l31] the registers
//                  r, r + 1 (r even) of ONE lane are then g and u of one element: no exchange pairs them, in either plan.
//   interleaved    weight row 2 j is the gate of column j, 2 j + 1 its up: operand row c is weight row 2 n0 + c, so the staged
//                  image, the lane maps and the scale rows are the plain kernel's over 2 n rows.
//   packed         gates are weight rows [0, n), ups [n, 2 n).  The image holds, per block B, 16 gate rows at LDS rows 32 B + t
//                  and the 16 matching up rows at 32 B + 16 + t, t = 0 ... 15: an LDS-DMA instruction (8 or 16 LDS rows) lies
//                  wholly in one half and goes through THAT half's descriptor - gate: rows [n0, n), up: rows [n + n0, 2 n) of the
//                  expert's slab - so a column tail never reads the other half or the next expert.  Row t holds output column
//                  n0 + 16 B + t in the gate half and n0 + 16 B + (t ^ 8) in the up half: the 16 lanes of a ds_read_b128
//                  phase (operand rows 16 h ... 16 h + 15: 8 gates, 8 ups) then read 16 different LDS rows mod 16, which is
//                  what the swizzle needs to stay conflict free.  A lane's scale bytes come through the descriptor of its
//                  row's half: two byte loads, one of them at the out-of-range offset (0), or-ed.
//   epilogue       h = pack2(acc[r] + bias, acc[r + 1] + bias): the bits of fa_moe_gemm_mxfp4.  out = act(lo(h), hi(h)), packed
//                  in pairs of adjacent columns: a lane holds columns 2 g + (0, 1) + 4 p, p = 0 ... 3, of the block's 16, and two
//                  v_permlane32_swap (p 0 <-> 2, 1 <-> 3) leave columns 8 g ... 8 g + 7: one 16-byte store a block.  The
//                  activation is a wave-uniform run-time switch around the epilogue.
#include "fa_common.h"
#include "fa_act.h"
#include "fa_moe_gemm.h"
#include "fa_moe_tile.h"
#include "fa_mx_cvt.h"
#include <type_traits>

namespace fa {

namespace {

// (cvt_fp4x2 and dequant8 - 8 codes times 2^(scale_byte - 127) -> the 8 bf16 of an MFMA operand: fa_mx_cvt.h)
// The one body of fa_moe_gemm_mxfp4's kernels (GLU 0: P = fa_moe_gemm_mxfp4_params) and fa_moe_gemm_mxfp4_glu's (GLU 1: interleaved,
// GLU 2: packed gate / up rows; P = fa_moe_gemm_mxfp4_glu_params, whose n counts OUTPUT columns).  With GLU 0 every
// `if constexpr (GLU ...)` falls away and the four kernels are what they were.
template <int BM, bool GATHER, int GLU, typename P>
__device__ __forceinline__ void moe_mxfp4_body(const P& s) {
    using E = Elem<bf16_tag>;
    constexpr int BN = MOE_GEMM_BN, BK = BM == MOE_GEMM_BM_DECODE ? MOE_GEMM_MXFP4_BK : MOE_GEMM_MXFP4_BK_WIDE;
    constexpr int WM = BM == 128 ? 2 : 1, WN = 4 / WM;          // waves along the rows | the columns of the tile
    constexpr int MB = BM / (32 * WM), NB = BN / (32 * WN);      // 32 x 32 blocks a wave owns: 2 x 2 | 1 x 1
    constexpr int XROWB = BK * 2, WROWB = BK / 2;                // bytes of a staged row: bf16 x | e2m1 codes
    constexpr int X_BYTES = BM * XROWB, W_BYTES = BN * WROWB, STAGE = X_BYTES + W_BYTES;
    constexpr int XCH = X_BYTES / 1024 / 4, WCH = W_BYTES / 1024 / 4;   // 1 KiB LDS-DMA instructions a wave issues per operand
    constexpr int XLPR = XROWB / 16, WLPR = WROWB / 16;          // lanes (16-byte pieces) per staged row
    constexpr int NG = BK / 32;                                  // scale groups per step
    constexpr int BNO = GLU ? MOE_GEMM_MXFP4_GLU_BN : BN;        // output columns of a tile
    constexpr int NSPAN = GLU == 2 ? 2 : 1;                      // spans of the expert's slabs a tile stages: packed: gate | up
    static_assert(XCH >= 1 && WCH >= 1 && 64 % XLPR == 0 && 64 % WLPR == 0 && BK % 64 == 0, "tile shapes");
    static_assert(WCH * (64 / WLPR) == 32 && 64 / WLPR <= 16, "a wave stages one 32-row block; an instruction lies in one 16-row half");
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, g = lane >> 5;
    const int M = (int)s.rows, N = s.n, K = s.k, nE = s.num_experts;
    const GemmTile tl = find_tile<BM>(static_cast<const int32_t*>(s.expert_offsets), nE, M, (int)blockIdx.x, lane);
    if (!tl.valid) return;
    const int seg = tl.seg, m0 = tl.m0, m_end = tl.m_end;
    const int n0 = (int)blockIdx.y * BNO;
    uint16_t* const outp = static_cast<uint16_t*>(s.out);

    if (seg == nE) {
        // rows behind every segment: +0, 16 bytes a thread
        for (int c = tid; c < BM * (BNO / 8); c += GEMM_THREADS) {
            const int m = m0 + c / (BNO / 8), n = n0 + (c % (BNO / 8)) * 8;
            if (m < m_end && n < N) *reinterpret_cast<u32x4*>(outp + (int64_t)m * s.out_row_stride + n) = u32x4{0u, 0u, 0u, 0u};
        }
        return;
    }

    const int wm_base = (wave / WN) * (MB * 32), wn_base = (wave % WN) * (NB * 32);
    const int KB = K / 2, KG = K / 32;                           // bytes of a row of codes | of scales
    const uint64_t w_at = reinterpret_cast<uint64_t>(s.w_blocks) + (uint64_t)((int64_t)seg * s.w_blocks_expert_stride);
    const uint64_t c_at = reinterpret_cast<uint64_t>(s.w_scales) + (uint64_t)((int64_t)seg * s.w_scales_expert_stride);
    const int NR = GLU ? 2 * N : N;                              // weight rows of an expert
    const int wrow0 = GLU == 1 ? 2 * n0 : n0;                    // the first weight row of the tile (packed: of its gate span)
    const int64_t w_bytes = (int64_t)NR * KB, c_bytes = (int64_t)NR * KG;        // this expert's slabs
    // packed: LDS row R of the image is row `rel` of the span of half (R >> 4) & 1, live while its output column n0 + rel < n
    auto packed_rel = [](int R) { return (R >> 5) * 16 + ((R & 15) ^ (((R >> 4) & 1) * 8)); };
    // packed: where operand row c - the gate (c even) or up (c odd) of tile column c >> 1 - lies in the image
    auto lds_row = [](int c) {
        if constexpr (GLU == 2) return (c & ~31) + (c & 1) * 16 + (((c >> 1) & 15) ^ ((c & 1) * 8));
        else return c;
    };
    const uint64_t x_at = reinterpret_cast<uint64_t>(s.x);
    const int64_t x_bytes = GATHER ? 0 : ((int64_t)(M - 1) * s.x_row_stride + K) * 2;

    // ---- lane maps of the loads: instruction `inst` fills 1 KiB, lane-linear; the swizzle is applied to the SOURCE column ----
    uint32_t x_voff[XCH], w_voff[WCH], c_voff[NB][NSPAN];
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
        if constexpr (GLU == 2) w_voff[i] = n0 + packed_rel(row) < N ? (uint32_t)((int64_t)packed_rel(row) * KB + cb) : kOobVoff;
        else w_voff[i] = wrow0 + row < NR ? (uint32_t)((int64_t)row * KB + cb) : kOobVoff;
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {                            // the scale row of the lane's weight row in block nb
        const int row = wn_base + nb * 32 + l31;
        if constexpr (GLU == 2) {                                // the lane's half alone is in range
            const int rel = packed_rel(lds_row(row));
#pragma unroll
            for (int h = 0; h < 2; ++h) c_voff[nb][h] = (row & 1) == h && n0 + rel < N ? (uint32_t)((int64_t)rel * KG) : kOobVoff;
        } else {
            c_voff[nb][0] = wrow0 + row < NR ? (uint32_t)((int64_t)row * KG) : kOobVoff;
        }
    }

    u32x4 xreg[GATHER ? XCH : 1];
    uint32_t sc[2][NB][NG];                                      // scale bytes, [stage]
    auto issue = [&](int k0, auto stage_c) {
        constexpr int stage = decltype(stage_c)::value;
        char* base = smem + stage * STAGE;
        // span h: from the tile's first row of that half to the end of the half (packed) or of the expert's slab
        __amdgpu_buffer_rsrc_t wr[NSPAN], cr[NSPAN];
#pragma unroll
        for (int h = 0; h < NSPAN; ++h) {
            const int64_t w_first = (int64_t)(wrow0 + h * N) * KB + k0 / 2;
            wr[h] = span_rsrc(w_at + (uint64_t)w_first, (GLU == 2 ? (int64_t)(h + 1) * N * KB : w_bytes) - w_first);
        }
#pragma unroll
        for (int i = 0; i < WCH; ++i)                            // (packed: instruction i lies in half (8 or 16) i / 16 % 2)
            buf_load_lds_b128(wr[GLU == 2 ? i * (64 / WLPR) / 16 % 2 : 0], base + X_BYTES + (wave * WCH + i) * 1024,
                              k0 + w_key[i] < K ? w_voff[i] : kOobVoff, 0);
#pragma unroll
        for (int h = 0; h < NSPAN; ++h) {
            const int64_t c_first = (int64_t)(wrow0 + h * N) * KG + k0 / 32;
            cr[h] = span_rsrc(c_at + (uint64_t)c_first, (GLU == 2 ? (int64_t)(h + 1) * N * KG : c_bytes) - c_first);
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                uint32_t b = __builtin_amdgcn_raw_buffer_load_b8(cr[0], k0 + 32 * j < K ? c_voff[nb][0] + (uint32_t)j : kOobVoff, 0, 0);
                if constexpr (GLU == 2)
                    b |= __builtin_amdgcn_raw_buffer_load_b8(cr[1], k0 + 32 * j < K ? c_voff[nb][1] + (uint32_t)j : kOobVoff, 0, 0);
                sc[stage][nb][j] = b;
            }
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
                const u32x4 q = lds_read_b128(sw + swz_row_off<BK / 4>(lds_row(wn_base + nb * 32 + l31), 32 * j + 16 * g));
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
    if constexpr (GLU != 0) {
        // ---- the gated epilogue: registers 2 p, 2 p + 1 are the gate and up of the block's output column (p & 1) + 4 (p >> 1) + 2 g ----
        auto bias_glu = [&](int up, int oc) -> float {           // the bias of output column oc's gate or up; columns >= n: +0, never read
            if (!hb || oc >= N) return 0.f;
            const int64_t at = (int64_t)seg * NR + (GLU == 1 ? 2 * oc + up : up * N + oc);
            if (bias32) return static_cast<const float*>(s.bias)[at];
            const uint32_t v = static_cast<const uint16_t*>(s.bias)[at];
            return E::lo(v);
        };
        const float alpha = s.alpha, limit = s.limit;
        auto gated = [&](auto act_c, uint32_t h) -> float {     // h: (g, u) as fa_moe_gemm_mxfp4 stores them
            constexpr int ACT = decltype(act_c)::value;
            if constexpr (ACT == FA_ACT_SWIGLU_OAI) {
                return act_swiglu_oai(E::lo(h), E::hi(h), alpha, limit);
            } else {
                float a, d;
                act_eval<ACT, false>(E::lo(h), a, d);
                return a * E::hi(h);
            }
        };
        auto epilogue = [&](auto act_c) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int oc0 = n0 + (wn_base + nb * 32) / 2;    // the block's 16 output columns
                float bv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) bv[r] = bias_glu(r & 1, oc0 + ((r >> 1) & 1) + 4 * (r >> 2) + 2 * g);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    const f32x16& a = acc[nb][mb];
                    float o[8];
#pragma unroll
                    for (int p = 0; p < 8; ++p)
                        o[p] = gated(act_c, hb ? E::pack2(a[2 * p] + bv[2 * p], a[2 * p + 1] + bv[2 * p + 1]) : E::pack2(a[2 * p], a[2 * p + 1]));
                    // columns 2 g + (0, 1) in p0, 4 + 2 g + (0, 1) in p1, 8 + .. in p2, 12 + .. in p3; the swaps with lane ^ 32
                    // leave columns 8 g + (0..7) in (p0, p2, p1, p3)
                    uint32_t p0 = E::pack2(o[0], o[1]), p1 = E::pack2(o[2], o[3]), p2 = E::pack2(o[4], o[5]), p3 = E::pack2(o[6], o[7]);
                    permlane32_swap(p0, p2);
                    permlane32_swap(p1, p3);
                    const int m = m0 + wm_base + mb * 32 + l31, n = oc0 + 8 * g;
                    if (m < m_end && n < N) *reinterpret_cast<u32x4*>(outp + (int64_t)m * s.out_row_stride + n) = u32x4{p0, p2, p1, p3};
                }
            }
        };
        switch (s.activation) {                                  // wave-uniform
            case FA_ACT_SILU: epilogue(std::integral_constant<int, FA_ACT_SILU>{}); break;
            case FA_ACT_RELU: epilogue(std::integral_constant<int, FA_ACT_RELU>{}); break;
            default:          epilogue(std::integral_constant<int, FA_ACT_SWIGLU_OAI>{}); break;
        }
        return;
    }
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

template <int BM, bool GATHER>
__global__ void __launch_bounds__(GEMM_THREADS) __attribute__((amdgpu_waves_per_eu(2))) moe_mxfp4_kernel(const fa_moe_gemm_mxfp4_params s) {
    moe_mxfp4_body<BM, GATHER, 0>(s);
}
template <int BM, bool GATHER, int GLU>
__global__ void __launch_bounds__(GEMM_THREADS) __attribute__((amdgpu_waves_per_eu(2))) moe_mxfp4_glu_kernel(const fa_moe_gemm_mxfp4_glu_params s) {
    moe_mxfp4_body<BM, GATHER, GLU>(s);
}

template <int BM>
void launch_g(const fa_moe_gemm_mxfp4_params& s, dim3 grid, hipStream_t stream) {
    if (s.sorted_slot) hipLaunchKernelGGL((moe_mxfp4_kernel<BM, true>), grid, dim3(GEMM_THREADS), 0, stream, s);
    else hipLaunchKernelGGL((moe_mxfp4_kernel<BM, false>), grid, dim3(GEMM_THREADS), 0, stream, s);
}
template <int BM, int GLU>
void launch_glu(const fa_moe_gemm_mxfp4_glu_params& s, dim3 grid, hipStream_t stream) {
    if (s.sorted_slot) hipLaunchKernelGGL((moe_mxfp4_glu_kernel<BM, true, GLU>), grid, dim3(GEMM_THREADS), 0, stream, s);
    else hipLaunchKernelGGL((moe_mxfp4_glu_kernel<BM, false, GLU>), grid, dim3(GEMM_THREADS), 0, stream, s);
}
template <int BM>
void launch_f(const fa_moe_gemm_mxfp4_glu_params& s, dim3 grid, hipStream_t stream) {
    if (s.gate_up == FA_MOE_GLU_INTERLEAVED) launch_glu<BM, 1>(s, grid, stream);
    else launch_glu<BM, 2>(s, grid, stream);
}

}  // namespace

void launch_moe_gemm_mxfp4_glu(const fa_moe_gemm_mxfp4_glu_params& s, hipStream_t stream) {
    const MoeGemmPlan pl = moe_gemm_mxfp4_glu_plan(s.rows, s.n, s.k, s.num_experts);
    const dim3 grid((unsigned)pl.grid_m, (unsigned)pl.grid_n);
    if (pl.bm == MOE_GEMM_BM_DECODE) launch_f<MOE_GEMM_BM_DECODE>(s, grid, stream);
    else launch_f<MOE_GEMM_BM_WIDE>(s, grid, stream);
}

void launch_moe_gemm_mxfp4(const fa_moe_gemm_mxfp4_params& s, hipStream_t stream) {
    const MoeGemmPlan pl = moe_gemm_mxfp4_plan(s.rows, s.n, s.k, s.num_experts);
    const dim3 grid((unsigned)pl.grid_m, (unsigned)pl.grid_n);
    if (pl.bm == MOE_GEMM_BM_DECODE) launch_g<MOE_GEMM_BM_DECODE>(s, grid, stream);
    else launch_g<MOE_GEMM_BM_WIDE>(s, grid, stream);
}

}  // namespace fa
