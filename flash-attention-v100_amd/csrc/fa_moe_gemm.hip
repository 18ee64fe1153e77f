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
//
// fa_moe_gemm_glu (GLU = true): the same body over a packed gate-up weight of 2 n columns, writing out[r, j] = round16(act(g) * u)
// with g, u = the two sums of output column j (+ bias), each ROUNDED to the io type first - the bits of fa_moe_gemm followed by
// fa_act_mul (fa_act.h's act_eval), without h.  A tile is BM x 64 OUTPUT columns over the same 128-wide weight image: tile column
// c < 64 is weight column n0 + c (gate), c >= 64 is n + n0 + (c - 64) (its up) - for "nk" a second source base for the LDS-DMA
// instructions of waves 2 - 3, for "kn" a per-lane source column; a column is out of range where n0 + c % 64 >= n, which masks a
// gate and its up together.  Wide plan: wave (wm, wn) takes the gate block at tile column 32 wn and the up block at 64 + 32 wn,
// so acc[0][mb] and acc[1][mb] hold g and u of one element in one lane and register and the epilogue is lane-local.  Decode
// plan: waves 0 - 1 hold gate blocks, waves 2 - 3 the up blocks; behind the k loop's last barrier the staging buffers are free,
// every wave writes its rounded block into a [32][128] image there and each lane then takes 8 gates and 8 ups of one row.  The
// activation is a wave-uniform run-time switch around the epilogue, not a template parameter.
#include "fa_common.h"
#include "fa_act.h"
#include "fa_moe_gemm.h"
#include "fa_moe_tile.h"
#include <type_traits>

namespace fa {

namespace {

// (fa_moe_gemm_mxfp4.hip holds a copy of this body's "nk" form - the +0 tail, the lane maps, issue / land / step and the
// epilogue - around another way of filling the A operand: a fix to one of them belongs in both files.)
// The one body of fa_moe_gemm's kernels (GLU false: P = fa_moe_gemm_params) and fa_moe_gemm_glu's (GLU true: P =
// fa_moe_gemm_glu_params, whose n counts OUTPUT columns).  GLU changes which weight rows / columns a tile stages and what the
// epilogue does with the accumulators, nothing else; with GLU false every `if constexpr (GLU)` falls away.
template <typename T, int BM, bool KN, bool GATHER, bool GLU, typename P>
__device__ __forceinline__ void moe_gemm_body(const P& s) {
    using E = Elem<T>;
    constexpr int BN = MOE_GEMM_BN, BK = MOE_GEMM_BK;
    constexpr int BNO = GLU ? MOE_GEMM_GLU_BN : BN;              // output columns of a tile; GLU: the weight image's halves pair up
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
    // the tile column of the wave's block nb.  GLU, wide: block 0 is the gate at 32 wn, block 1 its up at 64 + 32 wn, so that
    // acc[0][mb] and acc[1][mb] hold g and u of one element in one lane and register; GLU, decode: waves 0 - 1 gate, 2 - 3 up
    auto wcol = [&](int nb) { return GLU && NB == 2 ? (wave % WN) * 32 + nb * (BN / 2) : wn_base + nb * 32; };
    const uint64_t w_at = reinterpret_cast<uint64_t>(s.w) + (uint64_t)((int64_t)seg * s.w_expert_stride * 2);   // this expert's slab
    constexpr int NW = GLU ? 2 : 1;                              // weight columns per output column
    const int64_t w_bytes = (int64_t)N * K * 2 * NW;
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
            if constexpr (GLU) {
                // tile column c < 64: weight column n0 + c (gate); c >= 64: n + n0 + (c - 64) (its up), masked together
                const int c = cb / 2, half = c / BNO, cc = c % BNO;
                w_voff[i] = n0 + cc < N ? (uint32_t)((int64_t)row * N * 4 + (half * N + cc) * 2) : kOobVoff;
            } else {
                w_voff[i] = n0 + cb / 2 < N ? (uint32_t)((int64_t)row * N * 2 + cb) : kOobVoff;
            }
        } else {
            const int row = inst * 8 + lane / 8;                                      // n within the tile
            const int cb = swz_row_off<BK>(row, (lane % 8) * 16) - row * BK * 2;
            w_key[i] = cb / 2;
            if constexpr (GLU)                                                        // rows >= 64 (waves 2 - 3): the second source base of `issue`
                w_voff[i] = n0 + row % BNO < N ? (uint32_t)((int64_t)(row % BNO) * K * 2 + cb) : kOobVoff;
            else
                w_voff[i] = n0 + row < N ? (uint32_t)((int64_t)row * K * 2 + cb) : kOobVoff;
        }
    }

    u32x4 xreg[GATHER ? XCH : 1];
    auto issue = [&](int k0, int stage) {
        char* base = smem + stage * STAGE;
        // w: "nk" from W_e[n0, k0], "kn" from W_e[k0, n0]
        // (GLU: W_e has 2 n columns; "nk" waves 2 - 3 stage the up rows from n + n0 on)
        const int64_t w_first = GLU ? (KN ? ((int64_t)k0 * N * 2 + n0) * 2 : ((int64_t)(n0 + (wave / 2) * N) * K + k0) * 2)
                                    : (KN ? ((int64_t)k0 * N + n0) * 2 : ((int64_t)n0 * K + k0) * 2);
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
            w_tp[h][nb] = lds_pin(smem + X_BYTES + (KN ? swzt_row_off<BN>(4 * g + t_rr + 8 * h, wcol(nb) * 2 + t_cb) : 0));

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
                for (int nb = 0; nb < NB; ++nb) af[nb] = lds_read_b128(sw + swz_row_off<BK>(wcol(nb) + l31, 32 * ks + 16 * g));
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
    if constexpr (GLU) {
        // ---- the gated epilogue: g, u = the two finished sums (+ bias) ROUNDED to the io type, out = round16(act(g) * u) -
        // fa_act_mul's arithmetic (fa_act.h) on fa_moe_gemm's bits.  The activation is a wave-uniform run-time switch. ----
        const bool hb = s.bias != nullptr;
        auto bias_glu = [&](int half, int n) -> float {          // bias[seg, half n + n]; output columns >= n: +0, never read
            if (!hb || n >= N) return 0.f;
            const int64_t at = ((int64_t)seg * 2 + half) * N + n;
            if (bias32) return static_cast<const float*>(s.bias)[at];
            const uint32_t v = static_cast<const uint16_t*>(s.bias)[at];
            return E::lo(v);
        };
        // 8 rounded gates and ups of one row -> 8 outputs
        auto gated = [&](auto act_c, const u32x4& pg, const u32x4& pu) -> u32x4 {
            constexpr int ACT = decltype(act_c)::value;
            u32x4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float a0, a1, d;
                act_eval<ACT, false>(E::lo(pg[i]), a0, d);
                act_eval<ACT, false>(E::hi(pg[i]), a1, d);
                o[i] = E::pack2(a0 * E::lo(pu[i]), a1 * E::hi(pu[i]));
            }
            return o;
        };
        auto with_act = [&](auto&& body) {
            switch (s.activation) {
                case FA_ACT_SILU:      body(std::integral_constant<int, FA_ACT_SILU>{}); break;
                case FA_ACT_GELU:      body(std::integral_constant<int, FA_ACT_GELU>{}); break;
                case FA_ACT_GELU_TANH: body(std::integral_constant<int, FA_ACT_GELU_TANH>{}); break;
                case FA_ACT_RELU:      body(std::integral_constant<int, FA_ACT_RELU>{}); break;
                default:               body(std::integral_constant<int, FA_ACT_RELU2>{}); break;
            }
        };
        // the columns 8 (j >> 2) + 4 g + (j & 3) of accumulator registers 8 q + j, + bias, rounded in pairs
        auto rounded = [&](const f32x16& a, int q, int half, int col0) -> u32x4 {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float b = bias_glu(half, col0 + 16 * q + 8 * (j >> 2) + 4 * g + (j & 3));
                v[j] = hb ? a[8 * q + j] + b : a[8 * q + j];
            }
            return u32x4{E::pack2(v[0], v[1]), E::pack2(v[2], v[3]), E::pack2(v[4], v[5]), E::pack2(v[6], v[7])};
        };
        if constexpr (NB == 2) {
            // wide: acc[0][mb] and acc[1][mb] are g and u of the same elements: lane-local, then fa_moe_gemm's swap and store
            const int nb0 = n0 + wcol(0);
            with_act([&](auto act_c) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) {
                        const u32x4 o = gated(act_c, rounded(acc[0][mb], q, 0, nb0), rounded(acc[1][mb], q, 1, nb0));
                        uint32_t a0 = o[0], a1 = o[1], b0 = o[2], b1 = o[3];
                        permlane32_swap(a0, b0);
                        permlane32_swap(a1, b1);
                        const int m = m0 + wm_base + mb * 32 + l31, n = nb0 + 16 * q + 8 * g;
                        if (m < m_end && n < N) *reinterpret_cast<u32x4*>(outp + (int64_t)m * s.out_row_stride + n) = u32x4{a0, a1, b0, b1};
                    }
                }
            });
        } else {
            // decode: waves 0 - 1 hold gate blocks, waves 2 - 3 the matching up blocks.  Both stages are free behind the k loop's
            // last barrier: every wave writes its rounded block into a [32][128] image (swz_row_off<128>: 8 KiB), then each of the
            // 256 lanes takes the 8 gates and 8 ups of its (row, 8 columns)
            static_assert(BM * BN * 2 <= 2 * STAGE, "the exchange image fits the staging buffers");
            const int half = wave / 2, col0 = n0 + (wave % 2) * 32;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const u32x4 r = rounded(acc[0][0], q, half, col0);
                uint32_t a0 = r[0], a1 = r[1], b0 = r[2], b1 = r[3];
                permlane32_swap(a0, b0);
                permlane32_swap(a1, b1);                         // tile columns 32 wave + 16 q + 8 g + (0..7) of row l31
                lds_write_b128(smem + swz_row_off<BN>(l31, (wave * 32 + 16 * q + 8 * g) * 2), u32x4{a0, a1, b0, b1});
            }
            __syncthreads();
            const int row = tid / (BNO / 8), pc = tid % (BNO / 8);
            const u32x4 pg = lds_read_b128(smem + swz_row_off<BN>(row, pc * 16));
            const u32x4 pu = lds_read_b128(smem + swz_row_off<BN>(row, (BNO / 8 + pc) * 16));
            const int m = m0 + row, n = n0 + pc * 8;
            with_act([&](auto act_c) {
                const u32x4 o = gated(act_c, pg, pu);
                if (m < m_end && n < N) *reinterpret_cast<u32x4*>(outp + (int64_t)m * s.out_row_stride + n) = o;
            });
        }
        return;
    }
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

template <typename T, int BM, bool KN, bool GATHER>
__global__ void __launch_bounds__(GEMM_THREADS) moe_gemm_kernel(const fa_moe_gemm_params s) {
    moe_gemm_body<T, BM, KN, GATHER, false>(s);
}
template <typename T, int BM, bool KN, bool GATHER>
__global__ void __launch_bounds__(GEMM_THREADS) moe_glu_kernel(const fa_moe_gemm_glu_params s) {
    moe_gemm_body<T, BM, KN, GATHER, true>(s);
}

template <typename T, int BM, bool KN, bool GATHER>
void launch_k(const fa_moe_gemm_params& s, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((moe_gemm_kernel<T, BM, KN, GATHER>), grid, dim3(GEMM_THREADS), 0, stream, s);
}
template <typename T, int BM, bool KN, bool GATHER>
void launch_k(const fa_moe_gemm_glu_params& s, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((moe_glu_kernel<T, BM, KN, GATHER>), grid, dim3(GEMM_THREADS), 0, stream, s);
}
// P: fa_moe_gemm_params or fa_moe_gemm_glu_params
template <typename T, int BM, bool KN, typename P>
void launch_g(const P& s, dim3 grid, hipStream_t stream) {
    if (s.sorted_slot) launch_k<T, BM, KN, true>(s, grid, stream);
    else launch_k<T, BM, KN, false>(s, grid, stream);
}
template <typename T, int BM, typename P>
void launch_l(const P& s, dim3 grid, hipStream_t stream) {
    if (s.layout == FA_MOE_W_KN) launch_g<T, BM, true>(s, grid, stream);
    else launch_g<T, BM, false>(s, grid, stream);
}
template <typename T, typename P>
void launch_t(const P& s, const MoeGemmPlan& pl, hipStream_t stream) {
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

void launch_moe_gemm_glu(const fa_moe_gemm_glu_params& s, hipStream_t stream) {
    const MoeGemmPlan pl = moe_gemm_glu_plan(s.rows, s.n, s.k, s.num_experts, s.layout, s.dtype);
    if (s.dtype == FA_BF16) launch_t<bf16_tag>(s, pl, stream);
    else launch_t<fp16_tag>(s, pl, stream);
}

}  // namespace fa
