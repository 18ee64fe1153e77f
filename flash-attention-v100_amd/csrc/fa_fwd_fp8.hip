// fa_fwd_fp8.hip - attention forward with fp8-e4m3 Q, K and V on gfx950's block-scaled matrix pipe (dense and varlen,
// non-paged).  O is written in 16 bit (fa_params::o_dtype), LSE in fp32.
//
// The layout is fa_fwd_kernel's (fa_fwd.hip): workgroup = 4 waves x 32 query rows, 64-key tiles, S^T = K Q^T so that a lane
// owns ONE query row, the S^T accumulators packed straight into the B operand of O^T = V^T P^T, deferred rescale.  What
// differs: both products run on v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 operands and unit E8M0 scales (127 = 2^0) -
// twice the bf16 rate per clock, where the non-scaled v_mfma_f32_32x32x16_fp8_fp8 runs at the bf16 rate - and K / V are
// staged to LDS as stored (one byte per element, LDS-DMA, no conversion).
//
// Operand maps of the K = 64 form (tools/probes/probe_fp8_mfma.hip, exact integer data):
//   A: lane l (i = l & 31, g = l >> 5) holds A[i][k = 32 g + b] in byte b (0 .. 31) of its eight dwords,
//   B: lane l holds B[k = 32 g + b][j = l & 31] in byte b,
//   C/D: the 32 x 32 map of every 32x32 MFMA (fa_common.h): D[(r & 3) + 8 (r >> 2) + 4 g][l & 31] in register r.
// S^T = K Q^T (A = K rows, B = Q^T): k is the head dimension, both operands are 32 contiguous bytes of a row.
// O^T = V^T P^T: byte b of lane half g of the P^T fragment is register b & 15 of sacc[b >> 4] - the S^T accumulator pair of
// the 64-key tile, taken in register order - i.e. key(g, b) = 32 (b >> 4) + 8 ((b & 15) >> 2) + 4 g + (b & 3).  The V^T
// fragment (A, row = d) carries the same keys in the same bytes: its eight-byte quarter q (bytes 8 q .. 8 q + 7) holds keys
// 16 q + 8 (e >> 2) + 4 g + (e & 3), e = 0 .. 7, which is what one ds_read_b64_tr_b8 brings (per 16 lanes: 8 key rows x 16
// d-bytes in, lane c receives the eight keys of column c; probed in the same tool).
//
// P quantisation: P = exp2(s c - m_run) <= 2^FP8_RESCALE_THR = 256 under the deferred rescale (a tile only keeps the old
// maximum when no row of the wave exceeds it by more than 2^8), below e4m3's largest finite value 448, so
// v_cvt_pk_fp8_f32 never saturates.  The row sum l - and the LSE - are taken from the fp32 probabilities.
// Descales: q_descale k_descale fold into the softmax scale, v_descale into the final normalisation.
#include <cstring>
#include <type_traits>
#include "fa_common.h"

namespace fa {

constexpr int F8_BM = 128;                            // query rows per workgroup (32 per wave)
constexpr int F8_BN = 64;                             // keys per tile: one K = 64 MFMA of O^T
constexpr int F8_THREADS = 256;
constexpr float FP8_RESCALE_THR = 8.0f;               // log2 units: P <= 2^8 < 448 (e4m3 max)
static_assert(FP8_RESCALE_THR <= 8.0f, "P must stay below the e4m3 maximum (448)");

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));

template <int D> struct F8Smem {
    static constexpr int TILE = F8_BN * D;            // bytes of one K (or V) tile
    static constexpr int STAGE = 2 * TILE;            // K + V
    static constexpr int TOTAL = 2 * STAGE;           // double buffered
};

// e4m3 x e4m3 -> fp32, K = 64, unit scales (E8M0 127 = 2^0 on both operands)
__device__ __forceinline__ f32x16 mfma_e4m3(const u32x8& a, const u32x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(__builtin_bit_cast(i32x8, a), __builtin_bit_cast(i32x8, b), c,
                                                           0, 0, 0, 127, 0, 127);
}

// K tile: [64 keys][D bytes], 16-byte slots XOR-swizzled by row so that a ds_read_b128 of one slot from 8 consecutive rows
// touches eight different 16-byte bank groups (D 128: two rows per 256-byte line, D 64: four)
template <int D>
__device__ __forceinline__ int k8_off(int row, int col_byte) {
    const int f = D == 128 ? (row & 7) : ((row >> 2) & 3);
    return row * D + (col_byte ^ (f << 4));
}
// V tile: the slot XOR of fa_decode.hip's fp8 V image - the 8 keys x 2 slots one transposing read of 32 lanes covers land in
// 16 different bank groups (keys k and k + 8 of a quarter differ in the XOR's high bit)
template <int D>
__device__ __forceinline__ int v8_fv(int key) {
    return D == 128 ? ((((key >> 3) & 1) << 2) | (key & 3)) : (((key >> 3) & 1) << 1);
}
template <int D>
__device__ __forceinline__ int v8_off(int row, int col_byte) {
    return row * D + (col_byte ^ (v8_fv<D>(row) << 4));
}

// buffer descriptor over one (batch, head) slice of a byte tensor: rows past `nrows` read as zero
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc8(const void* base, int64_t row_stride, int nrows, int d) {
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    const int64_t bytes64 = nrows > 0 ? (int64_t)(nrows - 1) * row_stride + d : 0;
    const uint32_t bytes = __builtin_amdgcn_readfirstlane((uint32_t)(bytes64 > 0xffffffffll ? 0xffffffffll : bytes64));
    void* ptr = reinterpret_cast<void*>(((uint64_t)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(ptr, 0, (int)bytes, 0x00020000);
}

// the counted wait of fa_common.h (lds_tr_wait) over the four transposing reads of one V^T fragment
__device__ __forceinline__ void lds_tr_wait4(u32x2& a, u32x2& b, u32x2& c, u32x2& d, int n) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "i"(n));
}

// T: tag of the 16-bit output (fa_params::o_dtype); D: kernel width 64 or 128 (narrower rows through head_dim_v)
template <typename T, int D>
__global__ void __launch_bounds__(F8_THREADS, 2) fa_fwd_fp8_kernel(const KArgs a) {
    using E = Elem<T>;
    static_assert(D == 64 || D == 128, "fp8 forward: kernel widths 64 and 128");
    constexpr int KS = D / 64;                          // K = 64 steps of S^T
    constexpr int DBLKS = D / 32;                       // 32-column blocks of O
    constexpr int NKB = F8_BN / 32;                     // 32-key blocks per tile (2: one K = 64 step of O^T)
    constexpr int SPR = D / 16;                         // 16-byte slots per row
    constexpr int ROWS_PI = 64 / SPR;                   // rows of one LDS-DMA instruction (64 lanes x 16 bytes)
    constexpr int CHUNKS = F8_BN * SPR / F8_THREADS;    // DMA instructions per wave, tile and tensor
    constexpr int TILE = F8Smem<D>::TILE;
    constexpr int STAGE = F8Smem<D>::STAGE;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const fa_params& p = a.p;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const WorkItem w = a.flat_blocks
        ? decode_work_flat(blockIdx.x, a.flat_blocks, F8_BM, p.batch, p.nheads_q, p.nheads_k, p.cu_seqlens_q, lane)
        : decode_work(blockIdx.x, p.batch, p.nheads_q, p.nheads_k, a.n_qblocks);
    if (!w.valid) return;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int g = lane >> 5;

    // ---- per-sequence geometry (fa_fwd_kernel's, without paging / kv-cache) ----
    int seqlen_q = p.seqlen_q, seqlen_k = p.seqlen_k;
    int64_t q_row0 = 0, k_row0 = 0;
    if (p.cu_seqlens_q) {
        q_row0 = p.cu_seqlens_q[w.b];
        seqlen_q = p.cu_seqlens_q[w.b + 1] - (int)q_row0;
    }
    if (p.cu_seqlens_k) {
        k_row0 = p.cu_seqlens_k[w.b];
        seqlen_k = p.cu_seqlens_k[w.b + 1] - (int)k_row0;
    }
    if (a.seqlens_k) {                                                       // seqused_k
        const int su = a.seqlens_k[w.b];
        seqlen_k = su > 0 ? (su < seqlen_k ? su : seqlen_k) : 0;
    }
    seqlen_k = __builtin_amdgcn_readfirstlane(seqlen_k);
    seqlen_q = __builtin_amdgcn_readfirstlane(seqlen_q);
    k_row0 = (int64_t)__builtin_amdgcn_readfirstlane((int)k_row0);
    q_row0 = (int64_t)__builtin_amdgcn_readfirstlane((int)q_row0);

    const int off = seqlen_k - seqlen_q;               // bottom-right alignment
    const int wl = p.window_left;
    const int wr = p.is_causal ? 0 : p.window_right;
    const int n_pass = (a.pair_qblocks && (a.n_qblocks_total - 1 - w.qb) != w.qb) ? 2 : 1;
    auto qb_of = [&](int pass) { return pass == 0 ? w.qb : a.n_qblocks_total - 1 - w.qb; };
    auto tile_range = [&](int m0, int& t_min, int& t_max) {
        t_min = 0; t_max = (seqlen_k + F8_BN - 1) / F8_BN;
        const int m_last = (m0 + F8_BM < seqlen_q ? m0 + F8_BM : seqlen_q) - 1;
        if (wr >= 0) {
            const int kmax = m_last + off + wr;
            const int t = kmax < 0 ? 0 : kmax / F8_BN + 1;
            t_max = t < t_max ? t : t_max;
        }
        if (wl >= 0) {
            const int kmin = m0 + off - wl;
            if (kmin > 0) t_min = kmin / F8_BN;
        }
        if (m0 >= seqlen_q) t_max = t_min;
    };
    int m_block = 0, n_min = 0, n_max = 0;
    int wave_row0 = 0, my_row = 0;
    int lo = 0, hi = -1;                               // visible keys of my row: lo <= j <= hi
    int w_hi_min = 0, w_hi_max = 0, w_lo_max = 0, w_lo_min = 0;
    auto begin_pass = [&](int pass) {
        m_block = qb_of(pass) * F8_BM;
        tile_range(m_block, n_min, n_max);
        wave_row0 = m_block + wave * 32;
        my_row = wave_row0 + l31;
        lo = 0; hi = seqlen_k - 1;
        if (wr >= 0) { const int h2 = my_row + off + wr; hi = h2 < hi ? h2 : hi; }
        if (wl >= 0) { const int l2 = my_row + off - wl; lo = l2 > lo ? l2 : lo; }
        const int wrow_last = wave_row0 + 31;
        w_hi_min = seqlen_k - 1; w_hi_max = seqlen_k - 1; w_lo_max = 0;
        if (wr >= 0) {
            const int h0 = wave_row0 + off + wr, h1 = wrow_last + off + wr;
            w_hi_min = h0 < w_hi_min ? h0 : w_hi_min;
            w_hi_max = h1 < w_hi_max ? h1 : w_hi_max;
        }
        if (wl >= 0) { const int l1 = wrow_last + off - wl; w_lo_max = l1 > 0 ? l1 : 0; }
        w_lo_min = (wl >= 0 && wave_row0 + off - wl > 0) ? wave_row0 + off - wl : 0;
        if (wave_row0 >= seqlen_q) { w_hi_max = -1; w_hi_min = -1; }       // rows past the sequence: no active tile
    };

    // ---- pointers (byte tensors: strides in elements = bytes) ----
    const uint8_t* qp = reinterpret_cast<const uint8_t*>(p.q) + (p.cu_seqlens_q ? 0 : (int64_t)w.b * p.q_batch_stride)
                        + q_row0 * p.q_row_stride + (int64_t)w.h * p.q_head_stride;
    const uint8_t* kp = reinterpret_cast<const uint8_t*>(p.k) + (p.cu_seqlens_k ? 0 : (int64_t)w.b * p.k_batch_stride)
                        + k_row0 * p.k_row_stride + (int64_t)w.hk * p.k_head_stride;
    const uint8_t* vp = reinterpret_cast<const uint8_t*>(p.v) + (p.cu_seqlens_k ? 0 : (int64_t)w.b * p.v_batch_stride)
                        + k_row0 * p.v_row_stride + (int64_t)w.hk * p.v_head_stride;
    const int dv = valid_cols(p);                      // a multiple of 16: a 16-byte chunk is all valid or all missing

    // ---- Q fragments: B operand of S^T, lane holds Q[row][64 ks + 32 g .. + 31] ----
    const __amdgpu_buffer_rsrc_t q_rsrc = make_rsrc8(qp, p.q_row_stride, seqlen_q, dv);
    u32x8 qf[KS];
    auto load_q = [&](int row) {
        const uint32_t base = (uint32_t)row * (uint32_t)p.q_row_stride + 32 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4 h[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int c0 = 64 * ks + 32 * g + 16 * hf;
                h[hf] = buf_load_b128(q_rsrc, (row < seqlen_q && c0 < dv) ? base + 64 * ks + 16 * hf : kOobVoff, 0);
            }
            qf[ks] = u32x8{h[0][0], h[0][1], h[0][2], h[0][3], h[1][0], h[1][1], h[1][2], h[1][3]};
        }
    };

    // ---- staging: LDS-DMA, lane-linear destination, swizzle applied to the source column (an involution) ----
    uint32_t k_voff[CHUNKS], v_voff[CHUNKS];
    int k_lds[CHUNKS], v_lds[CHUNKS];
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        const int inst = wave * CHUNKS + i;
        const int row = inst * ROWS_PI + lane / SPR;
        const int slot = lane % SPR;
        const int k_cb = k8_off<D>(row, slot * 16) - row * D;              // logical byte column
        const int v_cb = v8_off<D>(row, slot * 16) - row * D;
        k_voff[i] = k_cb < dv ? (uint32_t)(row * p.k_row_stride + k_cb) : kOobVoff;
        v_voff[i] = v_cb < dv ? (uint32_t)(row * p.v_row_stride + v_cb) : kOobVoff;
        k_lds[i] = inst * 1024;
        v_lds[i] = TILE + inst * 1024;
    }
    const __amdgpu_buffer_rsrc_t k_rsrc = make_rsrc8(kp, p.k_row_stride, seqlen_k, dv);
    const __amdgpu_buffer_rsrc_t v_rsrc = make_rsrc8(vp, p.v_row_stride, seqlen_k, dv);
    const uint32_t k_tile_bytes = (uint32_t)(F8_BN * p.k_row_stride);
    const uint32_t v_tile_bytes = (uint32_t)(F8_BN * p.v_row_stride);
    auto load_tile = [&](int nb, auto stage_c) {
        constexpr int stage = decltype(stage_c)::value;
        char* base = smem + stage * STAGE;
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) buf_load_lds_b128(k_rsrc, base + k_lds[i], k_voff[i], (uint32_t)nb * k_tile_bytes);
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) buf_load_lds_b128(v_rsrc, base + v_lds[i], v_voff[i], (uint32_t)nb * v_tile_bytes);
    };

    // ---- accumulators, lane-constant LDS addresses ----
    f32x16 oacc[DBLKS];
#pragma unroll
    for (int d = 0; d < DBLKS; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
    float m_run = -INFINITY;     // running (deferred) max, log2 domain (scaled)
    float l_run = 0.f;           // this lane's partial row sum (its 32 keys per tile), fp32 probabilities
    // K rows: lane reads row 32 kb + l31, bytes 64 ks + 32 g + 16 hf (the swizzle only sees row bits < 5: kb is an immediate)
    const lds_char* k_ptr[KS][2];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) k_ptr[ks][hf] = lds_pin(smem + k8_off<D>(l31, 64 * ks + 32 * g + 16 * hf));
    // V^T quarters: 16-lane group gg = lane >> 4, source lane sl = lane & 15 brings key 16 q + key_l, bytes 8 (sl & 1) of
    // d-slot 2 d + (gg & 1) (the key's swizzle only sees key bits < 4: q is an immediate)
    const lds_char* v_ptr[DBLKS];
    {
        const int sl = lane & 15, gg = lane >> 4, jj = sl >> 1;
        const int key_l = (jj & 3) + 8 * (jj >> 2) + 4 * (gg >> 1);
#pragma unroll
        for (int d = 0; d < DBLKS; ++d)
            v_ptr[d] = lds_pin(smem + TILE + key_l * D + (((2 * d + (gg & 1)) ^ v8_fv<D>(key_l)) << 4) + 8 * (sl & 1));
    }
    const float qk_descale = p.q_descale * p.k_descale;                  // (the host turned 0 into 1)
    const float c = a.scale_log2e * qk_descale;

    auto compute_tile = [&](auto stage_c, int nb) {
        constexpr int stage = decltype(stage_c)::value;
        const int n0 = nb * F8_BN;
        // ---- S^T = K Q^T : sacc[kb][r] = S[my_row][n0 + 32 kb + row(r, g)] ----
        u32x8 kf[NKB][KS];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const u32x4 h0 = lds_read_b128(k_ptr[ks][0] + (stage * STAGE + kb * 32 * D));
                const u32x4 h1 = lds_read_b128(k_ptr[ks][1] + (stage * STAGE + kb * 32 * D));
                kf[kb][ks] = u32x8{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
            }
        f32x16 sacc[NKB];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[kb][r] = 0.f;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) sacc[kb] = mfma_e4m3(kf[kb][ks], qf[ks], sacc[kb]);
        __builtin_amdgcn_s_setprio(0);
        // ---- V^T fragments for O^T, issued now so that they land under the softmax ----
        __builtin_amdgcn_sched_barrier(0);
        u32x2 vq[DBLKS][4];
#pragma unroll
        for (int d = 0; d < DBLKS; ++d)
#pragma unroll
            for (int q = 0; q < 4; ++q) vq[d][q] = lds_read_tr8_nw(v_ptr[d], stage * STAGE + 16 * q * D);
        __builtin_amdgcn_sched_barrier(0);
        // ---- masking on edge tiles (fa_fwd_kernel's visibility bits) ----
        const bool need_mask = (n0 + F8_BN - 1 > w_hi_min) || (n0 < w_lo_max);
        if (need_mask) {
            const int lc = lo - n0 - 4 * g;
            const int hc = hi < lo ? lc : hi - n0 - 4 * g + 1;
            uint32_t visw[NKB];
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                int l = lc - 32 * kb, h = hc - 32 * kb;
                l = l < 0 ? 0 : (l > 32 ? 32 : l);
                h = h < 0 ? 0 : (h > 32 ? 32 : h);
                const uint32_t below_h = h >= 32 ? ~0u : ((1u << h) - 1u);
                const uint32_t below_l = l >= 32 ? ~0u : ((1u << l) - 1u);
                visw[kb] = below_h & ~below_l;
            }
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int cpos = (r & 3) + 8 * (r >> 2);
                    const uint32_t m = (uint32_t)((int32_t)(visw[kb] << (31 - cpos)) >> 31);
                    sacc[kb][r] = select_bits(sacc[kb][r], m, 0xff800000u);
                }
        }
        // ---- online softmax (log2 domain) with deferred rescale ----
        float mx = max3_f32(sacc[0][0], sacc[0][1], sacc[0][2]);
#pragma unroll
        for (int r = 3; r + 1 < 16; r += 2) mx = max3_f32(mx, sacc[0][r], sacc[0][r + 1]);
        mx = max3_f32(mx, sacc[0][15], sacc[1][0]);
#pragma unroll
        for (int r = 1; r + 1 < 16; r += 2) mx = max3_f32(mx, sacc[1][r], sacc[1][r + 1]);
        mx = fmaxf(mx, sacc[1][15]);
        mx = xhalf_max(mx) * c;
        // keep the old max unless some row of the wave would exceed it by > 2^THR (NaN-safe: -inf - -inf takes the rescale path)
        if (!__all(mx - m_run <= FP8_RESCALE_THR)) {
            const float m_new = fmaxf(m_run, mx);
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = fast_exp2(m_run - m_use);
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int d = 0; d < DBLKS; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[d][r] *= alpha;
        }
        const float m_use = (m_run == -INFINITY) ? 0.f : m_run;
        // P <= 2^FP8_RESCALE_THR = 256 here: exact range for e4m3 (max 448); l sums the fp32 values
        float psum = 0.f;
        u32x8 pf;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int w4 = 0; w4 < 4; ++w4) {
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    e[j] = fast_exp2(fmaf(sacc[kb][4 * w4 + j], c, -m_use));
                    psum += e[j];
                }
                int word = __builtin_amdgcn_cvt_pk_fp8_f32(e[0], e[1], 0, false);
                word = __builtin_amdgcn_cvt_pk_fp8_f32(e[2], e[3], word, true);
                pf[4 * kb + w4] = (uint32_t)word;
            }
        l_run += psum;
        // ---- O^T += V^T P^T : one K = 64 MFMA per 32 output columns ----
#pragma unroll
        for (int d = 0; d < DBLKS; ++d) {
            lds_tr_wait4(vq[d][0], vq[d][1], vq[d][2], vq[d][3], 4 * (DBLKS - 1 - d));
            const u32x8 vf = {vq[d][0][0], vq[d][0][1], vq[d][1][0], vq[d][1][1],
                              vq[d][2][0], vq[d][2][1], vq[d][3][0], vq[d][3][1]};
            oacc[d] = mfma_e4m3(vf, pf, oacc[d]);
        }
    };

    auto tile_step = [&](auto stage_c, int nb) {
        constexpr int stage = decltype(stage_c)::value;
        const bool has_next = nb + 1 < n_max;
        if (has_next) load_tile(nb + 1, std::integral_constant<int, stage ^ 1>{});
        const int n0 = nb * F8_BN;
        const bool wave_active = (n0 <= w_hi_max) && (n0 + F8_BN - 1 >= w_lo_min);
        if (wave_active) compute_tile(stage_c, nb);
        __syncthreads();
    };

    for (int pass = 0; pass < n_pass; ++pass) {
        begin_pass(pass);
        if (m_block >= seqlen_q) continue;
        load_q(my_row);
        if (n_min < n_max) load_tile(n_min, std::integral_constant<int, 0>{});
        __syncthreads();
        for (int nb = n_min; nb < n_max; nb += 2) {
            tile_step(std::integral_constant<int, 0>{}, nb);
            if (nb + 1 < n_max) tile_step(std::integral_constant<int, 1>{}, nb + 1);
        }

        // ---- epilogue: O v_descale / l, LSE ----
        const float l_tot = xhalf_sum(l_run);
        const float inv = l_tot > 0.f ? p.v_descale / l_tot : 0.f;
        if (my_row < seqlen_q) {
            int row_e = my_row, g_e = g;
            asm volatile("" : "+v"(row_e), "+v"(g_e));    // (store addresses formed here, not hoisted across the loop)
            uint16_t* op = reinterpret_cast<uint16_t*>(p.o) + (p.cu_seqlens_q ? 0 : (int64_t)w.b * p.o_batch_stride)
                           + (q_row0 + row_e) * p.o_row_stride + (int64_t)w.h * p.o_head_stride;
#pragma unroll
            for (int d = 0; d < DBLKS; ++d)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    u32x2 o2;
                    o2[0] = E::pack2(oacc[d][4 * rq + 0] * inv, oacc[d][4 * rq + 1] * inv);
                    o2[1] = E::pack2(oacc[d][4 * rq + 2] * inv, oacc[d][4 * rq + 3] * inv);
                    if (d * 32 + 8 * rq + 4 * g_e < dv) *reinterpret_cast<u32x2*>(op + d * 32 + 8 * rq + 4 * g_e) = o2;
                }
            if (g_e == 0) {
                const float lse = l_tot > 0.f ? (m_run + fast_log2(l_tot)) * kLn2 : -INFINITY;
                p.lse[(int64_t)w.b * p.lse_batch_stride + (int64_t)w.h * p.lse_head_stride + q_row0 + row_e] = lse;
            }
        }
        if (pass + 1 < n_pass) {
#pragma unroll
            for (int d = 0; d < DBLKS; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
            m_run = -INFINITY;
            l_run = 0.f;
        }
    }
}

template <typename T, int D>
static int launch_fwd_fp8_td(const KArgs& a, hipStream_t stream) {
    const int grid = a.flat_blocks ? a.flat_blocks * a.p.nheads_q
                                   : work_grid(a.p.batch, a.p.nheads_q, a.p.nheads_k, a.n_qblocks);
    if (grid == 0) return 0;
    const size_t smem = F8Smem<D>::TOTAL;
    auto kern = fa_fwd_fp8_kernel<T, D>;
    FA_SET_LDS_ONCE(kern, smem);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(F8_THREADS), smem, stream, a);
    return 0;
}

// fa_fwd / fa_varlen_fwd with fp8-e4m3 q, k, v (fa_api.hip has validated the request: no bias, dropout or paging,
// head_dim 64 / 128, descales > 0)
int launch_fwd_fp8(const KArgs& a, hipStream_t stream) {
    const bool bf = a.p.o_dtype == FA_BF16;
    switch (a.p.head_dim) {
        case 64:  return bf ? launch_fwd_fp8_td<bf16_tag, 64>(a, stream) : launch_fwd_fp8_td<fp16_tag, 64>(a, stream);
        case 128: return bf ? launch_fwd_fp8_td<bf16_tag, 128>(a, stream) : launch_fwd_fp8_td<fp16_tag, 128>(a, stream);
        default:  return -2;
    }
}

}  // namespace fa
