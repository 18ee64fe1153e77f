// fa_quant.hip - dynamic fp8-e4m3 quantisation of 16-bit activations: alone (fa_quant_fp8), behind fa_add_norm's forward
// (fa_add_norm_quant) and behind fa_act_mul's forward (fa_act_mul_quant); include/fa_mi355.h has the contract.  One rule, fp32,
// on the values y_j AFTER their rounding to the 16-bit type:
//     a      = fmaxf(+0, |y_0|, |y_1|, ..)     over the row, or over each aligned group of 128 columns (fa_rowmax.h)
//     a'     = has_ub ? fminf(a, scale_ub) : a
//     scale  = fmaxf(a' / 448.0f, 0x1p-64f)    quant_scale
//     inv    = 1.0f / scale                    fp8_inv_descale (fa_fp8_cvt.h)
//     code_j = e4m3(fminf(fmaxf(y_j * inv, -448), 448))        to_fp8x8 (fa_fp8_cvt.h)
// STATIC: the caller's scale, the last two lines alone - fa_kv_store's rule.  Every kernel holds y as the PACKED 16-bit pieces a
// 16-bit store would have written (u32x4 = 8 columns), so "after the rounding" is by construction, and the fused forms have the
// bits of fa_quant_fp8 on the 16-bit op's output: fa_add_norm_quant runs the bodies fa_add_norm runs (fa_add_norm.h) with an
// epilogue that packs instead of storing, fa_act_mul_quant evaluates fa_act.h's act_eval.
// Ownership:
//   fa_quant_fp8, n <= 512 (quant_small_kernel): a row lies one piece per lane in G adjacent lanes of a wave, G the smallest power
//     of two with 8 G >= n; a workgroup of 256 lanes takes 256 / G consecutive rows; no LDS.  Lanes past the row or past the last
//     row load nothing, hand in +0 and store nothing; every cross-lane read sits outside every lane-dependent branch.
//   fa_quant_fp8 at n > 512 and fa_act_mul_quant at every n (quant_wide_kernel): one workgroup per row - whole waves, at most 256
//     lanes up to FA_QUANT_WIDE_PIECES pieces (16384 columns) and 1024 lanes above - lane t owns the pieces t, t + threads, ..
//     (at most 8).  Every load of the row is issued before the first store.
//   fa_add_norm_quant: fa_add_norm.h's, which is fa_add_norm's: n <= 256 G lanes a row, above one workgroup of <= 256 lanes.
//   A group of 128 columns is 16 pieces: in every form 16 adjacent lanes, aligned at 16, hold them - one xor butterfly, no LDS.
//   The row maximum of the wide forms meets through LDS (row_block_max).
// A row of a 16-bit input that does not start on a 16-byte boundary is loaded element by element, a row of codes that does not
// start on an 8-byte boundary is stored byte by byte: the same bits.  No workspace, one launch, no atomics, every offset 64-bit.
#include <cstdint>
#include "fa_act.h"
#include "fa_add_norm.h"
#include "fa_fp8_cvt.h"
#include "fa_rowmax.h"
#include "fa_rowops.h"
#include "fa_rowsum.h"

#ifndef FA_QUANT_WIDE_PIECES
#define FA_QUANT_WIDE_PIECES 2048     // pieces of a row up to which <= 256 lanes own it (1024 above); profiles/quant.txt
#endif

namespace fa {

constexpr int QUANT_SMALL_MAX = 512;                        // n up to here: quant_small_kernel
constexpr int QUANT_THREADS = 256;
constexpr int QUANT_MAX_THREADS = 1024;
constexpr int QUANT_MAX_WAVES = QUANT_MAX_THREADS / 64;
constexpr int QUANT_NO_ACT = -1;                            // quant_wide_kernel's ACT for fa_quant_fp8: y = x

// The value unchanged, behind a statement the compiler does not look through and does not reorder against its like; `chain`
// ties it to what the piece before produced, so the pieces of a lane are worked on one after the other.  The kernels hold a row as
// packed 16-bit pieces (4 registers each) between the amax and the conversion; left alone hipcc widens all 64 values of a lane to
// fp32 at once, keeps them across the reduction, evaluates the 64 activations side by side - and spills.
__device__ __forceinline__ u32x4 quant_opaque(u32x4 v, float& chain) {
    asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(chain));
    __builtin_amdgcn_sched_barrier(0);
    return v;
}

struct QRule { int mode, has_ub; float scale, scale_ub; };

__device__ __forceinline__ float quant_scale(float a, const QRule& q) {
    const float ap = q.has_ub ? fminf(a, q.scale_ub) : a;
    return fmaxf(ap / 448.0f, 0x1p-64f);
}

// the host side of the wide ownership: a function of n alone
struct QuantShape { int group_log2, threads, pieces; };
static QuantShape quant_shape(int n, bool small_ok) {
    QuantShape s = {0, QUANT_THREADS, 1};
    const int np = n / 8;
    if (small_ok && n <= QUANT_SMALL_MAX) {
        while ((1 << s.group_log2) < np) ++s.group_log2;
        return s;
    }
    s.threads = np > FA_QUANT_WIDE_PIECES ? QUANT_MAX_THREADS : (np >= QUANT_THREADS ? QUANT_THREADS : (np + 63) / 64 * 64);
    const int per = (np + s.threads - 1) / s.threads;
    s.pieces = per <= 1 ? 1 : (per <= 2 ? 2 : (per <= 4 ? 4 : 8));   // the kernels are built for 1, 2, 4, 8 (absent pieces: +0)
    return s;
}

__device__ __forceinline__ bool quant_vec16(const uint16_t* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__device__ __forceinline__ bool quant_vec8(const uint8_t* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// one piece of a 16-bit row as a 16-bit store would hold it
__device__ __forceinline__ u32x4 quant_load8(const uint16_t* p, bool vec) {
    if (vec) return ld_nt16(p);
    u32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (uint32_t)p[2 * i] | ((uint32_t)p[2 * i + 1] << 16);
    // (one piece's eight loads are packed before the next piece's are issued: hipcc would otherwise hold every 16-bit element of
    //  the lane's pieces in a register of its own - 64 per input - and spill)
    asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]) : : "memory");
    return r;
}

__device__ __forceinline__ void quant_store8(uint8_t* c, bool vec, const u32x2& v) {
    if (vec) {
        *reinterpret_cast<u32x2*>(c) = v;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
    }
}

// round16(act(g) * u), or round16(act(g)): fa_act_mul.hip's forward on one piece
template <typename T, int ACT, bool GATED>
__device__ __forceinline__ u32x4 quant_act8(const u32x4& g, const u32x4& u) {
    using E = Elem<T>;
    u32x4 y;
    float chain = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float a0, a1, dv;
        uint32_t gi = g[i];
        if constexpr (ACT == FA_ACT_GELU) {                 // (erff: two columns after the other two - see quant_opaque)
            asm volatile("" : "+v"(gi), "+v"(chain));
            __builtin_amdgcn_sched_barrier(0);
        }
        act_eval<ACT, false>(E::lo(gi), a0, dv);
        act_eval<ACT, false>(E::hi(gi), a1, dv);
        if constexpr (GATED) {
            a0 = a0 * E::lo(u[i]);
            a1 = a1 * E::hi(u[i]);
        }
        y[i] = E::pack2(a0, a1);
        if constexpr (ACT == FA_ACT_GELU) asm volatile("" : "+v"(y[i]));       // (packed here, not at the end)
        chain = __builtin_bit_cast(float, y[i]);
    }
    return y;
}

// The rule on a row that lies one piece per lane in `lanes` adjacent lanes of a wave (on: the lane has a piece, at column d).
// crow / cvec: the row's codes and whether they take 8-byte stores.  EVERY lane of the wave must call this
template <typename T>
__device__ __forceinline__ void quant_emit_small(const QRule& q, uint8_t* crow, bool cvec, float* scales, int64_t row, int n,
                                                 const u32x4& y, bool on, int d, int lanes) {
    float s = q.scale;
    if (q.mode != FA_QUANT_STATIC) {
        const bool group = q.mode == FA_QUANT_GROUP;                    // (n % 128 == 0: lanes >= 16)
        const float a = row_group_max(on ? row_piece_amax<T>(y) : 0.f, group ? 16 : lanes);
        s = quant_scale(a, q);
        if (on && (d & (group ? 127 : 0x7fffffff)) == 0) scales[group ? row * (n >> 7) + (d >> 7) : row] = s;
    }
    if (on) quant_store8(crow + d, cvec, to_fp8x8<T>(y, fp8_inv_descale(s)));
}

// .. and on a row owned by whole waves, lane t the pieces t, t + threads, ..; slot: QUANT_MAX_WAVES floats of LDS that nothing
// else in flight uses.  EVERY lane of the workgroup must call this
template <typename T, int NP>
__device__ __forceinline__ void quant_emit_wide(const QRule& q, uint8_t* crow, bool cvec, float* scales, int64_t row, int n,
                                                const u32x4 (&y)[NP], const bool (&on)[NP], const int (&d)[NP], float* slot) {
    const int tid = (int)threadIdx.x;
    float chain = 0.f;                                      // (absent pieces hold +0: their amax is +0, their codes are not stored)
    if (q.mode == FA_QUANT_GROUP) {
        float* srow = scales + row * (n >> 7);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const u32x4 yp = quant_opaque(y[p], chain);
            const float s = quant_scale(row_group_max(row_piece_amax<T>(yp), 16), q);
            const u32x2 c = to_fp8x8<T>(quant_opaque(yp, chain), fp8_inv_descale(s));
            chain = __builtin_bit_cast(float, c[1]);
            if (on[p]) {
                if ((tid & 15) == 0) srow[d[p] >> 7] = s;
                quant_store8(crow + d[p], cvec, c);
            }
        }
        return;
    }
    float s = q.scale;
    if (q.mode == FA_QUANT_ROW) {
        float a = 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p) a = fmaxf(a, row_piece_amax<T>(quant_opaque(y[p], a)));
        s = quant_scale(row_block_max(a, slot, (int)blockDim.x >> 6, tid >> 6), q);
        if (tid == 0) scales[row] = s;
    }
    const float inv = fp8_inv_descale(s);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const u32x2 c = to_fp8x8<T>(quant_opaque(y[p], chain), inv);
        chain = __builtin_bit_cast(float, c[1]);
        if (on[p]) quant_store8(crow + d[p], cvec, c);
    }
}

// ---- fa_quant_fp8 and fa_act_mul_quant
struct QArgs {
    const uint16_t *x, *up;                                 // x: the input, or the gate; up: nullptr where ungated
    uint8_t* codes;
    float* scales;
    int64_t x_rs, up_rs, codes_rs, rows;
    int n, group_log2;
    QRule q;
};

template <typename T>
__global__ void __launch_bounds__(QUANT_THREADS) quant_small_kernel(const QArgs a) {
    const int lanes = 1 << a.group_log2;
    const int j = (int)threadIdx.x & (lanes - 1);
    const int d = 8 * j;
    const int64_t r = (int64_t)blockIdx.x * (QUANT_THREADS >> a.group_log2) + ((int)threadIdx.x >> a.group_log2);
    const bool on = d < a.n && r < a.rows;
    const int64_t row = r < a.rows ? r : 0;
    const uint16_t* xrow = a.x + row * a.x_rs;
    uint8_t* crow = a.codes + row * a.codes_rs;
    u32x4 y = {0, 0, 0, 0};
    if (on) y = quant_load8(xrow + d, quant_vec16(xrow));
    quant_emit_small<T>(a.q, crow, quant_vec8(crow), a.scales, row, a.n, y, on, d, lanes);
}

// TB: the most lanes a launch has (256 or 1024).  Both are built for the register budget of 1024 lanes a workgroup - 128, four
// waves a SIMD: left to itself hipcc takes 241 registers for the 256-lane form of a kernel that fits in 87
template <typename T, int ACT, bool GATED, int NP, int TB>
__global__ void __launch_bounds__(TB, QUANT_MAX_THREADS / TB) quant_wide_kernel(const QArgs a) {
    __shared__ float red[QUANT_MAX_WAVES];
    const int threads = (int)blockDim.x;
    const int64_t row = blockIdx.x;
    const uint16_t* xrow = a.x + row * a.x_rs;
    const uint16_t* urow = GATED ? a.up + row * a.up_rs : nullptr;
    uint8_t* crow = a.codes + row * a.codes_rs;
    const bool xvec = quant_vec16(xrow), uvec = GATED && quant_vec16(urow);
    u32x4 y[NP], u[NP];
    int d[NP];
    bool on[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        d[p] = 8 * ((int)threadIdx.x + p * threads);
        on[p] = d[p] < a.n;
        y[p] = u32x4{0, 0, 0, 0};
        u[p] = u32x4{0, 0, 0, 0};
        if (on[p]) {
            y[p] = quant_load8(xrow + d[p], xvec);
            if constexpr (GATED) u[p] = quant_load8(urow + d[p], uvec);
        }
    }
    if constexpr (ACT != QUANT_NO_ACT) {
        float chain = 0.f;                                  // (absent pieces: act(+0) * +0, never stored; no lane-dependent branch)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            y[p] = quant_opaque(quant_act8<T, ACT, GATED>(quant_opaque(y[p], chain), u[p]), chain);
            chain = __builtin_bit_cast(float, y[p][3]);
        }
    }
    quant_emit_wide<T, NP>(a.q, crow, quant_vec8(crow), a.scales, row, a.n, y, on, d, red);
}

template <typename T, int ACT, bool GATED>
static void launch_quant_wide(const QArgs& a, const QuantShape& sh, hipStream_t stream) {
    const dim3 g((unsigned)a.rows), b(sh.threads);
    if (sh.threads > QUANT_THREADS) {                       // (1024 lanes: more than 1024 pieces, so at least 2 a lane)
        switch (sh.pieces) {
        case 2:  hipLaunchKernelGGL((quant_wide_kernel<T, ACT, GATED, 2, QUANT_MAX_THREADS>), g, b, 0, stream, a); break;
        case 4:  hipLaunchKernelGGL((quant_wide_kernel<T, ACT, GATED, 4, QUANT_MAX_THREADS>), g, b, 0, stream, a); break;
        default: hipLaunchKernelGGL((quant_wide_kernel<T, ACT, GATED, 8, QUANT_MAX_THREADS>), g, b, 0, stream, a); break;
        }
        return;
    }
    switch (sh.pieces) {
    case 1:  hipLaunchKernelGGL((quant_wide_kernel<T, ACT, GATED, 1, QUANT_THREADS>), g, b, 0, stream, a); break;
    case 2:  hipLaunchKernelGGL((quant_wide_kernel<T, ACT, GATED, 2, QUANT_THREADS>), g, b, 0, stream, a); break;
    case 4:  hipLaunchKernelGGL((quant_wide_kernel<T, ACT, GATED, 4, QUANT_THREADS>), g, b, 0, stream, a); break;
    default: hipLaunchKernelGGL((quant_wide_kernel<T, ACT, GATED, 8, QUANT_THREADS>), g, b, 0, stream, a); break;
    }
}

template <typename T>
static void launch_quant_rows(const QArgs& a, const QuantShape& sh, hipStream_t stream) {
    if (a.n <= QUANT_SMALL_MAX) {
        const int per = QUANT_THREADS >> sh.group_log2;
        const dim3 g((unsigned)((a.rows + per - 1) / per)), b(QUANT_THREADS);
        hipLaunchKernelGGL((quant_small_kernel<T>), g, b, 0, stream, a);
        return;
    }
    launch_quant_wide<T, QUANT_NO_ACT, false>(a, sh, stream);
}

template <typename T, int ACT>
static void launch_quant_act(const QArgs& a, const QuantShape& sh, hipStream_t stream) {
    if (a.up) launch_quant_wide<T, ACT, true>(a, sh, stream);
    else      launch_quant_wide<T, ACT, false>(a, sh, stream);
}

template <typename T>
static void launch_quant_act_kind(const QArgs& a, int act, const QuantShape& sh, hipStream_t stream) {
    switch (act) {
        case FA_ACT_SILU:      launch_quant_act<T, FA_ACT_SILU>(a, sh, stream); break;
        case FA_ACT_GELU:      launch_quant_act<T, FA_ACT_GELU>(a, sh, stream); break;
        case FA_ACT_GELU_TANH: launch_quant_act<T, FA_ACT_GELU_TANH>(a, sh, stream); break;
        case FA_ACT_RELU:      launch_quant_act<T, FA_ACT_RELU>(a, sh, stream); break;
        default:               launch_quant_act<T, FA_ACT_RELU2>(a, sh, stream); break;
    }
}

static QRule quant_rule(int mode, int has_ub, float scale, float scale_ub) { return QRule{mode, has_ub, scale, scale_ub}; }

// The caller (fa_api.hip) has validated the block; rows > 0
void launch_quant_fp8(const fa_quant_fp8_params& s, hipStream_t stream) {
    QArgs a = {};
    a.x = static_cast<const uint16_t*>(s.x);
    a.codes = static_cast<uint8_t*>(s.codes);
    a.scales = static_cast<float*>(s.scales);
    a.x_rs = s.x_row_stride; a.codes_rs = s.codes_row_stride; a.rows = s.rows;
    a.n = s.n;
    a.q = quant_rule(s.mode, s.has_scale_ub, s.scale, s.scale_ub);
    const QuantShape sh = quant_shape(s.n, true);
    a.group_log2 = sh.group_log2;
    if (s.dtype == FA_BF16) launch_quant_rows<bf16_tag>(a, sh, stream);
    else                    launch_quant_rows<fp16_tag>(a, sh, stream);
}

void launch_act_mul_quant(const fa_act_mul_quant_params& s, hipStream_t stream) {
    QArgs a = {};
    a.x = static_cast<const uint16_t*>(s.gate); a.up = static_cast<const uint16_t*>(s.up);
    a.codes = static_cast<uint8_t*>(s.codes);
    a.scales = static_cast<float*>(s.scales);
    a.x_rs = s.gate_row_stride; a.up_rs = s.up_row_stride; a.codes_rs = s.codes_row_stride; a.rows = s.rows;
    a.n = s.n;
    a.q = quant_rule(s.mode, s.has_scale_ub, s.scale, s.scale_ub);
    const QuantShape sh = quant_shape(s.n, false);
    if (s.dtype == FA_BF16) launch_quant_act_kind<bf16_tag>(a, s.activation, sh, stream);
    else                    launch_quant_act_kind<fp16_tag>(a, s.activation, sh, stream);
}

// ---- fa_add_norm_quant: fa_add_norm.h's two bodies - the code fa_add_norm runs - with the epilogue below in place of the store
struct AnqArgs {
    AnArgs an;
    uint8_t* codes;
    float* scales;
    int64_t codes_rs;
    QRule q;
};

// the lane's pieces of `out` packed as fa_add_norm's store would have written them (absent pieces: +0), then the rule on the row
template <typename T, int NP>
struct AnqEmit {
    const AnqArgs& aq;
    float* red_max;                                       // quant_emit_wide's LDS (the small form: nullptr)
    u32x4 y[NP];
    __device__ __forceinline__ AnqEmit(const AnqArgs& aq_, float* red_max_) : aq(aq_), red_max(red_max_) {
#pragma unroll
        for (int p = 0; p < NP; ++p) y[p] = u32x4{0, 0, 0, 0};
    }
    __device__ __forceinline__ void piece(const AnArgs&, int p, int64_t, int, const float (&v)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) y[p][i] = Elem<T>::pack2(v[2 * i], v[2 * i + 1]);   // (row_store8's rounding)
    }
    __device__ __forceinline__ void row(int64_t row, bool act, int d, int lanes) {
        quant_emit_small<T>(aq.q, aq.codes + row * aq.codes_rs, true, aq.scales, row, aq.an.n, y[0], act, d, lanes);
    }
    __device__ __forceinline__ void row(int64_t row, const bool (&on)[NP], const int (&d)[NP]) {
        quant_emit_wide<T, NP>(aq.q, aq.codes + row * aq.codes_rs, true, aq.scales, row, aq.an.n, y, on, d, red_max);
    }
};

template <typename T, bool LN>
__global__ void __launch_bounds__(ROW_THREADS) add_norm_quant_small_kernel(const AnqArgs aq) {
    AnqEmit<T, 1> epi(aq, nullptr);
    an_small_body<T, LN>(aq.an, epi);
}

template <typename T, bool LN, int NP>
__global__ void __launch_bounds__(ROW_THREADS) add_norm_quant_wide_kernel(const AnqArgs aq) {
    __shared__ float red[2][ROW_WAVES];
    __shared__ float red_max[QUANT_MAX_WAVES];
    AnqEmit<T, NP> epi(aq, red_max);
    an_wide_body<T, LN, NP>(aq.an, red, epi);
}

template <typename T, bool LN>
static void launch_anq(const AnqArgs& a, const RowShape& sh, hipStream_t stream) {
    if (a.an.n <= ROW_SMALL_MAX) {
        const int per = ROW_THREADS >> sh.group_log2;
        const dim3 g((unsigned)((a.an.rows + per - 1) / per)), b(ROW_THREADS);
        hipLaunchKernelGGL((add_norm_quant_small_kernel<T, LN>), g, b, 0, stream, a);
        return;
    }
    const dim3 g((unsigned)a.an.rows), b(sh.threads);
    switch (sh.pieces) {
    case 1:  hipLaunchKernelGGL((add_norm_quant_wide_kernel<T, LN, 1>), g, b, 0, stream, a); break;
    case 2:  hipLaunchKernelGGL((add_norm_quant_wide_kernel<T, LN, 2>), g, b, 0, stream, a); break;
    case 4:  hipLaunchKernelGGL((add_norm_quant_wide_kernel<T, LN, 4>), g, b, 0, stream, a); break;
    default: hipLaunchKernelGGL((add_norm_quant_wide_kernel<T, LN, 8>), g, b, 0, stream, a); break;
    }
}

// The caller (fa_api.hip) has validated the block; rows > 0
void launch_add_norm_quant(const fa_add_norm_quant_params& sq, hipStream_t stream) {
    const fa_add_norm_params& s = sq.norm;
    const RowShape sh = row_shape(s.n);
    AnqArgs aq = {};
    aq.an = an_args(s, sh);                               // (out: null, never stored to)
    aq.codes = static_cast<uint8_t*>(sq.codes);
    aq.scales = static_cast<float*>(sq.scales);
    aq.codes_rs = sq.codes_row_stride;
    aq.q = quant_rule(sq.mode, sq.has_scale_ub, sq.scale, sq.scale_ub);
    const bool ln = !s.is_rms_norm;
    if (s.dtype == FA_BF16) {
        if (ln) launch_anq<bf16_tag, true>(aq, sh, stream);
        else    launch_anq<bf16_tag, false>(aq, sh, stream);
    } else {
        if (ln) launch_anq<fp16_tag, true>(aq, sh, stream);
        else    launch_anq<fp16_tag, false>(aq, sh, stream);
    }
}

}  // namespace fa
