// fa_mx_quant.hip - 16-bit expert weights to MXFP4 (fa_mx_quant) and back (fa_mx_dequant): the uint8 [E, n, k / 2] codes and
// uint8 [E, n, k / 32] E8M0 scale bytes fa_moe_gemm_mxfp4 reads.  include/fa_mi355.h states the rule on real values; here it is
// on bits, per block of 32 k of one weight row, x_i widened to fp32 (exact for fp16, subnormals included):
//     a16    = max over the block of the 15 magnitude bits of the 16-bit values (their integer order is the order of |x|, and a
//              NaN or an infinity is the largest); A = a16 as the fp32 bits of amax                        mx_amax_bits
//     byte   = 255 if A >= 0x7f800000; 127 if A == 0; else clamp((A >> 23) - 2 + (rceil and (A & 0x7fffff) > 0x400000), 2, 252)
//     code_i = v_cvt_scalef32_pk_fp4_bf16 / _f16 of x_i under the scale 2^(byte - 127), two elements an instruction into one byte
//              of a dword, the low nibble the first (mx_cvt2).  tools/probes/probe_cvt_fp4_quant.hip ran every finite bit pattern
//              of both types through it under the scale bytes 2, 3, 100, 126 .. 128, 140, 251 and 252 and found the header's
//              step 4 bit for bit: nearest e2m1 magnitude, a tie to the even code, above 6 to 6, the sign kept on a zero, 16-bit
//              subnormals counted (profiles/probe_cvt_fp4_quant.txt).  byte 255: every code 0, whatever the instruction gives.
// Ownership:
//   "nk" (mx_quant_nk_kernel, mx_dequant_nk_kernel): an expert is dense, so its n * k / 8 pieces of 8 elements - 16 bytes of w, one
//     dword of codes - are one flat run; 4 adjacent lanes hold a block, 16 adjacent lanes 4 scale bytes.  A workgroup of 256 lanes
//     takes 1024 pieces, a lane the pieces t, t + 256, ..: four 16-byte loads in flight, then per piece two xor steps inside the
//     quad for the amax, one dword of codes a lane and one dword of 4 scale bytes per 16 lanes (an expert's scales that do not
//     start on a 4-byte boundary: a byte per quad).  n * k / 8 is a multiple of 32: quads and groups of 16 are whole.  No LDS.
//   "kn" (mx_quant_kn_kernel, mx_dequant_kn_kernel): the 32 elements of a block lie n elements apart.  A workgroup of 256 lanes
//     takes a tile of 128 k x 64 n.  Lane t = 8 q + c holds the 8 columns 8 c .. 8 c + 7 of the 4 rows 4 q .. 4 q + 3: four 16-byte
//     loads along n, and wave v holds exactly block v of the tile.  The amax of a column is a packed 16-bit maximum over the lane's 4
//     rows and three xor steps (8, 16, 32) over the wave's 8 row groups.  The turn happens on the CODES, not on the 16-bit values:
//     a lane has for each of its 8 columns the 4 codes of its rows - 2 bytes of that column's code row - and writes them into an
//     LDS image [64 n][64 bytes] in which every 8 rows start 16 bytes further (row 8 c + i at 64 (8 c + i) + 16 c): the 64 lanes of a
//     wave then write 32 different dwords (4 c + q / 2, the two q of a dword its halves), and the 16-byte reads of the way out are
//     consecutive.  256 lanes read 16 bytes each - lane r row r / 4, k 32 (r % 4) .. - and store them: 64 contiguous bytes of codes
//     a row.  The scale bytes meet in an image [4 blocks][64 n] and leave as one dword a row (bytes where k / 32 is no multiple
//     of 4 or the row does not start on a 4-byte boundary).  fa_mx_dequant to "kn" is the same turn backwards.
//     Columns past n and rows past k are loaded as zeros and never stored; k is a multiple of 32, so a block is whole or absent.
// Every cross-lane read sits outside every lane-dependent branch; every load of a lane is issued before its first store; no
// atomics; every offset is 64-bit.  Dequantisation is v_cvt_scalef32_pk_bf16_fp4, as in fa_moe_gemm_mxfp4.hip, for the scale
// bytes 2 .. 252 and integer arithmetic (mx_deq_slow) for 0, 1, 253, 254 and 255.
#include <cstdint>
#include "fa_common.h"
#include "fa_rowops.h"

namespace fa {

constexpr int MXQ_THREADS = 256;
constexpr int MXQ_U = 4;                                    // pieces of a lane in the "nk" kernels
constexpr int MXQ_TK = 128, MXQ_TN = 64;                    // the "kn" tile
constexpr int MXQ_CIMG = MXQ_TN * 64 + (MXQ_TN / 8) * 16;   // its image of codes, bytes
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

struct MxArgs {
    const uint16_t* w;                                      // fa_mx_quant's input
    uint16_t* out;                                          // fa_mx_dequant's output
    uint8_t *blocks, *scales;                               // written by the one, read by the other
    int64_t w_es, blocks_es, scales_es;                     // expert strides: elements of w / out, bytes, bytes
    int n, k, rceil;
};

__device__ __forceinline__ uint32_t mx_pkmax(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

// the 15 magnitude bits of a 16-bit value as the fp32 bits of that magnitude (a NaN or infinity: >= 0x7f800000)
template <typename T>
__device__ __forceinline__ uint32_t mx_amax_bits(uint32_t a16) {
    if constexpr (__is_same(T, bf16_tag)) return a16 << 16;
    else return a16 >= 0x7c00u ? 0x7f800000u : __builtin_bit_cast(uint32_t, Elem<T>::lo(a16));
}

__device__ __forceinline__ uint32_t mx_scale_byte(uint32_t A, int rceil) {
    if (A >= 0x7f800000u) return 255u;
    if (A == 0u) return 127u;
    const int b = (int)(A >> 23) - 2 + ((rceil && (A & 0x7fffffu) > 0x400000u) ? 1 : 0);
    return (uint32_t)(b < 2 ? 2 : (b > 252 ? 252 : b));
}

// the scale operand of the conversion: 2^(byte - 127) for the bytes 2 .. 252 (255: the codes are dropped, any finite value will do)
__device__ __forceinline__ float mx_cvt_scale(uint32_t byte) { return __builtin_bit_cast(float, (byte == 255u ? 127u : byte) << 23); }

// `old` with byte SEL replaced by the codes of the two 16-bit values of `pair`: bits 0 .. 3 the low one's, 4 .. 7 the high one's
template <typename T, int SEL>
__device__ __forceinline__ uint32_t mx_cvt2(uint32_t old, uint32_t pair, float scale) {
    if constexpr (__is_same(T, bf16_tag)) return __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(old, __builtin_bit_cast(bf16x2, pair), scale, SEL);
    else return __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(old, __builtin_bit_cast(f16x2, pair), scale, SEL);
}

// one bf16 of e2m1(c) * 2^(b - 127) for the scale bytes the conversion instruction is not used for (0, 1, 253, 254, 255)
__device__ __forceinline__ uint32_t mx_deq_slow(uint32_t c, uint32_t b) {
    if (b == 255u) return 0x7fc0u;
    const uint32_t sign = (c & 8u) << 12, mag = c & 7u;
    if (mag == 0u) return sign;
    const int e = (int)(mag >> 1);                          // e = 0: 0.5; else (1 + (mag & 1) / 2) 2^(e - 1)
    const int ex = (int)b + (e == 0 ? -1 : e - 1);          // the biased bf16 exponent
    const uint32_t mant = e == 0 ? 0u : (mag & 1u) << 6;
    if (ex >= 255) return sign | 0x7f80u;
    if (ex <= 0) return sign | ((0x80u | mant) >> (1 - ex));    // a subnormal, exact: the shift is at most 2
    return sign | ((uint32_t)ex << 7) | mant;
}

// the two bf16 of byte SEL of `codes` (the low nibble first) under the scale byte b
template <int SEL>
__device__ __forceinline__ uint32_t mx_deq2(uint32_t codes, uint32_t b) {
    if (b - 2u <= 250u)
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, __builtin_bit_cast(float, b << 23), SEL));
    const uint32_t c = codes >> (8 * SEL);
    return mx_deq_slow(c & 15u, b) | (mx_deq_slow((c >> 4) & 15u, b) << 16);
}

// ---- "nk"
template <typename T>
__global__ void __launch_bounds__(MXQ_THREADS) mx_quant_nk_kernel(const MxArgs a) {
    const int64_t pieces = (int64_t)a.n * a.k / 8;
    const int64_t e = blockIdx.y;
    const uint16_t* w = a.w + e * a.w_es;
    uint8_t* blocks = a.blocks + e * a.blocks_es;
    uint8_t* scales = a.scales + e * a.scales_es;
    const bool s4 = (reinterpret_cast<uintptr_t>(scales) & 3) == 0;
    const int tid = (int)threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * (MXQ_THREADS * MXQ_U) + tid;
    u32x4 x[MXQ_U];
    bool on[MXQ_U];
#pragma unroll
    for (int u = 0; u < MXQ_U; ++u) {
        const int64_t i = first + u * MXQ_THREADS;
        on[u] = i < pieces;
        x[u] = u32x4{0, 0, 0, 0};
        if (on[u]) x[u] = ld_nt16(w + 8 * i);
    }
#pragma unroll
    for (int u = 0; u < MXQ_U; ++u) {
        const int64_t i = first + u * MXQ_THREADS;
        const uint32_t m = 0x7fff7fffu;
        const uint32_t pk = mx_pkmax(mx_pkmax(x[u][0] & m, x[u][1] & m), mx_pkmax(x[u][2] & m, x[u][3] & m));
        uint32_t a16 = max(pk & 0xffffu, pk >> 16);
        a16 = max(a16, (uint32_t)__shfl_xor((int)a16, 1));
        a16 = max(a16, (uint32_t)__shfl_xor((int)a16, 2));
        const uint32_t byte = mx_scale_byte(mx_amax_bits<T>(a16), a.rceil);
        const float sc = mx_cvt_scale(byte);
        uint32_t c = 0;
        c = mx_cvt2<T, 0>(c, x[u][0], sc);
        c = mx_cvt2<T, 1>(c, x[u][1], sc);
        c = mx_cvt2<T, 2>(c, x[u][2], sc);
        c = mx_cvt2<T, 3>(c, x[u][3], sc);
        if (byte == 255u) c = 0;
        const uint32_t b4 = byte | ((uint32_t)__shfl_down((int)byte, 4) << 8) | ((uint32_t)__shfl_down((int)byte, 8) << 16) |
                            ((uint32_t)__shfl_down((int)byte, 12) << 24);
        if (on[u]) {
            *reinterpret_cast<uint32_t*>(blocks + 4 * i) = c;
            if (s4) {
                if ((tid & 15) == 0) *reinterpret_cast<uint32_t*>(scales + (i >> 2)) = b4;
            } else if ((tid & 3) == 0) {
                scales[i >> 2] = (uint8_t)byte;
            }
        }
    }
}

__global__ void __launch_bounds__(MXQ_THREADS) mx_dequant_nk_kernel(const MxArgs a) {
    const int64_t pieces = (int64_t)a.n * a.k / 8;
    const int64_t e = blockIdx.y;
    const uint8_t* blocks = a.blocks + e * a.blocks_es;
    const uint8_t* scales = a.scales + e * a.scales_es;
    uint16_t* out = a.out + e * a.w_es;
    const int64_t first = (int64_t)blockIdx.x * (MXQ_THREADS * MXQ_U) + (int)threadIdx.x;
    uint32_t c[MXQ_U], b[MXQ_U];
    bool on[MXQ_U];
#pragma unroll
    for (int u = 0; u < MXQ_U; ++u) {
        const int64_t i = first + u * MXQ_THREADS;
        on[u] = i < pieces;
        c[u] = 0;
        b[u] = 127;
        if (on[u]) {
            c[u] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(blocks + 4 * i));
            b[u] = scales[i >> 2];
        }
    }
#pragma unroll
    for (int u = 0; u < MXQ_U; ++u) {
        const int64_t i = first + u * MXQ_THREADS;
        const u32x4 v = {mx_deq2<0>(c[u], b[u]), mx_deq2<1>(c[u], b[u]), mx_deq2<2>(c[u], b[u]), mx_deq2<3>(c[u], b[u])};
        if (on[u]) *reinterpret_cast<u32x4*>(out + 8 * i) = v;
    }
}

// ---- "kn"
// where row n of the tile's code image starts, and where the scale byte of block v, column n lies in the scale image
__device__ __forceinline__ int mx_cimg_row(int n) { return n * 64 + (n >> 3) * 16; }

// the tile's 4 scale bytes of row n, `nb` of them valid: global <-> the image's column n
__device__ __forceinline__ void mx_scales_out(uint8_t* dst, const uint8_t* simg, int n, int nb) {
    uint32_t s = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) s |= (uint32_t)simg[p * MXQ_TN + n] << (8 * p);
    if (nb == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(dst) = s;
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (p < nb) dst[p] = (uint8_t)(s >> (8 * p));
    }
}

template <typename T>
__global__ void __launch_bounds__(MXQ_THREADS) mx_quant_kn_kernel(const MxArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t cimg[MXQ_CIMG];
    __shared__ __attribute__((aligned(16))) uint8_t simg[4 * MXQ_TN];
    const int64_t e = blockIdx.z;
    const int n0 = (int)blockIdx.x * MXQ_TN, k0 = (int)blockIdx.y * MXQ_TK;
    const int tid = (int)threadIdx.x, c = tid & 7, q = tid >> 3, wave = tid >> 6;
    const uint16_t* w = a.w + e * a.w_es;
    const int ncol = n0 + 8 * c;
    u32x4 x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = k0 + 4 * q + j;
        x[j] = u32x4{0, 0, 0, 0};
        if (k < a.k && ncol < a.n) x[j] = ld_nt16(w + (int64_t)k * a.n + ncol);
    }
    uint32_t pk[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t m = 0x7fff7fffu;
        uint32_t v = mx_pkmax(mx_pkmax(x[0][d] & m, x[1][d] & m), mx_pkmax(x[2][d] & m, x[3][d] & m));
        v = mx_pkmax(v, (uint32_t)__shfl_xor((int)v, 8));
        v = mx_pkmax(v, (uint32_t)__shfl_xor((int)v, 16));
        v = mx_pkmax(v, (uint32_t)__shfl_xor((int)v, 32));
        pk[d] = v;
    }
    u32x2 sb = {0, 0};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int d = i >> 1, hi = i & 1;
        const uint32_t byte = mx_scale_byte(mx_amax_bits<T>((pk[d] >> (16 * hi)) & 0xffffu), a.rceil);
        const float sc = mx_cvt_scale(byte);
        // column 8 c + i of rows (4 q, 4 q + 1) and (4 q + 2, 4 q + 3) as pairs; h: the four codes, row 4 q in bits 0 .. 3
        const uint32_t p01 = hi ? (x[0][d] >> 16) | (x[1][d] & 0xffff0000u) : (x[0][d] & 0xffffu) | (x[1][d] << 16);
        const uint32_t p23 = hi ? (x[2][d] >> 16) | (x[3][d] & 0xffff0000u) : (x[2][d] & 0xffffu) | (x[3][d] << 16);
        uint32_t h = mx_cvt2<T, 1>(mx_cvt2<T, 0>(0u, p01, sc), p23, sc) & 0xffffu;
        if (byte == 255u) h = 0;
        *reinterpret_cast<uint16_t*>(cimg + mx_cimg_row(8 * c + i) + 2 * q) = (uint16_t)h;
        sb[i >> 2] |= byte << (8 * (i & 3));
    }
    if ((q & 7) == 0) *reinterpret_cast<u32x2*>(simg + wave * MXQ_TN + 8 * c) = sb;
    __syncthreads();
    const int n = tid >> 2, part = tid & 3;
    const u32x4 v = *reinterpret_cast<const u32x4*>(cimg + mx_cimg_row(n) + 16 * part);
    const int kb = a.k / 32;                                 // scale bytes of a row
    if (n0 + n < a.n && k0 + 32 * part < a.k)
        *reinterpret_cast<u32x4*>(a.blocks + e * a.blocks_es + (int64_t)(n0 + n) * (a.k / 2) + k0 / 2 + 16 * part) = v;
    if (tid < MXQ_TN && n0 + tid < a.n) {
        const int nb = kb - k0 / 32 < 4 ? kb - k0 / 32 : 4;
        mx_scales_out(a.scales + e * a.scales_es + (int64_t)(n0 + tid) * kb + k0 / 32, simg, tid, nb);
    }
}

__global__ void __launch_bounds__(MXQ_THREADS) mx_dequant_kn_kernel(const MxArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t cimg[MXQ_CIMG];
    __shared__ __attribute__((aligned(16))) uint8_t simg[4 * MXQ_TN];
    const int64_t e = blockIdx.z;
    const int n0 = (int)blockIdx.x * MXQ_TN, k0 = (int)blockIdx.y * MXQ_TK;
    const int tid = (int)threadIdx.x, c = tid & 7, q = tid >> 3, wave = tid >> 6;
    const int kb = a.k / 32;
    {
        const int n = tid >> 2, part = tid & 3;
        u32x4 v = {0, 0, 0, 0};
        if (n0 + n < a.n && k0 + 32 * part < a.k)
            v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.blocks + e * a.blocks_es + (int64_t)(n0 + n) * (a.k / 2) +
                                                                         k0 / 2 + 16 * part));
        uint32_t s = 0x7f7f7f7fu;                            // absent scale bytes: 127
        if (tid < MXQ_TN && n0 + tid < a.n) {
            const uint8_t* src = a.scales + e * a.scales_es + (int64_t)(n0 + tid) * kb + k0 / 32;
            const int nb = kb - k0 / 32 < 4 ? kb - k0 / 32 : 4;
            if (nb == 4 && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {
                s = *reinterpret_cast<const uint32_t*>(src);
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (p < nb) s = (s & ~(0xffu << (8 * p))) | ((uint32_t)src[p] << (8 * p));
            }
        }
        *reinterpret_cast<u32x4*>(cimg + mx_cimg_row(n) + 16 * part) = v;
        if (tid < MXQ_TN) {
#pragma unroll
            for (int p = 0; p < 4; ++p) simg[p * MXQ_TN + tid] = (uint8_t)(s >> (8 * p));
        }
    }
    __syncthreads();
    const u32x2 sb = *reinterpret_cast<const u32x2*>(simg + wave * MXQ_TN + 8 * c);
    uint32_t r01[8], r23[8];                                 // column 8 c + i: rows (4 q, 4 q + 1) and (4 q + 2, 4 q + 3)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t h = *reinterpret_cast<const uint16_t*>(cimg + mx_cimg_row(8 * c + i) + 2 * q);
        const uint32_t byte = (sb[i >> 2] >> (8 * (i & 3))) & 0xffu;
        r01[i] = mx_deq2<0>(h, byte);
        r23[i] = mx_deq2<1>(h, byte);
    }
    const int ncol = n0 + 8 * c;
    uint16_t* out = a.out + e * a.w_es;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t* r = j < 2 ? r01 : r23;
        u32x4 v;
#pragma unroll
        for (int p = 0; p < 4; ++p)
            v[p] = (j & 1) ? (r[2 * p] >> 16) | (r[2 * p + 1] & 0xffff0000u) : (r[2 * p] & 0xffffu) | (r[2 * p + 1] << 16);
        const int k = k0 + 4 * q + j;
        if (k < a.k && ncol < a.n) *reinterpret_cast<u32x4*>(out + (int64_t)k * a.n + ncol) = v;
    }
}

static dim3 mx_grid(int layout, int num_experts, int n, int k) {
    if (layout == FA_MOE_W_KN) return dim3((unsigned)((n + MXQ_TN - 1) / MXQ_TN), (unsigned)((k + MXQ_TK - 1) / MXQ_TK), (unsigned)num_experts);
    const int64_t pieces = (int64_t)n * k / 8, per = MXQ_THREADS * MXQ_U;
    return dim3((unsigned)((pieces + per - 1) / per), (unsigned)num_experts);
}

// The caller (fa_api.hip) has validated the blocks; num_experts, n, k > 0
void launch_mx_quant(const fa_mx_quant_params& s, hipStream_t stream) {
    MxArgs a = {};
    a.w = static_cast<const uint16_t*>(s.w);
    a.blocks = static_cast<uint8_t*>(s.blocks);
    a.scales = static_cast<uint8_t*>(s.scales);
    a.w_es = s.w_expert_stride; a.blocks_es = s.blocks_expert_stride; a.scales_es = s.scales_expert_stride;
    a.n = s.n; a.k = s.k; a.rceil = s.scale_rule == FA_MX_SCALE_RCEIL;
    const dim3 g = mx_grid(s.layout, s.num_experts, s.n, s.k), b(MXQ_THREADS);
    const bool bf = s.dtype == FA_BF16;
    if (s.layout == FA_MOE_W_KN) {
        if (bf) hipLaunchKernelGGL((mx_quant_kn_kernel<bf16_tag>), g, b, 0, stream, a);
        else    hipLaunchKernelGGL((mx_quant_kn_kernel<fp16_tag>), g, b, 0, stream, a);
    } else {
        if (bf) hipLaunchKernelGGL((mx_quant_nk_kernel<bf16_tag>), g, b, 0, stream, a);
        else    hipLaunchKernelGGL((mx_quant_nk_kernel<fp16_tag>), g, b, 0, stream, a);
    }
}

void launch_mx_dequant(const fa_mx_dequant_params& s, hipStream_t stream) {
    MxArgs a = {};
    a.out = static_cast<uint16_t*>(s.out);
    a.blocks = static_cast<uint8_t*>(const_cast<void*>(s.blocks));      // (read only by these kernels)
    a.scales = static_cast<uint8_t*>(const_cast<void*>(s.scales));
    a.w_es = s.out_expert_stride; a.blocks_es = s.blocks_expert_stride; a.scales_es = s.scales_expert_stride;
    a.n = s.n; a.k = s.k;
    const dim3 g = mx_grid(s.layout, s.num_experts, s.n, s.k), b(MXQ_THREADS);
    if (s.layout == FA_MOE_W_KN) hipLaunchKernelGGL(mx_dequant_kn_kernel, g, b, 0, stream, a);
    else                         hipLaunchKernelGGL(mx_dequant_nk_kernel, g, b, 0, stream, a);
}

}  // namespace fa
