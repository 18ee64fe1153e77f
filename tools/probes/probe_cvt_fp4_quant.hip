// Probe: does gfx950's v_cvt_scalef32_pk_fp4_bf16 / _f16 (2 x 16-bit -> 2 x e2m1 into one byte of a dword) round and saturate as
// fa_mx_quant's rule says (include/fa_mi355.h, step 4)?  Every one of the 65536 bit patterns of both types goes through the
// instruction under a handful of scale bytes, as element 0 and as element 1 of the pair and into each of the four bytes; the host
// compares with the rule: code = sign | nearest of 0, .5, 1, 1.5, 2, 3, 4, 6 to |x| / 2^(byte - 127), a tie to the even code, above
// 6 to 6, a negative value that rounds to zero 0x8.  NaN and +-inf inputs are outside the rule (their block is dropped) and are
// only reported.  `scale` is built as byte << 23, as fa_moe_gemm_mxfp4.hip builds it for the opposite conversion.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
typedef __bf16 b2 __attribute__((ext_vector_type(2)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

// thread t: pattern t & 0xffff; out[s * 65536 + t] = the dword after four conversions of (pattern, 1.0 * 2^(byte - 127))
template <bool BF>
__global__ void k(const uint32_t* scale_bytes, int ns, uint32_t* out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, pat = t & 0xffffu;
    for (int s = 0; s < ns; ++s) {
        const uint32_t sb = scale_bytes[s];
        const float sc = __builtin_bit_cast(float, sb << 23);
        const uint32_t one = BF ? (sb << 7) : 0x3c00u;       // bf16: 2^(byte - 127), code 2 after scaling; fp16: 1.0
        const uint32_t a = pat | (one << 16), b = one | (pat << 16);
        uint32_t r = 0xffffffffu;
        if constexpr (BF) {
            r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(r, __builtin_bit_cast(b2, a), sc, 0);
            r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(r, __builtin_bit_cast(b2, b), sc, 1);
            r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(r, __builtin_bit_cast(b2, a), sc, 2);
            r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(r, __builtin_bit_cast(b2, b), sc, 3);
        } else {
            r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(r, __builtin_bit_cast(h2, a), sc, 0);
            r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(r, __builtin_bit_cast(h2, b), sc, 1);
            r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(r, __builtin_bit_cast(h2, a), sc, 2);
            r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(r, __builtin_bit_cast(h2, b), sc, 3);
        }
        out[(size_t)s * 65536 + t] = r;
    }
}

static double value(uint32_t pat, bool bf) {
    if (bf) { const uint32_t u = pat << 16; float f; memcpy(&f, &u, 4); return f; }
    const int e = (pat >> 10) & 31, m = pat & 1023;
    const double v = e == 0 ? std::ldexp((double)m, -24) : (e == 31 ? (m ? NAN : INFINITY) : std::ldexp(1024.0 + m, e - 25));
    return (pat & 0x8000) ? -v : v;
}

static uint32_t rule(double x, int sb) {
    static const double grid[8] = {0, .5, 1, 1.5, 2, 3, 4, 6};
    double y = std::ldexp(std::fabs(x), 127 - sb);
    if (y > 6) y = 6;
    int best = 0;
    for (int c = 1; c < 8; ++c) {
        const double d = std::fabs(y - grid[c]), db = std::fabs(y - grid[best]);
        if (d < db || (d == db && (c & 1) == 0)) best = c;
    }
    return (uint32_t)best | (std::signbit(x) ? 8u : 0u);
}

int main() {
    const uint32_t sb[] = {2, 3, 100, 126, 127, 128, 140, 251, 252};
    const int ns = sizeof sb / sizeof sb[0];
    uint32_t *dsb, *dout;
    static uint32_t out[ns * 65536];
    if (hipMalloc(&dsb, sizeof sb) || hipMalloc(&dout, sizeof out)) return 2;
    hipMemcpy(dsb, sb, sizeof sb, hipMemcpyHostToDevice);
    for (int bf = 1; bf >= 0; --bf) {
        if (bf) hipLaunchKernelGGL(k<true>, dim3(256), dim3(256), 0, 0, dsb, ns, dout);
        else    hipLaunchKernelGGL(k<false>, dim3(256), dim3(256), 0, 0, dsb, ns, dout);
        if (hipMemcpy(out, dout, sizeof out, hipMemcpyDeviceToHost)) return 3;
        long bad = 0, bad_layout = 0, shown = 0;
        for (int s = 0; s < ns; ++s) {
            for (uint32_t p = 0; p < 65536; ++p) {
                const double x = value(p, bf);
                const uint32_t r = out[(size_t)s * 65536 + p];
                const double one = bf ? std::ldexp(1.0, (int)sb[s] - 127) : 1.0;
                const uint32_t c1 = rule(one, sb[s]);
                if (std::isnan(x) || std::isinf(x)) {
                    if (s == 4 && (p == 0x7f80 || p == 0xff80 || p == 0x7fc0 || p == 0x7c00 || p == 0xfc00 || p == 0x7e00))
                        printf("%s pattern %04x (non-finite), byte 127: dword %08x\n", bf ? "bf16" : "fp16", p, r);
                    continue;
                }
                const uint32_t c = rule(x, sb[s]);
                // bytes 0, 2: (pattern low, one high) -> low nibble the pattern's code; bytes 1, 3: the other way round
                const uint32_t want = (c | c1 << 4) | (c1 | c << 4) << 8 | (c | c1 << 4) << 16 | (c1 | c << 4) << 24;
                if (r != want) {
                    const bool value_wrong = (r & 15u) != c;
                    value_wrong ? ++bad : ++bad_layout;
                    if (shown++ < 12) printf("%s pattern %04x (%g) byte %u: got %08x want %08x\n", bf ? "bf16" : "fp16", p, x, sb[s], r, want);
                }
            }
        }
        printf("%s: %ld finite (pattern, scale byte) pairs whose code differs from the rule, %ld more where only the packing differs\n",
               bf ? "bf16" : "fp16", bad, bad_layout);
    }
    return 0;
}
