// Probe: semantics of gfx950's v_cvt_scalef32_pk_bf16_fp4 (2 x e2m1 -> 2 x bf16, one VALU op), as fa_moe_gemm_mxfp4.hip uses it.
// Questions: (1) which byte of the source dword does byte_sel = 0..3 name, (2) which nibble of that byte becomes element 0 of
// the result, (3) is `scale` (built as scale_byte << 23) applied exactly for scale bytes 2, 126..128 and 252, and (4) what do
// the bytes 0 and 255 (outside the op's contract) give with a zero code.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
#include <cstdint>
typedef __bf16 b2 __attribute__((ext_vector_type(2)));
__global__ void k(const uint32_t* words, const uint32_t* scale_bytes, float* out) {
    // thread t: word t / 8, scale (t % 8); writes 8 floats: byte_sel 0..3, elements 0..1
    const uint32_t w = words[threadIdx.x / 8];
    const float sc = __builtin_bit_cast(float, scale_bytes[threadIdx.x % 8] << 23);
    float* o = out + threadIdx.x * 8;
    b2 r;
    r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0); o[0] = (float)r[0]; o[1] = (float)r[1];
    r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1); o[2] = (float)r[0]; o[3] = (float)r[1];
    r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2); o[4] = (float)r[0]; o[5] = (float)r[1];
    r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3); o[6] = (float)r[0]; o[7] = (float)r[1];
}
int main() {
    static const float e2m1[16] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f, -0.f, -0.5f, -1.f, -1.5f, -2.f, -3.f, -4.f, -6.f};
    const uint32_t words[4] = {0x76543210u, 0xfedcba98u, 0x00000000u, 0x88888888u};
    const uint32_t sb[8] = {127, 126, 128, 2, 252, 0, 255, 1};
    uint32_t *dw, *ds; float* dout; float out[32 * 8];
    if (hipMalloc(&dw, sizeof words) || hipMalloc(&ds, sizeof sb) || hipMalloc(&dout, sizeof out)) return 2;
    hipMemcpy(dw, words, sizeof words, hipMemcpyHostToDevice);
    hipMemcpy(ds, sb, sizeof sb, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(1), dim3(32), 0, 0, dw, ds, dout);
    if (hipMemcpy(out, dout, sizeof out, hipMemcpyDeviceToHost)) return 3;
    int bad = 0;
    for (int t = 0; t < 32; ++t) {
        const uint32_t w = words[t / 8], s = sb[t % 8];
        printf("word %08x scale byte %3u:", w, s);
        for (int i = 0; i < 8; ++i) {
            printf(" %g", out[t * 8 + i]);
            // the storage order fa_moe_gemm_mxfp4 assumes: element i of the dword = nibble i (byte i / 2, low nibble first)
            const double want = std::ldexp((double)e2m1[(w >> (4 * i)) & 15], (int)s - 127);
            if (s >= 2 && s <= 252 && (double)out[t * 8 + i] != want) ++bad;
        }
        printf("\n");
    }
    printf("mismatches against 'byte_sel i = bits 8i+7..8i, low nibble first' over scale bytes 2..252: %d\n", bad);
    return 0;
}
