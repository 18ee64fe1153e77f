// (1) ds_read_b64_tr_b8: which LDS byte lands in which (lane, byte) - every lane passes its own address (lane * 8 in a 512-byte
//     region), the region holds byte = (address & 255) in pass A and (address >> 8) | marker in pass B.
// (2) v_mfma_f32_32x32x16_fp8_fp8 operand layout: assumed lane (i = l & 31, g = l >> 5) holds A[i][8 g + b] in byte b of its
//     64-bit operand, B[8 g + b][j = l & 31] likewise; C in the usual 32 x 32 map.  Checked against a host product of small
//     integers (exact in e4m3).
// (3) v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 x e4m3, unit E8M0 scales 127), the K = 64 form of fa_fwd_fp8.hip: assumed lane
//     (i, g) holds A[i][32 g + b] in byte b (0 .. 31) of its eight dwords, B[32 g + b][j = i] likewise; C in the usual map.
// (4) the forward's O^T = V^T P^T step: an S^T accumulator PAIR (two 32 x 32 C fragments, keys 0 .. 63) packed in register order
//     into the B operand (byte b of lane half g = key 32 (b >> 4) + 8 ((b & 15) >> 2) + 4 g + (b & 3)) and V^T read from the
//     swizzled [64 keys][128 bytes] LDS image of fa_fwd_fp8.hip with four ds_read_b64_tr_b8 per 32 columns.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cmath>
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __host__ inline uint8_t e4m3_of_small(int v) {   // v in -8..8 -> OCP e4m3fn code (exact)
    if (v == 0) return 0;
    const int s = v < 0; int a = s ? -v : v;
    int e = 0; while ((1 << (e + 1)) <= a) ++e;             // a in [2^e, 2^(e+1))
    const int m = ((a << 3) >> e) & 7;                       // 3 mantissa bits (a <= 8 -> exact for a = 1..8 except 5,7? 5 = 1.25 * 4 ok, 7 = 1.75 * 4 ok)
    return (uint8_t)((s << 7) | ((e + 7) << 3) | m);
}
__global__ void k(uint8_t* out_tr, float* out_c) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[1024];
    const int l = threadIdx.x;
    for (int i = l; i < 512; i += 64) { lds[i] = (uint8_t)(i & 255); lds[512 + i] = (uint8_t)(i >> 8); }
    __syncthreads();
    typedef __attribute__((address_space(3))) i32x2* lp;
    i32x2 a = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lp)(lds + l * 8));
    i32x2 b = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lp)(lds + 512 + l * 8));
    for (int j = 0; j < 8; ++j) {
        out_tr[l * 16 + j] = (uint8_t)(((j < 4 ? a[0] : a[1]) >> (8 * (j & 3))) & 255);
        out_tr[l * 16 + 8 + j] = (uint8_t)(((j < 4 ? b[0] : b[1]) >> (8 * (j & 3))) & 255);
    }
    // ---- MFMA layout ----
    const int i = l & 31, g = l >> 5;
    uint64_t av = 0, bv = 0;
    for (int bb = 0; bb < 8; ++bb) {
        const int kk = 8 * g + bb;
        av |= (uint64_t)e4m3_of_small(((i * 3 + kk * 5) % 9) - 4) << (8 * bb);      // A[i][kk]
        bv |= (uint64_t)e4m3_of_small(((i * 7 + kk * 2) % 7) - 3) << (8 * bb);      // B[kk][j = i]
    }
    f32x16 c;
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    c = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8((long)av, (long)bv, c, 0, 0, 0);
    for (int r = 0; r < 16; ++r) out_c[l * 16 + r] = c[r];
}
typedef int i32x8 __attribute__((ext_vector_type(8)));
__device__ __host__ inline int a64(int i, int k) { return ((i * 5 + k * 3) % 11) - 5; }      // asymmetric in (i, k)
__device__ __host__ inline int b64(int k, int j) { return ((k * 7 + j * 2) % 9) - 4; }
__device__ __host__ inline int pkey(int key, int j) { return ((key * 3 + j * 5) % 7) - 3; }  // P[j][key] (any sign: a layout test)
__device__ __host__ inline int vval(int key, int d) { return ((key * 5 + d * 3) % 9) - 4; }  // V[key][d], column-distinct
__device__ inline int v8_fv128(int key) { return (((key >> 3) & 1) << 2) | (key & 3); }
__global__ void k64(float* out_c, float* out_o) {
    __shared__ __attribute__((aligned(16))) uint8_t vs[64 * 128];
    const int l = threadIdx.x, i = l & 31, g = l >> 5;
    // (3) plain K = 64 product
    i32x8 av, bv;
    for (int w = 0; w < 8; ++w) {
        uint32_t aw = 0, bw = 0;
        for (int e = 0; e < 4; ++e) {
            const int kk = 32 * g + 4 * w + e;
            aw |= (uint32_t)e4m3_of_small(a64(i, kk)) << (8 * e);
            bw |= (uint32_t)e4m3_of_small(b64(kk, i)) << (8 * e);
        }
        av[w] = (int)aw; bv[w] = (int)bw;
    }
    f32x16 c;
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 0, 0, 0, 127, 0, 127);
    for (int r = 0; r < 16; ++r) out_c[l * 16 + r] = c[r];
    // (4) V image: logical byte d of key row `key` at key * 128 + (d ^ (fv(key) << 4))
    for (int x = l; x < 64 * 128; x += 64) {
        const int key = x / 128, d = x % 128;
        vs[key * 128 + (d ^ (v8_fv128(key) << 4))] = e4m3_of_small(vval(key, d));
    }
    __syncthreads();
    // P^T fragment from an S^T accumulator pair: register r of block kb holds key 32 kb + (r & 3) + 8 (r >> 2) + 4 g, query i
    i32x8 pf;
    for (int w = 0; w < 8; ++w) {
        uint32_t pw = 0;
        for (int e = 0; e < 4; ++e) {
            const int kb = w >> 2, r = 4 * (w & 3) + e;
            const int key = 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * g;
            pw |= (uint32_t)e4m3_of_small(pkey(key, i)) << (8 * e);
        }
        pf[w] = (int)pw;
    }
    const int sl = l & 15, gg = l >> 4, jj = sl >> 1;
    const int key_l = (jj & 3) + 8 * (jj >> 2) + 4 * (gg >> 1);
    typedef __attribute__((address_space(3))) i32x2* lp;
    for (int d = 0; d < 4; ++d) {
        const uint8_t* base = vs + key_l * 128 + (((2 * d + (gg & 1)) ^ v8_fv128(key_l)) << 4) + 8 * (sl & 1);
        i32x8 vf;
        for (int q = 0; q < 4; ++q) {
            const i32x2 t = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lp)(base + 16 * q * 128));
            vf[2 * q] = t[0]; vf[2 * q + 1] = t[1];
        }
        f32x16 o;
        for (int r = 0; r < 16; ++r) o[r] = 0.f;
        o = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf, pf, o, 0, 0, 0, 127, 0, 127);
        for (int r = 0; r < 16; ++r) out_o[(d * 64 + l) * 16 + r] = o[r];
    }
}
int main() {
    uint8_t* dtr; float* dc; uint8_t htr[1024]; float hc[1024];
    hipMalloc(&dtr, 1024); hipMalloc(&dc, 4096);
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, dtr, dc);
    hipMemcpy(htr, dtr, 1024, hipMemcpyDeviceToHost); hipMemcpy(hc, dc, 4096, hipMemcpyDeviceToHost);
    printf("ds_read_b64_tr_b8: result byte j of lane l <- (source lane, source byte) [each lane's 8 bytes sit at lane * 8]\n");
    for (int l = 0; l < 64; ++l) {
        printf("lane %2d:", l);
        for (int j = 0; j < 8; ++j) { const int addr = htr[l * 16 + j] | (htr[l * 16 + 8 + j] << 8); printf(" (%2d,%d)", addr >> 3, addr & 7); }
        printf("\n");
    }
    int bad = 0;
    for (int l = 0; l < 64; ++l) for (int r = 0; r < 16; ++r) {
        const int col = l & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        float want = 0.f;
        for (int kk = 0; kk < 16; ++kk) want += (float)(((row * 3 + kk * 5) % 9) - 4) * (float)(((col * 7 + kk * 2) % 7) - 3);
        if (hc[l * 16 + r] != want) { if (bad < 6) printf("C[%d][%d]: %g want %g\n", row, col, hc[l * 16 + r], want); ++bad; }
    }
    printf("mfma_f32_32x32x16_fp8_fp8 with byte b of lane (i, g) = A[i][8 g + b] / B[8 g + b][j]: %s (%d mismatches)\n", bad ? "DIFFERENT" : "as assumed", bad);
    float *d64c, *d64o;
    static float h64c[1024], h64o[4 * 1024];
    hipMalloc(&d64c, sizeof(h64c)); hipMalloc(&d64o, sizeof(h64o));
    hipLaunchKernelGGL(k64, dim3(1), dim3(64), 0, 0, d64c, d64o);
    hipMemcpy(h64c, d64c, sizeof(h64c), hipMemcpyDeviceToHost); hipMemcpy(h64o, d64o, sizeof(h64o), hipMemcpyDeviceToHost);
    int bad3 = 0, bad4 = 0;
    for (int l = 0; l < 64; ++l) for (int r = 0; r < 16; ++r) {
        const int col = l & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        float want = 0.f;
        for (int kk = 0; kk < 64; ++kk) want += (float)a64(row, kk) * (float)b64(kk, col);
        if (h64c[l * 16 + r] != want) { if (bad3 < 6) printf("K64 C[%d][%d]: %g want %g\n", row, col, h64c[l * 16 + r], want); ++bad3; }
        for (int d = 0; d < 4; ++d) {
            // O^T[d-row][query col] = sum over the 64 keys of V[key][32 d + row] P[col][key]
            float wo = 0.f;
            for (int key = 0; key < 64; ++key) wo += (float)vval(key, 32 * d + row) * (float)pkey(key, col);
            if (h64o[(d * 64 + l) * 16 + r] != wo) { if (bad4 < 6) printf("O^T[%d][%d]: %g want %g\n", 32 * d + row, col, h64o[(d * 64 + l) * 16 + r], wo); ++bad4; }
        }
    }
    printf("mfma_scale_f32_32x32x64_f8f6f4 with byte b of lane (i, g) = A[i][32 g + b] / B[32 g + b][j]: %s (%d mismatches)\n", bad3 ? "DIFFERENT" : "as assumed", bad3);
    printf("S^T accumulator pair as the 64-key B operand, V^T by ds_read_b64_tr_b8 in the matching key order: %s (%d mismatches)\n", bad4 ? "DIFFERENT" : "as assumed", bad4);
    return (bad || bad3 || bad4) ? 1 : 0;
}
