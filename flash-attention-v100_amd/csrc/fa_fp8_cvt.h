// fa_fp8_cvt.h - the fp8-e4m3 rounding rule of the KV-cache writers: fa_fwd_kvcache's append (fa_kvcache.hip) and fa_kv_store
// (fa_kv_store.hip) include this one definition, so both store the same code for the same value and descale.
//   code = e4m3(clamp(x * (1 / descale), -448, 448)), the hardware conversion (round to nearest even, OCP e4m3)
// and the way back, for fa_kv_gather (fa_kv_gather.hip):
//   value = round_to_nearest_even_to_16_bit(fp32(code) * descale): the exact conversion, ONE fp32 multiply, one rounding
#pragma once
#include "fa_common.h"

namespace fa {

// the reciprocal both writers multiply by: one fp32 division on the device
__device__ __forceinline__ float fp8_inv_descale(float descale) { return 1.0f / descale; }

// 8 x 16-bit -> 8 x fp8-e4m3 (OCP), value / descale, saturating at +-448
template <typename T>
__device__ __forceinline__ u32x2 to_fp8x8(const u32x4& x, float inv_descale) {
    using E = Elem<T>;
    u32x2 r = {0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a0 = fminf(fmaxf(E::lo(x[i]) * inv_descale, -448.f), 448.f);
        const float a1 = fminf(fmaxf(E::hi(x[i]) * inv_descale, -448.f), 448.f);
        if (i == 0) r[0] = __builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, r[0], false);
        if (i == 1) r[0] = __builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, r[0], true);
        if (i == 2) r[1] = __builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, r[1], false);
        if (i == 3) r[1] = __builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, r[1], true);
    }
    return r;
}

// 8 x fp8-e4m3 (OCP) -> 8 x 16-bit, code * descale.  (Not the cvt_scalef32 converts of fa_common.h: their scale operand
// contributes only its exponent, which is another function for a descale that is no power of two.)
template <typename T>
__device__ __forceinline__ u32x4 from_fp8x8(const u32x2& c, float descale) {
    using E = Elem<T>;
    const f32x2 f0 = __builtin_amdgcn_cvt_pk_f32_fp8(c[0], false), f1 = __builtin_amdgcn_cvt_pk_f32_fp8(c[0], true);
    const f32x2 f2 = __builtin_amdgcn_cvt_pk_f32_fp8(c[1], false), f3 = __builtin_amdgcn_cvt_pk_f32_fp8(c[1], true);
    u32x4 r;
    r[0] = E::pack2(f0[0] * descale, f0[1] * descale);
    r[1] = E::pack2(f1[0] * descale, f1[1] * descale);
    r[2] = E::pack2(f2[0] * descale, f2[1] * descale);
    r[3] = E::pack2(f3[0] * descale, f3[1] * descale);
    return r;
}

}  // namespace fa
