// fa_mx_cvt.h - e2m1 codes to bf16 on the device, shared by the kernels that read MXFP4 weights (fa_moe_gemm_mxfp4.hip,
// fa_moe_gemm_mxfp4_dgrad.hip): v_cvt_scalef32_pk_bf16_fp4, whose low nibble becomes the low bf16 and whose byte_sel counts bytes
// from bit 0 - the storage order (probed: tools/probes/probe_cvt_fp4.hip).
#pragma once
#include "fa_common.h"
#include <type_traits>

namespace fa {

namespace {

__device__ __forceinline__ uint32_t cvt_fp4x2(uint32_t w, float scale, std::integral_constant<int, 0>) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0));
}
__device__ __forceinline__ uint32_t cvt_fp4x2(uint32_t w, float scale, std::integral_constant<int, 1>) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1));
}
__device__ __forceinline__ uint32_t cvt_fp4x2(uint32_t w, float scale, std::integral_constant<int, 2>) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2));
}
__device__ __forceinline__ uint32_t cvt_fp4x2(uint32_t w, float scale, std::integral_constant<int, 3>) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
}
// 8 codes (one dword, element i in nibble i) times 2^(scale_byte - 127) -> the 8 bf16 of an MFMA operand
__device__ __forceinline__ u32x4 dequant8(uint32_t w, uint32_t scale_byte) {
    const float sc = __builtin_bit_cast(float, scale_byte << 23);
    return u32x4{cvt_fp4x2(w, sc, std::integral_constant<int, 0>{}), cvt_fp4x2(w, sc, std::integral_constant<int, 1>{}),
                 cvt_fp4x2(w, sc, std::integral_constant<int, 2>{}), cvt_fp4x2(w, sc, std::integral_constant<int, 3>{})};
}

}  // namespace

}  // namespace fa
