// fa_act.h - the activations of fa_act_mul / fa_act_mul_bwd (fa_act_mul.hip) and of fa_act_mul_quant (fa_quant.hip): ONE definition
// of act(g) and act'(g), so the quantising form rounds exactly the value the 16-bit op stores.  The fp32 order of every line is
// part of the contract (fa_act_mul.hip's header, include/fa_mi355.h).
#pragma once
#include <cmath>
#include "fa_common.h"

namespace fa {

constexpr float kActK2 = 1.5957691216057308f;               // 2 sqrt(2 / pi)
constexpr float kActC3 = 0.044715f;
constexpr float kAct3C3 = 0.134145f;
constexpr float kActRsqrt2 = 0.7071067811865476f;
constexpr float kActRsqrt2Pi = 0.3989422804014327f;

__device__ __forceinline__ float act_exp(float t) { return fast_exp2(t * kLog2e); }
__device__ __forceinline__ float act_sig(float t) { return fast_rcp(1.0f + act_exp(-t)); }
__device__ __forceinline__ float act_relu(float g) { return g <= 0.f ? 0.f : g; }

// act(g) and - WANT_D - act'(g)
template <int ACT, bool WANT_D>
__device__ __forceinline__ void act_eval(float g, float& a, float& d) {
    d = 0.f;
    if constexpr (ACT == FA_ACT_SILU) {
        const float s = act_sig(g);
        a = g * s;
        if constexpr (WANT_D) d = s * fmaf(g, 1.0f - s, 1.0f);
    } else if constexpr (ACT == FA_ACT_GELU_TANH) {
        const float q = g * g;
        const float w = (kActK2 * g) * fmaf(kActC3, q, 1.0f);
        const float s = act_sig(w);
        a = g * s;
        if constexpr (WANT_D) d = s * fmaf(g * (1.0f - s), kActK2 * fmaf(kAct3C3, q, 1.0f), 1.0f);
    } else if constexpr (ACT == FA_ACT_GELU) {
        const float ph = fmaf(0.5f, erff(g * kActRsqrt2), 0.5f);
        a = g * ph;
        if constexpr (WANT_D) d = fmaf(g, act_exp((g * g) * -0.5f) * kActRsqrt2Pi, ph);
    } else if constexpr (ACT == FA_ACT_RELU) {
        a = act_relu(g);
        if constexpr (WANT_D) d = g <= 0.f ? 0.f : (g > 0.f ? 1.0f : g);
    } else {
        const float r = act_relu(g);
        a = r * r;
        if constexpr (WANT_D) d = r + r;
    }
}

}  // namespace fa
