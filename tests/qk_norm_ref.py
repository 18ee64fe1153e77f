"""fp64 reference of the per-head RMSNorm for the tests of fa_qk_norm_rope_store (a plain helper module, like rotary_ref.py: no
fixtures).

  rms_norm_ref()   y = x / sqrt(mean(x^2) + float32(eps)) * (float32(offset) + w) in fp64 on the 16-bit (or fp32) inputs as they
                   are, over the last dimension.
  ulp16()          the output type's ulp at a value (fp16: never below the subnormal spacing 2^-24).
  bound()          |got - ref| <= 0.5 ulp16(ref) + 2^-16 |ref| per element: the ONE rounding of the kernel's fp32 result to the io
                   type, plus the fp32 evaluation.  The second term adds up, relative to the result, as: a sum of at most 256
                   positive fp32 terms, each rounded once, is off by at most (D - 1) 2^-24 <= 255 x 2^-24; the root halves that
                   (< 2^-17); the division by head_dim, the sum with eps, the root and the reciprocal round once each (4 x 2^-24),
                   offset + w and the two products once each (3 x 2^-24); 2^-17 + 7 x 2^-24 < 2^-16.  Derived, not measured."""
import numpy as np
import torch

MANT = {torch.bfloat16: 7, torch.float16: 10}                     # explicit mantissa bits of the io type
EMIN = {torch.bfloat16: -126, torch.float16: -14}                 # exponent of the smallest normal number


def rms_norm_ref(x, w, eps, offset=0.0):
    """x [..., D] tensor, w [D] tensor -> fp64 array of x's shape"""
    x = x.detach().double().cpu().numpy()
    w = w.detach().double().cpu().numpy()
    ms = np.mean(x * x, axis=-1, keepdims=True)
    return x / np.sqrt(ms + float(np.float32(eps))) * (float(np.float32(offset)) + w)


def ulp16(ref, dtype):
    a = np.abs(np.asarray(ref, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** EMIN[dtype])))
    return 2.0 ** (np.maximum(e, EMIN[dtype]) - MANT[dtype])


def bound(ref, dtype):
    return 0.5 * ulp16(ref, dtype) + 2.0 ** -16 * np.abs(ref)


def worst_ratio(got, ref, dtype):
    """max over elements of |got - ref| / bound; a non-finite output fails"""
    g = got.detach().double().cpu().numpy()
    assert np.isfinite(g).all(), "non-finite values in the kernel's output"
    return float(np.max(np.abs(g - ref) / bound(ref, dtype)))
