"""QK-norm in front of the serving prologue, still one launch, on the library's `fa_qk_norm_rope_store` kernel
(csrc/fa_qk_norm_rope_store.hip): a per-head RMSNorm of q and of k over headdim with a learned [headdim] weight (Qwen3, Gemma 3,
OLMo 2), then `rope_store.rope_and_store_kv` - q and k rotated at PER-TOKEN positions, K and V stored into a KV cache by slot.

    y = round16(x * rsqrt(mean(x^2) + eps) * (weight_offset + w))      fp32 inside, one rounding to the io type

and that 16-bit y is what the rotation sees, as in the HF modules: `qk_norm_rope_and_store_kv` leaves the bits of `qk_rms_norm`
followed by `rope_and_store_kv`, and with no weight at all the bits of `rope_and_store_kv`.  The sum of squares has a fixed order
(csrc/fa_rmsnorm.h): a head's bits do not depend on which other rows or heads are in the batch.

Training: `qk_norm_rope` is the same norm + rotation out of place and differentiable in q, k and both weights; its backward is
`qk_norm_rope_backward`, the library's `fa_qk_norm_rope_bwd` kernel (csrc/fa_qk_norm_rope_bwd.hip).  The backward treats both
16-bit roundings of the forward as the identity (straight-through), recomputes rstd from the saved pre-norm x with the forward's
fixed-order sum, and sums dw without atomics in an order that depends on the shapes alone: it is bitwise repeatable, and a head's
dx bits do not depend on what else is in the batch.

Not covered: LayerNorm or a bias, a norm over the whole hidden size, fp32 cos / sin, rotary dims that are not multiples of 16,
M-RoPE and xPos, sequence-mode addressing, per-head or device-resident descales; in the backward also 4-D [B, S, H, D] tensors
(callers `view`), a backward through the cache store, fp32 or fp8 x and a double backward.  Nothing here is exported through the
packages' `__all__` lists."""
import ctypes
from typing import Optional

import torch

from . import _lib
from . import _rowargs as _ra
from . import flash_attn_interface as _fi


def qk_norm_rope_and_store_kv(q, k, v, positions, rotary_cos, rotary_sin, k_cache=None, v_cache=None,
                              slot_mapping: Optional[torch.Tensor] = None, *, q_weight: Optional[torch.Tensor] = None,
                              k_weight: Optional[torch.Tensor] = None, eps: float = 1e-6, weight_offset: float = 0.0,
                              interleaved: bool = False, inplace: bool = True, k_out: bool = True,
                              k_descale: Optional[float] = None, v_descale: Optional[float] = None):
    """`rope_store.rope_and_store_kv` (same tensors, same rules, same defaults) with an RMSNorm of every head of q (q_weight) and
    of k (k_weight) in front of the rotation.  q_weight, k_weight: (headdim,), of k's dtype or float32, both of the same dtype;
    either may be None - that tensor is only rotated.  weight_offset: Gemma's (1 + w) is 1.0.
    positions, rotary_cos and rotary_sin may be None together: no rotation - the call is norm only, norm + store with caches.
    A row whose position is outside the tables is normalised and left unrotated; a row whose slot is < 0 or past the cache is
    normalised and rotated, only its cache write is skipped.  v is neither normalised nor rotated.  In place a normalised tensor
    is rewritten in every column.
    Returns (q_out, k_out): q and k themselves in place, None for a missing q or with k_out=False."""
    return _ra.rope_and_store("qk_norm", _lib.FaQkNormRopeStoreParams, _lib.call_qk_norm_rope_store,
                              (q_weight, k_weight, eps, weight_offset), True, ("", "", ""), q, k, v, positions, rotary_cos, rotary_sin,
                              k_cache, v_cache, slot_mapping, interleaved, inplace, k_out, k_descale, v_descale)


def qk_rms_norm(q, k, q_weight, k_weight, eps: float = 1e-6, *, weight_offset: float = 0.0, inplace: bool = False):
    """The norm alone, on the same kernel: every head of q (or None) and of k normalised with its weight (or left as it is where
    the weight is None).  Returns (q_out, k_out); out of place by default."""
    return qk_norm_rope_and_store_kv(q, k, None, None, None, None, q_weight=q_weight, k_weight=k_weight, eps=eps,
                                     weight_offset=weight_offset, inplace=inplace)


def qk_norm_rope_backward(dq_out, dk_out, q, k, positions, rotary_cos, rotary_sin, q_weight: Optional[torch.Tensor] = None,
                          k_weight: Optional[torch.Tensor] = None, eps: float = 1e-6, weight_offset: float = 0.0,
                          interleaved: bool = False, *, inplace: bool = False, need_dq: bool = True, need_dk: bool = True,
                          need_dw: bool = True):
    """The backward of the norm + rotation of `qk_norm_rope_and_store_kv` / `qk_norm_rope`, one launch (two with a weight
    gradient): dq_out / dk_out (total_rows, nheads, headdim) are the gradients of q_out / k_out, q / k the forward's PRE-NORM
    inputs; the other arguments are the forward's.  All four tensors may be views with a contiguous last dimension (the heads of a
    packed qkv gradient are taken without a copy).  q=None (then dq_out=None): no q heads.
        dy = conj_rope(dz) in fp32, not rounded;  no weight: dx = round16(dy) - the bits of the rotary backward;
        weight: xhat = x rstd, a = dy (weight_offset + w), c = mean_d(a xhat), dx = round16(rstd (a - xhat c)), dw = sum dy xhat
    with both 16-bit roundings of the forward treated as the identity.  Every row enters dw, rows whose position is outside the
    tables included.  inplace: dq is dq_out and dk is dk_out, rewritten where they are.  need_dq / need_dk / need_dw=False skip
    that output (None in its place); dq_weight / dk_weight are also None for a tensor without a weight.
    Returns (dq, dk, dq_weight, dk_weight); the weight gradients have the weights' dtype."""
    op = "qk_norm"
    T, Hk, D = _ra.k_shape(op, k)
    if dk_out is None or dk_out.dtype != k.dtype or tuple(dk_out.shape) != tuple(k.shape):
        raise RuntimeError(f"qk_norm: dk_out must have k's dtype and shape ({k.dtype}, {tuple(k.shape)})")
    if q is not None:
        _ra.q_like_k(op, q, k, T, D)
        if dq_out is None or dq_out.dtype != q.dtype or tuple(dq_out.shape) != tuple(q.shape):
            raise RuntimeError(f"qk_norm: dq_out must have q's dtype and shape ({q.dtype}, {tuple(q.shape)})")
    elif dq_out is not None:
        raise RuntimeError("qk_norm: dq_out without q")
    Hq = 0 if q is None else q.shape[1]
    _ra.head_dim(op, D)
    rope, rotary_dim, positions = _ra.optional_rope(op, positions, rotary_cos, rotary_sin, k.dtype, T, D)
    qw, kw = _ra.norm_weights(op, q, k, q_weight, k_weight)
    eps, weight_offset = _ra.scalars(op, eps, weight_offset)
    _ra.same_device(op, [dq_out, dk_out, q, k, positions, rotary_cos, rotary_sin, qw, kw], k, "k's")

    want_dq, want_dk = bool(need_dq) and q is not None, bool(need_dk)
    qi = None if q is None else _fi._prep(q, D)
    ki = _fi._prep(k, D)
    dqo = None if q is None else _ra.view(op, dq_out, D, inplace and want_dq, "dq_out")
    dko = _ra.view(op, dk_out, D, inplace and want_dk, "dk_out")
    if inplace:
        dq, dk = (dqo if want_dq else None), (dko if want_dk else None)
    else:
        dq = torch.empty(q.shape, dtype=q.dtype, device=q.device) if want_dq else None
        dk = torch.empty(k.shape, dtype=k.dtype, device=k.device) if want_dk else None
    dqw = torch.empty(D, dtype=qw.dtype, device=k.device) if (need_dw and qw is not None) else None
    dkw = torch.empty(D, dtype=kw.dtype, device=k.device) if (need_dw and kw is not None) else None
    if dq is None and dk is None and dqw is None and dkw is None:
        return None, None, None, None
    if T == 0 or (Hq == 0 and Hk == 0):                        # (nothing to launch: a sum over no rows is zero)
        for g in (dqw, dkw):
            if g is not None:
                g.zero_()
        return dq, dk, dqw, dkw

    s = _lib.FaQkNormRopeBwdParams()
    s.struct_size = ctypes.sizeof(_lib.FaQkNormRopeBwdParams)
    if qi is not None:
        s.q, s.dq_out = qi.data_ptr(), dqo.data_ptr()
        s.q_row_stride, s.q_head_stride = qi.stride(0), qi.stride(1)
        s.dqo_row_stride, s.dqo_head_stride = dqo.stride(0), dqo.stride(1)
    s.k, s.dk_out = ki.data_ptr(), dko.data_ptr()
    s.k_row_stride, s.k_head_stride = ki.stride(0), ki.stride(1)
    s.dko_row_stride, s.dko_head_stride = dko.stride(0), dko.stride(1)
    if dq is not None:
        s.dq = dq.data_ptr()
        s.dq_row_stride, s.dq_head_stride = dq.stride(0), dq.stride(1)
    if dk is not None:
        s.dk = dk.data_ptr()
        s.dk_row_stride, s.dk_head_stride = dk.stride(0), dk.stride(1)
    if rope:
        rotary_cos, rotary_sin = _ra.fill_rope(s, positions, rotary_cos, rotary_sin, rotary_dim, interleaved)
    s.total_rows, s.nheads_q, s.nheads_k, s.head_dim = T, Hq, Hk, D
    s.dtype = _fi._DTYPES[k.dtype]
    _ra.fill_norm(s, qw, kw, eps, weight_offset)
    if dqw is not None:
        s.dq_weight = dqw.data_ptr()
    if dkw is not None:
        s.dk_weight = dkw.data_ptr()
    nbytes = _lib.qk_norm_rope_bwd_workspace_bytes(s)
    ws = None
    if nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=k.device)
        s.workspace, s.workspace_bytes = ws.data_ptr(), nbytes
    with _fi._on_device(k.device):
        _lib.call_qk_norm_rope_bwd(s, _fi._stream(k.device))     # (queued: the tensors made here stay referenced until here)
    del qi, ki, dqo, dko, positions, rotary_cos, rotary_sin, qw, kw, ws
    return dq, dk, dqw, dkw


def qk_norm_rope(q, k, positions, rotary_cos, rotary_sin, q_weight: Optional[torch.Tensor] = None,
                 k_weight: Optional[torch.Tensor] = None, eps: float = 1e-6, weight_offset: float = 0.0, interleaved: bool = False):
    """The norm + rotation of `qk_norm_rope_and_store_kv(..., inplace=False)` without caches - the same kernel, the same bits -
    as a differentiable function: (q_out, k_out), with gradients for q, k, q_weight and k_weight through `qk_norm_rope_backward`.
    q (total_rows, nheads_q, headdim) or None, k (total_rows, nheads_k, headdim); positions, rotary_cos, rotary_sin may be None
    together (norm only); a weight of None leaves that tensor un-normalised.  No double backward."""
    from . import torch_ops as _ops                            # (registers torch.ops.flash_attn_mi355.qk_norm_rope)
    q_out, k_out = _ops.qk_norm_rope(q, k, positions, rotary_cos, rotary_sin, q_weight, k_weight, float(eps), float(weight_offset),
                                     bool(interleaved))
    return (None if q is None else q_out), k_out
