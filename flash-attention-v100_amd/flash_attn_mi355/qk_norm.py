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
from . import flash_attn_interface as _fi


def _ids(t, T, name):
    if t.dtype not in (torch.int64, torch.int32) or tuple(t.shape) != (T,):
        raise RuntimeError(f"qk_norm: {name} must be an int64 (or int32) tensor of shape ({T},)")
    return t.to(torch.int64).contiguous()


def _view(x, D, inplace, name):
    """the tensor as the kernel takes it: a view with 16-byte friendly strides as it is; anything else is copied - which in place
    would change the copy, so there it is an error"""
    p = _fi._prep(x, D)
    if inplace and p is not x:
        raise RuntimeError(f"qk_norm: in place needs a 16-byte aligned {name} whose strides are multiples of 8 elements "
                           f"(got strides {tuple(x.stride())}); pass inplace=False")
    return p


def _weight(w, D, dtype, name):
    if w.dtype not in (dtype, torch.float32):
        raise RuntimeError(f"qk_norm: {name} must have k's dtype ({dtype}) or float32, got {w.dtype}")
    if tuple(w.shape) != (D,):
        raise RuntimeError(f"qk_norm: {name} must have shape (headdim,) = ({D},), got {tuple(w.shape)}")
    w = w.contiguous()
    return w if w.data_ptr() % 16 == 0 else w.clone()


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
    if k.dtype not in _fi._DTYPES:
        raise RuntimeError(f"qk_norm: k must be fp16 or bf16, got {k.dtype}")
    if k.dim() != 3:
        raise RuntimeError(f"qk_norm: k must be (total_rows, nheads_k, headdim), got {tuple(k.shape)}")
    T, Hk, D = k.shape
    if q is not None:
        if q.dtype != k.dtype:
            raise RuntimeError(f"qk_norm: q must have k's dtype ({k.dtype}), got {q.dtype}")
        if q.dim() != 3 or q.shape[0] != T or q.shape[2] != D:
            raise RuntimeError(f"qk_norm: q must be (total_rows, nheads_q, headdim) = ({T}, *, {D}), got {tuple(q.shape)}")
    Hq = 0 if q is None else q.shape[1]
    if D % 8 != 0 or D > 256:
        raise RuntimeError(f"qk_norm: head dimension must be a multiple of 8 and <= 256, got {D}")
    cached = k_cache is not None or v_cache is not None
    if cached:
        if k_cache is None or v_cache is None:
            raise RuntimeError("qk_norm: k_cache and v_cache must both be given (or neither)")
        if v is None or slot_mapping is None:
            raise RuntimeError("qk_norm: caches need v and slot_mapping")
        if v.dtype != k.dtype:
            raise RuntimeError(f"qk_norm: v must have k's dtype ({k.dtype}), got {v.dtype}")
        if tuple(v.shape) != tuple(k.shape):
            raise RuntimeError(f"qk_norm: k and v must have the same shape (total_rows, nheads_k, headdim), got {tuple(k.shape)} / {tuple(v.shape)}")
        fp8 = k_cache.dtype == _fi._FP8
        if v_cache.dtype != k_cache.dtype or not (fp8 or k_cache.dtype == k.dtype):
            raise RuntimeError(f"qk_norm: k_cache / v_cache must both have k's dtype ({k.dtype}) or both be float8_e4m3fn, "
                               f"got {k_cache.dtype} / {v_cache.dtype}")
        if k_cache.dim() != 4 or tuple(k_cache.shape) != tuple(v_cache.shape):
            raise RuntimeError(f"qk_norm: k_cache and v_cache must have the same 4-D shape, got {tuple(k_cache.shape)} / {tuple(v_cache.shape)}")
        if tuple(k_cache.shape[2:]) != (Hk, D):
            raise RuntimeError(f"qk_norm: the cache's last two dimensions must be k's (nheads_k, headdim) = {(Hk, D)}, got {tuple(k_cache.shape[2:])}")
        if k_cache.stride(-1) != 1 or v_cache.stride(-1) != 1:
            raise RuntimeError("qk_norm: k_cache / v_cache must have a contiguous last dimension (a cache is never copied)")
    else:
        fp8 = False
        if v is not None or slot_mapping is not None:
            raise RuntimeError("qk_norm: v and slot_mapping go with k_cache / v_cache")
        if q is None and not k_out:
            raise RuntimeError("qk_norm: nothing to do - no caches, no q and k_out=False")
    if not fp8 and (k_descale is not None or v_descale is not None):
        raise RuntimeError("qk_norm: k_descale / v_descale go with a float8_e4m3fn cache")
    rope = [positions is not None, rotary_cos is not None, rotary_sin is not None]
    if any(rope) and not all(rope):
        raise RuntimeError("qk_norm: positions, rotary_cos and rotary_sin go together (all three, or none: no rotation)")
    rope = all(rope)
    rotary_dim = 0
    if rope:
        if rotary_cos.dtype != k.dtype or rotary_sin.dtype != k.dtype:
            raise RuntimeError(f"qk_norm: rotary_cos / rotary_sin must have k's dtype ({k.dtype}), got {rotary_cos.dtype} / {rotary_sin.dtype}")
        if rotary_cos.dim() != 2 or tuple(rotary_cos.shape) != tuple(rotary_sin.shape):
            raise RuntimeError("qk_norm: rotary_cos and rotary_sin must have the same shape (seqlen_ro, rotary_dim / 2)")
        rotary_dim = 2 * rotary_cos.shape[1]
        if rotary_dim == 0 or rotary_dim % 16 != 0:
            raise RuntimeError(f"qk_norm: rotary_dim must be a positive multiple of 16, got {rotary_dim}")
        if rotary_dim > D:
            raise RuntimeError(f"qk_norm: rotary_dim must be <= headdim ({rotary_dim} > {D})")
        positions = _ids(positions, T, "positions")
        rope = rotary_cos.shape[0] > 0                         # (an empty table: no row is rotated)
    if q_weight is not None and q is None:
        raise RuntimeError("qk_norm: q_weight without q")
    if q_weight is not None and k_weight is not None and q_weight.dtype != k_weight.dtype:
        raise RuntimeError(f"qk_norm: q_weight and k_weight must have the same dtype, got {q_weight.dtype} / {k_weight.dtype}")
    qw = None if q_weight is None else _weight(q_weight, D, k.dtype, "q_weight")
    kw = None if k_weight is None else _weight(k_weight, D, k.dtype, "k_weight")
    eps, weight_offset = float(eps), float(weight_offset)
    if not (0.0 <= eps < float("inf")):
        raise RuntimeError(f"qk_norm: eps must be finite and >= 0, got {eps}")
    if not (abs(weight_offset) < float("inf")):
        raise RuntimeError(f"qk_norm: weight_offset must be finite, got {weight_offset}")
    if cached:
        slot_mapping = _ids(slot_mapping, T, "slot_mapping")
    tensors = [q, k, v, positions, rotary_cos, rotary_sin, k_cache, v_cache, slot_mapping, qw, kw]
    _fi._check_device(*tensors)
    if any(t is not None and t.device != k.device for t in tensors):
        raise RuntimeError("qk_norm: every tensor must be on k's device")

    write_k = bool(k_out)
    qi = None if q is None else _view(q, D, inplace, "q")
    ki = _view(k, D, inplace and write_k, "k")
    if inplace:
        qo, ko = qi, (ki if write_k else None)
    else:
        qo = None if q is None else torch.empty(q.shape, dtype=q.dtype, device=q.device)
        ko = torch.empty(k.shape, dtype=k.dtype, device=k.device) if write_k else None
    if T == 0 or (Hq == 0 and Hk == 0):
        return qo, ko

    s = _lib.FaQkNormRopeStoreParams()
    s.struct_size = ctypes.sizeof(_lib.FaQkNormRopeStoreParams)
    if qi is not None:
        s.q, s.q_out = qi.data_ptr(), qo.data_ptr()
        s.q_row_stride, s.q_head_stride = qi.stride(0), qi.stride(1)
        s.qo_row_stride, s.qo_head_stride = qo.stride(0), qo.stride(1)
    s.k = ki.data_ptr()
    s.k_row_stride, s.k_head_stride = ki.stride(0), ki.stride(1)
    if ko is not None:
        s.k_out = ko.data_ptr()
        s.ko_row_stride, s.ko_head_stride = ko.stride(0), ko.stride(1)
    if rope:
        rotary_cos, rotary_sin = rotary_cos.contiguous(), rotary_sin.contiguous()
        s.positions = positions.data_ptr()
        s.rotary_cos, s.rotary_sin = rotary_cos.data_ptr(), rotary_sin.data_ptr()
        s.rotary_dim, s.seqlen_ro, s.rotary_interleaved = rotary_dim, rotary_cos.shape[0], 1 if interleaved else 0
    s.total_rows, s.nheads_q, s.nheads_k, s.head_dim = T, Hq, Hk, D
    s.dtype = s.cache_dtype = _fi._DTYPES[k.dtype]
    if qw is not None:
        s.q_weight = qw.data_ptr()
    if kw is not None:
        s.k_weight = kw.data_ptr()
    w = qw if qw is not None else kw
    s.weight_dtype = _lib.FA_FP32 if (w is not None and w.dtype == torch.float32) else s.dtype
    s.eps, s.weight_offset = eps, weight_offset
    vi = None
    if cached:
        vi = _fi._prep(v, D)
        s.v = vi.data_ptr()
        s.v_row_stride, s.v_head_stride = vi.stride(0), vi.stride(1)
        s.k_cache, s.v_cache = k_cache.data_ptr(), v_cache.data_ptr()
        s.kc_batch_stride, s.kc_row_stride, s.kc_head_stride = k_cache.stride(0), k_cache.stride(1), k_cache.stride(2)
        s.vc_batch_stride, s.vc_row_stride, s.vc_head_stride = v_cache.stride(0), v_cache.stride(1), v_cache.stride(2)
        s.num_blocks, s.page_block_size = k_cache.shape[0], k_cache.shape[1]
        s.slot_mapping = slot_mapping.data_ptr()
        if fp8:
            s.cache_dtype = _lib.FA_FP8_E4M3
            s.k_descale = 1.0 if k_descale is None else float(k_descale)
            s.v_descale = 1.0 if v_descale is None else float(v_descale)
    with _fi._on_device(k.device):
        _lib.call_qk_norm_rope_store(s, _fi._stream(k.device))   # (queued: the tensors made here stay referenced until here)
    del qi, ki, vi, positions, slot_mapping, rotary_cos, rotary_sin, qw, kw
    return qo, ko


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
    if k.dtype not in _fi._DTYPES:
        raise RuntimeError(f"qk_norm: k must be fp16 or bf16, got {k.dtype}")
    if k.dim() != 3:
        raise RuntimeError(f"qk_norm: k must be (total_rows, nheads_k, headdim), got {tuple(k.shape)}")
    T, Hk, D = k.shape
    if dk_out is None or dk_out.dtype != k.dtype or tuple(dk_out.shape) != tuple(k.shape):
        raise RuntimeError(f"qk_norm: dk_out must have k's dtype and shape ({k.dtype}, {tuple(k.shape)})")
    if q is not None:
        if q.dtype != k.dtype:
            raise RuntimeError(f"qk_norm: q must have k's dtype ({k.dtype}), got {q.dtype}")
        if q.dim() != 3 or q.shape[0] != T or q.shape[2] != D:
            raise RuntimeError(f"qk_norm: q must be (total_rows, nheads_q, headdim) = ({T}, *, {D}), got {tuple(q.shape)}")
        if dq_out is None or dq_out.dtype != q.dtype or tuple(dq_out.shape) != tuple(q.shape):
            raise RuntimeError(f"qk_norm: dq_out must have q's dtype and shape ({q.dtype}, {tuple(q.shape)})")
    elif dq_out is not None:
        raise RuntimeError("qk_norm: dq_out without q")
    Hq = 0 if q is None else q.shape[1]
    if D % 8 != 0 or D > 256:
        raise RuntimeError(f"qk_norm: head dimension must be a multiple of 8 and <= 256, got {D}")
    rope = [positions is not None, rotary_cos is not None, rotary_sin is not None]
    if any(rope) and not all(rope):
        raise RuntimeError("qk_norm: positions, rotary_cos and rotary_sin go together (all three, or none: no rotation)")
    rope = all(rope)
    rotary_dim = 0
    if rope:
        if rotary_cos.dtype != k.dtype or rotary_sin.dtype != k.dtype:
            raise RuntimeError(f"qk_norm: rotary_cos / rotary_sin must have k's dtype ({k.dtype}), got {rotary_cos.dtype} / {rotary_sin.dtype}")
        if rotary_cos.dim() != 2 or tuple(rotary_cos.shape) != tuple(rotary_sin.shape):
            raise RuntimeError("qk_norm: rotary_cos and rotary_sin must have the same shape (seqlen_ro, rotary_dim / 2)")
        rotary_dim = 2 * rotary_cos.shape[1]
        if rotary_dim == 0 or rotary_dim % 16 != 0:
            raise RuntimeError(f"qk_norm: rotary_dim must be a positive multiple of 16, got {rotary_dim}")
        if rotary_dim > D:
            raise RuntimeError(f"qk_norm: rotary_dim must be <= headdim ({rotary_dim} > {D})")
        positions = _ids(positions, T, "positions")
        rope = rotary_cos.shape[0] > 0                         # (an empty table: no row is rotated)
    if q_weight is not None and q is None:
        raise RuntimeError("qk_norm: q_weight without q")
    if q_weight is not None and k_weight is not None and q_weight.dtype != k_weight.dtype:
        raise RuntimeError(f"qk_norm: q_weight and k_weight must have the same dtype, got {q_weight.dtype} / {k_weight.dtype}")
    qw = None if q_weight is None else _weight(q_weight, D, k.dtype, "q_weight")
    kw = None if k_weight is None else _weight(k_weight, D, k.dtype, "k_weight")
    eps, weight_offset = float(eps), float(weight_offset)
    if not (0.0 <= eps < float("inf")):
        raise RuntimeError(f"qk_norm: eps must be finite and >= 0, got {eps}")
    if not (abs(weight_offset) < float("inf")):
        raise RuntimeError(f"qk_norm: weight_offset must be finite, got {weight_offset}")
    tensors = [dq_out, dk_out, q, k, positions, rotary_cos, rotary_sin, qw, kw]
    _fi._check_device(*tensors)
    if any(t is not None and t.device != k.device for t in tensors):
        raise RuntimeError("qk_norm: every tensor must be on k's device")

    want_dq, want_dk = bool(need_dq) and q is not None, bool(need_dk)
    qi = None if q is None else _fi._prep(q, D)
    ki = _fi._prep(k, D)
    dqo = None if q is None else _view(dq_out, D, inplace and want_dq, "dq_out")
    dko = _view(dk_out, D, inplace and want_dk, "dk_out")
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
        rotary_cos, rotary_sin = rotary_cos.contiguous(), rotary_sin.contiguous()
        s.positions = positions.data_ptr()
        s.rotary_cos, s.rotary_sin = rotary_cos.data_ptr(), rotary_sin.data_ptr()
        s.rotary_dim, s.seqlen_ro, s.rotary_interleaved = rotary_dim, rotary_cos.shape[0], 1 if interleaved else 0
    s.total_rows, s.nheads_q, s.nheads_k, s.head_dim = T, Hq, Hk, D
    s.dtype = _fi._DTYPES[k.dtype]
    if qw is not None:
        s.q_weight = qw.data_ptr()
    if kw is not None:
        s.k_weight = kw.data_ptr()
    w = qw if qw is not None else kw
    s.weight_dtype = _lib.FA_FP32 if (w is not None and w.dtype == torch.float32) else s.dtype
    s.eps, s.weight_offset = eps, weight_offset
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
