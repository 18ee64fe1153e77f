"""The prologue of a serving step in one launch on the library's `fa_rope_store` kernel (csrc/fa_rope_store.hip): rotate q and k at
PER-TOKEN positions and store the rotated K and V into a KV cache by slot.  What a vLLM-style engine does before every attention
call with `rotary_embedding` + `reshape_and_cache_flash`: a flat token batch, `positions[T]` and `slot_mapping[T]`, padding rows
with slot -1.  Here `apply_rotary_emb` (positions = row index + a per-sequence offset) followed by
`kv_store.store_kv_cache(slot_mapping=)` (no rotation) would take two launches, and positions that are not `offset + i` - the
nodes of a draft tree, re-packed tokens, padding rows - cannot be expressed at all.

The rotated bits are `apply_rotary_emb`'s and the cache holds what `apply_rotary_emb` + `store_kv_cache(slot_mapping=)` leave: the
kernels share the rotation and the fp8 rounding rule.  Without caches the call is the standalone rotation at per-token positions.

Not covered: fp32 cos / sin and rotary dims that are not multiples of 16 (`apply_rotary_emb` has them), a backward, sequence-mode
addressing (`store_kv_cache` has it), per-head or device-resident descales.  QK-norm in front of the rotation is
`qk_norm.qk_norm_rope_and_store_kv`'s.  Nothing here is exported through the packages' `__all__` lists."""
import ctypes
from typing import Optional

import torch

from . import _lib
from . import flash_attn_interface as _fi


def _ids(t, T, name):
    if t.dtype not in (torch.int64, torch.int32) or tuple(t.shape) != (T,):
        raise RuntimeError(f"rope_store: {name} must be an int64 (or int32) tensor of shape ({T},)")
    return t.to(torch.int64).contiguous()


def _view(x, D, inplace, name):
    """the tensor as the kernel takes it: a view with 16-byte friendly strides as it is; anything else is copied - which in place
    would rotate the copy, so there it is an error"""
    p = _fi._prep(x, D)
    if inplace and p is not x:
        raise RuntimeError(f"rope_store: in place needs a 16-byte aligned {name} whose strides are multiples of 8 elements "
                           f"(got strides {tuple(x.stride())}); pass inplace=False")
    return p


def rope_and_store_kv(q, k, v, positions, rotary_cos, rotary_sin, k_cache=None, v_cache=None,
                      slot_mapping: Optional[torch.Tensor] = None, *, interleaved: bool = False, inplace: bool = True,
                      k_out: bool = True, k_descale: Optional[float] = None, v_descale: Optional[float] = None):
    """q: (total_rows, nheads_q, headdim) fp16 / bf16, or None (a K / V-only call); k, v: (total_rows, nheads_k, headdim).  Views
    with a contiguous last dimension are taken as they are (the q, k and v heads of one packed (total, nheads_q + 2 nheads_k,
    headdim) qkv, for instance).
    positions (int64 or int32 (total_rows,)): row r of q and of k is rotated at positions[r]; a position < 0 or >= seqlen_ro
    leaves the row unrotated.  rotary_cos, rotary_sin: (seqlen_ro, rotary_dim / 2) of q's dtype, rotary_dim a multiple of 16 and
    <= headdim; the columns behind rotary_dim are not rotated.
    interleaved: rotate pairs (2t, 2t + 1) (GPT-J) instead of (t, t + rotary_dim / 2) (GPT-NeoX).  The default is False, as in
    `flash_attn.layers.rotary` - NOT the kv-cache op's `rotary_interleaved=True`.
    k_cache, v_cache: (num_blocks, page_block_size, nheads_k, headdim) pages or (batch_cache, seqlen_cache, nheads_k, headdim), of
    k's dtype or float8_e4m3fn; written in place, never copied.  slot_mapping (int64 or int32 (total_rows,)): row r goes to block
    slot // cache.shape[1], row slot % cache.shape[1]; a slot < 0 or >= cache.shape[0] * cache.shape[1] skips the cache write of
    that row (padding rows of a captured graph) - its q and k are still rotated.  The cache gets the rotated K and the unrotated V.
    Without caches (all three None; v None as well) the call only rotates.
    inplace: rotate q and k themselves (the default); False allocates the outputs.  k_out=False: the rotated K is only cached, k
    stays as it is.  k_descale, v_descale (fp8 caches only, default 1.0): stored code = e4m3(clamp(x / descale, +-448)).
    Returns (q_out, k_out): the rotated tensors (q and k themselves in place), None for a missing q or with k_out=False."""
    if k.dtype not in _fi._DTYPES:
        raise RuntimeError(f"rope_store: k must be fp16 or bf16, got {k.dtype}")
    if k.dim() != 3:
        raise RuntimeError(f"rope_store: k must be (total_rows, nheads_k, headdim), got {tuple(k.shape)}")
    T, Hk, D = k.shape
    if q is not None:
        if q.dtype != k.dtype:
            raise RuntimeError(f"rope_store: q must have k's dtype ({k.dtype}), got {q.dtype}")
        if q.dim() != 3 or q.shape[0] != T or q.shape[2] != D:
            raise RuntimeError(f"rope_store: q must be (total_rows, nheads_q, headdim) = ({T}, *, {D}), got {tuple(q.shape)}")
    Hq = 0 if q is None else q.shape[1]
    if D % 8 != 0 or D > 256:
        raise RuntimeError(f"rope_store: head dimension must be a multiple of 8 and <= 256, got {D}")
    cached = k_cache is not None or v_cache is not None
    if cached:
        if k_cache is None or v_cache is None:
            raise RuntimeError("rope_store: k_cache and v_cache must both be given (or neither: rotate only)")
        if v is None or slot_mapping is None:
            raise RuntimeError("rope_store: caches need v and slot_mapping")
        if v.dtype != k.dtype:
            raise RuntimeError(f"rope_store: v must have k's dtype ({k.dtype}), got {v.dtype}")
        if tuple(v.shape) != tuple(k.shape):
            raise RuntimeError(f"rope_store: k and v must have the same shape (total_rows, nheads_k, headdim), got {tuple(k.shape)} / {tuple(v.shape)}")
        fp8 = k_cache.dtype == _fi._FP8
        if v_cache.dtype != k_cache.dtype or not (fp8 or k_cache.dtype == k.dtype):
            raise RuntimeError(f"rope_store: k_cache / v_cache must both have k's dtype ({k.dtype}) or both be float8_e4m3fn, "
                               f"got {k_cache.dtype} / {v_cache.dtype}")
        if k_cache.dim() != 4 or tuple(k_cache.shape) != tuple(v_cache.shape):
            raise RuntimeError(f"rope_store: k_cache and v_cache must have the same 4-D shape, got {tuple(k_cache.shape)} / {tuple(v_cache.shape)}")
        if tuple(k_cache.shape[2:]) != (Hk, D):
            raise RuntimeError(f"rope_store: the cache's last two dimensions must be k's (nheads_k, headdim) = {(Hk, D)}, got {tuple(k_cache.shape[2:])}")
        if k_cache.stride(-1) != 1 or v_cache.stride(-1) != 1:
            raise RuntimeError("rope_store: k_cache / v_cache must have a contiguous last dimension (a cache is never copied)")
    else:
        fp8 = False
        if v is not None or slot_mapping is not None:
            raise RuntimeError("rope_store: v and slot_mapping go with k_cache / v_cache (without caches the call only rotates)")
        if q is None and not k_out:
            raise RuntimeError("rope_store: nothing to do - no caches, no q and k_out=False")
    if not fp8 and (k_descale is not None or v_descale is not None):
        raise RuntimeError("rope_store: k_descale / v_descale go with a float8_e4m3fn cache")
    if rotary_cos.dtype != k.dtype or rotary_sin.dtype != k.dtype:
        raise RuntimeError(f"rope_store: rotary_cos / rotary_sin must have k's dtype ({k.dtype}), got {rotary_cos.dtype} / {rotary_sin.dtype}")
    if rotary_cos.dim() != 2 or tuple(rotary_cos.shape) != tuple(rotary_sin.shape):
        raise RuntimeError("rope_store: rotary_cos and rotary_sin must have the same shape (seqlen_ro, rotary_dim / 2)")
    rotary_dim = 2 * rotary_cos.shape[1]
    if rotary_dim == 0 or rotary_dim % 16 != 0:
        raise RuntimeError(f"rope_store: rotary_dim must be a positive multiple of 16, got {rotary_dim} (apply_rotary_emb takes any even one)")
    if rotary_dim > D:
        raise RuntimeError(f"rope_store: rotary_dim must be <= headdim ({rotary_dim} > {D})")
    positions = _ids(positions, T, "positions")
    if cached:
        slot_mapping = _ids(slot_mapping, T, "slot_mapping")
    tensors = [q, k, v, positions, rotary_cos, rotary_sin, k_cache, v_cache, slot_mapping]
    _fi._check_device(*tensors)
    if any(t is not None and t.device != k.device for t in tensors):
        raise RuntimeError("rope_store: every tensor must be on k's device")

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
    rotary_cos, rotary_sin = rotary_cos.contiguous(), rotary_sin.contiguous()

    s = _lib.FaRopeStoreParams()
    s.struct_size = ctypes.sizeof(_lib.FaRopeStoreParams)
    if qi is not None:
        s.q, s.q_out = qi.data_ptr(), qo.data_ptr()
        s.q_row_stride, s.q_head_stride = qi.stride(0), qi.stride(1)
        s.qo_row_stride, s.qo_head_stride = qo.stride(0), qo.stride(1)
    s.k = ki.data_ptr()
    s.k_row_stride, s.k_head_stride = ki.stride(0), ki.stride(1)
    if ko is not None:
        s.k_out = ko.data_ptr()
        s.ko_row_stride, s.ko_head_stride = ko.stride(0), ko.stride(1)
    s.positions = positions.data_ptr()
    s.rotary_cos, s.rotary_sin = rotary_cos.data_ptr(), rotary_sin.data_ptr()
    s.rotary_dim, s.seqlen_ro, s.rotary_interleaved = rotary_dim, rotary_cos.shape[0], 1 if interleaved else 0
    s.total_rows, s.nheads_q, s.nheads_k, s.head_dim = T, Hq, Hk, D
    s.dtype = s.cache_dtype = _fi._DTYPES[k.dtype]
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
        _lib.call_rope_store(s, _fi._stream(k.device))       # (queued: the tensors made here stay referenced until here)
    del qi, ki, vi, positions, slot_mapping, rotary_cos, rotary_sin
    return qo, ko
