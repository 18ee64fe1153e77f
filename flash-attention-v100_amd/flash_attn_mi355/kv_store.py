"""Write a ragged packed batch of K / V rows into a KV cache on the library's `fa_kv_store` kernel (csrc/fa_kv_store.hip): the
step between a ragged prefill (`flash_attn_varlen_func`) and everything that reads a cache (`flash_attn_with_kvcache`,
`flash_attn_varlen_func(..., block_table=)`, tree decode, the shared-prefix operator).  What vLLM calls `reshape_and_cache_flash`,
plus the RoPE fusion the kv-cache op has for uniform batches.

One launch stores K and V; paged or contiguous caches of the input dtype or float8_e4m3fn.  The fp8 codes and the rotated bits are
the ones `flash_attn_with_kvcache(..., k=, v=)` would store: both kernels share the rounding rule and the rotation.

Not covered: `cache_leftpad`, per-token position ids for the rotation, a V-only or K-only store, per-head or device-resident
descales, and fusing the store into the varlen forward.  The way back, cache -> packed, is `kv_gather.gather_kv_cache`
(`kv_gather.move_kv_cache` composes the two to move rows inside a cache).  Nothing here is exported through the packages' `__all__`
lists."""
import ctypes
from typing import Optional

import torch

from . import _lib
from . import _rowargs as _ra
from . import flash_attn_interface as _fi


def store_kv_cache(k, v, k_cache, v_cache, *, slot_mapping: Optional[torch.Tensor] = None,
                   cu_seqlens: Optional[torch.Tensor] = None, cache_seqlens: Optional[torch.Tensor] = None,
                   block_table: Optional[torch.Tensor] = None, cache_batch_idx: Optional[torch.Tensor] = None,
                   rotary_cos: Optional[torch.Tensor] = None, rotary_sin: Optional[torch.Tensor] = None,
                   rotary_interleaved: bool = True, k_descale: Optional[float] = None,
                   v_descale: Optional[float] = None) -> None:
    """k, v: (total_rows, nheads_k, headdim) fp16 / bf16, same shape; views with a contiguous last dimension are taken as they are
    (the K and V heads of a packed (total, nheads_q + 2 nheads_k, headdim) qkv, for instance).
    k_cache, v_cache: (num_blocks, page_block_size, nheads_k, headdim) pages or (batch_cache, seqlen_cache, nheads_k, headdim), of
    k's dtype or float8_e4m3fn; written in place, never copied.

    Exactly one addressing mode:
    slot_mapping (int64 or int32 (total_rows,)): row r goes to block slot // cache.shape[1], row slot % cache.shape[1] of the
    cache as it is shaped; a slot < 0 or >= cache.shape[0] * cache.shape[1] skips the row (padding rows of a captured graph).
    cu_seqlens (int32 (batch + 1,)): row r of sequence b (index i = r - cu_seqlens[b]) goes to position cache_seqlens[b] + i
    (cache_seqlens int32 (batch,), None = 0) of that sequence - through block_table (int32 (batch, max_blocks): a paged cache) or
    into batch slot cache_batch_idx[b] (None: b) of a contiguous cache.  Positions at or past the capacity (max_blocks *
    page_block_size, or seqlen_cache) are dropped, as the kv-cache op's append drops them; so are rows behind cu_seqlens[-1].

    rotary_cos, rotary_sin ((seqlen_ro, rotary_dim / 2) of k's dtype; cu_seqlens mode only): K is rotated at its cache position
    before it is stored, with the kv-cache op's rule (`rotary_interleaved` defaults to True as there); a position outside the
    tables is stored unrotated.  V is never rotated.
    k_descale, v_descale (fp8 caches only, default 1.0): stored code = e4m3(clamp(x / descale, +-448))."""
    op = "kv_store"
    if k.dtype not in _fi._DTYPES:
        raise RuntimeError(f"kv_store: k must be fp16 or bf16, got {k.dtype}")
    if v.dtype != k.dtype:
        raise RuntimeError(f"kv_store: v must have k's dtype ({k.dtype}), got {v.dtype}")
    if k.dim() != 3 or tuple(k.shape) != tuple(v.shape):
        raise RuntimeError(f"kv_store: k and v must have the same shape (total_rows, nheads_k, headdim), got {tuple(k.shape)} / {tuple(v.shape)}")
    T, H, D = k.shape
    fp8 = _ra.cache_pair(op, k, H, D, k_cache, v_cache)
    _ra.head_dim(op, D)
    _ra.descales_need_fp8(op, fp8, k_descale, v_descale)
    _ra.one_mode(op, slot_mapping, cu_seqlens, "cache_seqlens")
    _ra.cache_last_dim(op, k_cache, v_cache)
    if rotary_cos is not None or rotary_sin is not None:
        if slot_mapping is not None:
            raise RuntimeError("kv_store: rotary needs cu_seqlens mode (a slot carries no position); rotate with apply_rotary_emb first")
        if rotary_cos is None or rotary_sin is None:
            raise RuntimeError("kv_store: rotary_cos and rotary_sin must both be given")
        if rotary_cos.dtype != k.dtype or rotary_sin.dtype != k.dtype:
            raise RuntimeError(f"kv_store: rotary_cos / rotary_sin must have k's dtype ({k.dtype})")
        if rotary_cos.dim() != 2 or tuple(rotary_cos.shape) != tuple(rotary_sin.shape):
            raise RuntimeError("kv_store: rotary_cos and rotary_sin must have the same shape (seqlen_ro, rotary_dim / 2)")
        if 2 * rotary_cos.shape[1] > D:
            raise RuntimeError("kv_store: rotary_dim must be <= headdim")

    s = _lib.FaKvStoreParams()
    s.struct_size = ctypes.sizeof(_lib.FaKvStoreParams)
    B = 0
    if slot_mapping is not None:
        _ra.slot_mode(op, cache_seqlens, "cache_seqlens", block_table, cache_batch_idx)
        slot_mapping = _ra.ids(op, slot_mapping, T, "slot_mapping")
    else:
        B, cu_seqlens, cache_seqlens, block_table, cache_batch_idx = _ra.sequence_mode(
            op, k_cache, cu_seqlens, cache_seqlens, "cache_seqlens", block_table, cache_batch_idx)
    # (the tensors made above stay referenced by these names until the launch is queued)
    _ra.same_device(op, [k, v, k_cache, v_cache, slot_mapping, cu_seqlens, cache_seqlens, block_table, cache_batch_idx, rotary_cos,
                         rotary_sin], k, "k's")
    if T == 0 or H == 0:
        return None

    k, v = _fi._prep(k, D), _fi._prep(v, D)               # (views with 16-byte friendly strides are taken as they are)
    s.k, s.v = k.data_ptr(), v.data_ptr()
    s.k_row_stride, s.k_head_stride = k.stride(0), k.stride(1)
    s.v_row_stride, s.v_head_stride = v.stride(0), v.stride(1)
    s.total_rows, s.nheads, s.head_dim = T, H, D
    s.dtype = _fi._DTYPES[k.dtype]
    _ra.fill_cache(s, k_cache, v_cache, fp8, k_descale, v_descale)
    _ra.fill_mode(s, slot_mapping, cu_seqlens, B, cache_seqlens, "cache_seqlens", block_table, cache_batch_idx)
    if rotary_cos is not None:                            # (sequence mode: checked above)
        rotary_cos, rotary_sin = rotary_cos.contiguous(), rotary_sin.contiguous()
        s.rotary_cos, s.rotary_sin = rotary_cos.data_ptr(), rotary_sin.data_ptr()
        s.rotary_dim, s.seqlen_ro = 2 * rotary_cos.shape[1], rotary_cos.shape[0]
        s.rotary_interleaved = 1 if rotary_interleaved else 0
    with _fi._on_device(k.device):
        _lib.call_kv_store(s, _fi._stream(k.device))          # (queued: the prepared tensors stay referenced until here)
    del slot_mapping, cu_seqlens, cache_seqlens, block_table, cache_batch_idx, rotary_cos, rotary_sin
    return None
