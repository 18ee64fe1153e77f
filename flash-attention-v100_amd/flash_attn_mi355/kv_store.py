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
from . import flash_attn_interface as _fi


def _i32(t, shape, name):
    if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"kv_store: {name} must be an int32 tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


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
    if k.dtype not in _fi._DTYPES:
        raise RuntimeError(f"kv_store: k must be fp16 or bf16, got {k.dtype}")
    if v.dtype != k.dtype:
        raise RuntimeError(f"kv_store: v must have k's dtype ({k.dtype}), got {v.dtype}")
    if k.dim() != 3 or tuple(k.shape) != tuple(v.shape):
        raise RuntimeError(f"kv_store: k and v must have the same shape (total_rows, nheads_k, headdim), got {tuple(k.shape)} / {tuple(v.shape)}")
    T, H, D = k.shape
    fp8 = k_cache.dtype == _fi._FP8
    if v_cache.dtype != k_cache.dtype or not (fp8 or k_cache.dtype == k.dtype):
        raise RuntimeError(f"kv_store: k_cache / v_cache must both have k's dtype ({k.dtype}) or both be float8_e4m3fn, "
                           f"got {k_cache.dtype} / {v_cache.dtype}")
    if k_cache.dim() != 4 or tuple(k_cache.shape) != tuple(v_cache.shape):
        raise RuntimeError(f"kv_store: k_cache and v_cache must have the same 4-D shape, got {tuple(k_cache.shape)} / {tuple(v_cache.shape)}")
    if tuple(k_cache.shape[2:]) != (H, D):
        raise RuntimeError(f"kv_store: the cache's last two dimensions must be k's (nheads_k, headdim) = {(H, D)}, got {tuple(k_cache.shape[2:])}")
    if D % 8 != 0 or D > 256:
        raise RuntimeError(f"kv_store: head dimension must be a multiple of 8 and <= 256, got {D}")
    if not fp8 and (k_descale is not None or v_descale is not None):
        raise RuntimeError("kv_store: k_descale / v_descale go with a float8_e4m3fn cache")
    if (slot_mapping is None) == (cu_seqlens is None):
        raise RuntimeError("kv_store: exactly one addressing mode - slot_mapping, or cu_seqlens (with cache_seqlens and block_table "
                           f"/ cache_batch_idx); {'both' if slot_mapping is not None else 'neither'} given")
    if k_cache.stride(-1) != 1 or v_cache.stride(-1) != 1:
        raise RuntimeError("kv_store: k_cache / v_cache must have a contiguous last dimension (a cache is never copied)")
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
    keep = []                                             # tensors made here stay referenced until the launch is queued
    if slot_mapping is not None:
        if cache_seqlens is not None or block_table is not None or cache_batch_idx is not None:
            raise RuntimeError("kv_store: slot_mapping takes no cache_seqlens, block_table or cache_batch_idx")
        if slot_mapping.dtype not in (torch.int64, torch.int32) or tuple(slot_mapping.shape) != (T,):
            raise RuntimeError(f"kv_store: slot_mapping must be an int64 (or int32) tensor of shape ({T},)")
        slot_mapping = slot_mapping.to(torch.int64).contiguous()
        keep.append(slot_mapping)
    else:
        if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1:
            raise RuntimeError("kv_store: cu_seqlens must be an int32 tensor of shape (batch + 1,)")
        B = cu_seqlens.numel() - 1
        cu_seqlens = cu_seqlens.contiguous()
        if cache_seqlens is not None:
            cache_seqlens = _i32(cache_seqlens, (B,), "cache_seqlens")
        if block_table is not None:
            if cache_batch_idx is not None:
                raise RuntimeError("kv_store: a paged cache (block_table) does not take cache_batch_idx")
            if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B:
                raise RuntimeError(f"kv_store: block_table must be an int32 tensor of shape ({B}, max_num_blocks_per_seq)")
            if block_table.stride(1) != 1:
                block_table = block_table.contiguous()
        elif cache_batch_idx is not None:
            cache_batch_idx = _i32(cache_batch_idx, (B,), "cache_batch_idx")
        elif k_cache.shape[0] < B:
            raise RuntimeError(f"kv_store: the cache has {k_cache.shape[0]} batch slots for {B} sequences (pass cache_batch_idx)")
        keep += [cu_seqlens, cache_seqlens, block_table, cache_batch_idx]
    tensors = [k, v, k_cache, v_cache, slot_mapping, cu_seqlens, cache_seqlens, block_table, cache_batch_idx, rotary_cos, rotary_sin]
    _fi._check_device(*tensors)
    if any(t is not None and t.device != k.device for t in tensors):
        raise RuntimeError("kv_store: every tensor must be on k's device")
    if T == 0 or H == 0:
        return None

    k, v = _fi._prep(k, D), _fi._prep(v, D)               # (views with 16-byte friendly strides are taken as they are)
    s.k, s.v = k.data_ptr(), v.data_ptr()
    s.k_row_stride, s.k_head_stride = k.stride(0), k.stride(1)
    s.v_row_stride, s.v_head_stride = v.stride(0), v.stride(1)
    s.k_cache, s.v_cache = k_cache.data_ptr(), v_cache.data_ptr()
    s.kc_batch_stride, s.kc_row_stride, s.kc_head_stride = k_cache.stride(0), k_cache.stride(1), k_cache.stride(2)
    s.vc_batch_stride, s.vc_row_stride, s.vc_head_stride = v_cache.stride(0), v_cache.stride(1), v_cache.stride(2)
    s.total_rows, s.nheads, s.head_dim = T, H, D
    s.dtype = _fi._DTYPES[k.dtype]
    s.cache_dtype = _lib.FA_FP8_E4M3 if fp8 else s.dtype
    s.num_blocks, s.page_block_size = k_cache.shape[0], k_cache.shape[1]
    if fp8:
        s.k_descale = 1.0 if k_descale is None else float(k_descale)
        s.v_descale = 1.0 if v_descale is None else float(v_descale)
    if slot_mapping is not None:
        s.slot_mapping = slot_mapping.data_ptr()
    else:
        s.cu_seqlens, s.batch = cu_seqlens.data_ptr(), B
        if cache_seqlens is not None:
            s.cache_seqlens = cache_seqlens.data_ptr()
        if block_table is not None:
            s.paged = 1
            s.block_table, s.block_table_batch_stride = block_table.data_ptr(), block_table.stride(0)
            s.max_blocks = block_table.shape[1]
        elif cache_batch_idx is not None:
            s.cache_batch_idx = cache_batch_idx.data_ptr()
        if rotary_cos is not None:
            rotary_cos, rotary_sin = rotary_cos.contiguous(), rotary_sin.contiguous()
            s.rotary_cos, s.rotary_sin = rotary_cos.data_ptr(), rotary_sin.data_ptr()
            s.rotary_dim, s.seqlen_ro = 2 * rotary_cos.shape[1], rotary_cos.shape[0]
            s.rotary_interleaved = 1 if rotary_interleaved else 0
    with _fi._on_device(k.device):
        _lib.call_kv_store(s, _fi._stream(k.device))          # (queued: `keep` and the prepared k / v stay referenced until here)
    del keep
    return None
