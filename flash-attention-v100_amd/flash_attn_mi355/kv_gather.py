"""Read ragged K / V rows out of a KV cache into packed (total_rows, nheads_k, headdim) tensors on the library's `fa_kv_gather`
kernel (csrc/fa_kv_gather.hip): `kv_store.store_kv_cache` read backwards.  What turns cache pages back into the packed or dense
K / V that the ops without a `block_table` take - the shared-prefix operator's prefix, the fp8 forward, every backward - and what
moves a sequence between caches or out of an fp8 cache into a 16-bit one.

One launch reads K and V; paged or contiguous caches of the output dtype (copied bit for bit) or float8_e4m3fn (dequantised:
`(cache.float() * descale).to(dtype)`, bit for bit).  Every output row is defined: a row that names nothing is zeros.

`move_kv_cache` is the two-launch composition gather -> store that moves rows INSIDE a cache: committing the accepted path of a
speculative-decoding tree, copying pages for beam search or copy-on-write forks.

Not covered: an inverse rotation, `cache_leftpad`, a K-only or V-only gather, per-head or device-resident descales, an fp8
output, fusing the gather into an attention op (the shared-prefix operator still takes a dense prefix: the caller gathers it).
Nothing here is exported through the packages' `__all__` lists."""
import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from . import _rowargs as _ra
from . import flash_attn_interface as _fi
from . import kv_store as _kv_store


def _viewable(t):
    """an output the kernel can write where it lies: contiguous last dimension, 16-byte aligned base, strides of whole 16 bytes"""
    return t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in t.stride()[:-1])


def gather_kv_cache(k_cache, v_cache, *, slot_mapping: Optional[torch.Tensor] = None,
                    cu_seqlens: Optional[torch.Tensor] = None, seq_offsets: Optional[torch.Tensor] = None,
                    block_table: Optional[torch.Tensor] = None, cache_batch_idx: Optional[torch.Tensor] = None,
                    total_rows: Optional[int] = None, dtype: Optional[torch.dtype] = None,
                    k_descale: Optional[float] = None, v_descale: Optional[float] = None,
                    out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """k_cache, v_cache: (num_blocks, page_block_size, nheads_k, headdim) pages or (batch_cache, seqlen_cache, nheads_k, headdim),
    fp16, bf16 or float8_e4m3fn; read only, never copied.  Returns (k, v): (total_rows, nheads_k, headdim) of `dtype`.

    Exactly one addressing mode, store_kv_cache's:
    slot_mapping (int64 or int32 (total_rows,)): row r is block slot // cache.shape[1], row slot % cache.shape[1] of the cache as
    it is shaped; a slot < 0 or >= cache.shape[0] * cache.shape[1] gives a row of zeros (padding rows of a captured graph).
    cu_seqlens (int32 (batch + 1,)): row r of sequence b (index i = r - cu_seqlens[b]) reads position seq_offsets[b] + i
    (seq_offsets int32 (batch,), None = 0) of that sequence - through block_table (int32 (batch, max_blocks): a paged cache) or
    from batch slot cache_batch_idx[b] (None: b) of a contiguous cache.  Positions at or past the capacity (max_blocks *
    page_block_size, or seqlen_cache) and rows behind cu_seqlens[-1] are zeros.

    dtype: fp16 or bf16, required for float8_e4m3fn caches; for a 16-bit cache None or the cache's dtype (a bit copy).
    k_descale, v_descale (fp8 caches only, default 1.0): value = round(float(code) * descale) - one fp32 multiply, one rounding.
    out=(k_out, v_out): existing (total_rows, nheads_k, headdim) tensors of `dtype`, written where they lie - views with a
    contiguous last dimension, a 16-byte aligned base and strides of whole 16 bytes (the K and V heads of a packed qkv buffer);
    any other `out` is an error, never a copy.  Without `out` fresh contiguous tensors are returned; cu_seqlens mode then needs
    total_rows (a host number: the call does not read cu_seqlens[-1] back), slot mode takes it from slot_mapping.
    No host synchronisation; capturable in a HIP graph."""
    op = "kv_gather"
    fp8 = k_cache.dtype == _fi._FP8
    if v_cache.dtype != k_cache.dtype or not (fp8 or k_cache.dtype in _fi._DTYPES):
        raise RuntimeError(f"kv_gather: k_cache / v_cache must both be fp16, bf16 or float8_e4m3fn, got {k_cache.dtype} / {v_cache.dtype}")
    _ra.cache_shape(op, k_cache, v_cache)
    H, D = k_cache.shape[2:]
    _ra.head_dim(op, D)
    if fp8:
        if dtype is None:
            raise RuntimeError("kv_gather: a float8_e4m3fn cache needs dtype= (torch.float16 or torch.bfloat16)")
        if dtype not in _fi._DTYPES:
            raise RuntimeError(f"kv_gather: dtype must be fp16 or bf16, got {dtype}")
    else:
        if dtype is not None and dtype != k_cache.dtype:
            raise RuntimeError(f"kv_gather: a 16-bit cache is copied bit for bit: dtype must be None or the cache's ({k_cache.dtype}), got {dtype}")
        dtype = k_cache.dtype
        _ra.descales_need_fp8(op, fp8, k_descale, v_descale)
    _ra.one_mode(op, slot_mapping, cu_seqlens, "seq_offsets")
    _ra.cache_last_dim(op, k_cache, v_cache)

    s = _lib.FaKvGatherParams()
    s.struct_size = ctypes.sizeof(_lib.FaKvGatherParams)
    B = 0
    if slot_mapping is not None:
        _ra.slot_mode(op, seq_offsets, "seq_offsets", block_table, cache_batch_idx)
        if slot_mapping.dtype not in (torch.int64, torch.int32) or slot_mapping.dim() != 1:
            raise RuntimeError("kv_gather: slot_mapping must be an int64 (or int32) tensor of shape (total_rows,)")
        if total_rows is not None and int(total_rows) != slot_mapping.numel():
            raise RuntimeError(f"kv_gather: total_rows {total_rows} is not slot_mapping's length {slot_mapping.numel()}")
        T = slot_mapping.numel()
        slot_mapping = slot_mapping.to(torch.int64).contiguous()
    else:
        B, cu_seqlens, seq_offsets, block_table, cache_batch_idx = _ra.sequence_mode(
            op, k_cache, cu_seqlens, seq_offsets, "seq_offsets", block_table, cache_batch_idx)
        if total_rows is None and out is None:
            raise RuntimeError("kv_gather: cu_seqlens mode needs total_rows= (or out=): the number of rows is a host quantity, "
                               "the call does not read cu_seqlens[-1] back from the device")
        T = int(total_rows) if total_rows is not None else int(out[0].shape[0])
        if T < 0:
            raise RuntimeError(f"kv_gather: total_rows must be >= 0, got {T}")
    # (the tensors made above stay referenced by these names until the launch is queued)
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise RuntimeError("kv_gather: out must be a pair (k_out, v_out)")
        k, v = out
        for t, name in ((k, "k_out"), (v, "v_out")):
            if t.dtype != dtype or tuple(t.shape) != (T, H, D):
                raise RuntimeError(f"kv_gather: {name} must be a {dtype} tensor of shape {(T, H, D)}, got {t.dtype} {tuple(t.shape)}")
            if not _viewable(t):
                raise RuntimeError(f"kv_gather: {name} must have a contiguous last dimension, a 16-byte aligned base and strides "
                                   "that are multiples of 16 bytes (an output is never copied behind the caller's back)")
    else:
        k = v = None
    _ra.same_device(op, [k_cache, v_cache, slot_mapping, cu_seqlens, seq_offsets, block_table, cache_batch_idx, k, v], k_cache,
                    "the cache's")
    if out is None:
        k = torch.empty((T, H, D), dtype=dtype, device=k_cache.device)
        v = torch.empty((T, H, D), dtype=dtype, device=k_cache.device)
    if T == 0 or H == 0:
        return k, v

    s.k, s.v = k.data_ptr(), v.data_ptr()
    s.k_row_stride, s.k_head_stride = k.stride(0), k.stride(1)
    s.v_row_stride, s.v_head_stride = v.stride(0), v.stride(1)
    s.total_rows, s.nheads, s.head_dim = T, H, D
    s.dtype = _fi._DTYPES[dtype]
    _ra.fill_cache(s, k_cache, v_cache, fp8, k_descale, v_descale)
    _ra.fill_mode(s, slot_mapping, cu_seqlens, B, seq_offsets, "seq_offsets", block_table, cache_batch_idx)
    with _fi._on_device(k_cache.device):
        _lib.call_kv_gather(s, _fi._stream(k_cache.device))   # (queued: the prepared tensors stay referenced until here)
    del slot_mapping, cu_seqlens, seq_offsets, block_table, cache_batch_idx
    return k, v


def move_kv_cache(k_cache, v_cache, src_slots, dst_slots) -> None:
    """Move rows inside a cache: row src_slots[r] -> row dst_slots[r] of k_cache and v_cache, for every r (slots as in
    store_kv_cache / gather_kv_cache: block = slot // cache.shape[1], row = slot % cache.shape[1]; int64 or int32 tensors of one
    length).  This is how the accepted path of a speculative-decoding tree is committed - the kv-cache op's tree mode appended all
    T draft nodes at cache_seqlens + t, the accepted nodes t_0 < t_1 < ... go to cache_seqlens + 0, 1, ... - and how pages are
    copied (beam search, copy-on-write forks: runs of slots).

    Two launches on the current stream: gather_kv_cache by src_slots into a staging pair, then store_kv_cache by dst_slots.
    Sources and destinations may overlap (slot L + 2 may be read for one row and written for another): the gather has finished, in
    stream order, before the store starts - one in-place kernel could not promise that.  A dst slot < 0 (or past the end) skips
    the row; a src slot < 0 or past the end stores a row of zeros.  Two rows with the same destination: one of them wins.
    Staging dtype: the cache's own for fp16 / bf16 caches (a bit copy); bf16 with descale 1.0 in both directions for
    float8_e4m3fn caches - every finite e4m3 value is a bf16 value, so the finite codes arrive unchanged.
    No host synchronisation; capturable in a HIP graph."""
    if src_slots.dim() != 1 or tuple(src_slots.shape) != tuple(dst_slots.shape):
        raise RuntimeError(f"kv_gather: src_slots and dst_slots must be 1-D tensors of one length, got {tuple(src_slots.shape)} / "
                           f"{tuple(dst_slots.shape)}")
    fp8 = k_cache.dtype == _fi._FP8
    kw = dict(k_descale=1.0, v_descale=1.0) if fp8 else {}
    k, v = gather_kv_cache(k_cache, v_cache, slot_mapping=src_slots, dtype=torch.bfloat16 if fp8 else None, **kw)
    _kv_store.store_kv_cache(k, v, k_cache, v_cache, slot_mapping=dst_slots, **kw)
    return None
