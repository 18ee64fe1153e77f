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
from typing import Optional

import torch

from . import _lib
from . import _rowargs as _ra

# what this op's messages add to the shared ones: without caches the call only rotates (_rowargs.rope_and_store's `hints`)
_HINTS = (": rotate only", " (without caches the call only rotates)", " (apply_rotary_emb takes any even one)")


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
    return _ra.rope_and_store("rope_store", _lib.FaRopeStoreParams, _lib.call_rope_store, None, False, _HINTS, q, k, v, positions,
                              rotary_cos, rotary_sin, k_cache, v_cache, slot_mapping, interleaved, inplace, k_out, k_descale, v_descale)
