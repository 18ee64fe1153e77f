"""Shared-prefix ("cascade") decode: attend a prefix that a whole batch shares ONCE, each sequence's own tokens as before, and
merge the two partial results through their log-sum-exps.

A decode step is bound by the bytes of the KV cache it reads (README: decode).  When every sequence of a batch starts with the
same system prompt, `flash_attn_with_kvcache` reads those bytes once per sequence; here they are read once per batch:

  1. one dense, non-causal `fa_fwd` of all B x T query rows over the prefix,
  2. one `flash_attn_with_kvcache` over each sequence's own tokens (the suffix),
  3. one `fa_merge_states` (csrc/fa_merge.hip) on the two (out, lse) pairs.

`merge_attention_states` is the merge alone - the device form of `sharding.merge_attention_shards`, which keeps its torch
implementation.  Forward only; nothing here is exported through the packages' `__all__` lists."""
import ctypes

import torch

from . import _lib
from . import flash_attn_interface as _fi

_FP8 = torch.float8_e4m3fn


def _mergeable(o):
    """what fa_merge_states takes as it is: a contiguous last dimension, base and strides multiples of 8 bytes (it moves 16-byte
    pieces where they are multiples of 16); anything else is copied"""
    ok = o.stride(-1) == 1 and o.data_ptr() % 8 == 0 and all(s % 4 == 0 for s in o.stride()[:-1])
    return o if ok else o.contiguous()


def _merge(outs, lses):
    """fa_merge_states on already checked [B, S, H, D] / fp32 [B, H, S] views -> fresh contiguous (out, lse)"""
    B, S, H, D = outs[0].shape
    out = torch.empty((B, S, H, D), dtype=outs[0].dtype, device=outs[0].device)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=outs[0].device)
    m = _lib.FaMergeParams()
    m.struct_size = ctypes.sizeof(_lib.FaMergeParams)
    m.n_parts, m.batch, m.seqlen, m.nheads, m.head_dim = len(outs), B, S, H, D
    m.dtype = _fi._DTYPES[out.dtype]
    keep = [_mergeable(o) for o in outs]                      # (copies stay alive until the launch is queued)
    for st, o, l in zip(m.parts, keep, lses):
        _lib.merge_state(st, o, l)
    _lib.merge_state(m.out, out, lse)
    if out.numel() > 0:
        with _fi._on_device(out.device):
            _lib.call_merge(m, _fi._stream(out.device))
    return out, lse


def merge_attention_states(outs, lses):
    """Combine attention computed over DISJOINT key sets into attention over their union, on the GPU (fa_merge_states).

    outs[s]: [B, S, H, D] fp16 / bf16 output of a forward op of this package over key set s; lses[s]: [B, H, S] fp32 log-sum-exp of
    the same call (natural log, -inf for rows that saw no key).  2 .. 8 parts, D a multiple of 8 and at most 256.  Both are taken
    as strided views (no copies; an `out` whose base or strides are not multiples of 8 bytes is copied first).
    Returns (out, lse) with LSE = logsumexp_s(lse_s), out = sum_s exp(lse_s - LSE) out_s in fp32 arithmetic - the semantics of
    `sharding.merge_attention_shards`.  A part with lse_s = -inf contributes nothing even if its out_s holds NaN; all parts -inf
    give out 0 and LSE -inf; with exactly one finite part the row is that part's row bit for bit.  Forward only."""
    outs, lses = list(outs), list(lses)
    _fi._check_device(*outs, *lses)
    if len(outs) != len(lses) or not 2 <= len(outs) <= _lib.FA_MERGE_MAX_PARTS:
        raise RuntimeError(f"merge_attention_states takes 2 .. {_lib.FA_MERGE_MAX_PARTS} (out, lse) pairs, got {len(outs)} / {len(lses)}")
    o0 = outs[0]
    if o0.dtype not in _fi._DTYPES or o0.dim() != 4:
        raise RuntimeError("outs must be fp16 or bf16 tensors of shape (B, S, H, D)")
    B, S, H, D = o0.shape
    if D % 8 != 0 or D > 256:
        raise RuntimeError("merge head dimension must be a multiple of 8 and <= 256")
    for i, (o, l) in enumerate(zip(outs, lses)):
        if o.dtype != o0.dtype or o.device != o0.device or l.device != o0.device:
            raise RuntimeError("every part must have the dtype and device of outs[0]")
        if l.dtype != torch.float32:
            raise RuntimeError("lses must be fp32")
        _fi._check_shape(o, (B, S, H, D), f"outs[{i}]")
        _fi._check_shape(l, (B, H, S), f"lses[{i}]")
    return _merge(outs, lses)


def flash_attn_with_shared_prefix(q, prefix_k, prefix_v, k_cache, v_cache, k=None, v=None, cache_seqlens=None,
                                  cache_batch_idx=None, cache_leftpad=None, block_table=None, softmax_scale=None, softcap=0.0,
                                  num_splits=0, k_descale=None, v_descale=None, sinks=None, return_softmax_lse=False, *,
                                  rotary_cos=None, rotary_sin=None, window_size=(-1, -1), alibi_slopes=None, tree_mask=None,
                                  tree_depths=None):
    """Attention of q over [prefix ; each sequence's own cache (+ the appended k, v)] with the prefix read once per batch.

    q [B, T, H, D] fp16 / bf16; prefix_k / prefix_v [S_p, H_k, D] or [1, S_p, H_k, D] in q's dtype: the keys / values every
    sequence of the batch starts with.  k_cache / v_cache and every other argument are `flash_attn_with_kvcache`'s and describe
    ONLY the tokens AFTER the prefix: contiguous, paged (block_table) or fp8-e4m3 caches (k_descale / v_descale),
    cache_seqlens counting suffix tokens, k / v appended at cache_seqlens as there.  Every query sees the whole prefix; the suffix
    is bottom-right causal as in the kv-cache op.  Returns out [B, T, H, D] (and the LSE [B, H, T] of the whole problem with
    return_softmax_lse).

    Three launches on the current stream, no host synchronisation (the call can be captured in a HIP graph):
      1. the suffix: `flash_attn_with_kvcache(..., causal=True)`, decode or general route as today.  It runs first because it
         validates the cache arguments: a rejected call then leaves nothing behind;
      2. the prefix: ONE non-causal `fa_fwd` with q viewed as a single sequence of B x T rows, [1, B T, H, D] - a view of q, no
         copy; its out is [B, T, H, D] again and its LSE [1, H, B T] is read as [B, H, T] through strides.  The mask is all-visible,
         so row order is free.  This layout was chosen over a permuted copy that packs a GQA group's heads as rows because it needs
         no extra pass over q and out, and the forward kernels already place the query heads of one kv-head on one XCD, whose L2
         serves the group's re-reads of the prefix;
      3. `fa_merge_states` on the two (out, lse) pairs.
    sinks go to the suffix call ONLY (a sink-inclusive LSE from both parts would count the sink twice); the merged LSE is then the
    sink-inclusive LSE of the whole problem.
    S_p == 0 returns the kv-cache call's result unchanged.  A sequence with an empty suffix (cache_seqlens[b] == 0, nothing
    appended, no sinks) returns the prefix part bit for bit.

    Out of scope, raised before anything is launched or allocated: in-kernel rotary (pass rotated q and k, as vLLM does: the
    suffix kernel's RoPE would leave the prefix pass with an unrotated q), sliding windows and ALiBi (both need global positions
    across the two parts), tree masks, an fp8 prefix or fp8 q, and any backward.  The keyword-only arguments after
    return_softmax_lse exist to say so by name.  What the kv-cache op rejects stays rejected, by that op and before its first
    launch: softcap with T > 1 among them (its causal mask is a window, and the op takes no softcap with a window)."""
    _fi._check_device(q, prefix_k, prefix_v, k_cache, v_cache, k, v)
    if rotary_cos is not None or rotary_sin is not None:
        raise RuntimeError("shared prefix: in-kernel rotary is not supported - pass rotated q and k (the prefix pass would see an unrotated q)")
    if tuple(window_size) != (-1, -1):
        raise RuntimeError("shared prefix: sliding windows are not supported (they need positions across prefix and suffix)")
    if alibi_slopes is not None:
        raise RuntimeError("shared prefix: ALiBi is not supported (it needs positions across prefix and suffix)")
    if tree_mask is not None or tree_depths is not None:
        raise RuntimeError("shared prefix: tree masks are not supported")
    if q.dtype == _FP8 or prefix_k.dtype == _FP8 or prefix_v.dtype == _FP8:
        raise RuntimeError("shared prefix: fp8 q or an fp8 prefix is not supported (fp8 suffix caches are)")
    if q.dtype not in _fi._DTYPES:
        raise RuntimeError("q must be fp16 or bf16")
    if prefix_k.dtype != q.dtype or prefix_v.dtype != q.dtype:
        raise RuntimeError("prefix_k / prefix_v must have the same dtype as q")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (q, prefix_k, prefix_v, k, v, sinks)):
        raise RuntimeError("shared prefix: forward only, no backward")
    if q.dim() != 4 or k_cache.dim() != 4:
        raise RuntimeError("q must be (B, T, H, D); k_cache / v_cache 4-D")
    B, T, H, D = q.shape
    if D % 8 != 0 or D > 256:
        raise RuntimeError("kvcache head dimension must be a multiple of 8 and <= 256")
    if prefix_k.dim() == 3:
        prefix_k = prefix_k[None]
    if prefix_v.dim() == 3:
        prefix_v = prefix_v[None]
    H_K = k_cache.shape[2]
    if prefix_k.dim() != 4 or prefix_k.shape[0] != 1:
        raise RuntimeError("prefix_k / prefix_v must be (S_p, H_k, D) or (1, S_p, H_k, D)")
    S_p = prefix_k.shape[1]
    _fi._check_shape(prefix_k, (1, S_p, H_K, D), "prefix_k")
    _fi._check_shape(prefix_v, (1, S_p, H_K, D), "prefix_v")
    suffix = _fi.flash_attn_with_kvcache(
        q, k_cache, v_cache, k=k, v=v, cache_seqlens=cache_seqlens, cache_batch_idx=cache_batch_idx, cache_leftpad=cache_leftpad,
        block_table=block_table, softmax_scale=softmax_scale, causal=True, softcap=softcap, num_splits=num_splits,
        return_softmax_lse=True, k_descale=k_descale, v_descale=v_descale, sinks=sinks)
    if S_p == 0:
        return suffix if return_softmax_lse else suffix[0]
    q1 = q.reshape(1, B * T, H, D)
    o_p, lse_p = _fi._dense_forward(q1, prefix_k, prefix_v, 0.0, softmax_scale, False, (-1, -1), softcap, None, False)[:2]
    out, lse = _merge([o_p.view(B, T, H, D), suffix[0]], [lse_p[0].view(H, B, T).permute(1, 0, 2), suffix[1]])
    return (out, lse) if return_softmax_lse else out
