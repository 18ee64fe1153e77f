"""torch.library registration of the five operators: `torch.ops.flash_attn_mi355.{fwd, bwd,
varlen_fwd, varlen_bwd, fwd_kvcache}` (and `fwd_kvcache_tree`: the kv-cache op with a tree attention mask; `merge_states`: the
LSE merge of attention states over disjoint key sets, fa_merge_states; `rotary` / `rotary_`: the standalone rotary embedding,
fa_rotary; `kv_store`: a ragged packed batch of K / V rows into a KV cache, fa_kv_store; `kv_gather` / `kv_move`: ragged K / V
rows out of a KV cache, fa_kv_gather, and gather -> store inside one cache; `rope_store_`: q / k rotated at per-token positions
and K / V stored by slot in one launch, fa_rope_store; `qk_norm_rope_store_`: the same behind a per-head RMSNorm of q and k,
fa_qk_norm_rope_store; `qk_norm_rope` / `qk_norm_rope_bwd`: that norm + rotation out of place with an autograd formula, and its
backward, fa_qk_norm_rope_bwd; `add_norm` / `add_norm_` / `add_norm_bwd`: residual add + RMSNorm / LayerNorm over the hidden size
with an autograd formula, its in-place form and its backward, fa_add_norm / fa_add_norm_bwd; `cross_entropy` / `cross_entropy_bwd`
/ `cross_entropy_bwd_`: the softmax cross-entropy loss over the vocabulary with an autograd formula, its backward and the backward
in place, fa_cross_entropy / fa_cross_entropy_bwd; `act_mul` / `act_and_mul` / `act_mul_bwd` / `act_and_mul_bwd` / `act_mul_bwd_`:
the gated activation act(gate) * up of the MLP on separate or packed tensors with autograd formulas, its backward and the backward
in place, fa_act_mul / fa_act_mul_bwd; `quant_fp8` / `add_norm_quant` / `act_mul_quant` / `act_and_mul_quant`: dynamic fp8-e4m3
quantisation alone and fused behind the forwards of add_norm and act_mul, fa_quant_fp8 / fa_add_norm_quant / fa_act_mul_quant, not
differentiable; `moe_route` / `moe_route_bwd` / `moe_sort` / `moe_permute` / `moe_combine` / `moe_combine_bwd`: top-k routing, the
stable sort of the (token, k) slots by expert, the permutation into per-expert segments and the weighted combine of a
mixture-of-experts block with autograd formulas, fa_moe_*, and `moe_gemm`, its forward grouped expert GEMM over `expert_offsets`,
fa_moe_gemm, not differentiable, `moe_gemm_wgrad`, its weight and bias gradients, fa_moe_gemm_wgrad, and `moe_linear`, the
differentiable expert layer built on them; `sample` / `sample_filter`: temperature / top-k / min-p / top-p token
sampling from logits and the filtered logits alone, fa_sample, not differentiable; `spec_accept` / `spec_walk` / `spec_verify`:
speculative-decoding verification, fa_spec_accept / fa_spec_walk, not differentiable - registered, but not listed in `__all__`).

Counterpart of the reference's TorchBind block (kernel/fused_mha_api.cpp:308-358: `fwd`, `bwd`,
`varlen_fwd`, `varlen_bwd`, `fwd_kvcache` under `flash_attn_v100_cuda`).  The argument ORDER follows
the reference schemas (include/mha.h:27-41, :67-87, :116-139, :170-195, :224-245); the tensor
LAYOUT is the public Python one - (B, S, H, D) / (T, H, D) - because this build takes strides
and never permutes ("replicate the Python API, not the alias").
The optional in-place outputs of the reference (`out` of fwd / varlen_fwd, `dq`, `dk`, `dv` of bwd:
include/mha.h:31,73-75) live in the separate ops `fwd_out`, `varlen_fwd_out` and `bwd_out`, which MUTATE
caller-allocated tensors (a torch.library op may not return an alias of an input); the plain ops return fresh
tensors.  `varlen_fwd` carries the reference's op-level extras `seqused_k`, `leftpad_k`, `zero_tensors`,
`num_splits` (include/mha.h:116-139).  `fwd` / `varlen_fwd` also take float8_e4m3fn q, k, v (the fp8 forward, descales 1,
forward only) and return a bf16 `out` for them.  Every op has a fake (meta) implementation so the path is traceable by
torch.compile / FakeTensorMode, and `fwd` / `varlen_fwd` carry autograd formulas that call the
`bwd` ops.

Import this module to register the ops (flash_attn_mi355/__init__.py does NOT import it, so
that plain users of the functional API pay nothing).
"""
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import act_mul as _act_mul
from . import add_norm as _add_norm
from . import cascade as _cascade
from . import cross_entropy as _ce
from . import flash_attn_interface as _fi
from . import kv_gather as _kv_gather
from . import kv_store as _kv_store
from . import qk_norm as _qk_norm
from . import quant as _quant
from . import rope_store as _rope_store
from . import rotary as _rotary
from . import sample as _sample
from . import spec_decode as _spec

_NS = "flash_attn_mi355"


def _rng_tensor(rng, device):
    seed = int(rng[0]) & 0xFFFFFFFFFFFFFFFF
    if seed >= 1 << 63:                         # int64 carrier: two's complement, lossless
        seed -= 1 << 64
    return torch.tensor([seed, int(rng[1])], dtype=torch.int64, device=device)


def _out_dtype(q: Tensor):
    """float8_e4m3fn q, k, v: the fp8 forward writes bf16 out (flash_attn_interface._dense_forward)"""
    return torch.bfloat16 if q.dtype == torch.float8_e4m3fn else q.dtype


def _no_fp8_backward(q: Tensor):
    if q.dtype == torch.float8_e4m3fn:
        raise RuntimeError("the fp8 (float8_e4m3fn) forward is forward-only: no backward")


def _rng_tuple(rng_state: Optional[Tensor]):
    if rng_state is None:
        return None
    s = rng_state.tolist()                      # host sync, as the reference's rng_state.cpu()
    return (int(s[0]) & 0xFFFFFFFFFFFFFFFF, int(s[1]))


# ------------------------------------------------------------------------------------------
# dense
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::fwd", mutates_args=(), device_types="cuda")
def fwd(q: Tensor, k: Tensor, v: Tensor, alibi_slopes: Optional[Tensor], p_dropout: float,
        softmax_scale: float, is_causal: bool, window_size_left: int, window_size_right: int,
        softcap: float, return_softmax: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    out, lse, dmask, _, rng, _ = _fi._dense_forward(
        q, k, v, p_dropout, softmax_scale, is_causal, (window_size_left, window_size_right), softcap,
        alibi_slopes, return_softmax)
    return out, lse, dmask, _rng_tensor(rng, q.device)


@fwd.register_fake
def _(q, k, v, alibi_slopes, p_dropout, softmax_scale, is_causal, window_size_left,
      window_size_right, softcap, return_softmax):
    B, M, H, D = q.shape
    N = k.shape[1]
    o_dtype = _out_dtype(q)
    out = q.new_empty((B, M, H, D), dtype=o_dtype)
    lse = q.new_empty((B, H, M), dtype=torch.float32)
    dmask = q.new_empty((B, H, M, N) if (return_softmax and p_dropout > 0.0) else (0,), dtype=o_dtype)
    return out, lse, dmask, q.new_empty((2,), dtype=torch.int64)


@torch.library.custom_op(f"{_NS}::bwd", mutates_args=(), device_types="cuda")
def bwd(dout: Tensor, q: Tensor, k: Tensor, v: Tensor, out: Tensor, softmax_lse: Tensor,
        alibi_slopes: Optional[Tensor], p_dropout: float, softmax_scale: float, is_causal: bool,
        window_size_left: int, window_size_right: int, softcap: float, deterministic: bool,
        rng_state: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    d = q.shape[-1]
    dpad = (d + 7) // 8 * 8
    q_, k_, v_, out_ = (_fi._prep(t, dpad) for t in (q, k, v, out))
    dq_, dk_, dv_ = _fi._grad_buffers(q_, k_, v_)
    softmax_d = _fi._dense_backward(dout, q_, k_, v_, out_, softmax_lse, alibi_slopes, p_dropout,
                                    softmax_scale, is_causal, (window_size_left, window_size_right),
                                    softcap, _rng_tuple(rng_state) if p_dropout > 0.0 else (0, 0),
                                    dq_, dk_, dv_, deterministic=deterministic)
    if dpad != d:
        dq_, dk_, dv_ = (t[..., :d].contiguous() for t in (dq_, dk_, dv_))
    return dq_, dk_, dv_, softmax_d


@bwd.register_fake
def _(dout, q, k, v, out, softmax_lse, alibi_slopes, p_dropout, softmax_scale, is_causal,
      window_size_left, window_size_right, softcap, deterministic, rng_state):
    B, M, H, _ = q.shape
    return (torch.empty_like(q), torch.empty_like(k), torch.empty_like(v),
            q.new_empty((B, H, M), dtype=torch.float32))


def _fwd_setup(ctx, inputs, output):
    (q, k, v, alibi_slopes, p_dropout, softmax_scale, is_causal, wl, wr, softcap, _) = inputs
    out, lse, _, rng_state = output
    ctx.save_for_backward(q, k, v, out, lse, rng_state, alibi_slopes)
    ctx.args = (p_dropout, softmax_scale, is_causal, wl, wr, softcap)


def _fwd_backward(ctx, dout, dlse, ddmask, drng):
    q, k, v, out, lse, rng_state, alibi_slopes = ctx.saved_tensors
    _no_fp8_backward(q)
    p_dropout, softmax_scale, is_causal, wl, wr, softcap = ctx.args
    dq, dk, dv, _ = bwd(dout, q, k, v, out, lse, alibi_slopes, p_dropout, softmax_scale, is_causal,
                        wl, wr, softcap, False, rng_state)
    return (dq, dk, dv) + (None,) * 8


fwd.register_autograd(_fwd_backward, setup_context=_fwd_setup)


# ------------------------------------------------------------------------------------------
# varlen
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::varlen_fwd", mutates_args=(), device_types="cuda")
def varlen_fwd(q: Tensor, k: Tensor, v: Tensor, cu_seqlens_q: Tensor, cu_seqlens_k: Tensor,
               block_table: Optional[Tensor], alibi_slopes: Optional[Tensor], max_seqlen_q: int,
               max_seqlen_k: int, p_dropout: float, softmax_scale: float, is_causal: bool,
               window_size_left: int, window_size_right: int, softcap: float,
               return_softmax: bool, seqused_k: Optional[Tensor] = None, leftpad_k: Optional[Tensor] = None,
               zero_tensors: bool = False, num_splits: int = 0) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    if num_splits > 1:
        raise RuntimeError("num_splits > 1 not supported")          # fused_mha_forward_varlen.cu:422
    out, lse, dmask, _, rng, _ = _fi._varlen_forward(
        q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, p_dropout, softmax_scale,
        is_causal, (window_size_left, window_size_right), softcap, alibi_slopes, return_softmax,
        block_table, seqused_k=seqused_k, leftpad_k=leftpad_k, zero_tensors=zero_tensors)
    return out, lse, dmask, _rng_tensor(rng, q.device)


@varlen_fwd.register_fake
def _(q, k, v, cu_seqlens_q, cu_seqlens_k, block_table, alibi_slopes, max_seqlen_q, max_seqlen_k,
      p_dropout, softmax_scale, is_causal, window_size_left, window_size_right, softcap,
      return_softmax, seqused_k=None, leftpad_k=None, zero_tensors=False, num_splits=0):
    T, H, D = q.shape
    o_dtype = _out_dtype(q)
    dmask = q.new_empty((T, H, max_seqlen_k) if (return_softmax and p_dropout > 0.0) else (0,), dtype=o_dtype)
    return (q.new_empty((T, H, D), dtype=o_dtype), q.new_empty((H, T), dtype=torch.float32), dmask,
            q.new_empty((2,), dtype=torch.int64))


@torch.library.custom_op(f"{_NS}::varlen_bwd", mutates_args=(), device_types="cuda")
def varlen_bwd(dout: Tensor, q: Tensor, k: Tensor, v: Tensor, out: Tensor, softmax_lse: Tensor,
               cu_seqlens_q: Tensor, cu_seqlens_k: Tensor, alibi_slopes: Optional[Tensor],
               max_seqlen_q: int, max_seqlen_k: int, p_dropout: float, softmax_scale: float,
               is_causal: bool, window_size_left: int, window_size_right: int, softcap: float,
               deterministic: bool, rng_state: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    d = q.shape[-1]
    dpad = (d + 7) // 8 * 8
    q_, k_, v_, out_ = (_fi._prep(t, dpad) for t in (q, k, v, out))
    dq_, dk_, dv_ = _fi._grad_buffers(q_, k_, v_)
    cu_q = cu_seqlens_q.to(torch.int32).contiguous()
    cu_k = cu_seqlens_k.to(torch.int32).contiguous()
    softmax_d = _fi._varlen_backward(dout, q_, k_, v_, out_, softmax_lse, cu_q, cu_k, alibi_slopes,
                                     max_seqlen_q, max_seqlen_k, p_dropout, softmax_scale, is_causal,
                                     (window_size_left, window_size_right), softcap,
                                     _rng_tuple(rng_state) if p_dropout > 0.0 else (0, 0),
                                     dq_, dk_, dv_, deterministic=deterministic)
    if dpad != d:
        dq_, dk_, dv_ = (t[..., :d].contiguous() for t in (dq_, dk_, dv_))
    return dq_, dk_, dv_, softmax_d


@varlen_bwd.register_fake
def _(dout, q, k, v, out, softmax_lse, cu_seqlens_q, cu_seqlens_k, alibi_slopes, max_seqlen_q,
      max_seqlen_k, p_dropout, softmax_scale, is_causal, window_size_left, window_size_right,
      softcap, deterministic, rng_state):
    T, H, _ = q.shape
    return (torch.empty_like(q), torch.empty_like(k), torch.empty_like(v),
            q.new_empty((H, T), dtype=torch.float32))


def _varlen_setup(ctx, inputs, output):
    (q, k, v, cu_q, cu_k, block_table, alibi_slopes, max_q, max_k, p_dropout, softmax_scale,
     is_causal, wl, wr, softcap, _, seqused_k, _leftpad, _zero, _splits) = inputs
    if block_table is not None:
        raise RuntimeError("backward through paged K/V (block_table) is not supported")
    if seqused_k is not None:
        raise RuntimeError("seqused_k is a forward-only argument (the reference's varlen_bwd has none)")
    out, lse, _, rng_state = output
    ctx.save_for_backward(q, k, v, out, lse, cu_q, cu_k, rng_state, alibi_slopes)
    ctx.args = (max_q, max_k, p_dropout, softmax_scale, is_causal, wl, wr, softcap)


def _varlen_backward_formula(ctx, dout, dlse, ddmask, drng):
    q, k, v, out, lse, cu_q, cu_k, rng_state, alibi_slopes = ctx.saved_tensors
    _no_fp8_backward(q)
    max_q, max_k, p_dropout, softmax_scale, is_causal, wl, wr, softcap = ctx.args
    dq, dk, dv, _ = varlen_bwd(dout, q, k, v, out, lse, cu_q, cu_k, alibi_slopes, max_q, max_k,
                               p_dropout, softmax_scale, is_causal, wl, wr, softcap, False, rng_state)
    return (dq, dk, dv) + (None,) * 17


varlen_fwd.register_autograd(_varlen_backward_formula, setup_context=_varlen_setup)


# ------------------------------------------------------------------------------------------
# in-place forms: the reference's optional `out` / `dq` / `dk` / `dv` arguments (include/mha.h:31,73-75)
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::fwd_out", mutates_args=("out",), device_types="cuda")
def fwd_out(q: Tensor, k: Tensor, v: Tensor, out: Tensor, alibi_slopes: Optional[Tensor], p_dropout: float,
            softmax_scale: float, is_causal: bool, window_size_left: int, window_size_right: int,
            softcap: float, return_softmax: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """writes `out` (shape / dtype of q, contiguous last dim); returns (softmax_lse, dmask, rng_state)"""
    _, lse, dmask, _, rng, _ = _fi._dense_forward(
        q, k, v, p_dropout, softmax_scale, is_causal, (window_size_left, window_size_right), softcap,
        alibi_slopes, return_softmax, out=out)
    return lse, dmask, _rng_tensor(rng, q.device)


@fwd_out.register_fake
def _(q, k, v, out, alibi_slopes, p_dropout, softmax_scale, is_causal, window_size_left, window_size_right,
      softcap, return_softmax):
    B, M, H, _ = q.shape
    dmask = q.new_empty((B, H, M, k.shape[1]) if (return_softmax and p_dropout > 0.0) else (0,))
    return q.new_empty((B, H, M), dtype=torch.float32), dmask, q.new_empty((2,), dtype=torch.int64)


@torch.library.custom_op(f"{_NS}::varlen_fwd_out", mutates_args=("out",), device_types="cuda")
def varlen_fwd_out(q: Tensor, k: Tensor, v: Tensor, out: Tensor, cu_seqlens_q: Tensor, cu_seqlens_k: Tensor,
                   seqused_k: Optional[Tensor], leftpad_k: Optional[Tensor], block_table: Optional[Tensor],
                   alibi_slopes: Optional[Tensor], max_seqlen_q: int, max_seqlen_k: int, p_dropout: float,
                   softmax_scale: float, zero_tensors: bool, is_causal: bool, window_size_left: int,
                   window_size_right: int, softcap: float, return_softmax: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """the reference's argument order (include/mha.h:116-139) with a caller-allocated `out`"""
    _, lse, dmask, _, rng, _ = _fi._varlen_forward(
        q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, p_dropout, softmax_scale,
        is_causal, (window_size_left, window_size_right), softcap, alibi_slopes, return_softmax,
        block_table, seqused_k=seqused_k, leftpad_k=leftpad_k, zero_tensors=zero_tensors, out=out)
    return lse, dmask, _rng_tensor(rng, q.device)


@varlen_fwd_out.register_fake
def _(q, k, v, out, cu_seqlens_q, cu_seqlens_k, seqused_k, leftpad_k, block_table, alibi_slopes, max_seqlen_q,
      max_seqlen_k, p_dropout, softmax_scale, zero_tensors, is_causal, window_size_left, window_size_right,
      softcap, return_softmax):
    T, H, _ = q.shape
    dmask = q.new_empty((T, H, max_seqlen_k) if (return_softmax and p_dropout > 0.0) else (0,))
    return q.new_empty((H, T), dtype=torch.float32), dmask, q.new_empty((2,), dtype=torch.int64)


@torch.library.custom_op(f"{_NS}::bwd_out", mutates_args=("dq", "dk", "dv"), device_types="cuda")
def bwd_out(dout: Tensor, q: Tensor, k: Tensor, v: Tensor, out: Tensor, softmax_lse: Tensor,
            dq: Tensor, dk: Tensor, dv: Tensor, alibi_slopes: Optional[Tensor], p_dropout: float,
            softmax_scale: float, is_causal: bool, window_size_left: int, window_size_right: int,
            softcap: float, deterministic: bool, rng_state: Optional[Tensor]) -> Tensor:
    """writes caller-allocated dq / dk / dv (shapes of q / k / v); returns softmax_d"""
    d = q.shape[-1]
    dpad = (d + 7) // 8 * 8
    for name, g, ref in (("dq", dq, q), ("dk", dk, k), ("dv", dv, v)):
        if g.dtype != ref.dtype or tuple(g.shape) != tuple(ref.shape) or g.stride(-1) != 1:
            raise RuntimeError(f"{name} must have the dtype and shape of its input and a contiguous last dimension")
    q_, k_, v_, out_ = (_fi._prep(t, dpad) for t in (q, k, v, out))
    direct = dpad == d and all(t.data_ptr() % 16 == 0 and all(st % 8 == 0 for st in t.stride()[:-1]) for t in (dq, dk, dv))
    dq_, dk_, dv_ = (dq, dk, dv) if direct else _fi._grad_buffers(q_, k_, v_)
    softmax_d = _fi._dense_backward(dout, q_, k_, v_, out_, softmax_lse, alibi_slopes, p_dropout,
                                    softmax_scale, is_causal, (window_size_left, window_size_right),
                                    softcap, _rng_tuple(rng_state) if p_dropout > 0.0 else (0, 0),
                                    dq_, dk_, dv_, deterministic=deterministic)
    if not direct:
        dq.copy_(dq_[..., :d]); dk.copy_(dk_[..., :d]); dv.copy_(dv_[..., :d])
    return softmax_d


@bwd_out.register_fake
def _(dout, q, k, v, out, softmax_lse, dq, dk, dv, alibi_slopes, p_dropout, softmax_scale, is_causal,
      window_size_left, window_size_right, softcap, deterministic, rng_state):
    B, M, H, _ = q.shape
    return q.new_empty((B, H, M), dtype=torch.float32)


# ------------------------------------------------------------------------------------------
# kv-cache (mutates the caches in place, like the reference op)
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::fwd_kvcache", mutates_args=("kcache", "vcache"), device_types="cuda")
def fwd_kvcache(q: Tensor, kcache: Tensor, vcache: Tensor, k: Optional[Tensor], v: Optional[Tensor],
                seqlens_k: Optional[Tensor], rotary_cos: Optional[Tensor], rotary_sin: Optional[Tensor],
                cache_batch_idx: Optional[Tensor], leftpad_k: Optional[Tensor],
                block_table: Optional[Tensor], alibi_slopes: Optional[Tensor], softmax_scale: float,
                is_causal: bool, window_size_left: int, window_size_right: int, softcap: float,
                is_rotary_interleaved: bool, num_splits: int) -> Tuple[Tensor, Tensor]:
    out, lse = _fi.flash_attn_with_kvcache(
        q, kcache, vcache, k=k, v=v, rotary_cos=rotary_cos, rotary_sin=rotary_sin,
        cache_seqlens=seqlens_k, cache_batch_idx=cache_batch_idx, cache_leftpad=leftpad_k,
        block_table=block_table, softmax_scale=softmax_scale, causal=is_causal,
        window_size=(window_size_left, window_size_right), softcap=softcap,
        rotary_interleaved=is_rotary_interleaved, alibi_slopes=alibi_slopes, num_splits=num_splits,
        return_softmax_lse=True)
    return out, lse


@fwd_kvcache.register_fake
def _(q, kcache, vcache, k, v, seqlens_k, rotary_cos, rotary_sin, cache_batch_idx, leftpad_k,
      block_table, alibi_slopes, softmax_scale, is_causal, window_size_left, window_size_right,
      softcap, is_rotary_interleaved, num_splits):
    B, T, H, _ = q.shape
    return torch.empty_like(q), q.new_empty((B, H, T), dtype=torch.float32)


@torch.library.custom_op(f"{_NS}::fwd_kvcache_tree", mutates_args=("kcache", "vcache"), device_types="cuda")
def fwd_kvcache_tree(q: Tensor, kcache: Tensor, vcache: Tensor, k: Optional[Tensor], v: Optional[Tensor],
                     seqlens_k: Optional[Tensor], rotary_cos: Optional[Tensor], rotary_sin: Optional[Tensor],
                     cache_batch_idx: Optional[Tensor], leftpad_k: Optional[Tensor],
                     block_table: Optional[Tensor], tree_mask: Tensor, tree_depths: Optional[Tensor],
                     softmax_scale: float, softcap: float, is_rotary_interleaved: bool,
                     num_splits: int) -> Tuple[Tensor, Tensor]:
    """fwd_kvcache for the nodes of a speculative-decoding draft tree: `tree_mask` (bool [B, T, T] / [T, T] or packed int32
    [B, T, W] / [T, W]) replaces the causal rule among the T new tokens, `tree_depths` gives their rotary positions
    (flash_attn_with_kvcache).  No ALiBi, no windows."""
    out, lse = _fi.flash_attn_with_kvcache(
        q, kcache, vcache, k=k, v=v, rotary_cos=rotary_cos, rotary_sin=rotary_sin,
        cache_seqlens=seqlens_k, cache_batch_idx=cache_batch_idx, cache_leftpad=leftpad_k,
        block_table=block_table, softmax_scale=softmax_scale, causal=False, softcap=softcap,
        rotary_interleaved=is_rotary_interleaved, num_splits=num_splits, return_softmax_lse=True,
        tree_mask=tree_mask, tree_depths=tree_depths)
    return out, lse


@fwd_kvcache_tree.register_fake
def _(q, kcache, vcache, k, v, seqlens_k, rotary_cos, rotary_sin, cache_batch_idx, leftpad_k, block_table,
      tree_mask, tree_depths, softmax_scale, softcap, is_rotary_interleaved, num_splits):
    B, T, H, _ = q.shape
    return torch.empty_like(q), q.new_empty((B, H, T), dtype=torch.float32)


# ------------------------------------------------------------------------------------------
# merge of attention states over disjoint key sets (shared-prefix decode, context parallelism)
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::merge_states", mutates_args=(), device_types="cuda")
def merge_states(outs: List[Tensor], lses: List[Tensor]) -> Tuple[Tensor, Tensor]:
    """cascade.merge_attention_states: outs[s] [B, S, H, D] fp16 / bf16, lses[s] [B, H, S] fp32, 2 .. 8 parts -> (out, lse).
    Forward only (no autograd formula)."""
    return _cascade.merge_attention_states(outs, lses)


@merge_states.register_fake
def _(outs, lses):
    B, S, H, D = outs[0].shape
    return outs[0].new_empty((B, S, H, D)), outs[0].new_empty((B, H, S), dtype=torch.float32)


# ------------------------------------------------------------------------------------------
# standalone rotary embedding (flash_attn.layers.rotary; csrc/fa_rotary.hip)
# ------------------------------------------------------------------------------------------
def _rotary_offsets(seqlen_offsets, seqlen_offset):
    return seqlen_offset if seqlen_offsets is None else seqlen_offsets


@torch.library.custom_op(f"{_NS}::rotary", mutates_args=(), device_types="cuda")
def rotary(x: Tensor, cos: Tensor, sin: Tensor, seqlen_offsets: Optional[Tensor], cu_seqlens: Optional[Tensor],
           seqlen_offset: int, max_seqlen: int, interleaved: bool, conjugate: bool) -> Tensor:
    """rotary.apply_rotary out of place: x [B, S, H, D] (or [T, H, D] with cu_seqlens and max_seqlen) fp16 / bf16, cos / sin
    [seqlen_ro, rotary_dim / 2]; positions i + seqlen_offset, or i + seqlen_offsets[b] with the int32 [B] tensor.  Returns a
    fresh contiguous tensor.  Differentiable in x: the backward is the same op with `not conjugate`."""
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    return _rotary._launch(x, out, cos, sin, interleaved, conjugate, _rotary_offsets(seqlen_offsets, seqlen_offset),
                           cu_seqlens, max_seqlen if cu_seqlens is not None else None)


@rotary.register_fake
def _(x, cos, sin, seqlen_offsets, cu_seqlens, seqlen_offset, max_seqlen, interleaved, conjugate):
    return x.new_empty(x.shape)


@torch.library.custom_op(f"{_NS}::rotary_", mutates_args=("x",), device_types="cuda")
def rotary_(x: Tensor, cos: Tensor, sin: Tensor, seqlen_offsets: Optional[Tensor], cu_seqlens: Optional[Tensor],
            seqlen_offset: int, max_seqlen: int, interleaved: bool, conjugate: bool) -> None:
    """`rotary` in place on x (a view with a contiguous last dimension is rotated where it lies)"""
    _rotary._launch(x, x, cos, sin, interleaved, conjugate, _rotary_offsets(seqlen_offsets, seqlen_offset),
                    cu_seqlens, max_seqlen if cu_seqlens is not None else None)


@rotary_.register_fake
def _(x, cos, sin, seqlen_offsets, cu_seqlens, seqlen_offset, max_seqlen, interleaved, conjugate):
    return None


def _rotary_setup(ctx, inputs, output):
    (_, cos, sin, seqlen_offsets, cu_seqlens, seqlen_offset, max_seqlen, interleaved, conjugate) = inputs
    ctx.save_for_backward(cos, sin, seqlen_offsets, cu_seqlens)
    ctx.args = (seqlen_offset, max_seqlen, interleaved, conjugate)


def _rotary_backward(ctx, dout):
    cos, sin, seqlen_offsets, cu_seqlens = ctx.saved_tensors
    seqlen_offset, max_seqlen, interleaved, conjugate = ctx.args
    if dout.stride(-1) != 1:
        dout = dout.contiguous()
    dx = rotary(dout, cos, sin, seqlen_offsets, cu_seqlens, seqlen_offset, max_seqlen, interleaved, not conjugate)
    return (dx,) + (None,) * 8


rotary.register_autograd(_rotary_backward, setup_context=_rotary_setup)


# ------------------------------------------------------------------------------------------
# KV-cache store (flash_attn_mi355.kv_store; csrc/fa_kv_store.hip)
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::kv_store", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def kv_store(k: Tensor, v: Tensor, k_cache: Tensor, v_cache: Tensor, slot_mapping: Optional[Tensor],
             cu_seqlens: Optional[Tensor], cache_seqlens: Optional[Tensor], block_table: Optional[Tensor],
             cache_batch_idx: Optional[Tensor], rotary_cos: Optional[Tensor], rotary_sin: Optional[Tensor],
             rotary_interleaved: bool, k_descale: float, v_descale: float) -> None:
    """kv_store.store_kv_cache: k / v [T, Hk, D] into k_cache / v_cache (in place) by slot_mapping, or by cu_seqlens with
    cache_seqlens and block_table / cache_batch_idx (optionally rotating K).  k_descale / v_descale are read for float8_e4m3fn
    caches only (pass 1.0 otherwise)."""
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    _kv_store.store_kv_cache(k, v, k_cache, v_cache, slot_mapping=slot_mapping, cu_seqlens=cu_seqlens, cache_seqlens=cache_seqlens,
                             block_table=block_table, cache_batch_idx=cache_batch_idx, rotary_cos=rotary_cos,
                             rotary_sin=rotary_sin, rotary_interleaved=rotary_interleaved,
                             k_descale=k_descale if fp8 else None, v_descale=v_descale if fp8 else None)


@kv_store.register_fake
def _(k, v, k_cache, v_cache, slot_mapping, cu_seqlens, cache_seqlens, block_table, cache_batch_idx, rotary_cos, rotary_sin,
      rotary_interleaved, k_descale, v_descale):
    return None


# ------------------------------------------------------------------------------------------
# KV-cache gather and move (flash_attn_mi355.kv_gather; csrc/fa_kv_gather.hip).  Reached as torch.ops.flash_attn_mi355.kv_gather /
# .kv_move; not in __all__
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::kv_gather", mutates_args=(), device_types="cuda")
def kv_gather(k_cache: Tensor, v_cache: Tensor, slot_mapping: Optional[Tensor], cu_seqlens: Optional[Tensor],
              seq_offsets: Optional[Tensor], block_table: Optional[Tensor], cache_batch_idx: Optional[Tensor],
              total_rows: int, dtype: torch.dtype, k_descale: float, v_descale: float) -> Tuple[Tensor, Tensor]:
    """kv_gather.gather_kv_cache: (k, v) [total_rows, Hk, D] of `dtype`, fresh contiguous tensors, read out of k_cache / v_cache by
    slot_mapping, or by cu_seqlens with seq_offsets and block_table / cache_batch_idx.  `dtype` is the cache's for a 16-bit cache;
    k_descale / v_descale are read for float8_e4m3fn caches only (pass 1.0 otherwise)."""
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    return _kv_gather.gather_kv_cache(k_cache, v_cache, slot_mapping=slot_mapping, cu_seqlens=cu_seqlens, seq_offsets=seq_offsets,
                                      block_table=block_table, cache_batch_idx=cache_batch_idx, total_rows=total_rows, dtype=dtype,
                                      k_descale=k_descale if fp8 else None, v_descale=v_descale if fp8 else None)


@kv_gather.register_fake
def _(k_cache, v_cache, slot_mapping, cu_seqlens, seq_offsets, block_table, cache_batch_idx, total_rows, dtype, k_descale,
      v_descale):
    shape = (total_rows, k_cache.shape[2], k_cache.shape[3])
    return k_cache.new_empty(shape, dtype=dtype), k_cache.new_empty(shape, dtype=dtype)


@torch.library.custom_op(f"{_NS}::kv_move", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def kv_move(k_cache: Tensor, v_cache: Tensor, src_slots: Tensor, dst_slots: Tensor) -> None:
    """kv_gather.move_kv_cache: rows src_slots[r] -> dst_slots[r] inside k_cache / v_cache (gather, then store)"""
    _kv_gather.move_kv_cache(k_cache, v_cache, src_slots, dst_slots)


@kv_move.register_fake
def _(k_cache, v_cache, src_slots, dst_slots):
    return None


# ------------------------------------------------------------------------------------------
# RoPE at per-token positions + KV-cache store, one launch (flash_attn_mi355.rope_store; csrc/fa_rope_store.hip).  Reached as
# torch.ops.flash_attn_mi355.rope_store_; not in __all__
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::rope_store_", mutates_args=("q", "k", "k_cache", "v_cache"), device_types="cuda")
def rope_store_(q: Tensor, k: Tensor, v: Tensor, positions: Tensor, rotary_cos: Tensor, rotary_sin: Tensor, k_cache: Tensor,
                v_cache: Tensor, slot_mapping: Tensor, interleaved: bool, k_descale: float, v_descale: float) -> None:
    """rope_store.rope_and_store_kv in place: q / k [T, H, D] are rotated at positions[T] where they are, the rotated k and v go
    into k_cache / v_cache by slot_mapping[T].  k_descale / v_descale are read for float8_e4m3fn caches only (pass 1.0 otherwise).
    The optional forms (no q, no write-back of k, no caches, out of place) stay with the Python function."""
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    _rope_store.rope_and_store_kv(q, k, v, positions, rotary_cos, rotary_sin, k_cache, v_cache, slot_mapping,
                                  interleaved=interleaved, inplace=True, k_out=True,
                                  k_descale=k_descale if fp8 else None, v_descale=v_descale if fp8 else None)


@rope_store_.register_fake
def _(q, k, v, positions, rotary_cos, rotary_sin, k_cache, v_cache, slot_mapping, interleaved, k_descale, v_descale):
    return None


# ------------------------------------------------------------------------------------------
# QK RMSNorm + RoPE at per-token positions + KV-cache store, one launch (flash_attn_mi355.qk_norm; csrc/fa_qk_norm_rope_store.hip).
# Reached as torch.ops.flash_attn_mi355.qk_norm_rope_store_; not in __all__
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::qk_norm_rope_store_", mutates_args=("q", "k", "k_cache", "v_cache"), device_types="cuda")
def qk_norm_rope_store_(q: Tensor, k: Tensor, v: Tensor, positions: Tensor, rotary_cos: Tensor, rotary_sin: Tensor, k_cache: Tensor,
                        v_cache: Tensor, slot_mapping: Tensor, q_weight: Optional[Tensor], k_weight: Optional[Tensor], eps: float,
                        weight_offset: float, interleaved: bool, k_descale: float, v_descale: float) -> None:
    """qk_norm.qk_norm_rope_and_store_kv in place: every head of q / k [T, H, D] is RMS-normalised with q_weight / k_weight [D]
    (None: not normalised) and rotated at positions[T] where it is, the normalised, rotated k and v go into k_cache / v_cache by
    slot_mapping[T].  k_descale / v_descale are read for float8_e4m3fn caches only (pass 1.0 otherwise).  The optional forms (no q,
    no write-back of k, no caches, no rotation, out of place) stay with the Python function."""
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    _qk_norm.qk_norm_rope_and_store_kv(q, k, v, positions, rotary_cos, rotary_sin, k_cache, v_cache, slot_mapping,
                                       q_weight=q_weight, k_weight=k_weight, eps=eps, weight_offset=weight_offset,
                                       interleaved=interleaved, inplace=True, k_out=True,
                                       k_descale=k_descale if fp8 else None, v_descale=v_descale if fp8 else None)


@qk_norm_rope_store_.register_fake
def _(q, k, v, positions, rotary_cos, rotary_sin, k_cache, v_cache, slot_mapping, q_weight, k_weight, eps, weight_offset, interleaved,
      k_descale, v_descale):
    return None


# ------------------------------------------------------------------------------------------
# QK RMSNorm + RoPE for training: the forward out of place on fa_qk_norm_rope_store's kernel, the backward on fa_qk_norm_rope_bwd
# (flash_attn_mi355.qk_norm; csrc/fa_qk_norm_rope_bwd.hip).  Reached as torch.ops.flash_attn_mi355.qk_norm_rope / .qk_norm_rope_bwd;
# not in __all__
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::qk_norm_rope", mutates_args=(), device_types="cuda")
def qk_norm_rope(q: Optional[Tensor], k: Tensor, positions: Optional[Tensor], rotary_cos: Optional[Tensor],
                 rotary_sin: Optional[Tensor], q_weight: Optional[Tensor], k_weight: Optional[Tensor], eps: float,
                 weight_offset: float, interleaved: bool) -> Tuple[Tensor, Tensor]:
    """qk_norm.qk_norm_rope_and_store_kv(..., inplace=False) without caches: (q_out, k_out), fresh contiguous tensors; q None:
    q_out is an empty (0,) tensor.  Differentiable in q, k, q_weight and k_weight (qk_norm_rope_bwd)."""
    q_out, k_out = _qk_norm.qk_norm_rope_and_store_kv(q, k, None, positions, rotary_cos, rotary_sin, q_weight=q_weight,
                                                      k_weight=k_weight, eps=eps, weight_offset=weight_offset,
                                                      interleaved=interleaved, inplace=False)
    return (k.new_empty((0,)) if q_out is None else q_out), k_out


@qk_norm_rope.register_fake
def _(q, k, positions, rotary_cos, rotary_sin, q_weight, k_weight, eps, weight_offset, interleaved):
    return (k.new_empty((0,)) if q is None else q.new_empty(q.shape)), k.new_empty(k.shape)


@torch.library.custom_op(f"{_NS}::qk_norm_rope_bwd", mutates_args=(), device_types="cuda")
def qk_norm_rope_bwd(dq_out: Optional[Tensor], dk_out: Tensor, q: Optional[Tensor], k: Tensor, positions: Optional[Tensor],
                     rotary_cos: Optional[Tensor], rotary_sin: Optional[Tensor], q_weight: Optional[Tensor],
                     k_weight: Optional[Tensor], eps: float, weight_offset: float, interleaved: bool, need_dq: bool,
                     need_dk: bool, need_dq_weight: bool, need_dk_weight: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """qk_norm.qk_norm_rope_backward out of place: (dq, dk, dq_weight, dk_weight), fresh tensors; an output that is not needed (or
    has no tensor: q None, a weight None) is an empty (0,) tensor and is not computed."""
    dq, dk, dqw, dkw = _qk_norm.qk_norm_rope_backward(dq_out, dk_out, q, k, positions, rotary_cos, rotary_sin, q_weight, k_weight,
                                                      eps, weight_offset, interleaved, need_dq=need_dq, need_dk=need_dk,
                                                      need_dw=need_dq_weight or need_dk_weight)
    none = lambda: k.new_empty((0,))                            # noqa: E731
    return (none() if dq is None else dq, none() if dk is None else dk,
            none() if (dqw is None or not need_dq_weight) else dqw, none() if (dkw is None or not need_dk_weight) else dkw)


@qk_norm_rope_bwd.register_fake
def _(dq_out, dk_out, q, k, positions, rotary_cos, rotary_sin, q_weight, k_weight, eps, weight_offset, interleaved, need_dq,
      need_dk, need_dq_weight, need_dk_weight):
    none = lambda: k.new_empty((0,))                            # noqa: E731
    return (q.new_empty(q.shape) if (need_dq and q is not None) else none(),
            k.new_empty(k.shape) if need_dk else none(),
            q_weight.new_empty(q_weight.shape) if (need_dq_weight and q_weight is not None) else none(),
            k_weight.new_empty(k_weight.shape) if (need_dk_weight and k_weight is not None) else none())


def _qk_norm_rope_setup(ctx, inputs, output):
    (q, k, positions, rotary_cos, rotary_sin, q_weight, k_weight, eps, weight_offset, interleaved) = inputs
    ctx.save_for_backward(q, k, positions, rotary_cos, rotary_sin, q_weight, k_weight)
    ctx.args = (eps, weight_offset, interleaved)


def _qk_norm_rope_backward(ctx, dq_out, dk_out):
    q, k, positions, rotary_cos, rotary_sin, q_weight, k_weight = ctx.saved_tensors
    eps, weight_offset, interleaved = ctx.args
    need = ctx.needs_input_grad                 # (q, k, positions, cos, sin, q_weight, k_weight, ...)
    dq, dk, dqw, dkw = qk_norm_rope_bwd(None if q is None else dq_out, dk_out, q, k, positions, rotary_cos, rotary_sin, q_weight,
                                        k_weight, eps, weight_offset, interleaved, need[0] and q is not None, need[1],
                                        need[5] and q_weight is not None, need[6] and k_weight is not None)
    pick = lambda g, on: g if on else None                      # noqa: E731
    return (pick(dq, need[0] and q is not None), pick(dk, need[1]), None, None, None,
            pick(dqw, need[5] and q_weight is not None), pick(dkw, need[6] and k_weight is not None), None, None, None)


qk_norm_rope.register_autograd(_qk_norm_rope_backward, setup_context=_qk_norm_rope_setup)


# ------------------------------------------------------------------------------------------
# residual add + RMSNorm / LayerNorm over the hidden size (flash_attn_mi355.add_norm; csrc/fa_add_norm.hip, fa_add_norm_bwd.hip).
# Reached as torch.ops.flash_attn_mi355.add_norm / .add_norm_ / .add_norm_bwd; not in __all__
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::add_norm", mutates_args=(), device_types="cuda")
def add_norm(x: Tensor, weight: Tensor, bias: Optional[Tensor], residual: Optional[Tensor], eps: float, weight_offset: float,
             is_rms_norm: bool, prenorm: bool, residual_in_fp32: bool) -> Tuple[Tensor, Tensor]:
    """add_norm.add_norm_forward out of place: (out, residual_out), fresh contiguous tensors; without a residual and without
    prenorm residual_out is an empty (0,) tensor.  Differentiable in x, weight, bias and residual (add_norm_bwd)."""
    out, ro = _add_norm.add_norm_forward(x, weight, bias, residual, eps=eps, weight_offset=weight_offset, is_rms_norm=is_rms_norm,
                                         prenorm=prenorm, residual_in_fp32=residual_in_fp32, inplace=False)
    return out, (x.new_empty((0,)) if ro is None else ro)


@add_norm.register_fake
def _(x, weight, bias, residual, eps, weight_offset, is_rms_norm, prenorm, residual_in_fp32):
    if residual is None and not prenorm:
        return x.new_empty(x.shape), x.new_empty((0,))
    ro_dtype = _add_norm.residual_out_dtype(x.dtype, None if residual is None else residual.dtype, residual_in_fp32)
    return x.new_empty(x.shape), x.new_empty(x.shape, dtype=ro_dtype)


@torch.library.custom_op(f"{_NS}::add_norm_", mutates_args=("x", "residual"), device_types="cuda")
def add_norm_(x: Tensor, residual: Optional[Tensor], weight: Tensor, bias: Optional[Tensor], eps: float, weight_offset: float,
              is_rms_norm: bool) -> None:
    """in place: residual <- x + residual (one rounding to residual's dtype), x <- norm(residual); without a residual x <- norm(x)"""
    _add_norm.add_norm_forward(x, weight, bias, residual, eps=eps, weight_offset=weight_offset, is_rms_norm=is_rms_norm,
                               inplace=True)


@add_norm_.register_fake
def _(x, residual, weight, bias, eps, weight_offset, is_rms_norm):
    return None


@torch.library.custom_op(f"{_NS}::add_norm_bwd", mutates_args=(), device_types="cuda")
def add_norm_bwd(dy: Tensor, z: Tensor, dres_out: Optional[Tensor], weight: Tensor, eps: float, weight_offset: float,
                 is_rms_norm: bool, dres_fp32: bool, need_dx: bool, need_dres: bool, need_dweight: bool,
                 need_dbias: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """add_norm.add_norm_backward out of place: (dx, dres, dweight, dbias), fresh tensors; an output that is not needed is an
    empty (0,) tensor and is not computed.  dres has dy's dtype, or float32 with dres_fp32."""
    dx, dres, dw, db = _add_norm.add_norm_backward(dy, z, weight, dres_out, eps=eps, weight_offset=weight_offset,
                                                   is_rms_norm=is_rms_norm, dres_dtype=torch.float32 if dres_fp32 else dy.dtype,
                                                   need_dx=need_dx, need_dres=need_dres, need_dw=need_dweight, need_db=need_dbias)
    none = lambda: dy.new_empty((0,))                           # noqa: E731
    return tuple(none() if t is None else t for t in (dx, dres, dw, db))


@add_norm_bwd.register_fake
def _(dy, z, dres_out, weight, eps, weight_offset, is_rms_norm, dres_fp32, need_dx, need_dres, need_dweight, need_dbias):
    none = lambda: dy.new_empty((0,))                           # noqa: E731
    return (dy.new_empty(dy.shape) if need_dx else none(),
            dy.new_empty(dy.shape, dtype=torch.float32 if dres_fp32 else dy.dtype) if need_dres else none(),
            weight.new_empty(weight.shape) if need_dweight else none(),
            weight.new_empty(weight.shape) if need_dbias else none())


def _add_norm_setup(ctx, inputs, output):
    (x, weight, bias, residual, eps, weight_offset, is_rms_norm, prenorm, residual_in_fp32) = inputs
    ctx.set_materialize_grads(False)
    # z: what the norm read - residual_out where there is one (without a residual it is the prenorm copy of x), else x itself
    has_ro = residual is not None or prenorm
    ctx.save_for_backward(output[1] if has_ro else x, weight)
    ctx.args = (eps, weight_offset, is_rms_norm)
    ctx.res_dtype = None if residual is None else residual.dtype
    ctx.io_dtype = x.dtype
    ctx.has_bias = bias is not None
    ctx.has_ro = has_ro


def _add_norm_backward(ctx, dout, dres_out):
    z, weight = ctx.saved_tensors
    eps, weight_offset, is_rms_norm = ctx.args
    need = ctx.needs_input_grad                 # (x, weight, bias, residual, ...)
    need_x, need_w, need_b = need[0], need[1], need[2] and ctx.has_bias
    need_r = need[3] and ctx.res_dtype is not None
    if dout is None:                            # (only residual_out was used: the norm contributes nothing)
        dout = torch.zeros(z.shape, dtype=ctx.io_dtype, device=z.device)
    if not ctx.has_ro:
        dres_out = None
    same = need_x and need_r and ctx.res_dtype == dout.dtype    # dx and dres hold the same bits: one tensor for both
    dx, dres, dw, db = add_norm_bwd(dout, z, dres_out, weight, eps, weight_offset, is_rms_norm, ctx.res_dtype == torch.float32,
                                    need_x, need_r and not same, need_w, need_b)
    pick = lambda g, on: g if on else None                      # noqa: E731
    return (pick(dx, need_x), pick(dw, need_w), pick(db, need_b), pick(dx if same else dres, need_r), None, None, None, None, None)


add_norm.register_autograd(_add_norm_backward, setup_context=_add_norm_setup)


# ------------------------------------------------------------------------------------------
# softmax cross-entropy over the vocabulary (flash_attn_mi355.cross_entropy; csrc/fa_cross_entropy.hip).
# Reached as torch.ops.flash_attn_mi355.cross_entropy / .cross_entropy_bwd / .cross_entropy_bwd_; not in __all__
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::cross_entropy", mutates_args=(), device_types="cuda")
def cross_entropy(logits: Tensor, labels: Tensor, label_smoothing: float, logit_scale: float, lse_square_scale: float,
                  ignore_index: int, inplace_backward: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """cross_entropy.cross_entropy_forward: (losses, z_losses, lse), fp32 of labels' shape.  Differentiable in logits through
    losses (cross_entropy_bwd; with inplace_backward cross_entropy_bwd_, which overwrites the logits with their gradient)."""
    losses, z_losses, lse = _ce.cross_entropy_forward(logits, labels, label_smoothing=label_smoothing, logit_scale=logit_scale,
                                                      lse_square_scale=lse_square_scale, ignore_index=ignore_index)
    return losses, z_losses, lse


@cross_entropy.register_fake
def _(logits, labels, label_smoothing, logit_scale, lse_square_scale, ignore_index, inplace_backward):
    new = lambda: logits.new_empty(labels.shape, dtype=torch.float32)   # noqa: E731
    return new(), new(), new()


@torch.library.custom_op(f"{_NS}::cross_entropy_bwd", mutates_args=(), device_types="cuda")
def cross_entropy_bwd(dlosses: Tensor, logits: Tensor, labels: Tensor, lse: Tensor, label_smoothing: float, logit_scale: float,
                      lse_square_scale: float, ignore_index: int) -> Tensor:
    """cross_entropy.cross_entropy_backward out of place: dlogits, a fresh contiguous tensor of logits' dtype and shape"""
    return _ce.cross_entropy_backward(dlosses, logits, labels, lse, label_smoothing=label_smoothing, logit_scale=logit_scale,
                                      lse_square_scale=lse_square_scale, ignore_index=ignore_index, inplace=False)


@cross_entropy_bwd.register_fake
def _(dlosses, logits, labels, lse, label_smoothing, logit_scale, lse_square_scale, ignore_index):
    return logits.new_empty(logits.shape)


@torch.library.custom_op(f"{_NS}::cross_entropy_bwd_", mutates_args=("logits",), device_types="cuda")
def cross_entropy_bwd_(dlosses: Tensor, logits: Tensor, labels: Tensor, lse: Tensor, label_smoothing: float, logit_scale: float,
                       lse_square_scale: float, ignore_index: int) -> None:
    """in place: logits <- dlogits; nothing is allocated"""
    _ce.cross_entropy_backward(dlosses, logits, labels, lse, label_smoothing=label_smoothing, logit_scale=logit_scale,
                               lse_square_scale=lse_square_scale, ignore_index=ignore_index, inplace=True)


@cross_entropy_bwd_.register_fake
def _(dlosses, logits, labels, lse, label_smoothing, logit_scale, lse_square_scale, ignore_index):
    return None


def _cross_entropy_setup(ctx, inputs, output):
    logits, labels, label_smoothing, logit_scale, lse_square_scale, ignore_index, inplace_backward = inputs
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(output[1], output[2])          # z_losses, lse
    ctx.save_for_backward(logits, labels, output[2])
    ctx.args = (label_smoothing, logit_scale, lse_square_scale, ignore_index)
    ctx.inplace = inplace_backward


def _cross_entropy_backward(ctx, dlosses, dz_losses, dlse):
    # (z_losses and lse are not differentiable: what arrives for them is dropped, as upstream marks them)
    none = (None,) * 6
    if dlosses is None or not ctx.needs_input_grad[0]:
        return (None,) + none
    logits, labels, lse = ctx.saved_tensors
    if dlosses.dtype != torch.float32:
        dlosses = dlosses.float()
    if ctx.inplace:
        cross_entropy_bwd_(dlosses, logits, labels, lse, *ctx.args)
        return (logits,) + none
    return (cross_entropy_bwd(dlosses, logits, labels, lse, *ctx.args),) + none


cross_entropy.register_autograd(_cross_entropy_backward, setup_context=_cross_entropy_setup)


# ------------------------------------------------------------------------------------------
# token sampling from logits (flash_attn_mi355.sample; csrc/fa_sample.hip).  Each of the four parameters is an optional
# [rows] tensor plus the number that holds where the tensor is None.
# Reached as torch.ops.flash_attn_mi355.sample / .sample_filter; not in __all__
# ------------------------------------------------------------------------------------------
def _sample_params(temperature, temperature_value, top_k, top_k_value, top_p, top_p_value, min_p, min_p_value):
    return dict(temperature=temperature_value if temperature is None else temperature,
                top_k=top_k_value if top_k is None else top_k,
                top_p=top_p_value if top_p is None else top_p,
                min_p=min_p_value if min_p is None else min_p)


@torch.library.custom_op(f"{_NS}::sample", mutates_args=(), device_types="cuda")
def sample(logits: Tensor, u: Tensor, temperature: Optional[Tensor], temperature_value: float, top_k: Optional[Tensor],
           top_k_value: int, top_p: Optional[Tensor], top_p_value: float, min_p: Optional[Tensor],
           min_p_value: float) -> Tuple[Tensor, Tensor, Tensor]:
    """sample.sample_forward: (ids int32, n_kept int32, lse fp32) of shape logits.shape[:-1] from one uniform number per row"""
    return _sample.sample_forward(logits, u, **_sample_params(temperature, temperature_value, top_k, top_k_value, top_p,
                                                              top_p_value, min_p, min_p_value))


@sample.register_fake
def _(logits, u, temperature, temperature_value, top_k, top_k_value, top_p, top_p_value, min_p, min_p_value):
    lead = logits.shape[:-1]
    return (logits.new_empty(lead, dtype=torch.int32), logits.new_empty(lead, dtype=torch.int32),
            logits.new_empty(lead, dtype=torch.float32))


@torch.library.custom_op(f"{_NS}::sample_filter", mutates_args=(), device_types="cuda")
def sample_filter(logits: Tensor, temperature: Optional[Tensor], temperature_value: float, top_k: Optional[Tensor],
                  top_k_value: int, top_p: Optional[Tensor], top_p_value: float, min_p: Optional[Tensor],
                  min_p_value: float) -> Tensor:
    """sample.filter_forward: the logits with everything outside the kept set at -inf, a fresh contiguous tensor"""
    return _sample.filter_forward(logits, **_sample_params(temperature, temperature_value, top_k, top_k_value, top_p, top_p_value,
                                                           min_p, min_p_value))


@sample_filter.register_fake
def _(logits, temperature, temperature_value, top_k, top_k_value, top_p, top_p_value, min_p, min_p_value):
    return logits.new_empty(logits.shape)


# ------------------------------------------------------------------------------------------
# speculative-decoding verification (flash_attn_mi355.spec_decode; csrc/fa_spec_verify.hip).  The temperature is an optional
# [B] tensor plus the number that holds where the tensor is None.
# Reached as torch.ops.flash_attn_mi355.spec_accept / .spec_walk / .spec_verify; not in __all__
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::spec_accept", mutates_args=(), device_types="cuda")
def spec_accept(target_logits: Tensor, draft_probs: Tensor, draft_ids: Tensor, u_accept: Tensor, u_recover: Tensor,
                parents: Optional[Tensor], temperature: Optional[Tensor], temperature_value: float) -> Tuple[Tensor, Tensor]:
    """spec_decode.accept_forward: (accept int32 [B, T], recovered int32 [B, T])"""
    return _spec.accept_forward(target_logits, draft_probs, draft_ids, u_accept, u_recover, parents=parents,
                                temperature=temperature_value if temperature is None else temperature)


@spec_accept.register_fake
def _(target_logits, draft_probs, draft_ids, u_accept, u_recover, parents, temperature, temperature_value):
    shape = draft_ids.shape
    return draft_ids.new_empty(shape, dtype=torch.int32), draft_ids.new_empty(shape, dtype=torch.int32)


def _spec_walk_fake(draft_ids):
    B, T = draft_ids.shape
    return (draft_ids.new_empty((B, T), dtype=torch.int32), draft_ids.new_empty((B,), dtype=torch.int32),
            draft_ids.new_empty((B, T), dtype=torch.int32))


@torch.library.custom_op(f"{_NS}::spec_walk", mutates_args=(), device_types="cuda")
def spec_walk(draft_ids: Tensor, target_ids: Tensor, parents: Optional[Tensor], accept: Optional[Tensor],
              recovered: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """spec_decode.walk: (out_tokens int32 [B, T], num_out int32 [B], path_nodes int32 [B, T])"""
    return _spec.walk(draft_ids, target_ids, parents=parents, accept=accept, recovered=recovered)


@spec_walk.register_fake
def _(draft_ids, target_ids, parents, accept, recovered):
    return _spec_walk_fake(draft_ids)


@torch.library.custom_op(f"{_NS}::spec_verify", mutates_args=(), device_types="cuda")
def spec_verify(target_logits: Tensor, draft_ids: Tensor, draft_probs: Optional[Tensor], parents: Optional[Tensor],
                temperature: Optional[Tensor], temperature_value: float, u_sample: Tensor, u_accept: Optional[Tensor],
                u_recover: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """spec_decode.verify_forward: (out_tokens, num_out, path_nodes) of a whole verification step"""
    return _spec.verify_forward(target_logits, draft_ids, draft_probs, parents,
                                temperature_value if temperature is None else temperature, u_sample, u_accept, u_recover)


@spec_verify.register_fake
def _(target_logits, draft_ids, draft_probs, parents, temperature, temperature_value, u_sample, u_accept, u_recover):
    return _spec_walk_fake(draft_ids)


# ------------------------------------------------------------------------------------------
# the gated activation of the MLP, act(gate) * up (flash_attn_mi355.act_mul; csrc/fa_act_mul.hip).
# Reached as torch.ops.flash_attn_mi355.act_mul / .act_and_mul / .act_mul_bwd / .act_and_mul_bwd / .act_mul_bwd_; not in __all__.
# `activation` is the name ("silu", "gelu", "gelu_tanh", "relu", "relu2").  A torch.library return cannot be optional: the
# ungated form (up None) has no dup, and act_mul_bwd returns an EMPTY tensor of shape (0,) in its place.
# ------------------------------------------------------------------------------------------
@torch.library.custom_op(f"{_NS}::act_mul", mutates_args=(), device_types="cuda")
def act_mul(gate: Tensor, up: Optional[Tensor], activation: str, inplace_backward: bool) -> Tensor:
    """act_mul.act_mul_forward: act(gate) * up (up None: act(gate)), a fresh contiguous tensor.  Differentiable in gate and up
    (act_mul_bwd; with inplace_backward act_mul_bwd_, which overwrites gate and up with their gradients)."""
    return _act_mul.act_mul_forward(gate, up, activation=activation)


@act_mul.register_fake
def _(gate, up, activation, inplace_backward):
    return gate.new_empty(gate.shape)


@torch.library.custom_op(f"{_NS}::act_and_mul", mutates_args=(), device_types="cuda")
def act_and_mul(x: Tensor, activation: str, inplace_backward: bool) -> Tensor:
    """act(x[..., :N]) * x[..., N:] of a packed [..., 2N]: a fresh contiguous [..., N].  Differentiable in x (act_and_mul_bwd: ONE
    packed gradient; with inplace_backward act_mul_bwd_ on the halves of x)."""
    gate, up = _act_mul._halves(x)
    return _act_mul.act_mul_forward(gate, up, activation=activation)


@act_and_mul.register_fake
def _(x, activation, inplace_backward):
    return x.new_empty(tuple(x.shape[:-1]) + (x.shape[-1] // 2,))


@torch.library.custom_op(f"{_NS}::act_mul_bwd", mutates_args=(), device_types="cuda")
def act_mul_bwd(dout: Tensor, gate: Tensor, up: Optional[Tensor], activation: str) -> Tuple[Tensor, Tensor]:
    """act_mul.act_mul_backward out of place: (dgate, dup), fresh contiguous tensors of gate's shape; up None: dup is an empty
    tensor of shape (0,)"""
    dgate, dup = _act_mul.act_mul_backward(dout, gate, up, activation=activation)
    return dgate, (gate.new_empty((0,)) if dup is None else dup)


@act_mul_bwd.register_fake
def _(dout, gate, up, activation):
    return gate.new_empty(gate.shape), gate.new_empty((0,) if up is None else gate.shape)


@torch.library.custom_op(f"{_NS}::act_and_mul_bwd", mutates_args=(), device_types="cuda")
def act_and_mul_bwd(dout: Tensor, x: Tensor, activation: str) -> Tensor:
    """the gradient of a packed [..., 2N] x: ONE fresh contiguous [..., 2N], both halves written by one launch"""
    gate, up = _act_mul._halves(x)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _act_mul.act_mul_backward(dout, gate, up, activation=activation, out=_act_mul._halves(dx))
    return dx


@act_and_mul_bwd.register_fake
def _(dout, x, activation):
    return x.new_empty(x.shape)


@torch.library.custom_op(f"{_NS}::act_mul_bwd_", mutates_args=("gate", "up"), device_types="cuda")
def act_mul_bwd_(dout: Tensor, gate: Tensor, up: Optional[Tensor], activation: str) -> None:
    """in place: gate <- dgate, up <- dup; nothing is allocated"""
    _act_mul.act_mul_backward(dout, gate, up, activation=activation, inplace=True)


@act_mul_bwd_.register_fake
def _(dout, gate, up, activation):
    return None


def _act_mul_setup(ctx, inputs, output):
    gate, up, activation, inplace_backward = inputs
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(gate, up)
    ctx.activation, ctx.inplace = activation, inplace_backward


def _act_mul_backward(ctx, dout):
    if dout is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
        return None, None, None, None
    gate, up = ctx.saved_tensors
    if ctx.inplace:
        act_mul_bwd_(dout, gate, up, ctx.activation)
        return gate, up, None, None
    dgate, dup = act_mul_bwd(dout, gate, up, ctx.activation)
    return dgate, (None if up is None else dup), None, None


act_mul.register_autograd(_act_mul_backward, setup_context=_act_mul_setup)


def _act_and_mul_setup(ctx, inputs, output):
    x, activation, inplace_backward = inputs
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(x)
    ctx.activation, ctx.inplace = activation, inplace_backward


def _act_and_mul_backward(ctx, dout):
    if dout is None or not ctx.needs_input_grad[0]:
        return None, None, None
    (x,) = ctx.saved_tensors
    if ctx.inplace:
        gate, up = _act_mul._halves(x)
        act_mul_bwd_(dout, gate, up, ctx.activation)
        return x, None, None
    return act_and_mul_bwd(dout, x, ctx.activation), None, None


act_and_mul.register_autograd(_act_and_mul_backward, setup_context=_act_and_mul_setup)


__all__ = ["fwd", "bwd", "varlen_fwd", "varlen_bwd", "fwd_kvcache", "fwd_kvcache_tree", "fwd_out", "varlen_fwd_out", "bwd_out",
           "merge_states", "rotary", "rotary_", "kv_store"]


# ------------------------------------------------------------------------------------------
# dynamic fp8-e4m3 quantisation, alone and behind the forwards of add_norm and act_mul (flash_attn_mi355.quant; csrc/fa_quant.hip).
# Reached as torch.ops.flash_attn_mi355.quant_fp8 / .add_norm_quant / .act_mul_quant / .act_and_mul_quant; not in __all__.
# `mode` is the name ("row", "group", "static"); scale goes with "static", scale_ub with the other two.  Functional, not
# differentiable: an input that requires grad raises by name.  A torch.library return cannot be optional: the static mode has no
# scales and add_norm_quant without residual / prenorm no residual_out - an EMPTY tensor of shape (0,) stands in their place.
# ------------------------------------------------------------------------------------------
def _scales_shape(x, mode):
    lead = tuple(x.shape[:-1])
    return (0,) if mode == "static" else (lead + (x.shape[-1] // _quant.GROUP,) if mode == "group" else lead)


def _fake_codes_scales(x, mode, last=None):
    shape = tuple(x.shape[:-1]) + (x.shape[-1] if last is None else last,)
    like = x.new_empty(shape, dtype=torch.float8_e4m3fn)
    return like, x.new_empty(_scales_shape(like, mode), dtype=torch.float32)


def _not_differentiable(op, names):
    """(backward, setup_context) of an op without a gradient: an input that requires grad raises by name at the call"""
    def setup(ctx, inputs, output):
        bad = [n for n, need in zip(names, ctx.needs_input_grad) if need]
        if bad:
            raise RuntimeError(f"{op}: {', '.join(bad)} requires grad, and {op} is not differentiable (detach it)")

    def backward(ctx, *grads):
        raise RuntimeError(f"{op} is not differentiable")
    return backward, setup


@torch.library.custom_op(f"{_NS}::quant_fp8", mutates_args=(), device_types="cuda")
def quant_fp8(x: Tensor, mode: str, scale: Optional[float], scale_ub: Optional[float]) -> Tuple[Tensor, Tensor]:
    """quant.quant_fp8: (codes, scales), fresh contiguous tensors; mode 'static': scales is an empty tensor of shape (0,)"""
    codes, scales = _quant.quant_fp8(x, mode=mode, scale=scale, scale_ub=scale_ub)
    return codes, (x.new_empty((0,), dtype=torch.float32) if scales is None else scales)


@quant_fp8.register_fake
def _(x, mode, scale, scale_ub):
    return _fake_codes_scales(x, mode)


@torch.library.custom_op(f"{_NS}::add_norm_quant", mutates_args=(), device_types="cuda")
def add_norm_quant(x: Tensor, residual: Optional[Tensor], weight: Tensor, bias: Optional[Tensor], eps: float, weight_offset: float,
                   is_rms_norm: bool, prenorm: bool, residual_in_fp32: bool, mode: str, scale: Optional[float],
                   scale_ub: Optional[float]) -> Tuple[Tensor, Tensor, Tensor]:
    """quant.add_norm_quant out of place: (codes, scales, residual_out); scales (mode 'static') and residual_out (no residual, no
    prenorm) are empty tensors of shape (0,) where there is none"""
    codes, scales, ro = _quant.add_norm_quant(x, residual, weight, bias, eps=eps, weight_offset=weight_offset, is_rms_norm=is_rms_norm,
                                              prenorm=prenorm, residual_in_fp32=residual_in_fp32, mode=mode, scale=scale,
                                              scale_ub=scale_ub)
    return (codes, x.new_empty((0,), dtype=torch.float32) if scales is None else scales,
            x.new_empty((0,)) if ro is None else ro)


@add_norm_quant.register_fake
def _(x, residual, weight, bias, eps, weight_offset, is_rms_norm, prenorm, residual_in_fp32, mode, scale, scale_ub):
    codes, scales = _fake_codes_scales(x, mode)
    if residual is None and not prenorm:
        return codes, scales, x.new_empty((0,))
    ro_dtype = _add_norm.residual_out_dtype(x.dtype, None if residual is None else residual.dtype, residual_in_fp32)
    return codes, scales, x.new_empty(x.shape, dtype=ro_dtype)


@torch.library.custom_op(f"{_NS}::act_mul_quant", mutates_args=(), device_types="cuda")
def act_mul_quant(gate: Tensor, up: Optional[Tensor], activation: str, mode: str, scale: Optional[float],
                  scale_ub: Optional[float]) -> Tuple[Tensor, Tensor]:
    """quant.act_mul_quant: (codes, scales) of act(gate) * up (up None: act(gate)); mode 'static': scales is empty, shape (0,)"""
    codes, scales = _quant.act_mul_quant(gate, up, activation=activation, mode=mode, scale=scale, scale_ub=scale_ub)
    return codes, (gate.new_empty((0,), dtype=torch.float32) if scales is None else scales)


@act_mul_quant.register_fake
def _(gate, up, activation, mode, scale, scale_ub):
    return _fake_codes_scales(gate, mode)


@torch.library.custom_op(f"{_NS}::act_and_mul_quant", mutates_args=(), device_types="cuda")
def act_and_mul_quant(x: Tensor, activation: str, mode: str, scale: Optional[float], scale_ub: Optional[float]) -> Tuple[Tensor, Tensor]:
    """quant.act_and_mul_quant on a packed [..., 2N]: (codes [..., N], scales)"""
    codes, scales = _quant.act_and_mul_quant(x, activation=activation, mode=mode, scale=scale, scale_ub=scale_ub)
    return codes, (x.new_empty((0,), dtype=torch.float32) if scales is None else scales)


@act_and_mul_quant.register_fake
def _(x, activation, mode, scale, scale_ub):
    return _fake_codes_scales(x, mode, last=x.shape[-1] // 2)


for _op, _names in ((quant_fp8, ("x",)), (add_norm_quant, ("x", "residual", "weight", "bias")), (act_mul_quant, ("gate", "up")),
                    (act_and_mul_quant, ("x",))):
    _bwd, _setup = _not_differentiable(_op._opoverload._schema.name.split("::")[-1], _names)
    _op.register_autograd(_bwd, setup_context=_setup)
del _op, _names, _bwd, _setup


# ------------------------------------------------------------------------------------------
# what surrounds the expert GEMMs of a mixture-of-experts block (flash_attn_mi355.moe; csrc/fa_moe.hip).
# Reached as torch.ops.flash_attn_mi355.moe_route / .moe_route_bwd / .moe_sort / .moe_permute / .moe_combine / .moe_combine_bwd;
# not in __all__.  All functional; every output shape is known on the host (M_max = T K + E (align - 1)), so every op has a fake
# implementation and is capturable.  A torch.library return cannot be optional: moe_combine_bwd returns an EMPTY tensor of shape
# (0,) in the place of a gradient that was not asked for.
# ------------------------------------------------------------------------------------------
from . import moe as _moe  # noqa: E402


@torch.library.custom_op(f"{_NS}::moe_route", mutates_args=(), device_types="cuda")
def moe_route(logits: Tensor, k: int, scoring: str, renormalize: bool, bias: Optional[Tensor], scale: float) -> Tuple[Tensor, Tensor]:
    """moe.moe_route_forward: (weights fp32 [T, k], ids int32 [T, k]).  The weights are differentiable in the logits
    (moe_route_bwd); ids is not differentiable."""
    return _moe.moe_route_forward(logits, k, scoring=scoring, renormalize=renormalize, bias=bias, scale=scale)


@moe_route.register_fake
def _(logits, k, scoring, renormalize, bias, scale):
    return (logits.new_empty((logits.shape[0], k), dtype=torch.float32), logits.new_empty((logits.shape[0], k), dtype=torch.int32))


@torch.library.custom_op(f"{_NS}::moe_route_bwd", mutates_args=(), device_types="cuda")
def moe_route_bwd(dweights: Tensor, logits: Tensor, ids: Tensor, scoring: str, renormalize: bool, bias: Optional[Tensor],
                  scale: float) -> Tensor:
    """moe.moe_route_backward: dlogits, a fresh contiguous tensor of the logits' dtype and shape, every element written"""
    return _moe.moe_route_backward(dweights, logits, ids, scoring=scoring, renormalize=renormalize, bias=bias, scale=scale)


@moe_route_bwd.register_fake
def _(dweights, logits, ids, scoring, renormalize, bias, scale):
    return logits.new_empty(logits.shape)


def _moe_route_setup(ctx, inputs, output):
    logits, k, scoring, renormalize, bias, scale = inputs
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(output[1])                      # ids
    ctx.save_for_backward(logits, output[1], bias)
    ctx.args = (scoring, renormalize, scale)


def _moe_route_backward(ctx, dweights, dids):
    none = (None,) * 5
    if dweights is None or not ctx.needs_input_grad[0]:
        return (None,) + none
    logits, ids, bias = ctx.saved_tensors
    scoring, renormalize, scale = ctx.args
    return (moe_route_bwd(dweights.contiguous(), logits, ids, scoring, renormalize, bias, scale),) + none


moe_route.register_autograd(_moe_route_backward, setup_context=_moe_route_setup)


@torch.library.custom_op(f"{_NS}::moe_sort", mutates_args=(), device_types="cuda")
def moe_sort(ids: Tensor, num_experts: int, align: int) -> Tuple[Tensor, Tensor, Tensor]:
    """moe.moe_sort: (sorted_slot int32 [T k + E (align - 1)], pos int32 [T, k], expert_offsets int32 [E + 1])"""
    return _moe.moe_sort(ids, num_experts, align=align)


@moe_sort.register_fake
def _(ids, num_experts, align):
    T, K = ids.shape
    return (ids.new_empty((_moe.sort_max_rows(T, K, num_experts, align),)), ids.new_empty((T, K)), ids.new_empty((num_experts + 1,)))


@torch.library.custom_op(f"{_NS}::moe_permute", mutates_args=(), device_types="cuda")
def moe_permute(x: Tensor, sorted_slot: Tensor, k: int, scale: Optional[Tensor], pos: Optional[Tensor]) -> Tensor:
    """moe.moe_permute_forward: xp [M_max, N], a fresh contiguous tensor.  Differentiable in x (moe_combine over pos, with the
    scale - or ones - as weights); pos is only read by the backward."""
    return _moe.moe_permute_forward(x, sorted_slot, k, scale=scale)


@moe_permute.register_fake
def _(x, sorted_slot, k, scale, pos):
    return x.new_empty((sorted_slot.shape[0], x.shape[1]))


def _moe_permute_setup(ctx, inputs, output):
    x, sorted_slot, k, scale, pos = inputs
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(sorted_slot, scale, pos)
    ctx.slots = (x.shape[0], k)


def _moe_permute_backward(ctx, dxp):
    if dxp is None or not ctx.needs_input_grad[0]:
        return None, None, None, None, None
    sorted_slot, scale, pos = ctx.saved_tensors
    T, k = ctx.slots
    if pos is None:
        # the inverse of sorted_slot, without a host synchronisation: padding rows (-1) are sent to a spare entry that is cut off
        idx = torch.where(sorted_slot >= 0, sorted_slot, T * k).long()
        rows = torch.arange(sorted_slot.shape[0], dtype=torch.int32, device=sorted_slot.device)
        pos = torch.full((T * k + 1,), -1, dtype=torch.int32, device=sorted_slot.device).scatter_(0, idx, rows)[:T * k].view(T, k)
    return moe_combine(dxp, scale, pos), None, None, None, None


moe_permute.register_autograd(_moe_permute_backward, setup_context=_moe_permute_setup)


@torch.library.custom_op(f"{_NS}::moe_combine", mutates_args=(), device_types="cuda")
def moe_combine(y: Tensor, weights: Optional[Tensor], pos: Tensor) -> Tensor:
    """moe.moe_combine_forward: out [T, N], a fresh contiguous tensor; weights None: ones.  Differentiable in y and weights
    (moe_combine_bwd)."""
    return _moe.moe_combine_forward(y, weights, pos)


@moe_combine.register_fake
def _(y, weights, pos):
    return y.new_empty((pos.shape[0], y.shape[1]))


@torch.library.custom_op(f"{_NS}::moe_combine_bwd", mutates_args=(), device_types="cuda")
def moe_combine_bwd(dout: Tensor, y: Tensor, weights: Tensor, pos: Tensor, need_dy: bool, need_dw: bool) -> Tuple[Tensor, Tensor]:
    """moe.moe_combine_backward: (dy [M_max, N], dw fp32 [T, k]); a gradient that is not needed is an empty tensor of shape (0,)"""
    dy, dw = _moe.moe_combine_backward(dout, y, weights, pos, need_dy=need_dy, need_dw=need_dw)
    return (y.new_empty((0,)) if dy is None else dy, y.new_empty((0,), dtype=torch.float32) if dw is None else dw)


@moe_combine_bwd.register_fake
def _(dout, y, weights, pos, need_dy, need_dw):
    return (y.new_empty(y.shape if need_dy else (0,)), y.new_empty(tuple(pos.shape) if need_dw else (0,), dtype=torch.float32))


def _moe_combine_setup(ctx, inputs, output):
    y, weights, pos = inputs
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(y, weights, pos)


def _moe_combine_backward(ctx, dout):
    y, weights, pos = ctx.saved_tensors
    need_dy, need_dw = ctx.needs_input_grad[0], weights is not None and ctx.needs_input_grad[1]
    if dout is None or not (need_dy or need_dw):
        return None, None, None
    if weights is None:                                          # unit weights: dy is the plain permute's scatter form
        weights = torch.ones(pos.shape, dtype=torch.float32, device=pos.device)
    dy, dw = moe_combine_bwd(dout.contiguous(), y, weights, pos, need_dy, need_dw)
    return (dy if need_dy else None), (dw if need_dw else None), None


moe_combine.register_autograd(_moe_combine_backward, setup_context=_moe_combine_setup)


# the grouped expert GEMM between permute and combine (moe.moe_gemm; csrc/fa_moe_gemm.hip): torch.ops.flash_attn_mi355.moe_gemm
@torch.library.custom_op(f"{_NS}::moe_gemm", mutates_args=(), device_types="cuda")
def moe_gemm(x: Tensor, w: Tensor, expert_offsets: Tensor, w_layout: str, bias: Optional[Tensor], sorted_slot: Optional[Tensor],
             top_k: Optional[int]) -> Tensor:
    """moe.moe_gemm: out [M_max, N], a fresh contiguous tensor (M_max = sorted_slot's length, or x's rows).  Functional and
    capturable: expert_offsets is device data and the output shape does not depend on it.  No autograd is registered."""
    return _moe.moe_gemm(x, w, expert_offsets, w_layout=w_layout, bias=bias, sorted_slot=sorted_slot, top_k=top_k)


@moe_gemm.register_fake
def _(x, w, expert_offsets, w_layout, bias, sorted_slot, top_k):
    M = x.shape[0] if sorted_slot is None else sorted_slot.shape[0]
    return x.new_empty((M, w.shape[1] if w_layout == "nk" else w.shape[2]))


# the weight / bias gradient of the grouped expert GEMM (moe.moe_gemm_wgrad; csrc/fa_moe_gemm_wgrad.hip) and the differentiable
# expert layer built on moe_gemm, moe_combine and it (moe.moe_linear): torch.ops.flash_attn_mi355.moe_gemm_wgrad / .moe_linear
@torch.library.custom_op(f"{_NS}::moe_gemm_wgrad", mutates_args=(), device_types="cuda")
def moe_gemm_wgrad(dy: Tensor, x: Tensor, expert_offsets: Tensor, w_layout: str, sorted_slot: Optional[Tensor], top_k: Optional[int],
                   need_dw: bool, need_dbias: bool, dw_fp32: bool, dbias_fp32: bool) -> Tuple[Tensor, Tensor]:
    """moe.moe_gemm_wgrad: (dw [E, N, K] / [E, K, N], dbias [E, N]), fresh contiguous tensors of dy's dtype (fp32 with dw_fp32 /
    dbias_fp32); a gradient that is not needed is an empty tensor of shape (0,)"""
    res = _moe.moe_gemm_wgrad(dy, x, expert_offsets, w_layout=w_layout, sorted_slot=sorted_slot, top_k=top_k,
                              dw_dtype=torch.float32 if dw_fp32 else None, need_dbias=need_dbias,
                              dbias_dtype=torch.float32 if dbias_fp32 else None, need_dw=need_dw)
    dw, dbias = res if need_dbias else (res, None)
    return (dy.new_empty((0,), dtype=torch.float32 if dw_fp32 else dy.dtype) if dw is None else dw,
            dy.new_empty((0,), dtype=torch.float32 if dbias_fp32 else dy.dtype) if dbias is None else dbias)


@moe_gemm_wgrad.register_fake
def _(dy, x, expert_offsets, w_layout, sorted_slot, top_k, need_dw, need_dbias, dw_fp32, dbias_fp32):
    E, N, K = expert_offsets.shape[0] - 1, dy.shape[1], x.shape[1]
    shape = (E, N, K) if w_layout == "nk" else (E, K, N)
    return (dy.new_empty(shape if need_dw else (0,), dtype=torch.float32 if dw_fp32 else dy.dtype),
            dy.new_empty((E, N) if need_dbias else (0,), dtype=torch.float32 if dbias_fp32 else dy.dtype))


@torch.library.custom_op(f"{_NS}::moe_linear", mutates_args=(), device_types="cuda")
def moe_linear(x: Tensor, w: Tensor, expert_offsets: Tensor, w_layout: str, bias: Optional[Tensor], sorted_slot: Optional[Tensor],
               top_k: Optional[int], pos: Optional[Tensor]) -> Tensor:
    """moe.moe_linear: moe_gemm's out, differentiable in x, w and bias (moe_gemm with the other layout, moe_combine over pos,
    moe_gemm_wgrad); pos is only read by the backward."""
    return _moe.moe_gemm(x.detach(), w.detach(), expert_offsets, w_layout=w_layout, bias=None if bias is None else bias.detach(),
                         sorted_slot=sorted_slot, top_k=top_k)


@moe_linear.register_fake
def _(x, w, expert_offsets, w_layout, bias, sorted_slot, top_k, pos):
    M = x.shape[0] if sorted_slot is None else sorted_slot.shape[0]
    return x.new_empty((M, w.shape[1] if w_layout == "nk" else w.shape[2]))


def _moe_linear_setup(ctx, inputs, output):
    x, w, expert_offsets, w_layout, bias, sorted_slot, top_k, pos = inputs
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(x, w, expert_offsets, sorted_slot, pos)
    ctx.args = (w_layout, top_k, None if bias is None else bias.dtype)


def _moe_linear_backward(ctx, dy):
    none = (None,) * 8
    need_dx, need_dw, need_db = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[4]
    if dy is None or not (need_dx or need_dw or need_db):
        return none
    x, w, expert_offsets, sorted_slot, pos = ctx.saved_tensors
    w_layout, top_k, bias_dtype = ctx.args
    if not (dy.stride(1) == 1 and dy.stride(0) % 8 == 0 and dy.stride(0) >= dy.shape[1] and dy.stride(0) <= _moe.GEMM_MAX_ROW_STRIDE
            and dy.storage_offset() % 8 == 0):
        dy = dy.contiguous()
    dx = dw = db = None
    if need_dx:
        dx = moe_gemm(dy, w, expert_offsets, "kn" if w_layout == "nk" else "nk", None, None, None)
        if sorted_slot is not None:
            T = x.shape[0]
            if pos is None:
                # the inverse of sorted_slot, without a host synchronisation (as moe_permute's backward)
                idx = torch.where(sorted_slot >= 0, sorted_slot, T * top_k).long()
                rows = torch.arange(sorted_slot.shape[0], dtype=torch.int32, device=sorted_slot.device)
                pos = torch.full((T * top_k + 1,), -1, dtype=torch.int32, device=sorted_slot.device).scatter_(0, idx, rows)[:T * top_k].view(T, top_k)
            dx = moe_combine(dx, None, pos)
    if need_dw or need_db:
        dw, db = moe_gemm_wgrad(dy, x, expert_offsets, w_layout, sorted_slot, top_k, need_dw, need_db, False,
                                bias_dtype == torch.float32)
    return dx, (dw if need_dw else None), None, None, (db if need_db else None), None, None, None


moe_linear.register_autograd(_moe_linear_backward, setup_context=_moe_linear_setup)
