"""Standalone rotary position embedding on the library's `fa_rotary` kernel (csrc/fa_rotary.hip): what upstream flash_attn ships as
`flash_attn.layers.rotary` - `apply_rotary_emb`, `apply_rotary_emb_qkv_`, `apply_rotary_emb_kv_`, `RotaryEmbedding` - with
upstream's names, argument order and defaults (note `interleaved=False` here; the kv-cache op's own `rotary_interleaved`
defaults to True).

One launch per rotated tensor, forward and backward (the backward is the same kernel with `conjugate`), no temporaries; views
are taken as they are (strides, no copies) and the arithmetic is the kv-cache op's in-kernel RoPE, bit for bit.  A row whose
position falls outside the cos / sin table is left unrotated, as in that op.

Out of scope: xPos scaling (`scale_base`), fp32 / fp8 x, per-token position ids (only a per-sequence offset), and fusing the
rotation into the attention kernels.  Nothing here is exported through the packages' `__all__` lists."""
import ctypes
from typing import Optional, Union

import torch

from . import _lib
from . import flash_attn_interface as _fi


def _check(x, cos, sin, seqlen_offsets, cu_seqlens, max_seqlen, name="x"):
    """every argument error, raised before any device work (the device check comes last, so the others also fire on CPU tensors).
    Returns (batch, seqlen, nheads, head_dim, rotary_dim, seqlen_ro)."""
    if x.dtype not in _fi._DTYPES:
        raise RuntimeError(f"rotary: {name} must be fp16 or bf16, got {x.dtype} (fp32 and fp8 are not supported)")
    if cos.dtype != sin.dtype or cos.dtype not in (x.dtype, torch.float32):
        raise RuntimeError(f"rotary: cos / sin must both have {name}'s dtype ({x.dtype}) or both be fp32, got {cos.dtype} / {sin.dtype}")
    if cos.dim() != 2 or tuple(cos.shape) != tuple(sin.shape):
        raise RuntimeError(f"rotary: cos and sin must have the same shape (seqlen_ro, rotary_dim / 2), got {tuple(cos.shape)} / {tuple(sin.shape)}")
    if cu_seqlens is None:
        if x.dim() != 4:
            raise RuntimeError(f"rotary: {name} must be (batch, seqlen, nheads, headdim), got {tuple(x.shape)}")
        batch, seqlen, nheads, head_dim = x.shape
    else:
        if max_seqlen is None:
            raise RuntimeError("rotary: cu_seqlens needs max_seqlen")
        if x.dim() != 3:
            raise RuntimeError(f"rotary: with cu_seqlens {name} must be (total_seqlen, nheads, headdim), got {tuple(x.shape)}")
        if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1:
            raise RuntimeError("rotary: cu_seqlens must be an int32 tensor of shape (batch + 1,)")
        _, nheads, head_dim = x.shape
        batch, seqlen = cu_seqlens.numel() - 1, int(max_seqlen)
    seqlen_ro, rotary_dim = cos.shape[0], 2 * cos.shape[1]
    if rotary_dim > head_dim:
        raise RuntimeError(f"rotary: rotary_dim must be <= headdim ({rotary_dim} > {head_dim})")
    if rotary_dim == 0:
        raise RuntimeError("rotary: cos / sin are empty (rotary_dim == 0)")
    if x.stride(-1) != 1:
        raise RuntimeError(f"rotary: the last dimension of {name} must be contiguous")
    if isinstance(seqlen_offsets, torch.Tensor):
        if seqlen_offsets.dtype != torch.int32 or tuple(seqlen_offsets.shape) != (batch,):
            raise RuntimeError(f"rotary: seqlen_offsets must be an int or an int32 tensor of shape ({batch},)")
    else:
        if int(seqlen_offsets) < 0:
            raise RuntimeError("rotary: seqlen_offsets must be >= 0")
        if seqlen_ro < seqlen + int(seqlen_offsets):
            raise RuntimeError(f"rotary: seqlen_ro must be >= seqlen + seqlen_offsets ({seqlen_ro} < {seqlen} + {int(seqlen_offsets)})")
    tensors = [x, cos, sin, cu_seqlens, seqlen_offsets if isinstance(seqlen_offsets, torch.Tensor) else None]
    _fi._check_device(*tensors)
    if any(t is not None and t.device != x.device for t in tensors):
        raise RuntimeError(f"rotary: every tensor must be on {name}'s device")
    return batch, seqlen, nheads, head_dim, rotary_dim, seqlen_ro


def _launch(x, out, cos, sin, interleaved, conjugate, seqlen_offsets, cu_seqlens, max_seqlen):
    """fa_rotary on checked arguments: x / out [B, S, H, D] (or [T, H, D] with cu_seqlens) views with a contiguous last
    dimension, out is x (in place) or does not overlap it"""
    batch, seqlen, nheads, head_dim, rotary_dim, seqlen_ro = _check(x, cos, sin, seqlen_offsets, cu_seqlens, max_seqlen)
    if x.numel() == 0:
        return out
    cos, sin = cos.contiguous(), sin.contiguous()
    r = _lib.FaRotaryParams()
    r.struct_size = ctypes.sizeof(_lib.FaRotaryParams)
    r.x, r.out = x.data_ptr(), out.data_ptr()
    if cu_seqlens is None:
        r.x_batch_stride, r.x_row_stride, r.x_head_stride = x.stride(0), x.stride(1), x.stride(2)
        r.o_batch_stride, r.o_row_stride, r.o_head_stride = out.stride(0), out.stride(1), out.stride(2)
    else:
        cu_seqlens = cu_seqlens.contiguous()
        r.x_row_stride, r.x_head_stride = x.stride(0), x.stride(1)
        r.o_row_stride, r.o_head_stride = out.stride(0), out.stride(1)
        r.cu_seqlens, r.total_rows = cu_seqlens.data_ptr(), x.shape[0]
    r.batch, r.seqlen, r.nheads, r.head_dim = batch, seqlen, nheads, head_dim
    r.rotary_dim, r.dtype = rotary_dim, _fi._DTYPES[x.dtype]
    r.cos, r.sin = cos.data_ptr(), sin.data_ptr()
    r.cos_sin_fp32 = 1 if cos.dtype == torch.float32 else 0
    r.seqlen_ro, r.interleaved, r.conjugate = seqlen_ro, 1 if interleaved else 0, 1 if conjugate else 0
    if isinstance(seqlen_offsets, torch.Tensor):
        seqlen_offsets = seqlen_offsets.contiguous()
        r.seqlen_offsets = seqlen_offsets.data_ptr()
    else:
        r.seqlen_offset = int(seqlen_offsets)
    with _fi._on_device(x.device):
        _lib.call_rotary(r, _fi._stream(x.device))           # (queued: cos / sin / offsets stay referenced until here)
    return out


def apply_rotary(x, cos, sin, seqlen_offsets: Union[int, torch.Tensor] = 0, cu_seqlens: Optional[torch.Tensor] = None,
                 max_seqlen: Optional[int] = None, interleaved=False, inplace=False, conjugate=False):
    """the rotation itself, no autograd (upstream's flash_attn.ops.triton.rotary.apply_rotary): returns x when inplace, else a
    fresh tensor"""
    out = x if inplace else torch.empty_like(x)
    if not inplace and (out.stride(-1) != 1 or out.numel() != x.numel()):
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    return _launch(x, out, cos, sin, interleaved, conjugate, seqlen_offsets, cu_seqlens, max_seqlen)


class ApplyRotaryEmb(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin, interleaved=False, inplace=False, seqlen_offsets=0, cu_seqlens=None, max_seqlen=None):
        out = apply_rotary(x, cos, sin, seqlen_offsets=seqlen_offsets, cu_seqlens=cu_seqlens, max_seqlen=max_seqlen,
                           interleaved=interleaved, inplace=inplace)
        if isinstance(seqlen_offsets, int):
            ctx.save_for_backward(cos, sin, cu_seqlens)
            ctx.seqlen_offsets = seqlen_offsets
        else:
            ctx.save_for_backward(cos, sin, cu_seqlens, seqlen_offsets)
            ctx.seqlen_offsets = None
        ctx.interleaved, ctx.inplace, ctx.max_seqlen = interleaved, inplace, max_seqlen
        if inplace:
            ctx.mark_dirty(x)
        return out

    @staticmethod
    def backward(ctx, do):
        seqlen_offsets = ctx.seqlen_offsets
        if seqlen_offsets is None:
            cos, sin, cu_seqlens, seqlen_offsets = ctx.saved_tensors
        else:
            cos, sin, cu_seqlens = ctx.saved_tensors
        if do.stride(-1) != 1:
            do = do.contiguous()
        dx = apply_rotary(do, cos, sin, seqlen_offsets=seqlen_offsets, cu_seqlens=cu_seqlens, max_seqlen=ctx.max_seqlen,
                          interleaved=ctx.interleaved, inplace=ctx.inplace, conjugate=True)
        return dx, None, None, None, None, None, None, None


def apply_rotary_emb(x, cos, sin, interleaved=False, inplace=False, seqlen_offsets: Union[int, torch.Tensor] = 0,
                     cu_seqlens: Optional[torch.Tensor] = None, max_seqlen: Optional[int] = None):
    """x: (batch, seqlen, nheads, headdim) fp16 / bf16, or (total_seqlen, nheads, headdim) with cu_seqlens (int32 (batch + 1,))
    and max_seqlen; a view with a contiguous last dimension is taken as it is.
    cos, sin: (seqlen_ro, rotary_dim / 2) of x's dtype or fp32, rotary_dim <= headdim; the first rotary_dim columns are rotated.
    interleaved: rotate pairs (2t, 2t + 1) (GPT-J) instead of (t, t + rotary_dim / 2) (GPT-NeoX).
    inplace: rotate x itself (and, in the backward, the incoming gradient).
    seqlen_offsets: an int or an int32 (batch,) tensor added to every row index of a sequence (the KV cache's length).  With an
    int, seqlen_ro >= seqlen + seqlen_offsets is required; with a tensor, rows whose position falls outside the table come back
    unrotated.
    Returns a tensor of x's shape.  Differentiable in x (the backward is the inverse rotation on the same kernel)."""
    return ApplyRotaryEmb.apply(x, cos, sin, interleaved, inplace, seqlen_offsets, cu_seqlens, max_seqlen)


apply_rotary_emb_func = apply_rotary_emb


def _qk_views(qkv, num_heads_q):
    """(q, k, qk) views of a packed qkv: qk is q and k as ONE [B, S, Hq + Hk, D] strided view (None where the layout has none)"""
    if qkv.dim() == 5:
        if qkv.shape[2] != 3:
            raise RuntimeError(f"rotary: qkv must be (batch, seqlen, 3, nheads, headdim), got {tuple(qkv.shape)}")
        if num_heads_q is not None:
            raise RuntimeError("rotary: num_heads_q goes with a (batch, seqlen, nheads_q + 2 nheads_k, headdim) qkv")
        B, S, _, H, D = qkv.shape
        q, k = qkv[:, :, 0], qkv[:, :, 1]
        qk = None
        if qkv.stride(2) == H * qkv.stride(3):
            qk = qkv.as_strided((B, S, 2 * H, D), (qkv.stride(0), qkv.stride(1), qkv.stride(3), qkv.stride(4)), qkv.storage_offset())
        return q, k, qk
    if qkv.dim() != 4 or num_heads_q is None:
        raise RuntimeError("rotary: qkv must be (batch, seqlen, 3, nheads, headdim), or (batch, seqlen, nheads_q + 2 nheads_k, "
                           "headdim) with num_heads_q")
    hq = int(num_heads_q)
    if hq <= 0 or (qkv.shape[2] - hq) % 2 != 0 or qkv.shape[2] <= hq:
        raise RuntimeError(f"rotary: {qkv.shape[2]} heads are not num_heads_q = {hq} plus twice a number of kv heads")
    hk = (qkv.shape[2] - hq) // 2
    return qkv[:, :, :hq], qkv[:, :, hq:hq + hk], qkv[:, :, :hq + hk]


def _rotate_qkv_(qkv, cos, sin, cos_k, sin_k, interleaved, seqlen_offsets, num_heads_q, conjugate):
    q, k, qk = _qk_views(qkv, num_heads_q)
    if cos_k is None and sin_k is None and qk is not None:
        _launch(qk, qk, cos, sin, interleaved, conjugate, seqlen_offsets, None, None)     # q and k: one launch
    else:
        cos_k, sin_k = (cos, sin) if cos_k is None else (cos_k, sin_k)
        if sin_k is None:
            raise RuntimeError("rotary: cos_k and sin_k must be given together")
        _check(k, cos_k, sin_k, seqlen_offsets, None, None, "k")                          # (before q is touched)
        _launch(q, q, cos, sin, interleaved, conjugate, seqlen_offsets, None, None)
        _launch(k, k, cos_k, sin_k, interleaved, conjugate, seqlen_offsets, None, None)
    return qkv


class ApplyRotaryEmbQKV_(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, cos_k=None, sin_k=None, interleaved=False, seqlen_offsets=0, num_heads_q=None):
        _rotate_qkv_(qkv, cos, sin, cos_k, sin_k, interleaved, seqlen_offsets, num_heads_q, False)
        if isinstance(seqlen_offsets, int):
            ctx.save_for_backward(cos, sin, cos_k, sin_k)
            ctx.seqlen_offsets = seqlen_offsets
        else:
            ctx.save_for_backward(cos, sin, cos_k, sin_k, seqlen_offsets)
            ctx.seqlen_offsets = None
        ctx.interleaved, ctx.num_heads_q = interleaved, num_heads_q
        ctx.mark_dirty(qkv)
        return qkv

    @staticmethod
    def backward(ctx, dqkv):
        seqlen_offsets = ctx.seqlen_offsets
        if seqlen_offsets is None:
            cos, sin, cos_k, sin_k, seqlen_offsets = ctx.saved_tensors
        else:
            cos, sin, cos_k, sin_k = ctx.saved_tensors
        if dqkv.stride(-1) != 1:
            dqkv = dqkv.contiguous()
        _rotate_qkv_(dqkv, cos, sin, cos_k, sin_k, ctx.interleaved, seqlen_offsets, ctx.num_heads_q, True)
        return dqkv, None, None, None, None, None, None, None


def apply_rotary_emb_qkv_(qkv, cos, sin, cos_k=None, sin_k=None, interleaved=False,
                          seqlen_offsets: Union[int, torch.Tensor] = 0, num_heads_q: Optional[int] = None):
    """qkv: (batch, seqlen, 3, nheads, headdim), or (batch, seqlen, nheads_q + 2 nheads_k, headdim) with num_heads_q (GQA / MQA).
    Rotates q and k IN PLACE - one launch over the heads of q and k as one strided view when cos_k / sin_k are not given, one
    launch each otherwise (k then uses cos_k / sin_k) -; v is never read or written.  Returns qkv."""
    return ApplyRotaryEmbQKV_.apply(qkv, cos, sin, cos_k, sin_k, interleaved, seqlen_offsets, num_heads_q)


class ApplyRotaryEmbKV_(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kv, cos, sin, interleaved=False, seqlen_offsets=0):
        if kv.dim() != 5 or kv.shape[2] != 2:
            raise RuntimeError(f"rotary: kv must be (batch, seqlen, 2, nheads, headdim), got {tuple(kv.shape)}")
        k = kv[:, :, 0]
        _launch(k, k, cos, sin, interleaved, False, seqlen_offsets, None, None)
        if isinstance(seqlen_offsets, int):
            ctx.save_for_backward(cos, sin)
            ctx.seqlen_offsets = seqlen_offsets
        else:
            ctx.save_for_backward(cos, sin, seqlen_offsets)
            ctx.seqlen_offsets = None
        ctx.interleaved = interleaved
        ctx.mark_dirty(kv)
        return kv

    @staticmethod
    def backward(ctx, dkv):
        seqlen_offsets = ctx.seqlen_offsets
        if seqlen_offsets is None:
            cos, sin, seqlen_offsets = ctx.saved_tensors
        else:
            cos, sin = ctx.saved_tensors
        if dkv.stride(-1) != 1:
            dkv = dkv.contiguous()
        dk = dkv[:, :, 0]
        _launch(dk, dk, cos, sin, ctx.interleaved, True, seqlen_offsets, None, None)
        return dkv, None, None, None, None


def apply_rotary_emb_kv_(kv, cos, sin, interleaved=False, seqlen_offsets: Union[int, torch.Tensor] = 0):
    """kv: (batch, seqlen, 2, nheads, headdim).  Rotates k IN PLACE; v is never read or written.  Returns kv."""
    return ApplyRotaryEmbKV_.apply(kv, cos, sin, interleaved, seqlen_offsets)


class RotaryEmbedding(torch.nn.Module):
    """Upstream's rotary module: keeps a cos / sin cache, cos[i, t] = cos(i * base^(-2t / dim)), grown on demand and held in the
    dtype of the tensors it rotates.  pos_idx_in_fp32: positions are generated in fp32 (a bf16 arange loses integers above
    256) and inv_freq is kept in fp32.  xPos (`scale_base`) is not implemented."""

    def __init__(self, dim: int, base=10000.0, interleaved=False, scale_base=None, pos_idx_in_fp32=True, device=None):
        super().__init__()
        if scale_base is not None:
            raise NotImplementedError("RotaryEmbedding: scale_base (xPos) is not supported")
        self.dim = dim
        self.base = float(base)
        self.pos_idx_in_fp32 = pos_idx_in_fp32
        self.register_buffer("inv_freq", self._compute_inv_freq(device), persistent=False)
        self.interleaved = interleaved
        self.scale_base = scale_base
        self.scale = None
        self._seq_len_cached = 0
        self._cos_cached = None
        self._sin_cached = None
        self._cos_k_cached = None
        self._sin_k_cached = None

    def _compute_inv_freq(self, device=None):
        return 1.0 / (self.base ** (torch.arange(0, self.dim, 2, device=device, dtype=torch.float32) / self.dim))

    def _update_cos_sin_cache(self, seqlen, device=None, dtype=None):
        # rebuilt when the sequence grows, the device changes (tracing), or the dtype does
        if (seqlen > self._seq_len_cached or self._cos_cached is None or self._cos_cached.device != device
                or self._cos_cached.dtype != dtype or (self.training and self._cos_cached.is_inference())):
            self._seq_len_cached = seqlen
            if self.pos_idx_in_fp32:
                t = torch.arange(seqlen, device=device, dtype=torch.float32)
                # inv_freq may have been cast with the module (model.bfloat16()): recompute it in fp32
                inv_freq = self.inv_freq if self.inv_freq.dtype == torch.float32 else self._compute_inv_freq(device=device)
            else:
                t = torch.arange(seqlen, device=device, dtype=self.inv_freq.dtype)
                inv_freq = self.inv_freq
            freqs = torch.outer(t, inv_freq.to(device=t.device))
            self._cos_cached = torch.cos(freqs).to(dtype)
            self._sin_cached = torch.sin(freqs).to(dtype)

    def forward(self, qkv: torch.Tensor, kv: Optional[torch.Tensor] = None, seqlen_offset: Union[int, torch.Tensor] = 0,
                max_seqlen: Optional[int] = None, num_heads_q: Optional[int] = None):
        """qkv: (batch, seqlen, 3, nheads, headdim) or (batch, seqlen, nheads_q + 2 nheads_k, headdim) with num_heads_q when kv
        is None; else the query (batch, seqlen, nheads, headdim) next to kv (batch, seqlen, 2, nheads, headdim).
        seqlen_offset: int or int32 (batch,) tensor (then pass max_seqlen, which sizes the cache).
        Rotates IN PLACE; returns qkv, or (q, kv)."""
        seqlen = qkv.shape[1]
        if max_seqlen is not None:
            self._update_cos_sin_cache(max_seqlen, device=qkv.device, dtype=qkv.dtype)
        elif isinstance(seqlen_offset, int):
            self._update_cos_sin_cache(seqlen + seqlen_offset, device=qkv.device, dtype=qkv.dtype)
        if self._cos_cached is None:
            raise RuntimeError("RotaryEmbedding: a tensor seqlen_offset needs max_seqlen (it sizes the cos / sin cache)")
        if kv is None:
            return apply_rotary_emb_qkv_(qkv, self._cos_cached, self._sin_cached, interleaved=self.interleaved,
                                         seqlen_offsets=seqlen_offset, num_heads_q=num_heads_q)
        q = apply_rotary_emb_func(qkv, self._cos_cached, self._sin_cached, interleaved=self.interleaved, inplace=True,
                                  seqlen_offsets=seqlen_offset)
        kv = apply_rotary_emb_kv_(kv, self._cos_cached, self._sin_cached, interleaved=self.interleaved,
                                  seqlen_offsets=seqlen_offset)
        return q, kv


__all__ = ["apply_rotary", "apply_rotary_emb", "apply_rotary_emb_func", "apply_rotary_emb_qkv_", "apply_rotary_emb_kv_",
           "RotaryEmbedding"]
