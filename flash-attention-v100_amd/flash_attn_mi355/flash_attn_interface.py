"""Python operator API of the MI355X fused attention path.

Mirrors the reference's operator layer name for name
(flash_attn_v100/flash_attn_interface.py:115-127, :272-289, :323-343, :393-401):
`flash_attn_func`, `flash_attn_varlen_func`, `flash_attn_with_kvcache` (+ `_gpu` aliases),
same positional/keyword arguments, defaults and return conventions.  Differences, all
deliberate (DESIGN.md "divergences"):
  * tensors are handed to the C ABI (include/fa_mi355.h) with their strides - none of the
    reference's permute().contiguous() copies (flash_attn_interface.py:36-53,67);
  * fp16 AND bf16; any head_dim <= 256 (zero-padded to 64/128/256 on the host);
  * `return_attn_probs=True` works with dropout_p == 0 (returns an empty dmask) instead of
    raising (kernel/fused_mha_forward.cu:371);
  * `flash_attn_with_kvcache` accepts fp8-e4m3 caches with `k_descale` / `v_descale`;
  * `flash_attn_func` / `flash_attn_varlen_func` accept float8_e4m3fn q, k AND v (forward only, bf16 out; the varlen
    function takes `q_descale` / `k_descale` / `v_descale`);
  * attention sinks (one learned logit per query head in the softmax denominator, no value: gpt-oss):
    `flash_attn_sinks_func` for the dense layout, keyword `sinks` of `flash_attn_varlen_func` and
    `flash_attn_with_kvcache` (the C ABI's *_ext entry points).
There is no CPU fallback: tensors must live on an AMD GPU and the HIP library must load.

Structure of the host code: each op checks its arguments and allocates its outputs itself; the ~60 fields of `fa_params`
are filled in ONE place, `_fill_params` (layouts "bshd", "thd", paged K / V; fp8 q / k / v and fp8 caches; the optional
gradient block), for the dense and varlen forwards and backwards and for the slow path of `flash_attn_with_kvcache`
(whose cached fast path copies a filled struct and rewrites the pointers).  `_attach_workspace` (query, allocate, attach
- on q's device) and `_finish_out` (the caller's `out`, or the slice off the head-dim padding) are shared by those
paths; the two backwards are one body, `_backward`; the five autograd classes share `_save_ctx`,
`_grad_buffers`, `_autograd_backward` and `_cut_grads`.
"""
import collections
import ctypes
import os
import traceback
import warnings
from typing import Optional, Tuple, Union

import torch

from . import _lib
from ._lib import FaParams

_DTYPES = {torch.float16: _lib.FA_FP16, torch.bfloat16: _lib.FA_BF16}


def maybe_contiguous(x):
    return x.contiguous() if x is not None and not x.is_contiguous() else x


def _padded_head_dim(d: int) -> int:
    if d <= 64:
        return 64
    if d <= 128:
        return 128
    if d <= 256:
        return 256          # functional, not yet tuned (register spills): DESIGN.md section 8
    raise RuntimeError(f"head dimension {d} > 256 is not supported (reference limit, fused_mha_forward.cu:337)")


def _prep(x: torch.Tensor, d8: int) -> torch.Tensor:
    """Last dim contiguous, 16-byte aligned rows; the head dim is padded only up to the next multiple of 8
    (`d8`, as the reference does, flash_attn_interface.py:44-49).  The kernel width (64 / 128 / 256) is NOT
    materialised: the C ABI's head_dim_v makes the kernels read the missing columns as zeros."""
    d = x.shape[-1]
    if d != d8:
        x = torch.nn.functional.pad(x, [0, d8 - d])
    ok = x.stride(-1) == 1 and x.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in x.stride()[:-1])
    return x if ok else x.contiguous()


def _set_head_dim(p, d8: int):
    """kernel width + valid columns"""
    p.head_dim = _padded_head_dim(d8)
    p.head_dim_v = d8 if d8 != p.head_dim else 0


def _check_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("flash_attn_mi355: tensors must be on the GPU (no CPU fallback)")


def _check_shape(t, shape, name):
    """CHECK_SHAPE of the reference (kernel/fused_mha_forward.cu:324-340, fused_mha_forward_kvcache.cu:488-598):
    the C ABI only sees pointers and strides, so a mismatched tensor must be rejected here."""
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")


_FP8 = torch.float8_e4m3fn


def _is_fp8_qkv(q, k, v):
    """all three float8_e4m3fn: the fp8 forward (fa_fwd_fp8.hip); a mix of fp8 and 16-bit inputs raises"""
    n = sum(t.dtype == _FP8 for t in (q, k, v))
    if 0 < n < 3:
        raise RuntimeError("q, k and v must all be float8_e4m3fn (the fp8 forward) or all fp16 / bf16")
    return n == 3


def _check_fp8_options(head_size_og, dropout_p, softcap, alibi_slopes, paged=False, sinks=None):
    """what the fp8 forward does not cover: raised here, before anything is allocated or launched"""
    if sinks is not None:
        raise RuntimeError("fp8 forward: attention sinks are not supported")
    if head_size_og > 128:
        raise RuntimeError(f"fp8 forward: head dimension {head_size_og} is not supported (at most 128)")
    if dropout_p > 0.0:
        raise RuntimeError("fp8 forward: dropout is not supported")
    if softcap > 0.0:
        raise RuntimeError("fp8 forward: softcap is not supported")
    if alibi_slopes is not None:
        raise RuntimeError("fp8 forward: ALiBi is not supported")
    if paged:
        raise RuntimeError("fp8 forward: paged k / v (block_table) is not supported with fp8 q")


def _check_sinks(sinks, nheads_q, q, dropout_p=0.0):
    """attention sinks ([H_Q], any floating dtype, on q's device) -> the contiguous fp32 tensor the kernels read, or None.
    Raised here, before anything is allocated: a wrong shape, dtype or device, fp8 q / k / v, dropout.  The cast is
    differentiable, so a gradient returns in the caller's dtype (a bf16 nn.Parameter gets a bf16 gradient)."""
    if sinks is None:
        return None
    if not isinstance(sinks, torch.Tensor):
        raise RuntimeError("sinks must be a tensor of shape [nheads_q]")
    if q.dtype == _FP8:
        raise RuntimeError("attention sinks are not supported with fp8 (float8_e4m3fn) q / k / v")
    if dropout_p > 0.0:
        raise RuntimeError("attention sinks are not supported with dropout")
    if not sinks.is_floating_point() or sinks.dtype == _FP8:
        raise RuntimeError(f"sinks must have a floating dtype (fp32, bf16, fp16), got {sinks.dtype}")
    if tuple(sinks.shape) != (nheads_q,):
        raise RuntimeError(f"sinks must have shape ({nheads_q},) (one logit per query head), got {tuple(sinks.shape)}")
    if sinks.device != q.device:
        raise RuntimeError(f"sinks must be on q's device ({q.device}), got {sinks.device}")
    return sinks.to(torch.float32).contiguous()


def _check_fp8_no_grad(*tensors, grad_enabled=None):
    """grad_enabled: the caller's grad mode (inside an autograd.Function's forward torch.is_grad_enabled() is False)"""
    if grad_enabled is None:
        grad_enabled = torch.is_grad_enabled()
    if grad_enabled and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError("the fp8 (float8_e4m3fn) forward is forward-only: no backward")


def _prep8(x: torch.Tensor, d16: int) -> torch.Tensor:
    """_prep for fp8 tensors: the head dim zero-padded to a multiple of 16 (`d16`; the kernels read whole 16-byte chunks),
    16-byte aligned rows"""
    d = x.shape[-1]
    if d != d16:
        x = torch.nn.functional.pad(x.view(torch.uint8), [0, d16 - d]).view(_FP8)      # (code 0x00 = +0.0)
    ok = x.stride(-1) == 1 and x.data_ptr() % 16 == 0 and all(s % 16 == 0 for s in x.stride()[:-1])
    return x if ok else x.contiguous()


def _check_qkv(q, k, v):
    if q.dtype not in _DTYPES:
        raise RuntimeError("q must be fp16 or bf16")
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise RuntimeError("k/v must have the same dtype as q")
    if q.dim() != k.dim() or k.dim() != v.dim():
        raise RuntimeError("q, k, v must have the same number of dimensions")
    if q.shape[-1] != k.shape[-1] or q.shape[-1] != v.shape[-1]:
        raise RuntimeError("q, k, v must have the same head dimension")


def _check_out(out, q):
    """optional caller-allocated output (reference: fused_mha_forward.cu:392-396)"""
    if out.dtype != q.dtype:
        raise RuntimeError("out must have the same dtype as q")
    if not out.is_cuda:
        raise RuntimeError("out must be on the GPU")
    if out.stride(-1) != 1:
        raise RuntimeError("out must have contiguous last dimension")
    if tuple(out.shape) != tuple(q.shape):
        raise RuntimeError("out shape must match q shape")


def _usable_out(out, dpad, head_size_og):
    """a caller-allocated out can be written in place when its rows are 16-byte aligned and unpadded"""
    return (out is not None and dpad == head_size_og and out.data_ptr() % 16 == 0 and
            all(st % 8 == 0 for st in out.stride()[:-1]))


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device) -> int:
    """raw handle of torch's current stream on `device` (the stream the reference launches on: fused_mha_forward.cu:416)"""
    if _raw_stream is not None:
        idx = device.index
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)
    return torch.cuda.current_stream(device).cuda_stream


class _on_device:
    """`with _on_device(dev)` that costs nothing when `dev` is already current (the usual case; the context manager
    itself was ~3 us of the ~25 us a call spends on the host: tools/host_overhead.py)"""
    __slots__ = ("idx", "prev")

    def __init__(self, device):
        self.idx = device.index
        self.prev = None

    def __enter__(self):
        if self.idx is not None:
            cur = torch.cuda.current_device()
            if cur != self.idx:
                self.prev = cur
                torch.cuda.set_device(self.idx)
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _set3(p, name, t, layout):
    """layout 'bshd': [B,S,H,D]; 'thd': [T,H,D]; 'pshd': paged [nblk,page,H,D]."""
    if layout in ("bshd", "pshd"):
        setattr(p, name + "_batch_stride", t.stride(0))
        setattr(p, name + "_row_stride", t.stride(1))
        setattr(p, name + "_head_stride", t.stride(2))
    else:
        setattr(p, name + "_batch_stride", 0)
        setattr(p, name + "_row_stride", t.stride(0))
        setattr(p, name + "_head_stride", t.stride(1))


def _alibi(p, alibi_slopes, batch, nheads):
    if alibi_slopes.dtype != torch.float32 or not alibi_slopes.is_cuda:
        raise RuntimeError("alibi_slopes must be fp32 on the GPU")
    if alibi_slopes.stride(-1) != 1:
        raise RuntimeError("alibi_slopes last dim must be contiguous")
    if not (tuple(alibi_slopes.shape) == (nheads,) or tuple(alibi_slopes.shape) == (batch, nheads)):
        raise RuntimeError("alibi_slopes must be [H_Q] or [B, H_Q]")
    p.alibi_slopes = _ptr(alibi_slopes)
    p.alibi_batch_stride = alibi_slopes.stride(0) if alibi_slopes.dim() == 2 else 0


def _philox(p, dropout_p, batch, nheads, device, rng=None):
    """dropout_p > 0: seed/offset from the default GPU generator; the offset advances by B*H*32 per call
    (kernel/fused_mha_forward.cu:377-386)."""
    p.p_dropout = float(dropout_p)
    if rng is None:
        gen = torch.cuda.default_generators[device.index if device.index is not None
                                            else torch.cuda.current_device()]
        seed, offset = gen.initial_seed(), gen.get_offset()
        gen.set_offset(offset + batch * nheads * 32)
        rng = (seed, offset)
    p.philox_seed, p.philox_offset = rng[0] & 0xFFFFFFFFFFFFFFFF, rng[1]
    return rng


def _workspace(nbytes, device):
    if nbytes <= 0:
        return None
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _attach_workspace(p, query, device):
    """Ask `query` (a *_workspace_bytes export) what the launch of `p` needs, allocate it and attach it: (workspace or None,
    bytes asked for).  Call it inside `_on_device(device)`: the query reads the CURRENT device's CU count, which must be
    the device of the launch.  The caller keeps the tensor until the launch is enqueued."""
    nbytes = int(query(ctypes.byref(p)))
    ws = _workspace(nbytes, device)
    if ws is not None:
        p.workspace, p.workspace_bytes = _ptr(ws), ws.numel()
    return ws, nbytes


def _base_params(_q, dtype, scale, causal, window_size, softcap):
    p = FaParams()
    p.dtype = p.kv_dtype = _DTYPES[dtype]
    p.softmax_scale = float(scale)
    p.softcap = float(softcap)
    p.is_causal = int(bool(causal))
    p.window_left, p.window_right = int(window_size[0]), int(window_size[1])
    p.k_descale = p.v_descale = 1.0
    return p


def _fill_params(layout, q, k, v, o, lse, dims, seqlen_q, seqlen_k, softmax_scale, causal, window_size, softcap, alibi_slopes,
                 flags=0, dropout_p=0.0, rng=None, descales=(None, None, None), cu_seqlens=None, seqused_k=None,
                 block_table=None, grads=None):
    """The one place fa_params is filled: (p, rng) for every attention launch but the cached decode fast path.

    layout: 'bshd' - q / k / v / o [B, S, H, D], lse [B, H, S] - or 'thd' - [T, H, D], lse [H, T], with cu_seqlens =
    (cu_seqlens_q, cu_seqlens_k) as contiguous int32 tensors; with a block_table (contiguous int32 [B, max_blocks]) k / v are
    paged [num_blocks, page, Hk, D].  The tensors are the ones the kernels see (_prep / _prep8 done); dims = (batch, H_Q, H_K,
    their head dim), which every caller has at hand (reading them off the tensors again costs 0.4 us a call); seqlen_q /
    seqlen_k are the dense lengths or the varlen maxima.  float8_e4m3fn q (then k and v too) selects the fp8 forward and its bf16
    out, float8_e4m3fn k with a 16-bit q an fp8 cache; descales = (q, k, v) scalars, None = 1, read for fp8 tensors only.
    grads = (dout, dq, dk, dv, softmax_d) for a backward: a None gradient stays NULL with zero strides, so its kernel does
    not run.  rng: the forward's (seed, offset) for a backward, None to draw from the default generator (dropout_p > 0)."""
    if k.dtype == _FP8:                                  # an fp8 cache or, with an fp8 q, the fp8 forward (bf16 out)
        fp8_q = q.dtype == _FP8
        p = _base_params(q, torch.bfloat16 if fp8_q else q.dtype, softmax_scale, causal, window_size, softcap)
        p.kv_dtype = _lib.FA_FP8_E4M3
        if fp8_q:
            p.dtype = _lib.FA_FP8_E4M3
            p.o_dtype = _lib.FA_BF16
            p.q_descale = 1.0 if descales[0] is None else float(descales[0])
        p.k_descale = 1.0 if descales[1] is None else float(descales[1])
        p.v_descale = 1.0 if descales[2] is None else float(descales[2])
    else:
        p = _base_params(q, q.dtype, softmax_scale, causal, window_size, softcap)
    p.q, p.k, p.v, p.o, p.lse = _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse)
    kv_layout = layout if block_table is None else "pshd"
    _set3(p, "q", q, layout); _set3(p, "k", k, kv_layout); _set3(p, "v", v, kv_layout)
    _set3(p, "o", o, layout)
    B, H_Q, H_K, D = dims
    p.batch, p.nheads_q, p.nheads_k = B, H_Q, H_K
    _set_head_dim(p, D)
    if layout == "thd":
        p.seqlen_q, p.seqlen_k = int(seqlen_q), int(seqlen_k)
        p.lse_batch_stride, p.lse_head_stride = 0, lse.stride(0)
        p.cu_seqlens_q, p.cu_seqlens_k = _ptr(cu_seqlens[0]), _ptr(cu_seqlens[1])
        p.total_q = q.shape[0]
        p.total_k = k.shape[0] if block_table is None else 0
        p.seqused_k = _ptr(seqused_k)
    else:
        p.seqlen_q, p.seqlen_k = seqlen_q, seqlen_k
        p.lse_batch_stride, p.lse_head_stride = lse.stride(0), lse.stride(1)
    if block_table is not None:
        p.block_table = _ptr(block_table)
        p.block_table_batch_stride = block_table.stride(0)
        p.page_block_size = k.shape[1]
    if grads is not None:
        dout, dq, dk, dv, softmax_d = grads
        p.dout, p.dq, p.dk, p.dv, p.softmax_d = _ptr(dout), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(softmax_d)
        for name, t in (("do", dout), ("dq", dq), ("dk", dk), ("dv", dv)):
            if t is not None:
                _set3(p, name, t, layout)
    if flags:
        p.flags = flags
    if alibi_slopes is not None:
        _alibi(p, alibi_slopes, B, H_Q)
    if dropout_p > 0.0:
        return p, _philox(p, dropout_p, B, H_Q, q.device, rng=rng)
    p.p_dropout = float(dropout_p)
    return p, (0, 0)


def _finish_out(out, out_, dpad, head_size_og):
    """what a forward returns for the tensor the kernel wrote: the caller's `out` (copied into when the kernel could not write
    it directly), else out_ (head dim dpad) without the head-dim padding.  The forwards return out_ themselves in the usual case
    (no caller's out, no padding) and come here for the rest."""
    if out is not None and out_ is not out:
        out.copy_(out_[..., :head_size_og])
        return out
    return out_ if dpad == head_size_og else out_[..., :head_size_og].contiguous()


# ======================================================================================
# DENSE ATTENTION (B, M, H, D)
# ======================================================================================
# Opt-in experiment (include/fa_mi355.h: FA_FLAG_FWD_KEY_SPLIT; a net loss at the shapes it was built for, profiles/r06_fwd_split.txt):
# causal launches of at most one wave of 256-row blocks split the key range of their heavy blocks.  FA_FWD_SPLIT=1 at import.
FWD_SPLIT = os.environ.get("FA_FWD_SPLIT", "0") == "1"


def _dense_forward(q, k, v, dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes,
                   return_softmax, out=None, keep_window=False, sinks=None):
    """One fa_fwd call on [B, S, H, D] views (any strides with a contiguous last dim).  float8_e4m3fn q, k, v (descales 1)
    run the fp8 forward: bf16 out, fp32 LSE.  keep_window (sharding.py only):
    FA_FLAG_KEEP_WINDOW - a right window of >= seqlen_k keys stays a window where it still hides keys (seqlen_q >
    seqlen_k); the public functions keep the reference's normalisation, which drops it.  sinks: contiguous fp32 [H_Q]
    attention sinks (_check_sinks) or None - with sinks the call goes through fa_fwd_ext."""
    _check_device(q, k, v)
    fp8 = _is_fp8_qkv(q, k, v)
    if fp8:
        if sinks is not None:
            raise RuntimeError("fp8 forward: attention sinks are not supported")
        if out is not None or keep_window:
            raise RuntimeError("fp8 forward: no caller-allocated out / sharding window")
    else:
        _check_qkv(q, k, v)
    if q.dim() != 4:
        raise RuntimeError("q, k, v must be (batch, seqlen, nheads, headdim)")
    B, M, H_Q, head_size_og = q.shape
    N, H_K = k.shape[1], k.shape[2]
    _check_shape(k, (B, N, H_K, head_size_og), "k")
    _check_shape(v, (B, N, H_K, head_size_og), "v")
    if fp8:
        _check_fp8_options(head_size_og, dropout_p, softcap, alibi_slopes)
        dpad, prep, o_dtype = (head_size_og + 15) // 16 * 16, _prep8, torch.bfloat16
    else:
        if out is not None:
            _check_out(out, q)
        dpad, prep, o_dtype = (head_size_og + 7) // 8 * 8, _prep, q.dtype
        _padded_head_dim(dpad)                               # raises above 256
    q_, k_, v_ = prep(q, dpad), prep(k, dpad), prep(v, dpad)
    if softmax_scale is None:
        softmax_scale = head_size_og ** -0.5

    out_ = out if _usable_out(out, dpad, head_size_og) else torch.empty((B, M, H_Q, dpad), dtype=o_dtype, device=q.device)
    lse = torch.empty((B, H_Q, M), dtype=torch.float32, device=q.device)
    split = FWD_SPLIT and not fp8
    flags = (_lib.FA_FLAG_KEEP_WINDOW if keep_window else 0) | (_lib.FA_FLAG_FWD_KEY_SPLIT if split else 0)
    p, rng = _fill_params("bshd", q_, k_, v_, out_, lse, (B, H_Q, H_K, dpad), M, N, softmax_scale, causal, window_size,
                          softcap, alibi_slopes, flags, dropout_p)
    dmask = torch.empty((0,), dtype=o_dtype, device=q.device)
    if return_softmax and dropout_p > 0.0:
        dmask = torch.zeros((B, H_Q, M, N), dtype=o_dtype, device=q.device)
        p.dmask = _ptr(dmask)
    if q_.numel() > 0:                                   # (an empty query block is a no-op)
        with _on_device(q.device):
            # (non-zero only with the opt-in key split of one-wave causal launches, include/fa_mi355.h: FA_FLAG_FWD_KEY_SPLIT)
            ws = _attach_workspace(p, _lib.lib.fa_fwd_workspace_bytes, q.device) if (split and N > 0) else None
            _lib.call_ext("fa_fwd", p, None if sinks is None else _lib.ext_params(sinks), _stream(q.device))
    res = out_ if (out is None and dpad == head_size_og) else _finish_out(out, out_, dpad, head_size_og)
    return res, lse, dmask, (q_, k_, v_, out_), rng, softmax_scale


# Opt-in experiment (include/fa_mi355.h: FA_FLAG_DS_HANDOFF; break-even on BASELINE config 2, profiles/r06_ds_handoff.txt): the dense
# D = 128 backward hands dS from the dK/dV kernel to a one-GEMM dQ kernel instead of recomputing S and dP.  FA_BWD_DS=1 at import.
DS_HANDOFF = os.environ.get("FA_BWD_DS", "0") == "1"


def _backward(layout, dout, q_, k_, v_, out_, lse, cu_seqlens, seqlen_q, seqlen_k, alibi_slopes, dropout_p, softmax_scale,
              causal, window_size, softcap, rng, dq_, dk_, dv_, flags, sinks, dsinks):
    """One fa_bwd ('bshd') / fa_varlen_bwd ('thd') call: the body of _dense_backward and _varlen_backward.  Returns
    softmax_d, which is allocated on the empty-query path too (where nothing is launched)."""
    H_Q, dpad = q_.shape[-2], q_.shape[-1]
    batch = q_.shape[0] if layout == "bshd" else cu_seqlens[0].numel() - 1
    dout_ = _prep(dout, dpad)
    softmax_d = torch.empty((batch, H_Q, q_.shape[1]) if layout == "bshd" else (H_Q, q_.shape[0]),
                            dtype=torch.float32, device=q_.device)
    if (dk_ is None) != (dv_ is None):
        raise RuntimeError("dk and dv are computed together: pass both or neither")
    if q_.numel() == 0:                                  # no queries: nothing flows into K / V
        if dk_ is not None:
            dk_.zero_(); dv_.zero_()
        if dsinks is not None:
            dsinks.zero_()
        return softmax_d
    p, _ = _fill_params(layout, q_, k_, v_, out_, lse, (batch, H_Q, k_.shape[-2], dpad), seqlen_q, seqlen_k, softmax_scale,
                        causal, window_size, softcap, alibi_slopes, flags, dropout_p, rng, cu_seqlens=cu_seqlens,
                        grads=(dout_, dq_, dk_, dv_, softmax_d))
    with _on_device(q_.device):
        ws = _attach_workspace(p, _lib.lib.fa_bwd_workspace_bytes, q_.device)
        ext = None if sinks is None else _lib.ext_params(sinks, dsinks)
        _lib.call_ext("fa_bwd" if layout == "bshd" else "fa_varlen_bwd", p, ext, _stream(q_.device))
    return softmax_d


def _dense_backward(dout, q_, k_, v_, out_, lse, alibi_slopes, dropout_p, softmax_scale, causal,
                    window_size, softcap, rng, dq_, dk_, dv_, keep_window=False, deterministic=False, sinks=None,
                    dsinks=None):
    """One fa_bwd call; dq_/dk_/dv_ are caller-allocated [B, S, H, dpad] views (written in place).  dq_ = None, or
    dk_ = dv_ = None, skips that gradient's kernel (autograd's needs_input_grad).

    `deterministic`: every backward form is atomic-free and run-to-run repeatable; what the flag adds is BATCH INVARIANCE -
    small dK/dV launches (batch x kv-heads x key blocks < the CUs' slots) otherwise split their query rows over several
    workgroups and sum fp32 partials, so the last bit of dK / dV depends on batch x heads and the CU count.  True sets
    FA_FLAG_NO_DKV_SPLIT (include/fa_mi355.h): one workgroup per key block, the same bits at every batch size.

    sinks / dsinks: the forward's fp32 [H_Q] attention sinks and a caller-allocated fp32 [H_Q] for their gradient (or
    None): fa_bwd_ext.  dq_ = dk_ = dv_ = None with dsinks given computes the sinks' gradient only."""
    flags = ((_lib.FA_FLAG_KEEP_WINDOW if keep_window else 0) | (_lib.FA_FLAG_NO_DKV_SPLIT if deterministic else 0) |
             (_lib.FA_FLAG_DS_HANDOFF if DS_HANDOFF else 0))
    return _backward("bshd", dout, q_, k_, v_, out_, lse, None, q_.shape[1], k_.shape[1], alibi_slopes, dropout_p,
                     softmax_scale, causal, window_size, softcap, rng, dq_, dk_, dv_, flags, sinks, dsinks)


# ---- what the autograd classes share (and the backward ops of torch_ops.py / sharding.py: _grad_buffers) ----
def _save_ctx(ctx, res, alibi_slopes, sinks, dropout_p, causal, window_size, softcap, deterministic, head_size_og,
              max_seqlens=(None, None)):
    """what every autograd backward needs, from `res`, _dense_forward's / _varlen_forward's return tuple.  One form for the
    five classes: the saved tensors end in (lse, alibi_slopes, sinks) - sinks None where the class has none - and the dense
    classes keep max_seqlen_q / max_seqlen_k = None."""
    _, lse, _, saved, rng, softmax_scale = res
    ctx.save_for_backward(*saved, lse, alibi_slopes, sinks)
    ctx.dropout_p = dropout_p
    ctx.softmax_scale = softmax_scale
    ctx.causal = causal
    ctx.window_size = window_size
    ctx.softcap = softcap
    ctx.deterministic = deterministic
    ctx.head_size_og = head_size_og
    ctx.max_seqlen_q, ctx.max_seqlen_k = max_seqlens
    ctx.rng = rng


def _autograd_result(ctx, res):
    """what an autograd forward returns with return_attn_probs: (out, lse, dmask), the last two non-differentiable"""
    ctx.mark_non_differentiable(res[1], res[2])
    return res[:3]


def _grad_buffers(q_, k_, v_, need_q=True, need_kv=True):
    """(dq_, dk_, dv_) padded like the prepared q_ / k_ / v_; a gradient nobody needs is None"""
    dpad = q_.shape[-1]
    dq_ = _prep(torch.empty_like(q_), dpad) if need_q else None
    if not need_kv:
        return dq_, None, None
    return dq_, _prep(torch.empty_like(k_), dpad), _prep(torch.empty_like(v_), dpad)


def _autograd_backward(ctx, saved_tensors, dout, dq_, dk_, dv_, dsinks=None):
    """the backward launch from what _save_ctx kept (saved_tensors = ctx.saved_tensors, unpacked once by the caller):
    dense, or varlen when _save_ctx was given max_seqlens"""
    *saved, lse, alibi_slopes, sinks = saved_tensors
    if ctx.max_seqlen_q is None:                         # a dense class: saved = (q_, k_, v_, out_)
        _dense_backward(dout, *saved, lse, alibi_slopes, ctx.dropout_p, ctx.softmax_scale, ctx.causal, ctx.window_size,
                        ctx.softcap, ctx.rng, dq_, dk_, dv_, deterministic=ctx.deterministic, sinks=sinks, dsinks=dsinks)
    else:                                                # FlashAttnVarlenFunc: saved = (q_, k_, v_, out_, cu_seqlens_q, cu_seqlens_k)
        _varlen_backward(dout, *saved[:4], lse, saved[4], saved[5], alibi_slopes, ctx.max_seqlen_q, ctx.max_seqlen_k,
                         ctx.dropout_p, ctx.softmax_scale, ctx.causal, ctx.window_size, ctx.softcap, ctx.rng,
                         dq_, dk_, dv_, deterministic=ctx.deterministic, sinks=sinks, dsinks=dsinks)


def _cut_grads(ctx, dq_, dk_, dv_):
    """(dq, dk, dv) without the head-dim padding, None where inputs 0 / 1 / 2 of the Function need no gradient"""
    d, need = ctx.head_size_og, ctx.needs_input_grad
    return (dq_[..., :d] if need[0] else None, dk_[..., :d] if need[1] else None, dv_[..., :d] if need[2] else None)


class FlashAttnFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, dropout_p, softmax_scale, causal, window_size, softcap,
                alibi_slopes, deterministic, return_softmax, is_grad_enabled):
        is_grad = is_grad_enabled and any(x.requires_grad for x in [q, k, v])
        res = _dense_forward(q, k, v, dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes, return_softmax)
        if is_grad:
            _save_ctx(ctx, res, alibi_slopes, None, dropout_p, causal, window_size, softcap, deterministic, q.shape[-1])
        return _autograd_result(ctx, res) if return_softmax else res[0]

    @staticmethod
    def backward(ctx, dout, *args):
        saved, need = ctx.saved_tensors, ctx.needs_input_grad
        dq_, dk_, dv_ = _grad_buffers(saved[0], saved[1], saved[2], need[0], need[1] or need[2])
        _autograd_backward(ctx, saved, dout, dq_, dk_, dv_)
        return _cut_grads(ctx, dq_, dk_, dv_) + (None,) * 10


class FlashAttnSinksFunc(torch.autograd.Function):
    """FlashAttnFunc with attention sinks (fp32 [H_Q], already checked and cast: _check_sinks): the same dense forward and
    backward host code through fa_fwd_ext / fa_bwd_ext; the sinks' gradient when they require grad.  No dropout."""

    @staticmethod
    def forward(ctx, q, k, v, sinks, softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic,
                return_softmax, is_grad_enabled):
        is_grad = is_grad_enabled and any(x.requires_grad for x in [q, k, v, sinks])
        res = _dense_forward(q, k, v, 0.0, softmax_scale, causal, window_size, softcap, alibi_slopes, return_softmax,
                             sinks=sinks)
        if is_grad:
            _save_ctx(ctx, res, alibi_slopes, sinks, 0.0, causal, window_size, softcap, deterministic, q.shape[-1])
        return _autograd_result(ctx, res) if return_softmax else res[0]

    @staticmethod
    def backward(ctx, dout, *args):
        saved, need = ctx.saved_tensors, ctx.needs_input_grad
        dq_, dk_, dv_ = _grad_buffers(saved[0], saved[1], saved[2], need[0], need[1] or need[2])
        dsinks = torch.empty_like(saved[-1]) if need[3] else None
        _autograd_backward(ctx, saved, dout, dq_, dk_, dv_, dsinks)
        return _cut_grads(ctx, dq_, dk_, dv_) + (dsinks,) + (None,) * 8


class FlashAttnQKVPackedFunc(torch.autograd.Function):
    """qkv [B, S, 3, H, D]: q/k/v are strided views of the packed tensor in both directions -
    dq/dk/dv are written straight into one dqkv allocation (no concatenation pass)."""

    @staticmethod
    def forward(ctx, qkv, dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes,
                deterministic, return_softmax, is_grad_enabled):
        if qkv.dtype == _FP8:
            _check_fp8_no_grad(qkv, grad_enabled=is_grad_enabled)
        is_grad = is_grad_enabled and qkv.requires_grad
        res = _dense_forward(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], dropout_p, softmax_scale, causal, window_size,
                             softcap, alibi_slopes, return_softmax)
        if is_grad:
            _save_ctx(ctx, res, alibi_slopes, None, dropout_p, causal, window_size, softcap, deterministic, qkv.shape[-1])
        return _autograd_result(ctx, res) if return_softmax else res[0]

    @staticmethod
    def backward(ctx, dout, *args):
        saved = ctx.saved_tensors
        q_ = saved[0]
        B, S, H, dpad = q_.shape
        dqkv = torch.empty((B, S, 3, H, dpad), dtype=q_.dtype, device=q_.device)
        _autograd_backward(ctx, saved, dout, dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2])
        return (dqkv[..., :ctx.head_size_og],) + (None,) * 9


class FlashAttnKVPackedFunc(torch.autograd.Function):
    """q [B, Sq, H, D], kv [B, Sk, 2, Hk, D]; dk/dv are written into one dkv allocation."""

    @staticmethod
    def forward(ctx, q, kv, dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes,
                deterministic, return_softmax, is_grad_enabled):
        if _is_fp8_qkv(q, kv, kv):
            _check_fp8_no_grad(q, kv, grad_enabled=is_grad_enabled)
        is_grad = is_grad_enabled and any(x.requires_grad for x in [q, kv])
        res = _dense_forward(q, kv[:, :, 0], kv[:, :, 1], dropout_p, softmax_scale, causal, window_size, softcap,
                             alibi_slopes, return_softmax)
        if is_grad:
            _save_ctx(ctx, res, alibi_slopes, None, dropout_p, causal, window_size, softcap, deterministic, q.shape[-1])
        return _autograd_result(ctx, res) if return_softmax else res[0]

    @staticmethod
    def backward(ctx, dout, *args):
        saved = ctx.saved_tensors
        q_, k_ = saved[0], saved[1]
        B, Sk, Hk, dpad = k_.shape
        dq_ = _prep(torch.empty_like(q_), dpad)
        dkv = torch.empty((B, Sk, 2, Hk, dpad), dtype=q_.dtype, device=q_.device)
        _autograd_backward(ctx, saved, dout, dq_, dkv[:, :, 0], dkv[:, :, 1])
        d = ctx.head_size_og
        return (dq_[..., :d], dkv[..., :d]) + (None,) * 9


def _warn_deterministic(deterministic):
    if deterministic:
        # the reference warns and clears the flag (flash_attn_interface.py:129-131); our backward is atomic-free, i.e. always
        # run-to-run deterministic - the flag is kept and additionally makes the gradients batch-invariant (no split dK/dV
        # launches: `_dense_backward`).
        warnings.warn("Forward is always deterministic. Backward on gfx950 is atomic-free and "
                      "deterministic as well; deterministic=True also disables the split dK/dV launches "
                      "(batch-invariant gradients).", RuntimeWarning)
    return bool(deterministic)


def flash_attn_func(q, k, v, dropout_p: float = 0.0, softmax_scale: float = None,
                    causal: bool = False, window_size: Tuple[int, int] = (-1, -1),
                    softcap: float = 0.0, alibi_slopes: Optional[torch.Tensor] = None,
                    deterministic: bool = False, return_attn_probs: bool = False):
    """Dense Flash Attention (B, M, H, D)

    fp8: with q, k and v all torch.float8_e4m3fn the forward runs on the fp8 matrix pipe (head dim <= 128, no dropout,
    softcap or ALiBi; forward only) and returns a bfloat16 `out` and the fp32 LSE.  The inputs are taken as they are
    (descales 1): for tensors that dequantise as code * descale pass softmax_scale * q_descale * k_descale and multiply
    `out` by v_descale (flash_attn_varlen_func also takes the three descales as keywords)."""
    deterministic = _warn_deterministic(deterministic)
    try:
        if _is_fp8_qkv(q, k, v):
            _check_fp8_no_grad(q, k, v)
            out, lse, dmask, _, _, _ = _dense_forward(q, k, v, dropout_p, softmax_scale, causal, window_size, softcap,
                                                      alibi_slopes, return_attn_probs)
            return (out, lse, dmask) if return_attn_probs else out
        return FlashAttnFunc.apply(q, k, v, dropout_p, softmax_scale, causal, window_size, softcap,
                                   alibi_slopes, deterministic, return_attn_probs,
                                   torch.is_grad_enabled())
    except Exception as e:
        print(f"[MI355X FA2 DENSE FAILED] {type(e).__name__}: {e}")
        traceback.print_exc()
        raise


def flash_attn_sinks_func(q, k, v, sinks, *, softmax_scale: float = None, causal: bool = False,
                          window_size: Tuple[int, int] = (-1, -1), softcap: float = 0.0,
                          alibi_slopes: Optional[torch.Tensor] = None, deterministic: bool = False,
                          return_attn_probs: bool = False):
    """Dense attention (B, M, H, D) with attention sinks: `sinks` [H_Q] (any floating dtype, on q's device; natural-log
    units) holds one logit per query head that joins the softmax denominator and carries no value (gpt-oss):
        out_i = sum_j e^{x_ij} v_j / (e^{s_h} + sum_j e^{x_ij}),   LSE_i = log(e^{s_h} + sum_j e^{x_ij})
    with x_ij the final score (softmax_scale q.k, softcap, ALiBi).  Otherwise flash_attn_func without dropout: the other
    arguments mean the same, return_attn_probs returns (out, sink-inclusive LSE, empty dmask).  Differentiable in q, k,
    v and sinks (the sinks' gradient in their own dtype).  Not with fp8 q / k / v."""
    deterministic = _warn_deterministic(deterministic)
    try:
        s32 = _check_sinks(sinks, q.shape[-2], q)
        if s32 is None:
            raise RuntimeError("flash_attn_sinks_func needs sinks (flash_attn_func is the function without them)")
        return FlashAttnSinksFunc.apply(q, k, v, s32, softmax_scale, causal, window_size, softcap, alibi_slopes,
                                        deterministic, return_attn_probs, torch.is_grad_enabled())
    except Exception as e:
        print(f"[MI355X FA2 SINKS FAILED] {type(e).__name__}: {e}")
        traceback.print_exc()
        raise


# ======================================================================================
# VARLEN ATTENTION (T, H, D)
# ======================================================================================
def _varlen_forward(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p,
                    softmax_scale, causal, window_size, softcap, alibi_slopes, return_attn_probs,
                    block_table, seqused_k=None, leftpad_k=None, zero_tensors=False, out=None,
                    k_descale=None, v_descale=None, q_descale=None, sinks=None):
    """One fa_varlen_fwd call on [T, H, D] tensors (K/V optionally paged [nblk, page, Hk, D]).
    float8_e4m3fn q, k, v (non-paged) run the fp8 forward: bf16 out, value = code * q/k/v_descale.
    seqused_k clamps the keys of each sequence (include/template.h:65-68); zero_tensors pre-fills out / lse / dmask
    (fused_mha_forward_varlen.cu:538-542); leftpad_k is validated and, like in the reference kernel (the pointer is a
    parameter that is never read, fused_mha_forward_varlen.cu:37), not applied.  sinks: contiguous fp32 [H_Q]
    attention sinks (_check_sinks) or None - with sinks the call goes through fa_varlen_fwd_ext."""
    if cu_seqlens_k is None:
        # paged callers that carry lengths only (seqused_k, as vLLM-style wrappers do): the prefix sums the op wants
        if block_table is None or seqused_k is None:
            raise RuntimeError("cu_seqlens_k may be omitted only for paged k / v with seqused_k")
        cu_seqlens_k = torch.nn.functional.pad(seqused_k.cumsum(0, dtype=torch.int32), (1, 0))
    _check_device(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, leftpad_k)
    fp8_q = q.dtype == _FP8
    if fp8_q:
        _is_fp8_qkv(q, k, v)
        _check_fp8_options(q.shape[-1], dropout_p, softcap, alibi_slopes, paged=block_table is not None, sinks=sinks)
        if out is not None:
            raise RuntimeError("fp8 forward: no caller-allocated out")
    elif q.dtype not in _DTYPES:
        raise RuntimeError("q must be fp16 or bf16")
    fp8 = not fp8_q and k.dtype == torch.float8_e4m3fn
    if fp8:
        # this build's extension (as in flash_attn_with_kvcache): a paged fp8-e4m3 cache, value = code * descale; forward only
        if v.dtype != k.dtype or block_table is None:
            raise RuntimeError("fp8 k/v through the varlen op: paged k and v (block_table), both float8_e4m3fn")
        if q.shape[-1] not in (64, 128) or dropout_p > 0.0:
            raise RuntimeError("fp8 k/v: head dimension 64 or 128, no dropout")
    elif k.dtype != q.dtype or v.dtype != q.dtype:
        raise RuntimeError("k/v must have the same dtype as q")
    if q.dim() != 3:
        raise RuntimeError("q must be (total_q, nheads, headdim)")
    if block_table is None:
        if k.dim() != 3 or v.dim() != 3:
            raise RuntimeError("k, v must be (total_k, nheads_k, headdim)")
        _check_shape(v, k.shape, "v")
    else:
        if k.dim() != 4 or v.dim() != 4:
            raise RuntimeError("paged k, v must be (num_blocks, page_block_size, nheads_k, headdim)")
        _check_shape(v, k.shape, "v")
        if leftpad_k is not None:
            raise RuntimeError("Paged KV and leftpad_k are not supported simultaneously")
    if k.shape[-1] != q.shape[-1]:
        raise RuntimeError("q, k, v must have the same head dimension")
    if cu_seqlens_q.dim() != 1 or cu_seqlens_k.dim() != 1 or cu_seqlens_q.numel() != cu_seqlens_k.numel():
        raise RuntimeError("cu_seqlens_q and cu_seqlens_k must be 1-D of size batch + 1")
    nb = cu_seqlens_q.numel() - 1
    for name, t in (("seqused_k", seqused_k), ("leftpad_k", leftpad_k)):
        if t is not None:
            if t.dtype != torch.int32:
                raise RuntimeError(f"{name} must have dtype int32")
            if t.dim() != 1 or t.numel() != nb or not t.is_contiguous():
                raise RuntimeError(f"{name} must be 1D, contiguous, with size == batch_size")
    if block_table is not None and block_table.shape[0] != nb:
        raise RuntimeError("block_table must have one row per sequence")
    cu_seqlens_q = cu_seqlens_q.to(torch.int32).contiguous()
    cu_seqlens_k = cu_seqlens_k.to(torch.int32).contiguous()
    head_size_og = q.size(-1)
    dpad = (head_size_og + 15) // 16 * 16 if fp8_q else (head_size_og + 7) // 8 * 8
    _padded_head_dim(dpad)                                   # raises above 256
    prep = _prep8 if fp8_q else _prep
    q_, k_, v_ = prep(q, dpad), prep(k, dpad), prep(v, dpad)
    if softmax_scale is None:
        softmax_scale = head_size_og ** -0.5
    T_Q, H_Q = q_.shape[0], q_.shape[1]
    dims = (cu_seqlens_q.numel() - 1, H_Q, k_.shape[-2], dpad)

    o_dtype = torch.bfloat16 if fp8_q else q.dtype           # (the fp8 forward writes bf16)
    if out is not None:
        _check_out(out, q)
    out_ = out if _usable_out(out, dpad, head_size_og) else torch.empty((T_Q, H_Q, dpad), dtype=o_dtype, device=q.device)
    lse = torch.empty((H_Q, T_Q), dtype=torch.float32, device=q.device)
    if zero_tensors:
        out_.zero_()
        lse.fill_(float("-inf"))
    if block_table is not None:
        block_table = block_table.to(torch.int32).contiguous()
    p, rng = _fill_params("thd", q_, k_, v_, out_, lse, dims, max_seqlen_q, max_seqlen_k, softmax_scale, causal, window_size,
                          softcap, alibi_slopes, 0, dropout_p, None, (q_descale, k_descale, v_descale),
                          (cu_seqlens_q, cu_seqlens_k), seqused_k, block_table)
    dmask = torch.empty((0,), dtype=o_dtype, device=q.device)
    if return_attn_probs and dropout_p > 0.0:
        dmask = torch.zeros((T_Q, H_Q, max_seqlen_k), dtype=o_dtype, device=q.device)
        p.dmask = _ptr(dmask)
    with _on_device(q.device):
        # (decode issued through this op - the same few query tokens per sequence over paged K / V - runs the decode kernels
        #  when their split-KV workspace is there: fa_api.hip varlen_decode_route)
        ws = _attach_workspace(p, _lib.lib.fa_fwd_workspace_bytes, q.device)
        if q_.numel() > 0:
            _lib.call_ext("fa_varlen_fwd", p, None if sinks is None else _lib.ext_params(sinks), _stream(q.device))
    res = out_ if (out is None and dpad == head_size_og) else _finish_out(out, out_, dpad, head_size_og)
    return res, lse, dmask, (q_, k_, v_, out_, cu_seqlens_q, cu_seqlens_k), rng, softmax_scale


def _varlen_backward(dout, q_, k_, v_, out_, lse, cu_seqlens_q, cu_seqlens_k, alibi_slopes,
                     max_seqlen_q, max_seqlen_k, dropout_p, softmax_scale, causal, window_size,
                     softcap, rng, dq_, dk_, dv_, deterministic=False, sinks=None, dsinks=None):
    """One fa_varlen_bwd call (fa_varlen_bwd_ext with attention sinks; see _dense_backward for sinks / dsinks)."""
    return _backward("thd", dout, q_, k_, v_, out_, lse, (cu_seqlens_q, cu_seqlens_k), max_seqlen_q, max_seqlen_k,
                     alibi_slopes, dropout_p, softmax_scale, causal, window_size, softcap, rng, dq_, dk_, dv_,
                     _lib.FA_FLAG_NO_DKV_SPLIT if deterministic else 0, sinks, dsinks)


class FlashAttnVarlenFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p,
                softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic,
                return_attn_probs, block_table, is_grad_enabled, sinks=None):
        is_grad = is_grad_enabled and any(x is not None and x.requires_grad for x in [q, k, v, sinks])
        res = _varlen_forward(
            q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p, softmax_scale,
            causal, window_size, softcap, alibi_slopes, return_attn_probs, block_table, sinks=sinks)
        if is_grad:
            if block_table is not None:
                raise RuntimeError("backward through paged K/V (block_table) is not supported")
            _save_ctx(ctx, res, alibi_slopes, sinks, dropout_p, causal, window_size, softcap, deterministic,
                      q.size(-1), (max_seqlen_q, max_seqlen_k))
        return _autograd_result(ctx, res) if return_attn_probs else res[0]

    @staticmethod
    def backward(ctx, dout, *args):
        saved, need = ctx.saved_tensors, ctx.needs_input_grad
        with_sinks = len(need) > 17                         # (apply() was given the optional 18th argument)
        dq_, dk_, dv_ = _grad_buffers(saved[0], saved[1], saved[2], need[0], need[1] or need[2])
        dsinks = torch.empty_like(saved[-1]) if (with_sinks and need[17]) else None
        _autograd_backward(ctx, saved, dout, dq_, dk_, dv_, dsinks)
        grads = _cut_grads(ctx, dq_, dk_, dv_) + (None,) * 14
        return grads + (dsinks,) if with_sinks else grads


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q: int,
                           max_seqlen_k: int, dropout_p: float = 0.0, softmax_scale: float = None,
                           causal: bool = False, window_size: Tuple[int, int] = (-1, -1),
                           softcap: float = 0.0, alibi_slopes: Optional[torch.Tensor] = None,
                           deterministic: bool = False, return_attn_probs: bool = False,
                           block_table: Optional[torch.Tensor] = None, *,
                           seqused_k: Optional[torch.Tensor] = None,
                           k_descale: Optional[float] = None, v_descale: Optional[float] = None,
                           q_descale: Optional[float] = None, sinks: Optional[torch.Tensor] = None):
    """Varlen Flash Attention (T, H, D).  seqused_k ([B] int32, forward only): use only the first seqused_k[b] keys
    of sequence b (the op-level argument of the reference, include/mha.h:116-139).  Paged k / v may be float8_e4m3fn
    (value = code * k_descale / v_descale; forward only) - this build's extension, as in flash_attn_with_kvcache.
    q, k and v may all be float8_e4m3fn (non-paged; value = code * q_descale / k_descale / v_descale, None = 1): the
    fp8 forward of flash_attn_func, bfloat16 `out`, forward only.
    sinks ([H_Q], any floating dtype): attention sinks, one logit per query head in the softmax denominator with no value
    (flash_attn_sinks_func); differentiable like q, k, v; not with fp8 q / k / v or dropout.  The LSE returned is the
    sink-inclusive one."""
    deterministic = _warn_deterministic(deterministic)
    try:
        s32 = _check_sinks(sinks, q.shape[-2], q, dropout_p)
        fp8 = k.dtype == torch.float8_e4m3fn or q.dtype == torch.float8_e4m3fn
        if seqused_k is not None or fp8:
            if torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (q, k, v, sinks)):
                raise RuntimeError("seqused_k / fp8 k, v are forward-only (the reference's backward op has neither)")
            out, lse, dmask, _, _, _ = _varlen_forward(
                q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p, softmax_scale, causal,
                window_size, softcap, alibi_slopes, return_attn_probs, block_table, seqused_k=seqused_k,
                k_descale=k_descale, v_descale=v_descale, q_descale=q_descale, sinks=s32)
            return (out, lse, dmask) if return_attn_probs else out
        if s32 is not None:
            return FlashAttnVarlenFunc.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
                                             max_seqlen_k, dropout_p, softmax_scale, causal,
                                             window_size, softcap, alibi_slopes, deterministic,
                                             return_attn_probs, block_table, torch.is_grad_enabled(), s32)
        return FlashAttnVarlenFunc.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
                                         max_seqlen_k, dropout_p, softmax_scale, causal,
                                         window_size, softcap, alibi_slopes, deterministic,
                                         return_attn_probs, block_table, torch.is_grad_enabled())
    except Exception as e:
        print(f"[MI355X FA2 VARLEN FAILED] {type(e).__name__}: {e}")
        traceback.print_exc()
        raise


# ======================================================================================
# KV ATTENTION
# ======================================================================================
def flash_attn_with_kvcache(q, k_cache, v_cache, k=None, v=None, rotary_cos=None, rotary_sin=None,
                            cache_seqlens: Optional[Union[int, torch.Tensor]] = None,
                            cache_batch_idx: Optional[torch.Tensor] = None,
                            cache_leftpad: Optional[torch.Tensor] = None,
                            block_table: Optional[torch.Tensor] = None,
                            softmax_scale: Optional[float] = None, causal: bool = False,
                            window_size: Tuple[int, int] = (-1, -1), softcap: float = 0.0,
                            rotary_interleaved: bool = True,
                            alibi_slopes: Optional[torch.Tensor] = None, num_splits: int = 0,
                            return_softmax_lse: bool = False, *,
                            k_descale: Optional[float] = None, v_descale: Optional[float] = None,
                            sinks: Optional[torch.Tensor] = None,
                            tree_mask: Optional[torch.Tensor] = None, tree_depths: Optional[torch.Tensor] = None):
    """FlashAttention with KV cache (B, M, H, D). k_cache / v_cache are updated in place.

    A decode step is launch-bound at small batch (two kernels of 10-15 us), so the host side matters: the argument checks
    and the ~60 fields of fa_params depend only on the tensors' GEOMETRY (dtypes, shapes, strides, which optionals are
    given) and the scalar options - a serving loop repeats one geometry thousands of times.  The filled struct is kept per
    geometry (`_KV_PLANS`); a repeat call copies it and writes the dozen pointers (tools/host_overhead.py).

    sinks ([H_Q], any floating dtype, on q's device): attention sinks, one logit per query head in the softmax
    denominator with no value (flash_attn_sinks_func); the LSE returned is the sink-inclusive one.  Forward only.

    tree_mask: the T_q (2 .. 64) query tokens are the nodes of a speculative-decoding draft tree.  Every node sees the
    committed cache plus the new tokens its mask row names: bool [B, T_q, T_q] or [T_q, T_q] (row = query node, column = key
    node; packed to words on the device), or already packed int32 [B, T_q, W] / [T_q, W] with W = ceil(T_q / 32) (bit c & 31
    of word c >> 5 = key node c).  The mask replaces the causal rule (`causal` has no further effect); `window_size` must be
    (-1, -1) and ALiBi is not supported.  The nodes' K / V come with the call (k, v with T_q tokens) or already sit at the end
    of the cache.  tree_depths (int32 [B, T_q] or [T_q]): node t is rotated at position cache_seqlens + depth[t] while its
    cache slot stays cache_seqlens + t; required with rotary_cos, ignored without."""
    key = _kv_plan_key(q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, cache_seqlens, cache_batch_idx, cache_leftpad,
                       block_table, softmax_scale, causal, window_size, softcap, rotary_interleaved, alibi_slopes,
                       num_splits, k_descale, v_descale, sinks, tree_mask, tree_depths)
    plan = _KV_PLANS.get(key) if key is not None else None
    if plan is not None:
        _KV_PLANS.move_to_end(key)
        tmpl, ws_bytes, lse_shape = plan
        pp = FaParams.from_buffer_copy(tmpl)
        out = torch.empty_like(q)
        lse = torch.empty(lse_shape, dtype=torch.float32, device=q.device)
        pp.q, pp.k, pp.v, pp.o, pp.lse = q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(), lse.data_ptr()
        if cache_seqlens is not None: pp.cache_seqlens = cache_seqlens.data_ptr()
        if block_table is not None: pp.block_table = block_table.data_ptr()
        if k is not None: pp.k_new = k.data_ptr(); pp.v_new = v.data_ptr()
        if rotary_cos is not None: pp.rotary_cos = rotary_cos.data_ptr(); pp.rotary_sin = rotary_sin.data_ptr()
        if cache_batch_idx is not None: pp.cache_batch_idx = cache_batch_idx.data_ptr()
        if cache_leftpad is not None: pp.cache_leftpad = cache_leftpad.data_ptr()
        if alibi_slopes is not None: pp.alibi_slopes = alibi_slopes.data_ptr()
        if ws_bytes:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
            pp.workspace = ws.data_ptr()
        # (the sinks' geometry is part of the key; their pointer is written on every call, like the others)
        s32 = None if sinks is None else sinks.to(torch.float32).contiguous()
        with _on_device(q.device):
            if tree_mask is not None:
                # (the tree tensors' geometry is part of the key too; bool masks are packed on the device on every call)
                words = _pack_tree_mask(tree_mask) if tree_mask.dtype == torch.bool else tree_mask
                _lib.call_tree(pp, None if s32 is None else _lib.ext_params(s32),
                               _lib.tree_params(words, tree_depths if rotary_cos is not None else None), _stream(q.device))
            else:
                _lib.call_ext("fa_fwd_kvcache", pp, None if s32 is None else _lib.ext_params(s32), _stream(q.device))
        return (out, lse) if return_softmax_lse else out
    assert k_cache.stride(-1) == 1, "k_cache must have contiguous last dimension"
    assert v_cache.stride(-1) == 1, "v_cache must have contiguous last dimension"
    s32 = _check_sinks(sinks, q.shape[-2], q)
    tree_words, tree_depths = _check_tree(tree_mask, tree_depths, q, k, window_size, alibi_slopes, rotary_cos)
    _check_device(q, k_cache, v_cache, k, v)
    if q.dtype not in _DTYPES:
        raise RuntimeError("q must be fp16 or bf16")
    q, k, v = [maybe_contiguous(x) for x in (q, k, v)]
    B, T_Q, H_Q, D = q.shape
    if softmax_scale is None:
        softmax_scale = D ** (-0.5)
    if cache_seqlens is not None and isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((B,), cache_seqlens, dtype=torch.int32, device=k_cache.device)
    cache_seqlens = maybe_contiguous(cache_seqlens)
    cache_batch_idx = maybe_contiguous(cache_batch_idx)
    cache_leftpad = maybe_contiguous(cache_leftpad)
    block_table = maybe_contiguous(block_table)
    for name, t in (("cache_seqlens", cache_seqlens), ("cache_batch_idx", cache_batch_idx),
                    ("cache_leftpad", cache_leftpad), ("block_table", block_table)):
        if t is not None and t.dtype != torch.int32:
            raise RuntimeError(f"{name} must have dtype int32")
    if D % 8 != 0 or D > 256:
        raise RuntimeError("kvcache head dimension must be a multiple of 8 and <= 256")
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    if fp8 and v_cache.dtype != k_cache.dtype:
        raise RuntimeError("kcache and vcache must have the same dtype")
    if not fp8 and (k_cache.dtype != q.dtype or v_cache.dtype != q.dtype):
        raise RuntimeError("kcache/vcache must have the same dtype as q (or float8_e4m3fn)")
    if fp8 and D not in (64, 128):
        raise RuntimeError("fp8 KV caches are served by the decode kernel: head dimension 64 or 128")
    paged = block_table is not None
    if q.dim() != 4 or k_cache.dim() != 4:
        raise RuntimeError("q must be (B, T, H, D); k_cache / v_cache 4-D")
    H_K = k_cache.shape[2]
    # reference: fused_mha_forward_kvcache.cu:488-598 (CHECK_SHAPE)
    _check_shape(v_cache, k_cache.shape, "v_cache")
    if k_cache.shape[-1] != D:
        raise RuntimeError(f"k_cache / v_cache head dimension must be {D}")
    if H_Q % H_K != 0:
        raise RuntimeError("H_Q must be divisible by H_K for GQA/MQA")
    if not paged and cache_batch_idx is None and k_cache.shape[0] < B:
        raise RuntimeError("k_cache batch is smaller than the query batch")
    if paged:
        if block_table.dim() != 2 or block_table.shape[0] != B:
            raise RuntimeError("block_table must be (batch, max_num_blocks_per_seq)")
    for name, t in (("cache_seqlens", cache_seqlens), ("cache_batch_idx", cache_batch_idx),
                    ("cache_leftpad", cache_leftpad)):
        if t is not None and (t.dim() != 1 or t.numel() != B):
            raise RuntimeError(f"{name} must be 1D with size == batch_size")
    if k is not None and v is not None:
        if k.dtype != q.dtype or v.dtype != q.dtype:
            raise RuntimeError("k/v (new) must have the same dtype as q")
        _check_shape(k, (B, k.shape[1], H_K, D), "k")
        _check_shape(v, k.shape, "v")
    if rotary_cos is not None and rotary_sin is not None and tuple(rotary_sin.shape) != tuple(rotary_cos.shape):
        raise RuntimeError("rotary_sin must have the same shape as rotary_cos")

    out = torch.empty_like(q)
    lse = torch.empty((B, H_Q, T_Q), dtype=torch.float32, device=q.device)
    if k is not None and v is None:
        raise RuntimeError("If key is supplied, value must also be passed in")
    if rotary_cos is not None:
        if rotary_sin is None:
            raise RuntimeError("rotary_sin must be given with rotary_cos")
        if rotary_cos.dtype != q.dtype or rotary_sin.dtype != q.dtype:
            raise RuntimeError("rotary_cos must have the same dtype as query")
        if rotary_cos.dim() != 2 or not rotary_cos.is_contiguous() or not rotary_sin.is_contiguous():
            raise RuntimeError("rotary_cos/rotary_sin must be contiguous 2D tensors")
        if rotary_cos.shape[1] * 2 > q.shape[-1]:
            raise RuntimeError("rotary_dim must be <= headdim")
    # (head dim: width 64 / 128 / 256; narrower rows read as zeros past D.  The tree flag is set before the workspace
    #  query, which answers for the route a tree call takes)
    p, _ = _fill_params("bshd", q, k_cache, v_cache, out, lse, (B, H_Q, H_K, D), T_Q,
                        block_table.shape[1] * k_cache.shape[1] if paged else k_cache.shape[1], softmax_scale, causal,
                        window_size, softcap, alibi_slopes, _lib.FA_FLAG_TREE_MASK if tree_words is not None else 0,
                        descales=(None, k_descale, v_descale), block_table=block_table)
    # what only this op has: the cache index tensors, the new tokens, the in-kernel rotation, the split count
    p.cache_seqlens = _ptr(cache_seqlens)
    p.cache_batch_idx = _ptr(cache_batch_idx)
    p.cache_leftpad = _ptr(cache_leftpad)
    if k is not None:
        p.k_new, p.v_new = _ptr(k), _ptr(v)
        _set3(p, "knew", k, "bshd"); _set3(p, "vnew", v, "bshd")
        p.seqlen_new = k.shape[1]
    if rotary_cos is not None:
        p.rotary_cos, p.rotary_sin = _ptr(rotary_cos), _ptr(rotary_sin)
        p.rotary_dim = rotary_cos.shape[1] * 2
        p.seqlen_ro = rotary_cos.shape[0]
        p.rotary_interleaved = int(bool(rotary_interleaved))
    p.num_splits = int(num_splits)
    ext = None if s32 is None else _lib.ext_params(s32)
    with _on_device(q.device):
        ws, ws_bytes = _attach_workspace(p, _lib.lib.fa_fwd_kvcache_workspace_bytes, q.device)
        if tree_words is not None:
            _lib.call_tree(p, ext, _lib.tree_params(tree_words, tree_depths), _stream(q.device))
        else:
            _lib.call_ext("fa_fwd_kvcache", p, ext, _stream(q.device))
    if key is not None:                                  # (the call went through: this geometry passes every check)
        while len(_KV_PLANS) >= _KV_PLANS_MAX:           # least recently used geometry out (a workload whose geometry keeps
            _KV_PLANS.popitem(last=False)                # changing must not wipe the plans of the steady ones)
        _KV_PLANS[key] = (bytes(p), ws_bytes, tuple(lse.shape))
    if return_softmax_lse:
        return out, lse
    return out


_KV_PLANS = collections.OrderedDict()
_KV_PLANS_MAX = 256
_TREE_BITS = {}                                          # device -> int32 [32]: 1 << i (bit 31 as the sign bit)


def _pack_tree_mask(mask: torch.Tensor) -> torch.Tensor:
    """bool [..., T, T] (row = query node, column = key node) -> int32 [..., T, ceil(T / 32)] visibility words, bit c & 31 of
    word c >> 5 = column c.  A few device ops and no host sync, so the call stays capturable in a HIP graph."""
    T = mask.shape[-1]
    W = (T + 31) // 32
    bits = _TREE_BITS.get(mask.device)
    if bits is None:
        sh = torch.arange(32, dtype=torch.int32, device=mask.device)
        bits = _TREE_BITS[mask.device] = torch.bitwise_left_shift(torch.ones_like(sh), sh)
    m = mask
    if W * 32 != T:
        m = torch.nn.functional.pad(m, (0, W * 32 - T))
    # (distinct powers of two: the int32 sum is exact, bit 31 being -2^31)
    return (m.reshape(*m.shape[:-1], W, 32).to(torch.int32) * bits).sum(-1, dtype=torch.int32)


def _check_tree(tree_mask, tree_depths, q, k, window_size, alibi_slopes, rotary_cos):
    """flash_attn_with_kvcache's tree arguments: (packed int32 words, depths or None), or (None, None) without a tree"""
    if tree_mask is None:
        if tree_depths is not None:
            raise RuntimeError("tree_depths needs tree_mask")
        return None, None
    if q.dim() != 4:
        raise RuntimeError("q must be (B, T, H, D)")
    B, T = q.shape[0], q.shape[1]
    if not isinstance(tree_mask, torch.Tensor) or tree_mask.device != q.device:
        raise RuntimeError("tree_mask must be a tensor on the same device as q")
    if not 2 <= T <= 64:
        raise RuntimeError(f"tree_mask: the tree must have 2 .. 64 query tokens (got {T})")
    W = (T + 31) // 32
    if tree_mask.dtype == torch.bool:
        if tuple(tree_mask.shape) not in ((B, T, T), (T, T)):
            raise RuntimeError(f"tree_mask (bool) must have shape ({B}, {T}, {T}) or ({T}, {T})")
        words = _pack_tree_mask(tree_mask)
    elif tree_mask.dtype == torch.int32:
        if tuple(tree_mask.shape) not in ((B, T, W), (T, W)):
            raise RuntimeError(f"tree_mask (packed int32) must have shape ({B}, {T}, {W}) or ({T}, {W})")
        words = tree_mask.contiguous()
    else:
        raise RuntimeError("tree_mask must have dtype bool or (packed) int32")
    if tuple(window_size) != (-1, -1):
        raise RuntimeError("tree_mask: window_size must be (-1, -1)")
    if alibi_slopes is not None:
        raise RuntimeError("tree_mask: ALiBi is not supported (its distance term needs tree positions)")
    if k is not None and k.shape[1] != T:
        raise RuntimeError(f"tree_mask: k / v must bring the tree's {T} tokens (or be None: the nodes already sit in the cache)")
    if rotary_cos is None:
        return words, None                               # (depths only feed the in-kernel RoPE)
    if tree_depths is None:
        raise RuntimeError("tree_mask with rotary_cos needs tree_depths (node t sits at position cache_seqlens + depth[t])")
    if not isinstance(tree_depths, torch.Tensor) or tree_depths.device != q.device or tree_depths.dtype != torch.int32:
        raise RuntimeError("tree_depths must be an int32 tensor on the same device as q")
    if tuple(tree_depths.shape) not in ((B, T), (T,)):
        raise RuntimeError(f"tree_depths must have shape ({B}, {T}) or ({T},)")
    return words, tree_depths.contiguous()


def _geom(t):
    return None if t is None else (t.dtype, t.shape, t.stride(), t.device.index)


def _kv_plan_key(q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, cache_seqlens, cache_batch_idx, cache_leftpad,
                 block_table, softmax_scale, causal, window_size, softcap, rotary_interleaved, alibi_slopes, num_splits,
                 k_descale, v_descale, sinks=None, tree_mask=None, tree_depths=None):
    """Everything flash_attn_with_kvcache's checks and fa_params fields depend on, except the data pointers - or None
    when the call needs the slow path anyway: an int cache_seqlens, descales given as tensors, or ANY input the slow path
    would route through maybe_contiguous() (the template holds the strides of the tensors the kernel was launched on: a
    view such as hidden[:, -1:] or block_table[:, :n] has a unit last stride but is not contiguous, and its copy's
    strides under the original's data pointer would read the wrong rows)."""
    if not isinstance(q, torch.Tensor) or isinstance(cache_seqlens, int):
        return None
    if isinstance(k_descale, torch.Tensor) or isinstance(v_descale, torch.Tensor):
        return None
    for t in (q, k, v, cache_seqlens, cache_batch_idx, cache_leftpad, block_table, tree_mask, tree_depths):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() == 0 or not t.is_contiguous()):
            return None
    return (_geom(q), _geom(k_cache), _geom(v_cache), _geom(k), _geom(v), _geom(rotary_cos), _geom(rotary_sin),
            _geom(cache_seqlens), _geom(cache_batch_idx), _geom(cache_leftpad), _geom(block_table), _geom(alibi_slopes),
            softmax_scale, bool(causal), tuple(window_size), float(softcap), bool(rotary_interleaved), int(num_splits),
            None if k_descale is None else float(k_descale), None if v_descale is None else float(v_descale),
            _geom(sinks), _geom(tree_mask), _geom(tree_depths))


# ======================================================================================
# PACKED ENTRY POINTS (upstream flash-attn API)
# ======================================================================================
def flash_attn_qkvpacked_func(qkv, dropout_p: float = 0.0, softmax_scale: float = None,
                              causal: bool = False, window_size: Tuple[int, int] = (-1, -1),
                              softcap: float = 0.0, alibi_slopes: Optional[torch.Tensor] = None,
                              deterministic: bool = False, return_attn_probs: bool = False):
    """qkv: (B, S, 3, H, D).  Same semantics as flash_attn_func(qkv[:,:,0], qkv[:,:,1], qkv[:,:,2])."""
    deterministic = _warn_deterministic(deterministic)
    return FlashAttnQKVPackedFunc.apply(qkv, dropout_p, softmax_scale, causal, window_size, softcap,
                                        alibi_slopes, deterministic, return_attn_probs,
                                        torch.is_grad_enabled())


def flash_attn_kvpacked_func(q, kv, dropout_p: float = 0.0, softmax_scale: float = None,
                             causal: bool = False, window_size: Tuple[int, int] = (-1, -1),
                             softcap: float = 0.0, alibi_slopes: Optional[torch.Tensor] = None,
                             deterministic: bool = False, return_attn_probs: bool = False):
    """q: (B, Sq, H, D), kv: (B, Sk, 2, Hk, D)."""
    deterministic = _warn_deterministic(deterministic)
    return FlashAttnKVPackedFunc.apply(q, kv, dropout_p, softmax_scale, causal, window_size, softcap,
                                       alibi_slopes, deterministic, return_attn_probs,
                                       torch.is_grad_enabled())


def flash_attn_varlen_qkvpacked_func(qkv, cu_seqlens, max_seqlen: int, dropout_p: float = 0.0,
                                     softmax_scale: float = None, causal: bool = False,
                                     window_size: Tuple[int, int] = (-1, -1), softcap: float = 0.0,
                                     alibi_slopes: Optional[torch.Tensor] = None,
                                     deterministic: bool = False, return_attn_probs: bool = False):
    """qkv: (T, 3, H, D) - strided views into the packed tensor, no unpacking copy in forward."""
    return flash_attn_varlen_func(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu_seqlens, cu_seqlens, max_seqlen,
                                  max_seqlen, dropout_p, softmax_scale, causal, window_size, softcap,
                                  alibi_slopes, deterministic, return_attn_probs)


def flash_attn_varlen_kvpacked_func(q, kv, cu_seqlens_q, cu_seqlens_k, max_seqlen_q: int,
                                    max_seqlen_k: int, dropout_p: float = 0.0,
                                    softmax_scale: float = None, causal: bool = False,
                                    window_size: Tuple[int, int] = (-1, -1), softcap: float = 0.0,
                                    alibi_slopes: Optional[torch.Tensor] = None,
                                    deterministic: bool = False, return_attn_probs: bool = False):
    """q: (Tq, H, D), kv: (Tk, 2, Hk, D)."""
    return flash_attn_varlen_func(q, kv[:, 0], kv[:, 1], cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
                                  max_seqlen_k, dropout_p, softmax_scale, causal, window_size, softcap,
                                  alibi_slopes, deterministic, return_attn_probs)


flash_attn_gpu = flash_attn_func
flash_attn_varlen_gpu = flash_attn_varlen_func
flash_attn_with_kvcache_gpu = flash_attn_with_kvcache

__all__ = [
    "flash_attn_func", "flash_attn_gpu",
    "flash_attn_varlen_func", "flash_attn_varlen_gpu",
    "flash_attn_with_kvcache", "flash_attn_with_kvcache_gpu",
    "flash_attn_qkvpacked_func", "flash_attn_kvpacked_func",
    "flash_attn_varlen_qkvpacked_func", "flash_attn_varlen_kvpacked_func",
]
