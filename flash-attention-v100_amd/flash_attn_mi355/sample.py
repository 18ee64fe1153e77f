"""Token sampling from logits on the library's `fa_sample` kernel (csrc/fa_sample.hip): temperature, top-k, min-p, top-p and one
inverse-CDF draw per row - the serving-side end of the row ops: a decode step that has gone through `qk_norm_rope_and_store_kv`,
`flash_attn_with_kvcache`, `add_norm` and the LM head turns its `[..., V]` logits (fp16, bf16 or fp32) into int32 token ids in ONE
launch, instead of eager torch's sort, softmax, cumsum, mask and multinomial.  The rules (include/fa_mi355.h), per row:

    v_j  = float(logits_j), a NaN counts as -inf;  the order: larger value first, then lower index;  j* = the first token
    empty row (all -inf): id = -1, n_kept = 0, lse = -inf
    greedy row (!(temperature > 0), or v_j* = +inf): id = j*, n_kept = 1
    x_j  = v_j * (1 / temperature)   one rounding;   e_j = exp(x_j - x_j*);   q_j = floor(e_j * 2^40)   an integer mass
    top_k  keeps the first k of the order (1 <= k < the number of tokens above -inf; anything else: off)
    min_p  then drops the tokens with e_j < min(min_p, 1)              (min_p <= 0 or NaN: off)
    top_p  then keeps the smallest prefix whose mass reaches ceil(top_p * the mass left)   (top_p >= 1 or NaN: off; <= 0: one token)
    id   = the kept token of smallest index whose index-order running mass exceeds min(floor(u * Q), Q - 1),  Q the kept mass

Everything after the q_j is integer arithmetic, so a row's result depends on its values, its parameters and its u alone - not on
the batch it is in, its index or its alignment - and is bitwise repeatable.  The kernel holds no RNG: `u` is one fp32 uniform
number per row, drawn here with `torch.rand(generator=...)` where the caller passes none, so a call is capturable in a graph
(pass `u`).  Every parameter is a number or a tensor of one value per row: a mixed greedy / sampled batch is one call.
exp(t) is exp2(t * log2(e)) on the hardware's exp2; `lse` (return_lse) is m + log(s) of the fixed-order running (max, sum-exp) of
csrc/fa_lse.h over x: the log-probability of a token under the UNFILTERED distribution is x_id - lse.

Not covered: repetition / presence / frequency penalties and logit bias; an in-kernel RNG and per-row seeds; top-n log-prob
outputs; typical-p and the like; vocab > 2^20; in-place `top_k_top_p_filter` (rejection sampling and draft-tree verification for
speculative decoding: `spec_decode`).  Nothing here is exported through the packages' `__all__` lists."""
import ctypes

import torch

from . import _lib
from . import _rowargs as _ra
from . import flash_attn_interface as _fi

_OP = "sample"
_CODES = {torch.float16: _lib.FA_FP16, torch.bfloat16: _lib.FA_BF16, torch.float32: _lib.FA_FP32}
VOCAB_MAX = 1 << 20


def _rows(t, V):
    """[..., V] as the [rows, V] view the kernel takes (cross_entropy._rows' rule): a view whose last dimension is contiguous and
    whose rows flatten to one stride >= V as it is; anything else is copied"""
    v = t
    if t.dim() != 2:
        try:
            v = t.view(-1, V)
        except RuntimeError:
            v = None
    if v is not None and v.stride(1) == 1 and (v.shape[0] <= 1 or v.stride(0) >= V):
        return v
    return t.contiguous().view(-1, V)


def _check(logits):
    if logits.dtype not in _CODES:
        raise RuntimeError(f"{_OP}: logits must be fp16, bf16 or fp32, got {logits.dtype}")
    if logits.dim() < 1 or logits.shape[-1] < 1:
        raise RuntimeError(f"{_OP}: logits must be [..., V] with V >= 1, got {tuple(logits.shape)}")
    if logits.shape[-1] > VOCAB_MAX:
        raise RuntimeError(f"{_OP}: V must be <= 2^20, got {logits.shape[-1]}")
    return logits.shape[-1]


def _params(logits, temperature, top_k, top_p, min_p):
    rows = logits.numel() // logits.shape[-1]
    return [_ra.row_param(_OP, temperature, rows, torch.float32, "temperature"),
            _ra.row_param(_OP, top_k, rows, torch.int32, "top_k"),
            _ra.row_param(_OP, top_p, rows, torch.float32, "top_p"),
            _ra.row_param(_OP, min_p, rows, torch.float32, "min_p")]


def _launch(logits, V, params, u, want_ids, want_n, want_lse, want_filtered):
    """one fa_sample call over logits' [rows, V] view: (ids, n_kept, lse, filtered), None where not asked for"""
    lead = logits.shape[:-1]
    tensors = [t for t, _ in params]
    _ra.same_device(_OP, [logits, u] + tensors, logits, "logits'")
    dev = logits.device
    xi = _rows(logits, V)
    rows = xi.shape[0]
    ids = torch.empty(lead, dtype=torch.int32, device=dev) if want_ids else None
    n_kept = torch.empty(lead, dtype=torch.int32, device=dev) if want_n else None
    lse = torch.empty(lead, dtype=torch.float32, device=dev) if want_lse else None
    filtered = torch.empty(logits.shape, dtype=logits.dtype, device=dev) if want_filtered else None
    if rows == 0:
        return ids, n_kept, lse, filtered
    s = _lib.FaSampleParams()
    s.struct_size = ctypes.sizeof(_lib.FaSampleParams)
    s.logits, s.logits_row_stride = xi.data_ptr(), xi.stride(0)
    s.rows, s.vocab, s.dtype = rows, V, _CODES[xi.dtype]
    if u is not None:
        s.u = u.data_ptr()
    for name, (t, value) in zip(("temperature", "top_k", "top_p", "min_p"), params):
        if t is not None:
            setattr(s, name, t.data_ptr())
        else:
            setattr(s, name + "_value", value)
    for name, t in (("ids", ids), ("n_kept", n_kept), ("lse", lse)):
        if t is not None:
            setattr(s, name, t.data_ptr())
    if filtered is not None:
        s.filtered, s.filtered_row_stride = filtered.data_ptr(), V
    nbytes = _lib.sample_workspace_bytes(s)
    ws = _fi._workspace(nbytes, dev)
    if ws is not None:
        s.workspace, s.workspace_bytes = ws.data_ptr(), nbytes
    with _fi._on_device(dev):
        _lib.call_sample(s, _fi._stream(dev))                  # (queued: the tensors made here stay referenced until here)
    del xi, ws, tensors
    return ids, n_kept, lse, filtered


def _uniforms(logits, u, generator):
    """u as the kernel takes it: fp32, one value per row, contiguous; drawn with torch.rand where the caller passes none"""
    rows = logits.numel() // logits.shape[-1]
    if u is None:
        return torch.rand(rows, dtype=torch.float32, device=logits.device, generator=generator)
    if generator is not None:
        raise RuntimeError(f"{_OP}: pass u or generator, not both")
    if not isinstance(u, torch.Tensor) or u.dtype != torch.float32 or u.numel() != rows:
        raise RuntimeError(f"{_OP}: u must be a float32 tensor of one value per row ({rows})")
    return u.reshape(-1).contiguous()


def sample_forward(logits, u, *, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    """The op alone: (ids int32, n_kept int32, lse fp32), each of shape logits.shape[:-1], from `u` (fp32, one value per row; None
    only where every row is greedy by a temperature NUMBER that is not above 0).  One launch; the logits are taken as the view
    they are."""
    V = _check(logits)
    params = _params(logits, temperature, top_k, top_p, min_p)
    if u is not None:
        u = _uniforms(logits, u, None)
    elif params[0][0] is not None or params[0][1] > 0:
        raise RuntimeError(f"{_OP}: u is needed unless temperature is a number that is not above 0")
    ids, n_kept, lse, _ = _launch(logits, V, params, u, True, True, True, False)
    return ids, n_kept, lse


def sample(logits, *, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, u=None, generator=None, return_lse=False,
           return_n_kept=False):
    """int32 token ids of shape logits.shape[:-1] by the rules at the top of this module; with return_lse / return_n_kept a tuple
    (ids[, lse][, n_kept]).  Each of temperature / top_k / top_p / min_p is a number or a tensor of one value per row.  u: the
    uniform numbers (fp32, one per row) - drawn with torch.rand(generator=generator) where None."""
    V = _check(logits)
    params = _params(logits, temperature, top_k, top_p, min_p)
    _fi._check_device(logits)
    u = _uniforms(logits, u, generator)
    from . import torch_ops as _ops                            # (registers torch.ops.flash_attn_mi355.sample)
    (tt, tv), (kt, kv), (pt, pv), (mt, mv) = params
    ids, n_kept, lse = _ops.sample(logits, u, tt, 1.0 if tv is None else tv, kt, 0 if kv is None else kv,
                                   pt, 1.0 if pv is None else pv, mt, 0.0 if mv is None else mv)
    out = (ids,) + ((lse,) if return_lse else ()) + ((n_kept,) if return_n_kept else ())
    return out if len(out) > 1 else ids


def filter_forward(logits, *, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    """The op alone for `filtered`: a fresh contiguous tensor of logits' dtype and shape"""
    V = _check(logits)
    params = _params(logits, temperature, top_k, top_p, min_p)
    return _launch(logits, V, params, None, False, False, False, True)[3]


def top_k_top_p_filter(logits, *, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    """The logits with everything outside the kept set at -inf (a kept logit keeps its own bits - the temperature only decides
    what is kept): a fresh contiguous tensor of logits' dtype and shape.  A greedy row keeps its first maximum alone."""
    V = _check(logits)
    params = _params(logits, temperature, top_k, top_p, min_p)
    _fi._check_device(logits)
    from . import torch_ops as _ops                            # (registers torch.ops.flash_attn_mi355.sample_filter)
    (tt, tv), (kt, kv), (pt, pv), (mt, mv) = params
    del V
    return _ops.sample_filter(logits, tt, 1.0 if tv is None else tv, kt, 0 if kv is None else kv,
                              pt, 1.0 if pv is None else pv, mt, 0.0 if mv is None else mv)


def greedy(logits):
    """The first maximum of every row (a NaN counts as -inf; -1 for a row of -inf): int32 of shape logits.shape[:-1]"""
    V = _check(logits)
    _fi._check_device(logits)
    params = _params(logits, 0.0, 0, 1.0, 0.0)
    return _launch(logits, V, params, None, True, False, False, False)[0]
