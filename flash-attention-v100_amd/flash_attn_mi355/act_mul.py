"""The gated activation of the MLP, `act(gate) * up`, with its backward, on the library's `fa_act_mul` / `fa_act_mul_bwd` kernels
(csrc/fa_act_mul.hip): SwiGLU (Llama, Qwen, Mistral), GeGLU (Gemma) and the ungated activations - what upstream ships as
`flash_attn.ops.activations` and vLLM as `silu_and_mul` / `gelu_and_mul` / `gelu_tanh_and_mul`.  gate, up and every result are
fp16 or bf16 `[..., N]`; the forward reads each input once and writes the result once, the backward reads dout, gate and up and
writes dgate and dup: one launch each, no workspace, no temporary.  All arithmetic is fp32 with ONE rounding to the io type (not
the two roundings of `F.silu(gate) * up` in 16 bits), in exactly this order - every operation rounds once, fma is one rounding:

    g = float(gate_j);  u = float(up_j);  d = float(dout_j)
    out_j   = round16(act(g) * u)                                   up is None: round16(act(g))
    dgate_j = round16((d * u) * act'(g))                            up is None: round16(d * act'(g))
    dup_j   = round16(d * act(g))
    e(t)    = exp2(t * log2e)      fp32 product with log2e rounded to fp32, then the hardware exp2 (v_exp_f32)
    sig(t)  = rcp(1 + e(-t))       the hardware reciprocal (v_rcp_f32)
    "silu"       s = sig(g);   act = g * s;   act' = s * fma(g, 1 - s, 1)
    "gelu_tanh"  q = g * g;   w = (K2 * g) * fma(C3, q, 1);   s = sig(w);   act = g * s
                 act' = s * fma(g * (1 - s), K2 * fma(3 C3, q, 1), 1)
                 K2 = 2 sqrt(2 / pi), C3 = 0.044715, 3 C3 = 0.134145, each rounded to fp32.  0.5 (1 + tanh z) = sig(2 z), so
                 there is no tanh and no 1 + t that cancels for negative g; w = 2 z.
    "gelu"       ph = fma(0.5, erff(g * sqrt(1/2)), 0.5);   act = g * ph            (the erf form; erff is the device library's)
                 act' = fma(g, e((g * g) * -0.5) * sqrt(1 / (2 pi)), ph)
    "relu"       act = 0 if g <= 0 else g;   act' = 0 if g <= 0 else (1 if g > 0 else g)
    "relu2"      r = relu(g);   act = r * r;   act' = r + r

Special values are what these lines give literally - which is not always what torch gives - and none is a fault, a device assert
or a host synchronisation:
    g = +-0      silu, gelu_tanh: s = 0.5, act = +-0, act' = 0.5.  gelu: ph = 0.5, act = +-0, act' = 0.5.  relu, relu2: act = +0,
                 act' = 0 (torch's convention at 0; upstream's relu_bwd passes the gradient at 0).
    g = -100     (any finite g for which e overflows) silu, gelu_tanh: e = +inf, s = rcp(+inf) = 0, act = -0, act' = -0 -
                 never NaN.  gelu: erff = -1, ph = 0, act = -0, act' = fma(-100, 0, 0) = 0.
    g = +100     s = 1, act = g, act' = 1 (gelu: ph = 1, the density is 0).
    g = +inf     act = +inf for every activation.  act' = NaN for silu, gelu_tanh (fma(inf, 0, 1)) and gelu (fma(inf, 0, 1));
                 relu: 1, relu2: +inf.
    g = -inf     silu, gelu_tanh, gelu: act = -inf * 0 = NaN, act' = NaN.  relu, relu2: act = +0, act' = 0.
    |g| >= 2^64  gelu_tanh: q = g * g overflows; the forward is still g or -0, the backward is NaN.  bf16 only.
    g = NaN      NaN, forward and backward, for every activation (the ReLUs compare with `g <= 0`, which a NaN fails).
    0 * inf      act(g) = 0 times u = +-inf, or d = 0 times an infinite factor, is NaN as in IEEE arithmetic.
A result below 2^-126 in magnitude may be flushed to zero by the hardware exp2 and reciprocal.

An element's bits depend on its own operands alone - not on N, the row, the layout, the address alignment (a row that does not
start on a 16-byte boundary, and the last N % 8 columns, are taken element by element: the same values) or in place.

Tensors are `[..., N]`.  A view with a contiguous last dimension whose rows flatten to one stride >= N is taken as it is: the
halves of a packed `[..., 2N]` tensor, a `[:, :N]` view of padded rows.  Anything else is copied - which in place would change
the copy, so there it is an error.  CPU tensors raise: there is no torch fallback.

An fp8-quantised output in the place of the 16-bit one is `quant.act_mul_quant` / `quant.act_and_mul_quant` (the forward only).

Not covered: a bias and its gradient (a column sum), fp32 io, `F.glu`'s sigmoid gate, fusing into the GEMMs on either side, an
`Mlp` module, and a double backward.  Nothing here is exported through the packages' `__all__` lists."""
import ctypes

import torch

from . import _lib
from . import _rowargs as _ra
from . import flash_attn_interface as _fi

_OP = "act_mul"
ACTIVATIONS = {"silu": _lib.FA_ACT_SILU, "gelu": _lib.FA_ACT_GELU, "gelu_tanh": _lib.FA_ACT_GELU_TANH, "relu": _lib.FA_ACT_RELU,
               "relu2": _lib.FA_ACT_RELU2}


def _act(activation):
    if activation not in ACTIVATIONS:
        raise RuntimeError(f"{_OP}: activation must be one of {sorted(ACTIVATIONS)}, got {activation!r}")
    return ACTIVATIONS[activation]


def _rows(t, N, inplace, name):
    """[..., N] as the [rows, N] view the kernels take (cross_entropy._rows' rule): a view whose last dimension is contiguous
    and whose rows flatten to one stride >= N as it is; anything else is copied - in place, that is an error"""
    v = t
    if t.dim() != 2:
        try:
            v = t.view(-1, N)
        except RuntimeError:
            v = None
    if v is not None and (v.stride(1) == 1 or N == 1) and (v.shape[0] <= 1 or v.stride(0) >= N):
        return v
    if inplace:
        raise RuntimeError(f"{_OP}: in place needs {name} with a contiguous last dimension whose rows flatten to one stride "
                           f"(got strides {tuple(t.stride())}); pass it contiguous or go out of place")
    return t.contiguous().view(-1, N)


def _check(gate, up, others):
    """N; gate sets dtype and shape, `others` = [(name, tensor or None)] must match it"""
    if gate.dtype not in _fi._DTYPES:
        raise RuntimeError(f"{_OP}: gate must be fp16 or bf16, got {gate.dtype}")
    if gate.dim() < 1 or gate.shape[-1] < 1:
        raise RuntimeError(f"{_OP}: gate must be [..., N] with N >= 1, got {tuple(gate.shape)}")
    for name, t in [("up", up)] + others:
        if t is None:
            continue
        if t.dtype != gate.dtype:
            raise RuntimeError(f"{_OP}: {name} must have gate's dtype ({gate.dtype}), got {t.dtype}")
        if tuple(t.shape) != tuple(gate.shape):
            raise RuntimeError(f"{_OP}: {name} must have gate's shape {tuple(gate.shape)}, got {tuple(t.shape)}")
    return gate.shape[-1]


def act_mul_forward(gate, up=None, *, activation="silu", out=None):
    """The forward alone, no autograd: act(gate) * up, or act(gate) where up is None, of gate's dtype and shape.  out: the
    tensor to write - a fresh contiguous one by default; it may be gate or up themselves (in place), or any view the kernel
    takes as it is."""
    act = _act(activation)
    N = _check(gate, up, [("out", out)])
    _ra.same_device(_OP, [gate, up, out], gate, "gate's")
    dev = gate.device
    gi = _rows(gate, N, out is gate, "gate")
    ui = None if up is None else _rows(up, N, out is up, "up")
    if out is None:
        out = torch.empty(gate.shape, dtype=gate.dtype, device=dev)
    oi = gi if out is gate else ui if out is up else _rows(out, N, True, "out")
    if gi.shape[0] == 0:
        return out
    s = _lib.FaActMulParams()
    s.struct_size = ctypes.sizeof(_lib.FaActMulParams)
    s.gate, s.gate_row_stride = gi.data_ptr(), gi.stride(0)
    if ui is not None:
        s.up, s.up_row_stride = ui.data_ptr(), ui.stride(0)
    s.out, s.out_row_stride = oi.data_ptr(), oi.stride(0)
    s.rows, s.n, s.dtype, s.activation = gi.shape[0], N, _fi._DTYPES[gate.dtype], act
    with _fi._on_device(dev):
        _lib.call_act_mul(s, _fi._stream(dev))                 # (queued: the tensors made here stay referenced until here)
    del gi, ui, oi
    return out


def act_mul_backward(dout, gate, up=None, *, activation="silu", inplace=False, out=None):
    """(dgate, dup) - dup None where up is None - from dout and the forward's inputs: one launch.  inplace: dgate is the gate
    tensor and dup the up tensor themselves, rewritten where they are - nothing is allocated.  out=(dgate, dup) (dup None for
    the ungated form): the tensors to write, e.g. the two halves of one packed [..., 2N] gradient - no `cat`."""
    act = _act(activation)
    if inplace and out is not None:
        raise RuntimeError(f"{_OP}: inplace=True and out= exclude each other")
    dg = dp = None
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise RuntimeError(f"{_OP}: out must be the pair (dgate, dup)")
        dg, dp = out
        if dg is None or (dp is None) != (up is None):
            raise RuntimeError(f"{_OP}: out must hold dgate, and dup exactly where up is given")
    N = _check(gate, up, [("dout", dout), ("out[0]", dg), ("out[1]", dp)])
    _ra.same_device(_OP, [dout, gate, up, dg, dp], gate, "gate's")
    dev = gate.device
    gi = _rows(gate, N, inplace, "gate")
    ui = None if up is None else _rows(up, N, inplace, "up")
    di = _rows(dout, N, False, "dout")
    if inplace:
        dg, dp, dgi, dpi = gate, up, gi, ui
    else:
        if out is None:
            dg = torch.empty(gate.shape, dtype=gate.dtype, device=dev)
            dp = None if up is None else torch.empty(gate.shape, dtype=gate.dtype, device=dev)
        dgi = _rows(dg, N, True, "out[0]")
        dpi = None if dp is None else _rows(dp, N, True, "out[1]")
    if gi.shape[0] == 0:
        return dg, dp
    s = _lib.FaActMulBwdParams()
    s.struct_size = ctypes.sizeof(_lib.FaActMulBwdParams)
    s.dout, s.dout_row_stride = di.data_ptr(), di.stride(0)
    s.gate, s.gate_row_stride = gi.data_ptr(), gi.stride(0)
    s.dgate, s.dgate_row_stride = dgi.data_ptr(), dgi.stride(0)
    if ui is not None:
        s.up, s.up_row_stride = ui.data_ptr(), ui.stride(0)
        s.dup, s.dup_row_stride = dpi.data_ptr(), dpi.stride(0)
    s.rows, s.n, s.dtype, s.activation = gi.shape[0], N, _fi._DTYPES[gate.dtype], act
    with _fi._on_device(dev):
        _lib.call_act_mul_bwd(s, _fi._stream(dev))             # (queued: the tensors made here stay referenced until here)
    del gi, ui, di, dgi, dpi
    return dg, dp


def _halves(x):
    """(gate, up) of a packed [..., 2N]: the first half and the second, as in vLLM"""
    if x.dim() < 1 or x.shape[-1] < 2 or x.shape[-1] % 2:
        raise RuntimeError(f"{_OP}: a packed input must be [..., 2N] with N >= 1, got {tuple(x.shape)}")
    N = x.shape[-1] // 2
    return x[..., :N], x[..., N:]


def act_mul(gate, up=None, *, activation="silu", inplace_backward=False):
    """act(gate) * up (up None: act(gate)) with the formulas at the top of this module; differentiable in gate and up
    (`act_mul_backward`), no double backward.  inplace_backward=True: the backward writes dgate over gate and dup over up (they
    must not be used afterwards) and allocates nothing."""
    _act(activation)
    _fi._check_device(gate, up)
    from . import torch_ops as _ops                            # (registers torch.ops.flash_attn_mi355.act_mul)
    return _ops.act_mul(gate, up, activation, bool(inplace_backward))


def act_and_mul(x, *, activation="silu", inplace_backward=False):
    """act(x[..., :N]) * x[..., N:] of a packed [..., 2N] (gate first, as in vLLM): [..., N].  Differentiable in x: the backward
    allocates ONE [..., 2N] gradient and writes both halves into it - with inplace_backward=True it writes them over x instead."""
    _act(activation)
    _halves(x)
    _fi._check_device(x)
    from . import torch_ops as _ops
    return _ops.act_and_mul(x, activation, bool(inplace_backward))
