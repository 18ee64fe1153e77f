"""Dynamic fp8-e4m3 (`torch.float8_e4m3fn`) quantisation of fp16 / bf16 activations on the library's `fa_quant_fp8`,
`fa_add_norm_quant` and `fa_act_mul_quant` kernels (csrc/fa_quant.hip): alone, fused behind `add_norm`'s forward and fused behind
`act_mul`'s forward - what a caller needs to feed fp8 GEMMs with per-token or 1x128 block scales, or the fp8 q / k / v attention
forward, without reading the 16-bit activations back from memory.  One rule in all three ops, fp32 throughout; y_j are the values
to quantise AFTER their rounding to the 16-bit dtype (`quant_fp8`: x itself):

    a      = fmaxf(+0, |y_0|, |y_1|, ..)       over the row ("row"), or over each aligned group of 128 columns ("group")
    a'     = fminf(a, scale_ub) if scale_ub is given else a
    scale  = fmaxf(a' / 448, 2^-64)            one IEEE division; the floor keeps 1 / scale finite for an all-zero row
    inv    = 1 / scale                         one IEEE division
    code_j = e4m3(fminf(fmaxf(y_j * inv, -448), 448))           the hardware conversion: round to nearest even, saturating

mode:
    "row"     a dynamic scale per row.  scales: float32 `x.shape[:-1]`.
    "group"   a dynamic scale per 128 columns; N must be a multiple of 128.  scales: float32 `x.shape[:-1] + (N // 128,)`.
    "static"  `scale` is the caller's Python float, finite and > 0: only the last two lines run, scales is None.  This is the
              rule `store_kv_cache` writes fp8 caches with, and what `flash_attn_func` / `flash_attn_varlen_func` read as fp8
              q, k, v with that descale.
`code * scale` approximates y.  `scale_ub` (dynamic modes only, finite and > 0) caps the amax: larger values saturate.

Fused means bit-identical to unfused, codes and scales, in every mode:
    add_norm_quant(x, residual, w, ..)  ==  quant_fp8(add_norm(x, w, residual=residual, ..))     and the same residual_out
    act_mul_quant(gate, up, ..)         ==  quant_fp8(act_mul(gate, up, ..))
The fused kernels do the 16-bit op's arithmetic in its order, round to the 16-bit dtype and apply the rule to that value; the
16-bit output itself is never written.  A row's codes and scale depend on that row alone - not on the batch or the row's index.

Special values are what the lines above give literally, the same in all three ops; none is a fault, a device assert or a host
synchronisation:
    an all-zero row (group)    scale = 2^-64 (the floor); every code is +0, or -0 for y = -0
    y_j = NaN                  fmaxf skips it: the scale and the other codes are those of the row without it; its own code is
                               that of -448 (0xFE): NaN * inv = NaN, fmaxf(NaN, -448) = -448.  A row of NaNs alone: a = 0
    y_j = +-inf, no scale_ub   a = inf: scale = inf is returned, inv = 0, every finite y gives +-0 and the infinite ones
                               inf * 0 = NaN -> 0xFE
    y_j = +-inf with scale_ub  the scale is finite (at most scale_ub / 448): +-inf saturates to +-448
    "static"                   NaN -> 0xFE (-448), +-inf -> +-448
No code is ever the e4m3 NaN (0x7F / 0xFF).

Tensors are `[..., N]`, N a multiple of 8: up to 65536 for `quant_fp8` and `act_mul_quant`, up to 16384 for `add_norm_quant`
(`add_norm`'s range).  A view with a contiguous last dimension whose rows flatten to one stride is taken as it is; rows that do
not start on a 16-byte boundary are read element by element - the same bits.  CPU tensors raise: there is no torch fallback.
Not differentiable: a tensor that requires grad raises.

Out of scope: a backward or a straight-through estimator; device-resident static scales; per-tensor dynamic scales (a grid-wide
reduction); E8M0 / MX power-of-two scales; e5m2 and the fnuz formats; column-major or transposed scales and codes; fp4; fusing
into a GEMM; also writing the 16-bit output.  Nothing here is exported through the packages' `__all__` lists."""
import ctypes
import math

import torch

from . import _lib
from . import _rowargs as _ra
from . import act_mul as _act_mul
from . import add_norm as _add_norm
from . import flash_attn_interface as _fi

MODES = {"row": _lib.FA_QUANT_ROW, "group": _lib.FA_QUANT_GROUP, "static": _lib.FA_QUANT_STATIC}
GROUP = 128
MAX_N = 65536
FP8_MAX = 448.0
SCALE_FLOOR = 2.0 ** -64


def _rule(op, mode, scale, scale_ub, N):
    """(mode code, scale, has_scale_ub, scale_ub) as the blocks take them"""
    if mode not in MODES:
        raise RuntimeError(f"{op}: mode must be one of {sorted(MODES)}, got {mode!r}")
    if mode == "static":
        if scale is None:
            raise RuntimeError(f"{op}: mode='static' needs scale")
        if scale_ub is not None:
            raise RuntimeError(f"{op}: scale_ub goes with the dynamic modes, not with mode='static'")
        scale = float(scale)
        if not (0.0 < scale < math.inf):
            raise RuntimeError(f"{op}: scale must be finite and > 0, got {scale}")
        return MODES[mode], scale, 0, 0.0
    if scale is not None:
        raise RuntimeError(f"{op}: scale is given with mode='static' only (mode={mode!r} computes it)")
    if mode == "group" and N % GROUP != 0:
        raise RuntimeError(f"{op}: mode='group' needs N to be a multiple of {GROUP}, got {N}")
    if scale_ub is None:
        return MODES[mode], 0.0, 0, 0.0
    scale_ub = float(scale_ub)
    if not (0.0 < scale_ub < math.inf):
        raise RuntimeError(f"{op}: scale_ub must be finite and > 0, got {scale_ub}")
    return MODES[mode], 0.0, 1, scale_ub


def _no_grad(op, **tensors):
    if torch.is_grad_enabled():
        for name, t in tensors.items():
            if t is not None and t.requires_grad:
                raise RuntimeError(f"{op}: {name} requires grad, and {op} is not differentiable (detach it)")


def _check_n(op, x, name, max_n=MAX_N):
    if x.dtype not in _fi._DTYPES:
        raise RuntimeError(f"{op}: {name} must be fp16 or bf16, got {x.dtype}")
    if x.dim() < 1:
        raise RuntimeError(f"{op}: {name} must have at least one dimension")
    N = x.shape[-1]
    if N % 8 != 0 or not (8 <= N <= max_n):
        raise RuntimeError(f"{op}: N must be a multiple of 8 in [8, {max_n}], got {N}")
    return N


def _code_rows(t, N):
    """a codes tensor [..., N] as the [rows, N] view the kernels write: never a copy"""
    try:
        v = t if t.dim() == 2 else t.view(-1, N)
    except RuntimeError:
        v = None
    if v is None or v.stride(1) != 1 or not (v.shape[0] <= 1 or v.stride(0) >= N):
        raise RuntimeError(f"quant: out[0] needs a contiguous last dimension and rows that flatten to one stride >= N "
                           f"(got strides {tuple(t.stride())})")
    return v


def _scales_shape(like, N, mode):
    lead = tuple(like.shape[:-1])
    return lead + (N // GROUP,) if mode == "group" else lead


def _outputs(op, like, N, mode, out, codes_align=1):
    """(codes, scales, codes as [rows, N], scales or None): fresh contiguous tensors, or the caller's out=(codes, scales)"""
    sshape = _scales_shape(like, N, mode)
    if out is None:
        codes = torch.empty(like.shape, dtype=_fi._FP8, device=like.device)
        scales = None if mode == "static" else torch.empty(sshape, dtype=torch.float32, device=like.device)
        return codes, scales, codes.view(-1, N), scales
    _check_out(op, like, sshape, mode, out)
    codes, scales = out
    ci = _code_rows(codes, N)
    if codes_align > 1 and (ci.data_ptr() % codes_align or ci.stride(0) % codes_align):
        raise RuntimeError(f"{op}: out[0] must be {codes_align}-byte aligned with a row stride that is a multiple of {codes_align}")
    return codes, scales, ci, scales


def _check_out(op, like, sshape, mode, out):
    """the caller's out=(codes, scales) against the input's shape and the mode (None: nothing to check)"""
    if out is None:
        return
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise RuntimeError(f"{op}: out must be the pair (codes, scales)")
    codes, scales = out
    if codes is None or codes.dtype != _fi._FP8 or tuple(codes.shape) != tuple(like.shape):
        raise RuntimeError(f"{op}: out[0] must be float8_e4m3fn of shape {tuple(like.shape)}")
    if (scales is None) != (mode == "static"):
        raise RuntimeError(f"{op}: out[1] must be None with mode='static' and the scales tensor otherwise")
    if scales is not None and (scales.dtype != torch.float32 or tuple(scales.shape) != sshape or not scales.is_contiguous()):
        raise RuntimeError(f"{op}: out[1] must be contiguous float32 of shape {sshape}")


def _out_list(out):
    return list(out) if isinstance(out, (tuple, list)) else []


def _fill_rule(s, rule):
    s.mode, s.scale, s.has_scale_ub, s.scale_ub = rule


def quant_fp8(x, *, mode="row", scale=None, scale_ub=None, out=None):
    """(codes, scales) of x [..., N] fp16 / bf16 by the rule at the top of this module: codes float8_e4m3fn of x's shape, scales
    float32 (None with mode='static').  One launch that reads x once.  out=(codes, scales): the tensors to write."""
    op = "quant_fp8"
    N = _check_n(op, x, "x")
    rule = _rule(op, mode, scale, scale_ub, N)
    _check_out(op, x, _scales_shape(x, N, mode), mode, out)
    _no_grad(op, x=x)
    _ra.same_device(op, [x] + _out_list(out), x, "x's")
    xi = _act_mul._rows(x, N, False, "x")
    codes, scales, ci, si = _outputs(op, x, N, mode, out)
    if xi.shape[0] == 0:
        return codes, scales
    s = _lib.FaQuantFp8Params()
    s.struct_size = ctypes.sizeof(_lib.FaQuantFp8Params)
    s.x, s.x_row_stride = xi.data_ptr(), xi.stride(0)
    s.codes, s.codes_row_stride = ci.data_ptr(), ci.stride(0)
    if si is not None:
        s.scales = si.data_ptr()
    s.rows, s.n, s.dtype = xi.shape[0], N, _fi._DTYPES[x.dtype]
    _fill_rule(s, rule)
    with _fi._on_device(x.device):
        _lib.call_quant_fp8(s, _fi._stream(x.device))          # (queued: the tensors made here stay referenced until here)
    del xi, ci
    return codes, scales


def add_norm_quant(x, residual, weight, bias=None, *, eps: float = 1e-6, weight_offset: float = 0.0, is_rms_norm: bool = True,
                   prenorm: bool = False, residual_in_fp32: bool = False, inplace_residual: bool = False, mode="row", scale=None,
                   scale_ub=None, out=None):
    """(codes, scales, residual_out): `add_norm`'s forward (every option of `add_norm.add_norm_forward`; residual may be None)
    with `quant_fp8` of its output in the place of the 16-bit out - the same bits as the two calls, one launch, no 16-bit out.
    residual_out is what `add_norm_forward` returns: None without a residual and without prenorm; float32 if residual is float32
    or residual_in_fp32.  inplace_residual: residual_out is residual itself where it has residual_out's dtype."""
    op = "add_norm_quant"
    N = _add_norm._check_x(x)
    rule = _rule(op, mode, scale, scale_ub, N)
    _check_out(op, x, _scales_shape(x, N, mode), mode, out)
    if weight is None:
        raise RuntimeError(f"{op}: weight must not be None")
    _no_grad(op, x=x, residual=residual, weight=weight, bias=bias)
    w = _add_norm._param(weight, N, x.dtype, "weight")
    b = None
    if bias is not None:
        b = _add_norm._param(bias, N, x.dtype, "bias")
        if b.dtype != w.dtype:
            raise RuntimeError(f"{op}: bias must have weight's dtype ({w.dtype}), got {b.dtype}")
    if residual is not None:
        if residual.dtype not in (x.dtype, torch.float32):
            raise RuntimeError(f"{op}: residual must have x's dtype ({x.dtype}) or float32, got {residual.dtype}")
        if tuple(residual.shape) != tuple(x.shape):
            raise RuntimeError(f"{op}: residual must have x's shape {tuple(x.shape)}, got {tuple(residual.shape)}")
    eps, weight_offset = _ra.scalars(op, eps, weight_offset)
    _ra.same_device(op, [x, w, b, residual] + _out_list(out), x, "x's")

    ro_dtype = _add_norm.residual_out_dtype(x.dtype, None if residual is None else residual.dtype, residual_in_fp32)
    xi = _add_norm._rows(x, N, False, "x")
    ri = ro = roi = None
    if residual is not None:
        r_inplace = inplace_residual and residual.dtype == ro_dtype
        ri = _add_norm._rows(residual, N, r_inplace, "residual")
        if r_inplace:
            ro, roi = residual, ri
    if (residual is not None or prenorm) and ro is None:
        ro = torch.empty(x.shape, dtype=ro_dtype, device=x.device)
        roi = ro.view(-1, N)
    codes, scales, ci, si = _outputs(op, x, N, mode, out, codes_align=8)
    rows = xi.shape[0]
    if rows == 0:
        return codes, scales, ro

    io = _fi._DTYPES[x.dtype]
    s = _lib.FaAddNormQuantParams()
    s.struct_size = ctypes.sizeof(_lib.FaAddNormQuantParams)
    n = s.norm
    n.struct_size = ctypes.sizeof(_lib.FaAddNormParams)
    n.x, n.x_row_stride = xi.data_ptr(), xi.stride(0)
    if ri is not None:
        n.residual, n.residual_row_stride = ri.data_ptr(), ri.stride(0)
        n.residual_dtype = _add_norm._code(ri.dtype, io)
    if roi is not None:
        n.residual_out, n.residual_out_row_stride = roi.data_ptr(), roi.stride(0)
        n.residual_out_dtype = _add_norm._code(roi.dtype, io)
    n.weight = w.data_ptr()
    if b is not None:
        n.bias = b.data_ptr()
    n.rows, n.n, n.dtype = rows, N, io
    n.weight_dtype = _add_norm._code(w.dtype, io)
    n.is_rms_norm = 1 if is_rms_norm else 0
    n.eps, n.weight_offset = eps, weight_offset
    s.codes, s.codes_row_stride = ci.data_ptr(), ci.stride(0)
    if si is not None:
        s.scales = si.data_ptr()
    _fill_rule(s, rule)
    with _fi._on_device(x.device):
        _lib.call_add_norm_quant(s, _fi._stream(x.device))     # (queued: the tensors made here stay referenced until here)
    del xi, ri, roi, ci, w, b
    return codes, scales, ro


def act_mul_quant(gate, up=None, *, activation="silu", mode="row", scale=None, scale_ub=None, out=None):
    """(codes, scales) of act(gate) * up (up None: act(gate)) with `act_mul`'s activations: the bits of
    `quant_fp8(act_mul(gate, up, activation=activation))`, one launch, no 16-bit tensor in between.  gate, up: [..., N] fp16 /
    bf16, N a multiple of 8 up to 65536."""
    op = "act_mul_quant"
    act = _act_mul._act(activation)
    N = _check_n(op, gate, "gate")
    if up is not None and (up.dtype != gate.dtype or tuple(up.shape) != tuple(gate.shape)):
        raise RuntimeError(f"{op}: up must have gate's dtype and shape ({gate.dtype}, {tuple(gate.shape)}), got {up.dtype}, "
                           f"{tuple(up.shape)}")
    rule = _rule(op, mode, scale, scale_ub, N)
    _check_out(op, gate, _scales_shape(gate, N, mode), mode, out)
    _no_grad(op, gate=gate, up=up)
    _ra.same_device(op, [gate, up] + _out_list(out), gate, "gate's")
    gi = _act_mul._rows(gate, N, False, "gate")
    ui = None if up is None else _act_mul._rows(up, N, False, "up")
    codes, scales, ci, si = _outputs(op, gate, N, mode, out)
    if gi.shape[0] == 0:
        return codes, scales
    s = _lib.FaActMulQuantParams()
    s.struct_size = ctypes.sizeof(_lib.FaActMulQuantParams)
    s.gate, s.gate_row_stride = gi.data_ptr(), gi.stride(0)
    if ui is not None:
        s.up, s.up_row_stride = ui.data_ptr(), ui.stride(0)
    s.codes, s.codes_row_stride = ci.data_ptr(), ci.stride(0)
    if si is not None:
        s.scales = si.data_ptr()
    s.rows, s.n, s.dtype, s.activation = gi.shape[0], N, _fi._DTYPES[gate.dtype], act
    _fill_rule(s, rule)
    with _fi._on_device(gate.device):
        _lib.call_act_mul_quant(s, _fi._stream(gate.device))   # (queued: the tensors made here stay referenced until here)
    del gi, ui, ci
    return codes, scales


def act_and_mul_quant(x, *, activation="silu", mode="row", scale=None, scale_ub=None, out=None):
    """`act_mul_quant` on the halves of a packed [..., 2N] (gate first, as in vLLM): codes [..., N]"""
    _act_mul._act(activation)
    gate, up = _act_mul._halves(x)
    _no_grad("act_and_mul_quant", x=x)
    return act_mul_quant(gate, up, activation=activation, mode=mode, scale=scale, scale_ub=scale_ub, out=out)
