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
into a GEMM; also writing the 16-bit output.  Nothing here is exported through the packages' `__all__` lists.

Weights are another matter: `quant_mxfp4` / `dequant_mxfp4` at the end of this module turn 16-bit expert weights into the MXFP4
codes and E8M0 scale bytes `moe.moe_gemm_mxfp4` reads, and back (csrc/fa_mx_quant.hip); their rule is in their docstrings."""
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


# ------------------------------------------------------------------------------------------
# MXFP4 weights: fa_mx_quant / fa_mx_dequant (csrc/fa_mx_quant.hip) - the tensors moe.moe_gemm_mxfp4 reads, made and unmade
# ------------------------------------------------------------------------------------------
MX_LAYOUTS = {"nk": _lib.FA_MOE_W_NK, "kn": _lib.FA_MOE_W_KN}
MX_SCALE_RULES = {"floor": _lib.FA_MX_SCALE_FLOOR, "rceil": _lib.FA_MX_SCALE_RCEIL}
MX_MAX_K, MX_MAX_N = 32768, 65536


def _mx_layout(op, w_layout):
    if w_layout not in MX_LAYOUTS:
        raise RuntimeError(f"{op}: w_layout must be one of {sorted(MX_LAYOUTS)}, got {w_layout!r}")
    return MX_LAYOUTS[w_layout]


def _mx_dims(op, N, K):
    if K % 32 != 0 or K > MX_MAX_K:
        raise RuntimeError(f"{op}: K must be a multiple of 32 up to {MX_MAX_K}, got {K}")
    if N % 8 != 0 or N > MX_MAX_N:
        raise RuntimeError(f"{op}: N must be a multiple of 8 up to {MX_MAX_N}, got {N}")


def _mx_experts(op, t, name, dtypes, shape=None):
    """`t` as the [E, rows, cols] view the kernels address, each expert dense, the expert stride free: never a copy"""
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
        raise RuntimeError(f"{op}: {name} must be a tensor of dtype {' or '.join(str(d) for d in dtypes)}, got "
                           f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.dim() not in (2, 3):
        raise RuntimeError(f"{op}: {name} must have 2 or 3 dimensions, got {t.dim()}")
    v = t.unsqueeze(0) if t.dim() == 2 else t
    if shape is not None and tuple(v.shape) != tuple(shape):
        raise RuntimeError(f"{op}: {name} must have shape {tuple(shape)[3 - t.dim():]}, got {tuple(t.shape)}")
    if v.numel() and not (v.stride(2) == 1 and v.stride(1) == v.shape[2] and (v.shape[0] == 1 or v.stride(0) >= v.shape[1] * v.shape[2])):
        raise RuntimeError(f"{op}: {name} needs a contiguous last dimension, dense experts and an expert stride that is at least an "
                           f"expert (got strides {tuple(t.stride())})")
    return v


def _mx_es(v):
    return v.stride(0) if v.shape[0] > 1 else v.shape[1] * v.shape[2]


def _mx_placement(op, named):
    """the C ABI's rules of place, by name and before any device work: `named` = (name, [E, rows, cols] view, alignment in bytes
    of its address and expert stride or 0); no two of the tensors may share a byte (experts interleaved in one buffer do not)"""
    spans = []
    for name, v, align in named:
        stride, row = _mx_es(v) * v.element_size(), v.shape[1] * v.shape[2] * v.element_size()
        if align and (v.data_ptr() % align or stride % align):
            raise RuntimeError(f"{op}: {name} must be {align}-byte aligned with an expert stride that is a multiple of {align} bytes "
                               f"(got address % {align} = {v.data_ptr() % align}, stride {stride} bytes)")
        spans.append((v.data_ptr(), name, stride, row, (v.shape[0] - 1) * stride + row))
    spans.sort()
    for i, (a0, na, sa, ra, ba) in enumerate(spans):
        for b0, nb, sb, rb, _ in spans[i + 1:]:
            delta = b0 - a0
            if delta < ba and not (sa == sb and ra <= delta and delta + rb <= sa):
                raise RuntimeError(f"{op}: {na} overlaps {nb}")


def quant_mxfp4(w, *, w_layout="nk", scale_rule="floor", out=None):
    """(blocks, scales) of the expert weights w, fp16 or bf16: w_layout "nk" [E, N, K] or "kn" [E, K, N] (2-D: one expert), the last
    dimension contiguous, each expert dense and 16-byte aligned (an expert stride that is a multiple of 8 elements, of 16 bytes for
    blocks; any for scales) - a view is taken as it is, never copied.  K is cut into blocks of 32.  blocks uint8
    [E, N, K / 2] and scales uint8 [E, N, K / 32] in BOTH layouts: what `moe.moe_gemm_mxfp4` reads, element k in byte k // 2, the low
    nibble for even k.  One launch (csrc/fa_mx_quant.hip).  Per block of 32 elements x_i of one weight row:
        a NaN or +-inf among them    scale byte 255 (the whole block is NaN), every code byte 0
        amax = max |x_i| = 0         scale byte 127, every code the signed zero
        else amax = m 2^e, 1 <= m < 2   scale_rule "floor" (OCP): b = e - 2 + 127; "rceil" (the smallest power of two under which
                                     nothing saturates): b = e - 2 + (m > 1.5) + 127; the byte is clamp(b, 2, 252)
        code_i                       the sign of x_i and the nearest of 0, .5, 1, 1.5, 2, 3, 4, 6 to |x_i| / 2^(byte - 127), a tie to
                                     the even code, above 6 to 6
    A row's bits depend on its 32 elements alone, and "kn" gives the bits of "nk" on the transposed weights.  out=(blocks, scales):
    the tensors to write, which may be expert-strided views.  K a multiple of 32 up to 32768, N a multiple of 8 up to 65536."""
    op = "quant_mxfp4"
    layout = _mx_layout(op, w_layout)
    if scale_rule not in MX_SCALE_RULES:
        raise RuntimeError(f"{op}: scale_rule must be one of {sorted(MX_SCALE_RULES)}, got {scale_rule!r}")
    wv = _mx_experts(op, w, "w", tuple(_fi._DTYPES))
    E = wv.shape[0]
    N, K = (wv.shape[1], wv.shape[2]) if w_layout == "nk" else (wv.shape[2], wv.shape[1])
    _mx_dims(op, N, K)
    _no_grad(op, w=w)
    lead = (E,) if w.dim() == 3 else ()
    if out is None:
        blocks = torch.empty(lead + (N, K // 2), dtype=torch.uint8, device=w.device)
        scales = torch.empty(lead + (N, K // 32), dtype=torch.uint8, device=w.device)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise RuntimeError(f"{op}: out must be the pair (blocks, scales)")
        blocks, scales = out
    bv = _mx_experts(op, blocks, "out[0]" if out is not None else "blocks", (torch.uint8,), (E, N, K // 2))
    sv = _mx_experts(op, scales, "out[1]" if out is not None else "scales", (torch.uint8,), (E, N, K // 32))
    if blocks.dim() != w.dim() or scales.dim() != w.dim():
        raise RuntimeError(f"{op}: out[0] and out[1] must have w's number of dimensions")
    if wv.numel():
        _mx_placement(op, [("w", wv, 16), ("out[0]", bv, 16), ("out[1]", sv, 0)])
    _ra.same_device(op, [w, blocks, scales], w, "w's")
    if wv.numel() == 0:
        return blocks, scales
    s = _lib.FaMxQuantParams()
    s.struct_size = ctypes.sizeof(_lib.FaMxQuantParams)
    s.w, s.blocks, s.scales = wv.data_ptr(), bv.data_ptr(), sv.data_ptr()
    s.w_expert_stride, s.blocks_expert_stride, s.scales_expert_stride = _mx_es(wv), _mx_es(bv), _mx_es(sv)
    s.num_experts, s.n, s.k = E, N, K
    s.dtype, s.layout, s.scale_rule, s.elem_format = _fi._DTYPES[w.dtype], layout, MX_SCALE_RULES[scale_rule], _lib.FA_MX_ELEM_E2M1
    with _fi._on_device(w.device):
        _lib.call_mx_quant(s, _fi._stream(w.device))          # (queued: the views made here stay referenced until here)
    del wv, bv, sv
    return blocks, scales


def dequant_mxfp4(blocks, scales, *, w_layout="nk", out=None):
    """bf16 weights e2m1(code) * 2^(scale byte - 127) of blocks uint8 [E, N, K / 2] and scales uint8 [E, N, K / 32] (2-D: one
    expert; expert-strided views are taken as they are): [E, N, K], or with w_layout "kn" [E, K, N].  One launch
    (csrc/fa_mx_quant.hip).  Exact for the scale bytes 2 .. 252 - `moe.moe_gemm_mxfp4`'s definition of a weight; byte 255 makes the
    block NaN; bytes 0, 1, 253, 254 give the formula's value rounded to bf16 (include/fa_mi355.h).  out: the tensor to write."""
    op = "dequant_mxfp4"
    layout = _mx_layout(op, w_layout)
    bv = _mx_experts(op, blocks, "blocks", (torch.uint8,))
    E, N, K = bv.shape[0], bv.shape[1], 2 * bv.shape[2]
    _mx_dims(op, N, K)
    sv = _mx_experts(op, scales, "scales", (torch.uint8,), (E, N, K // 32))
    if scales.dim() != blocks.dim():
        raise RuntimeError(f"{op}: scales must have blocks' number of dimensions")
    shape = (N, K) if w_layout == "nk" else (K, N)
    lead = (E,) if blocks.dim() == 3 else ()
    if out is None:
        out = torch.empty(lead + shape, dtype=torch.bfloat16, device=blocks.device)
    elif isinstance(out, torch.Tensor) and out.dim() != blocks.dim():
        raise RuntimeError(f"{op}: out must have blocks' number of dimensions")
    ov = _mx_experts(op, out, "out", (torch.bfloat16,), (E,) + shape)
    if ov.numel():
        _mx_placement(op, [("blocks", bv, 16), ("scales", sv, 0), ("out", ov, 16)])
    _ra.same_device(op, [blocks, scales, out], blocks, "blocks'")
    if ov.numel() == 0:
        return out
    s = _lib.FaMxDequantParams()
    s.struct_size = ctypes.sizeof(_lib.FaMxDequantParams)
    s.blocks, s.scales, s.out = bv.data_ptr(), sv.data_ptr(), ov.data_ptr()
    s.blocks_expert_stride, s.scales_expert_stride, s.out_expert_stride = _mx_es(bv), _mx_es(sv), _mx_es(ov)
    s.num_experts, s.n, s.k = E, N, K
    s.dtype, s.layout, s.elem_format = _lib.FA_BF16, layout, _lib.FA_MX_ELEM_E2M1
    with _fi._on_device(blocks.device):
        _lib.call_mx_dequant(s, _fi._stream(blocks.device))    # (queued: the views made here stay referenced until here)
    del bv, sv, ov
    return out
