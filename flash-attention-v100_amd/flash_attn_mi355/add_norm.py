"""Residual add + RMSNorm / LayerNorm over the whole hidden size in one launch, on the library's `fa_add_norm` kernel
(csrc/fa_add_norm.hip), and its backward `fa_add_norm_bwd` (csrc/fa_add_norm_bwd.hip): the other memory-bound op of a transformer
layer, what `flash_attn.ops.rms_norm` / `flash_attn.ops.layer_norm` / `flash_attn.ops.triton.layer_norm` fuse upstream and what
vLLM calls `fused_add_rms_norm`.  x is fp16 or bf16 `[..., N]`; all arithmetic is fp32:

    z            = x                                      (no residual)
    z            = round_res(float(x) + float(residual))  one fp32 add, one rounding to residual_out's dtype
    residual_out = z                                      (returned with prenorm=True; fp32 if residual is fp32 or residual_in_fp32)
    RMSNorm:   y = round16((z * rstd) * g + b)            rstd = 1 / sqrt(mean(z^2) + eps)
    LayerNorm: y = round16(((z - mean) * rstd) * g + b)   mean = mean(z), rstd = 1 / sqrt(mean((z - mean)^2) + eps), two passes
    g = weight_offset + weight                            (weight_offset 1.0: Gemma / zero-centred weights);  b: optional bias

The norm reads the STORED z, as the HF modules and vLLM do: `add_norm(x, w, residual=r)` leaves exactly the bits of
`add_norm(residual_out, w)`, and the backward recomputes mean / rstd from the saved z - the forward saves nothing else.  Every row
sum has a fixed order that depends on N alone (csrc/fa_rowsum.h): a row's bits do not depend on what else is in the batch.  For
N <= 256 an RMSNorm without bias has the bits of `qk_norm.qk_rms_norm` on a head of N columns.

The backward treats both roundings as the identity (straight-through) and sums dweight / dbias without atomics in an order that
depends on (rows, N, bias) alone: bitwise repeatable.

An fp8-quantised output in the place of the 16-bit one is `quant.add_norm_quant` (the forward only).

Not covered: dropout, rowscale / layerscale, the parallel-residual second branch (x1 / weight1 / bias1), fp32 or fp8 x,
N > 16384 or N that is not a multiple of 8, and a double backward.  Nothing here is exported through the packages' `__all__`
lists."""
import ctypes
from typing import Optional

import torch

from . import _lib
from . import _rowargs as _ra
from . import flash_attn_interface as _fi

MAX_N = 16384


def _rows(t, N, inplace, name):
    """[..., N] as the [rows, N] view the kernel takes: a view with a 16-byte friendly row stride as it is; anything else is
    copied - which in place would change the copy, so there it is an error"""
    v = t
    if t.dim() != 2:
        try:
            v = t.view(-1, N)
        except RuntimeError:
            v = None
    if v is not None and v.stride(1) == 1 and v.stride(0) % 8 == 0 and v.data_ptr() % 16 == 0 \
            and (v.shape[0] <= 1 or v.stride(0) >= N):
        return v
    if inplace:
        raise RuntimeError(f"add_norm: in place needs a 16-byte aligned {name} with a contiguous last dimension whose rows flatten "
                           f"to one stride that is a multiple of 8 elements (got strides {tuple(t.stride())})")
    return t.contiguous().view(-1, N)


def _param(w, N, dtype, name):
    return _ra.weight("add_norm", w, N, dtype, name, of="x", dim="N")


def _check_x(x, name="x"):
    if x.dtype not in _fi._DTYPES:
        raise RuntimeError(f"add_norm: {name} must be fp16 or bf16, got {x.dtype}")
    if x.dim() < 1:
        raise RuntimeError(f"add_norm: {name} must have at least one dimension")
    N = x.shape[-1]
    if N % 8 != 0 or not (8 <= N <= MAX_N):
        raise RuntimeError(f"add_norm: the hidden size must be a multiple of 8 in [8, {MAX_N}], got {N}")
    return N


def _code(dtype, io):
    return _lib.FA_FP32 if dtype == torch.float32 else io


def residual_out_dtype(x_dtype, residual_dtype, residual_in_fp32):
    """fp32 if the residual is fp32 or residual_in_fp32, x's dtype otherwise"""
    return torch.float32 if (residual_dtype == torch.float32 or residual_in_fp32) else x_dtype


def add_norm_forward(x, weight, bias=None, residual=None, *, eps: float = 1e-6, weight_offset: float = 0.0, is_rms_norm: bool = True,
                     prenorm: bool = False, residual_in_fp32: bool = False, inplace: bool = False):
    """The forward alone, no autograd: (out, residual_out).  residual_out is None without a residual and without prenorm.
    inplace: out is x itself, and residual_out is residual itself where it has residual_out's dtype."""
    N = _check_x(x)
    if weight is None:
        raise RuntimeError("add_norm: weight must not be None")
    w = _param(weight, N, x.dtype, "weight")
    b = None
    if bias is not None:
        b = _param(bias, N, x.dtype, "bias")
        if b.dtype != w.dtype:
            raise RuntimeError(f"add_norm: bias must have weight's dtype ({w.dtype}), got {b.dtype}")
    if residual is not None:
        if residual.dtype not in (x.dtype, torch.float32):
            raise RuntimeError(f"add_norm: residual must have x's dtype ({x.dtype}) or float32, got {residual.dtype}")
        if tuple(residual.shape) != tuple(x.shape):
            raise RuntimeError(f"add_norm: residual must have x's shape {tuple(x.shape)}, got {tuple(residual.shape)}")
    eps, weight_offset = _ra.scalars("add_norm", eps, weight_offset)
    _ra.same_device("add_norm", [x, w, b, residual], x, "x's")

    ro_dtype = residual_out_dtype(x.dtype, None if residual is None else residual.dtype, residual_in_fp32)
    want_ro = residual is not None or prenorm
    xi = _rows(x, N, inplace, "x")
    out = x if inplace else torch.empty(x.shape, dtype=x.dtype, device=x.device)
    oi = xi if inplace else out.view(-1, N)
    ri = ro = roi = None
    if residual is not None:
        r_inplace = inplace and residual.dtype == ro_dtype
        ri = _rows(residual, N, r_inplace, "residual")
        if r_inplace:
            ro, roi = residual, ri
    if want_ro and ro is None:
        ro = torch.empty(x.shape, dtype=ro_dtype, device=x.device)
        roi = ro.view(-1, N)
    rows = xi.shape[0]
    if rows == 0:
        return out, ro

    io = _fi._DTYPES[x.dtype]
    s = _lib.FaAddNormParams()
    s.struct_size = ctypes.sizeof(_lib.FaAddNormParams)
    s.x, s.x_row_stride = xi.data_ptr(), xi.stride(0)
    s.out, s.out_row_stride = oi.data_ptr(), oi.stride(0)
    if ri is not None:
        s.residual, s.residual_row_stride = ri.data_ptr(), ri.stride(0)
        s.residual_dtype = _code(ri.dtype, io)
    if roi is not None:
        s.residual_out, s.residual_out_row_stride = roi.data_ptr(), roi.stride(0)
        s.residual_out_dtype = _code(roi.dtype, io)
    s.weight = w.data_ptr()
    if b is not None:
        s.bias = b.data_ptr()
    s.rows, s.n, s.dtype = rows, N, io
    s.weight_dtype = _code(w.dtype, io)
    s.is_rms_norm = 1 if is_rms_norm else 0
    s.eps, s.weight_offset = eps, weight_offset
    with _fi._on_device(x.device):
        _lib.call_add_norm(s, _fi._stream(x.device))           # (queued: the tensors made here stay referenced until here)
    del xi, oi, ri, roi, w, b
    return out, ro


def add_norm_backward(dy, z, weight, dres_out=None, *, eps: float = 1e-6, weight_offset: float = 0.0, is_rms_norm: bool = True,
                      dres_dtype: Optional[torch.dtype] = None, inplace: bool = False, need_dx: bool = True, need_dres: bool = False,
                      need_dw: bool = True, need_db: bool = False):
    """The backward of `add_norm`, one launch (two with a weight or bias gradient): dy [..., N] (fp16 / bf16) is the gradient of
    out, z the forward's residual_out (x itself where the forward had no residual; dy's dtype or float32), dres_out the gradient of
    residual_out under prenorm (z's dtype) or None; weight, eps, weight_offset, is_rms_norm are the forward's.
        a = dy g, xhat = z rstd (LayerNorm: (z - mean) rstd);  RMSNorm: dz = rstd (a - xhat mean(a xhat));
        LayerNorm: dz = rstd ((a - mean(a)) - xhat mean(a xhat));  dz += dres_out;  dweight = sum_rows dy xhat,  dbias = sum_rows dy
    with both roundings of the forward treated as the identity.  dx = round16(dz) has dy's dtype; dres = dz rounded to dres_dtype
    (the forward residual's dtype; default dy's) is the residual's gradient - where the two dtypes agree they hold the same bits,
    and a caller may ask for dx alone and use it for both.  inplace: dx is dy, rewritten where it is.  need_*=False skips that
    output (None in its place).  Returns (dx, dres, dweight, dbias); dweight / dbias have weight's dtype."""
    N = _check_x(dy, "dy")
    if z.dtype not in (dy.dtype, torch.float32) or tuple(z.shape) != tuple(dy.shape):
        raise RuntimeError(f"add_norm: z must have dy's shape {tuple(dy.shape)} and dy's dtype ({dy.dtype}) or float32, got "
                           f"{tuple(z.shape)} / {z.dtype}")
    if dres_out is not None and (dres_out.dtype != z.dtype or tuple(dres_out.shape) != tuple(dy.shape)):
        raise RuntimeError(f"add_norm: dres_out must have z's dtype and shape ({z.dtype}, {tuple(z.shape)})")
    dres_dtype = dy.dtype if dres_dtype is None else dres_dtype
    if dres_dtype not in (dy.dtype, torch.float32):
        raise RuntimeError(f"add_norm: dres_dtype must be dy's dtype ({dy.dtype}) or float32, got {dres_dtype}")
    if weight is None:
        raise RuntimeError("add_norm: weight must not be None")
    w = _param(weight, N, dy.dtype, "weight")
    eps, weight_offset = _ra.scalars("add_norm", eps, weight_offset)
    _ra.same_device("add_norm", [dy, z, dres_out, w], dy, "dy's")

    dev = dy.device
    dyi = _rows(dy, N, inplace and need_dx, "dy")
    zi = _rows(z, N, False, "z")
    droi = None if dres_out is None else _rows(dres_out, N, False, "dres_out")
    dx = dxi = dres = dresi = None
    if need_dx:
        dx = dy if inplace else torch.empty(dy.shape, dtype=dy.dtype, device=dev)
        dxi = dyi if inplace else dx.view(-1, N)
    if need_dres:
        dres = torch.empty(dy.shape, dtype=dres_dtype, device=dev)
        dresi = dres.view(-1, N)
    dw = torch.empty(N, dtype=w.dtype, device=dev) if need_dw else None
    db = torch.empty(N, dtype=w.dtype, device=dev) if need_db else None
    if dx is None and dres is None and dw is None and db is None:
        return None, None, None, None
    rows = dyi.shape[0]
    if rows == 0:                                              # (nothing to launch: a sum over no rows is zero)
        for g in (dw, db):
            if g is not None:
                g.zero_()
        return dx, dres, dw, db

    io = _fi._DTYPES[dy.dtype]
    s = _lib.FaAddNormBwdParams()
    s.struct_size = ctypes.sizeof(_lib.FaAddNormBwdParams)
    s.dy, s.dy_row_stride = dyi.data_ptr(), dyi.stride(0)
    s.z, s.z_row_stride = zi.data_ptr(), zi.stride(0)
    if droi is not None:
        s.dres_out, s.dres_out_row_stride = droi.data_ptr(), droi.stride(0)
    if dxi is not None:
        s.dx, s.dx_row_stride = dxi.data_ptr(), dxi.stride(0)
    if dresi is not None:
        s.dres, s.dres_row_stride = dresi.data_ptr(), dresi.stride(0)
    s.weight = w.data_ptr()
    if dw is not None:
        s.dweight = dw.data_ptr()
    if db is not None:
        s.dbias = db.data_ptr()
    s.rows, s.n, s.dtype = rows, N, io
    s.z_dtype, s.dres_dtype, s.weight_dtype = _code(zi.dtype, io), _code(dres_dtype, io), _code(w.dtype, io)
    s.is_rms_norm = 1 if is_rms_norm else 0
    s.eps, s.weight_offset = eps, weight_offset
    nbytes = _lib.add_norm_bwd_workspace_bytes(s)
    ws = _fi._workspace(nbytes, dev)
    if ws is not None:
        s.workspace, s.workspace_bytes = ws.data_ptr(), nbytes
    with _fi._on_device(dev):
        _lib.call_add_norm_bwd(s, _fi._stream(dev))            # (queued: the tensors made here stay referenced until here)
    del dyi, zi, droi, dxi, dresi, w, ws
    return dx, dres, dw, db


def add_norm(x, weight, bias=None, residual=None, *, eps: float = 1e-6, weight_offset: float = 0.0, is_rms_norm: bool = True,
             prenorm: bool = False, residual_in_fp32: bool = False, inplace: bool = False):
    """out = norm(x + residual) (RMSNorm, or LayerNorm with is_rms_norm=False) with the formulas at the top of this module.
    x: [..., N] fp16 / bf16; weight, bias: (N,) of x's dtype or float32 (bias optional, weight's dtype); residual: x's shape, x's
    dtype or float32, or None.  Returns out, or (out, residual_out) with prenorm=True; residual_out is float32 if residual is
    float32 or residual_in_fp32, else x's dtype, and without a residual it is x (converted).
    Differentiable in x, residual, weight and bias (`add_norm_backward`); no double backward.
    inplace=True: out is x itself and, where the dtypes agree, residual_out is residual itself (vLLM's fused_add_rms_norm);
    no autograd."""
    _fi._check_device(x, weight, bias, residual)
    if inplace:
        out, ro = add_norm_forward(x, weight, bias, residual, eps=eps, weight_offset=weight_offset, is_rms_norm=is_rms_norm,
                                   prenorm=prenorm, residual_in_fp32=residual_in_fp32, inplace=True)
    else:
        from . import torch_ops as _ops                        # (registers torch.ops.flash_attn_mi355.add_norm)
        out, ro = _ops.add_norm(x, weight, bias, residual, float(eps), float(weight_offset), bool(is_rms_norm), bool(prenorm),
                                bool(residual_in_fp32))
    return (out, ro) if prenorm else out


def fused_add_rms_norm_(x, residual, weight, eps: float = 1e-6):
    """vLLM's fused_add_rms_norm, in place: residual <- x + residual (rounded to residual's dtype), x <- RMSNorm(residual) weight.
    residual must have x's dtype or float32.  Returns (x, residual), the tensors themselves."""
    if residual is None:
        raise RuntimeError("add_norm: fused_add_rms_norm_ needs a residual")
    from . import torch_ops as _ops
    _fi._check_device(x, residual, weight)
    _ops.add_norm_(x, residual, weight, None, float(eps), 0.0, True)
    return x, residual
