"""What the upstream-named norm modules share: the arguments that are not served, and the call into flash_attn_mi355.add_norm."""
import torch

from flash_attn_mi355 import add_norm as _an


def unsupported(name, why):
    raise RuntimeError(f"flash_attn_mi355: argument `{name}` is not supported by the fused norm ({why})")


def check_dropout(dropout_p, rowscale=None, layerscale=None, return_dropout_mask=False):
    if dropout_p != 0.0:
        unsupported("dropout_p", f"got {dropout_p}; dropout is not fused - modules pass 0 in eval mode")
    if rowscale is not None:
        unsupported("rowscale", "row scaling is not fused")
    if layerscale is not None:
        unsupported("layerscale", "layer scaling is not fused")
    if return_dropout_mask:
        unsupported("return_dropout_mask", "there is no dropout")


def norm(x, weight, bias, residual, eps, prenorm, residual_in_fp32, is_rms_norm, weight_offset=0.0, out=None, residual_out=None):
    """add_norm with upstream's return convention (out, or (out, residual_out) with prenorm) and optional caller-owned outputs"""
    if weight is None:
        unsupported("weight", "a norm without a weight is not served; pass ones")
    if out is None and residual_out is None:
        return _an.add_norm(x, weight, bias, residual, eps=eps, weight_offset=weight_offset, is_rms_norm=is_rms_norm,
                            prenorm=prenorm, residual_in_fp32=residual_in_fp32)
    ro_dtype = _an.residual_out_dtype(x.dtype, None if residual is None else residual.dtype, residual_in_fp32)
    if out is not None and (out.dtype != x.dtype or tuple(out.shape) != tuple(x.shape)):
        raise RuntimeError(f"flash_attn_mi355: `out` must have x's dtype and shape ({x.dtype}, {tuple(x.shape)})")
    if residual_out is not None and (residual_out.dtype != ro_dtype or tuple(residual_out.shape) != tuple(x.shape)):
        raise RuntimeError(f"flash_attn_mi355: `residual_out` must have dtype {ro_dtype} and x's shape {tuple(x.shape)}")
    want_ro = prenorm or residual_out is not None
    res = _an.add_norm(x, weight, bias, residual, eps=eps, weight_offset=weight_offset, is_rms_norm=is_rms_norm,
                       prenorm=want_ro, residual_in_fp32=residual_in_fp32)
    y, ro = res if want_ro else (res, None)
    if out is not None:
        y = out.copy_(y)
    if residual_out is not None:
        ro = residual_out.copy_(ro)
    return (y, ro) if prenorm else y


def param(n, value, device, dtype):
    return torch.nn.Parameter(torch.full((n,), value, device=device, dtype=dtype))
