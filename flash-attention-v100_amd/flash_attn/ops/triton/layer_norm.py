"""`flash_attn.ops.triton.layer_norm` with upstream's names and argument lists (`layer_norm_fn`, `rms_norm_fn`, `RMSNorm`), served
by flash_attn_mi355.add_norm (the `fa_add_norm` / `fa_add_norm_bwd` HIP kernels; no Triton).  Not served - a RuntimeError names
the argument: a non-zero dropout_p, rowscale, the parallel-residual branch x1 / weight1 / bias1, return_dropout_mask=True and an
out_dtype other than x's."""
import torch

from .. import _norm


def layer_norm_fn(x, weight, bias, residual=None, x1=None, weight1=None, bias1=None, eps=1e-6, dropout_p=0.0, rowscale=None,
                  prenorm=False, residual_in_fp32=False, zero_centered_weight=False, is_rms_norm=False, return_dropout_mask=False,
                  out_dtype=None, out=None, residual_out=None):
    _norm.check_dropout(dropout_p, rowscale, None, return_dropout_mask)
    for name, t in (("x1", x1), ("weight1", weight1), ("bias1", bias1)):
        if t is not None:
            _norm.unsupported(name, "the parallel-residual second branch is not fused")
    if out_dtype is not None and out_dtype != x.dtype:
        _norm.unsupported("out_dtype", f"out has x's dtype {x.dtype}, got {out_dtype}")
    return _norm.norm(x, weight, bias, residual, eps, prenorm, residual_in_fp32, is_rms_norm,
                      weight_offset=1.0 if zero_centered_weight else 0.0, out=out, residual_out=residual_out)


def rms_norm_fn(x, weight, bias, residual=None, x1=None, weight1=None, bias1=None, eps=1e-6, dropout_p=0.0, rowscale=None,
                prenorm=False, residual_in_fp32=False, zero_centered_weight=False, return_dropout_mask=False, out_dtype=None,
                out=None, residual_out=None):
    return layer_norm_fn(x, weight, bias, residual, x1, weight1, bias1, eps, dropout_p, rowscale, prenorm, residual_in_fp32,
                         zero_centered_weight, True, return_dropout_mask, out_dtype, out, residual_out)


class RMSNorm(torch.nn.Module):
    def __init__(self, hidden_size, eps=1e-5, dropout_p=0.0, zero_centered_weight=False, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.drop = torch.nn.Dropout(dropout_p) if dropout_p > 0.0 else None
        self.zero_centered_weight = zero_centered_weight
        self.weight = _norm.param(hidden_size, 0.0 if zero_centered_weight else 1.0, device, dtype)
        self.register_parameter("bias", None)

    def reset_parameters(self):
        if self.zero_centered_weight:
            torch.nn.init.zeros_(self.weight)
        else:
            torch.nn.init.ones_(self.weight)

    def forward(self, x, residual=None, prenorm=False, residual_in_fp32=False):
        return rms_norm_fn(x, self.weight, self.bias, residual=residual, eps=self.eps,
                           dropout_p=self.drop.p if self.drop is not None and self.training else 0.0, prenorm=prenorm,
                           residual_in_fp32=residual_in_fp32, zero_centered_weight=self.zero_centered_weight)
