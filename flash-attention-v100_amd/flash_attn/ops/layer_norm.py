"""`flash_attn.ops.layer_norm` with upstream's names and argument lists: the fused dropout-add-norm extension's LayerNorm entry
points, served by flash_attn_mi355.add_norm (the `fa_add_norm` / `fa_add_norm_bwd` HIP kernels).  Dropout, rowscale and layerscale
are not fused: a non-zero dropout_p, rowscale, layerscale or return_dropout_mask=True raise a RuntimeError that names the argument."""
import torch

from . import _norm


def layer_norm(x, weight, bias, epsilon):
    return _norm.norm(x, weight, bias, None, epsilon, False, False, False)


def dropout_add_layer_norm(x0, residual, weight, bias, dropout_p, epsilon, rowscale=None, layerscale=None, prenorm=False,
                           residual_in_fp32=False, return_dropout_mask=False):
    """residual_in_fp32 only has an effect if residual is None: otherwise the residual's dtype is residual.dtype"""
    _norm.check_dropout(dropout_p, rowscale, layerscale, return_dropout_mask)
    return _norm.norm(x0, weight, bias, residual, epsilon, prenorm, residual_in_fp32, False)


class DropoutAddLayerNorm(torch.nn.Module):
    def __init__(self, hidden_size, prenorm=False, p=0.0, eps=1e-5, residual_in_fp32=False, device=None, dtype=None):
        super().__init__()
        self.prenorm = prenorm
        self.p = p
        self.eps = eps
        self.residual_in_fp32 = residual_in_fp32
        self.weight = _norm.param(hidden_size, 1.0, device, dtype)
        self.bias = _norm.param(hidden_size, 0.0, device, dtype)

    def reset_parameters(self):
        torch.nn.init.ones_(self.weight)
        torch.nn.init.zeros_(self.bias)

    def forward(self, x0, residual=None):
        return dropout_add_layer_norm(x0, residual, self.weight, self.bias, self.p if self.training else 0.0, self.eps,
                                      prenorm=self.prenorm, residual_in_fp32=self.residual_in_fp32)
