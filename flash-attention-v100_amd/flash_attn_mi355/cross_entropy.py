"""Softmax cross-entropy over the vocabulary with its backward, on the library's `fa_cross_entropy` / `fa_cross_entropy_bwd`
kernels (csrc/fa_cross_entropy.hip): what upstream ships as `flash_attn.losses.cross_entropy.CrossEntropyLoss` and
`flash_attn.ops.triton.cross_entropy.cross_entropy_loss`.  logits are fp16, bf16 or fp32 `[..., V]`, labels int64 (or int32)
`[...]`; the logits are read once forward, read and written once backward, and never copied to fp32.  All arithmetic is fp32, in
exactly this order (ls = label_smoothing, z = lse_square_scale; `1 - ls` and `ls / V` are fp32 operations on the host):

    l_j     = logit_scale * float(x_j)                              one rounding
    lse     = m + log(s),   m = max_j l_j,  s = sum_j exp(l_j - m)  a running (m, s) in a fixed order (csrc/fa_lse.h)
    loss    = fma(-(1 - ls), l_label, lse)                          ls == 0: lse - l_label
    loss    = fma(-(ls / V), sum_j l_j, loss)                       only with ls > 0; sum_j l_j is not formed otherwise
    z_loss  = (z * lse) * lse;   loss = loss + z_loss
    g       = dloss * logit_scale;   F = fma(2 z, lse, 1);   p_j = exp(l_j - lse)
    dx_j    = round_x(g * (((p_j * F) - (1 - ls) [j == label]) - ls / V))

exp(t) is exp2(t * log2(e)) on the hardware's exp2 (fp32 product, then v_exp_f32); log is the library logf.  The forward saves
`lse` and nothing else; the backward recomputes nothing but p_j.

Corner cases, all defined, none a fault or a host synchronisation: label == ignore_index gives loss = z_loss = +0 and a dx row of
+0 (lse is still written); a label outside [0, V) gives loss = z_loss = NaN and a NaN dx row (the label is only compared, never
used as an address); x_j = -inf (a masked vocabulary entry) adds exactly 0 to s and to sum_j l_j and has p_j = 0; a row that is
-inf throughout, or holds +inf or a NaN, has lse = NaN (what the formulas give literally).  rows == 0 returns empty outputs
without a launch.

A row's bits depend on (V, dtype) and the row's values alone - not on the number of rows, the row's index, its address alignment
(GPT-2's V = 50257 makes every odd row misaligned: it is read element by element, the same values) or the device.

Not covered: vocabulary-parallel `process_group` and `precomputed_lse`, computing the gradient inside the forward (Liger's
form), fusing the LM-head GEMM, class weights, fp8 logits, and a double backward.  Nothing here is exported through the packages'
`__all__` lists."""
import ctypes

import torch

from . import _lib
from . import _rowargs as _ra
from . import flash_attn_interface as _fi

_OP = "cross_entropy"
_CODES = {torch.float16: _lib.FA_FP16, torch.bfloat16: _lib.FA_BF16, torch.float32: _lib.FA_FP32}


def _rows(t, V, inplace):
    """[..., V] as the [rows, V] view the kernels take: a view whose last dimension is contiguous and whose rows flatten to one
    stride >= V as it is (a `[:, :V]` view of a padded buffer included); anything else is copied - which in place would change
    the copy, so there it is an error"""
    v = t
    if t.dim() != 2:
        try:
            v = t.view(-1, V)
        except RuntimeError:
            v = None
    if v is not None and v.stride(1) == 1 and (v.shape[0] <= 1 or v.stride(0) >= V):
        return v
    if inplace:
        raise RuntimeError(f"{_OP}: in place needs logits with a contiguous last dimension whose rows flatten to one stride "
                           f"(got strides {tuple(t.stride())}); pass inplace=False")
    return t.contiguous().view(-1, V)


def _check(logits, labels):
    """(V, labels as int64 [rows])"""
    if logits.dtype not in _CODES:
        raise RuntimeError(f"{_OP}: logits must be fp16, bf16 or fp32, got {logits.dtype}")
    if logits.dim() < 1 or logits.shape[-1] < 1:
        raise RuntimeError(f"{_OP}: logits must be [..., V] with V >= 1, got {tuple(logits.shape)}")
    if tuple(labels.shape) != tuple(logits.shape[:-1]):
        raise RuntimeError(f"{_OP}: labels must have logits' leading shape {tuple(logits.shape[:-1])}, got {tuple(labels.shape)}")
    rows = labels.numel()
    return logits.shape[-1], _ra.ids(_OP, labels.reshape(-1), rows, "labels")


def _fill_common(s, xi, lab, V, scalars):
    s.logits, s.logits_row_stride = xi.data_ptr(), xi.stride(0)
    s.labels = lab.data_ptr()
    s.rows, s.vocab, s.dtype = xi.shape[0], V, _CODES[xi.dtype]
    s.label_smoothing, s.logit_scale, s.lse_square_scale, s.ignore_index = scalars


def cross_entropy_forward(logits, labels, *, label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100):
    """The forward alone, no autograd: (losses, z_losses, lse), fp32 of labels' shape.  One launch where the vocabulary fits one
    chunk, two (partials, then their merge) otherwise; the logits are taken as the view they are."""
    V, lab = _check(logits, labels)
    scalars = _ra.loss_scalars(_OP, label_smoothing, logit_scale, lse_square_scale, ignore_index)
    _ra.same_device(_OP, [logits, labels], logits, "logits'")
    dev = logits.device
    xi = _rows(logits, V, False)
    rows = xi.shape[0]
    losses, z_losses, lse = (torch.empty(labels.shape, dtype=torch.float32, device=dev) for _ in range(3))
    if rows == 0:
        return losses, z_losses, lse
    s = _lib.FaCrossEntropyParams()
    s.struct_size = ctypes.sizeof(_lib.FaCrossEntropyParams)
    _fill_common(s, xi, lab, V, scalars)
    s.losses, s.z_losses, s.lse = losses.data_ptr(), z_losses.data_ptr(), lse.data_ptr()
    nbytes = _lib.cross_entropy_workspace_bytes(s)
    ws = _fi._workspace(nbytes, dev)
    if ws is not None:
        s.workspace, s.workspace_bytes = ws.data_ptr(), nbytes
    with _fi._on_device(dev):
        _lib.call_cross_entropy(s, _fi._stream(dev))           # (queued: the tensors made here stay referenced until here)
    del xi, lab, ws
    return losses, z_losses, lse


def cross_entropy_backward(dlosses, logits, labels, lse, *, label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0,
                           ignore_index=-100, inplace=False):
    """dlogits (logits' dtype and shape) from dlosses (labels' shape; a broadcast view is taken with its stride 0, no copy), the
    forward's logits, labels and lse and the forward's scalars: one launch, no workspace.  inplace: dlogits is the logits
    tensor itself, rewritten where it is - nothing is allocated."""
    V, lab = _check(logits, labels)
    scalars = _ra.loss_scalars(_OP, label_smoothing, logit_scale, lse_square_scale, ignore_index)
    if tuple(dlosses.shape) != tuple(labels.shape) or tuple(lse.shape) != tuple(labels.shape):
        raise RuntimeError(f"{_OP}: dlosses and lse must have labels' shape {tuple(labels.shape)}, got {tuple(dlosses.shape)} / "
                           f"{tuple(lse.shape)}")
    if dlosses.dtype != torch.float32 or lse.dtype != torch.float32:
        raise RuntimeError(f"{_OP}: dlosses and lse must be float32, got {dlosses.dtype} / {lse.dtype}")
    _ra.same_device(_OP, [dlosses, logits, labels, lse], logits, "logits'")
    dev = logits.device
    xi = _rows(logits, V, inplace)
    rows = xi.shape[0]
    dx = logits if inplace else torch.empty(logits.shape, dtype=logits.dtype, device=dev)
    dxi = xi if inplace else dx.view(-1, V)
    if rows == 0:
        return dx
    dl = dlosses
    if dl.dim() != 1:
        try:
            dl = dl.view(-1)                                   # (an expanded scalar flattens to stride 0)
        except RuntimeError:
            dl = dl.reshape(-1)
    if dl.stride(0) < 0:
        dl = dl.contiguous()
    lsei = lse.reshape(-1).contiguous()
    s = _lib.FaCrossEntropyBwdParams()
    s.struct_size = ctypes.sizeof(_lib.FaCrossEntropyBwdParams)
    _fill_common(s, xi, lab, V, scalars)
    s.dlosses, s.dlosses_stride = dl.data_ptr(), dl.stride(0)
    s.lse = lsei.data_ptr()
    s.dlogits, s.dlogits_row_stride = dxi.data_ptr(), dxi.stride(0)
    with _fi._on_device(dev):
        _lib.call_cross_entropy_bwd(s, _fi._stream(dev))       # (queued: the tensors made here stay referenced until here)
    del xi, dxi, lab, dl, lsei
    return dx


def cross_entropy(logits, labels, *, label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100,
                  inplace_backward=False):
    """(losses, z_losses) with the formulas at the top of this module; losses already include z_losses.  Differentiable in the
    logits (`cross_entropy_backward`); z_losses and the labels are not differentiable; no double backward.
    inplace_backward=True: the backward writes the gradient over the logits (they must not be used afterwards) and allocates
    nothing."""
    _fi._check_device(logits, labels)
    from . import torch_ops as _ops                            # (registers torch.ops.flash_attn_mi355.cross_entropy)
    losses, z_losses, _ = _ops.cross_entropy(logits, labels, float(label_smoothing), float(logit_scale), float(lse_square_scale),
                                             int(ignore_index), bool(inplace_backward))
    return losses, z_losses
