"""`flash_attn.ops.triton.cross_entropy` with upstream's name and argument list; nothing here is Triton - the implementation is the
`fa_cross_entropy` / `fa_cross_entropy_bwd` HIP kernels (flash_attn_mi355.cross_entropy).  The vocabulary-parallel form is not
served: a `process_group` or a `precomputed_lse` raises a RuntimeError that names the argument."""
from flash_attn_mi355 import cross_entropy as _ce


def unsupported(name, why):
    raise RuntimeError(f"flash_attn_mi355: argument `{name}` is not supported by the fused cross-entropy ({why})")


def cross_entropy_loss(logits, labels, precomputed_lse=None, label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0,
                       ignore_index=-100, inplace_backward=False, process_group=None):
    """logits (batch, vocab) fp16 / bf16 / fp32, labels (batch,) -> (losses, z_losses), fp32 (batch,); losses already include
    z_losses = lse_square_scale * lse^2, and z_losses carries no gradient.  label_smoothing in [0, 1); logit_scale multiplies the
    logits before the loss; a label equal to ignore_index gives a loss of 0; inplace_backward writes the gradient over the
    logits."""
    if process_group is not None:
        unsupported("process_group", "the vocabulary-parallel loss is not built; gather the logits")
    if precomputed_lse is not None:
        unsupported("precomputed_lse", "the forward computes lse itself")
    return _ce.cross_entropy(logits, labels, label_smoothing=label_smoothing, logit_scale=logit_scale,
                             lse_square_scale=lse_square_scale, ignore_index=ignore_index, inplace_backward=inplace_backward)
