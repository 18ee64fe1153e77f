"""`flash_attn.losses.cross_entropy` with upstream's names and argument lists, served by flash_attn_mi355.cross_entropy (the
`fa_cross_entropy` / `fa_cross_entropy_bwd` HIP kernels).  `process_group` and `precomputed_lse` are not served and raise a
RuntimeError that names the argument."""
import torch

from flash_attn.ops.triton.cross_entropy import cross_entropy_loss


class CrossEntropyLoss(torch.nn.Module):
    def __init__(self, ignore_index=-100, reduction="mean", label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0,
                 inplace_backward=False, process_group=None, return_z_loss=False):
        """lse_square_scale: the z-loss weight (0 disables it); inplace_backward: the backward writes the gradient over the
        logits; return_z_loss: forward returns (loss, z_loss), the z-loss reduced like the loss and without a gradient."""
        super().__init__()
        if reduction not in ["mean", "none", "sum"]:
            raise NotImplementedError("Only support reduction = 'mean' or 'none' or 'sum'")
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.label_smoothing = label_smoothing
        self.logit_scale = logit_scale
        self.lse_square_scale = lse_square_scale
        self.inplace_backward = inplace_backward
        self.process_group = process_group
        self.return_z_loss = return_z_loss

    def forward(self, input, target, precomputed_lse=None):
        """input (batch, vocab), target (batch,) -> the loss, reduced as `reduction` says ("mean": over the targets that are not
        ignore_index, counted on the device), or (loss, z_loss) with return_z_loss"""
        loss, z_loss = cross_entropy_loss(input, target, precomputed_lse=precomputed_lse, label_smoothing=self.label_smoothing,
                                          logit_scale=self.logit_scale, lse_square_scale=self.lse_square_scale,
                                          ignore_index=self.ignore_index, inplace_backward=self.inplace_backward,
                                          process_group=self.process_group)
        if self.reduction == "mean":
            n = (target != self.ignore_index).sum()
            loss = loss.sum() / n
            if self.return_z_loss:                            # (not reduced where nobody looks at it: two launches less)
                z_loss = z_loss.sum() / n
        elif self.reduction == "sum":
            loss = loss.sum()
            if self.return_z_loss:
                z_loss = z_loss.sum()
        return (loss, z_loss) if self.return_z_loss else loss
