"""`flash_attn.ops`: upstream's module path for the fused norms (flash_attn.ops.rms_norm, flash_attn.ops.layer_norm,
flash_attn.ops.triton.layer_norm), served by flash_attn_mi355.add_norm (the `fa_add_norm` / `fa_add_norm_bwd` HIP kernels), and for the activations of the MLP
(flash_attn.ops.activations), served by flash_attn_mi355.act_mul (the `fa_act_mul` / `fa_act_mul_bwd` HIP kernels)."""
