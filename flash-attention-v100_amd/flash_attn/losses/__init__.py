"""`flash_attn.losses`: upstream's module path for the fused cross-entropy loss (flash_attn.losses.cross_entropy)."""
