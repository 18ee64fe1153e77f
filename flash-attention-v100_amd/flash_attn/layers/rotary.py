"""`flash_attn.layers.rotary` with upstream's names: the implementation is flash_attn_mi355/rotary.py (the `fa_rotary` HIP kernel)."""
from flash_attn_mi355.rotary import (  # noqa: F401
    RotaryEmbedding,
    apply_rotary,
    apply_rotary_emb,
    apply_rotary_emb_func,
    apply_rotary_emb_kv_,
    apply_rotary_emb_qkv_,
)

__all__ = ["apply_rotary_emb", "apply_rotary_emb_func", "apply_rotary_emb_qkv_", "apply_rotary_emb_kv_", "RotaryEmbedding"]
