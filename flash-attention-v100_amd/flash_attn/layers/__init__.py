"""`flash_attn.layers`: upstream's module path for the rotary embedding layer (flash_attn.layers.rotary)."""
