"""`flash_attn.ops.triton`: upstream's module path of `layer_norm` and `cross_entropy`; nothing here is Triton - the names are kept so
that callers' imports work, the implementations are the `fa_add_norm` and `fa_cross_entropy` HIP kernels."""
