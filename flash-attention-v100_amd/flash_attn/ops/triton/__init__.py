"""`flash_attn.ops.triton`: upstream's module path of `layer_norm`; nothing here is Triton - the names are kept so that callers'
imports work, the implementation is the `fa_add_norm` HIP kernel."""
