"""ctypes binding of libfa_mi355.so (the C ABI in include/fa_mi355.h).

The library is the product: there is NO CPU / PyTorch fallback.  If it is missing or does
not match the header this module raises at import time."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FA_MI355_LIB") or os.path.join(_HERE, "libfa_mi355.so")   # env: A/B experiment builds

FA_FP16, FA_BF16, FA_FP8_E4M3, FA_FP32 = 0, 1, 2, 3
FA_ABI_VERSION = 4
FA_FLAG_KEEP_WINDOW = 1
FA_FLAG_NO_DKV_SPLIT = 2
FA_FLAG_DS_HANDOFF = 4
FA_FLAG_FWD_KEY_SPLIT = 8
FA_FLAG_TREE_MASK = 16
FA_ACT_SILU, FA_ACT_GELU, FA_ACT_GELU_TANH, FA_ACT_RELU, FA_ACT_RELU2 = 0, 1, 2, 3, 4    # enum fa_act
FA_QUANT_ROW, FA_QUANT_GROUP, FA_QUANT_STATIC = 0, 1, 2                                  # enum fa_quant_mode
FA_MOE_SOFTMAX, FA_MOE_SIGMOID = 0, 1                                                    # enum fa_moe_scoring
FA_MOE_W_NK, FA_MOE_W_KN = 0, 1                                                          # enum fa_moe_w_layout

_i64, _i32, _f32, _u64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_uint64
_ptr = ctypes.c_void_p


class FaParams(ctypes.Structure):
    """Mirror of `struct fa_params` - field order MUST match include/fa_mi355.h
    (checked against the header by tests/test_abi.py and against sizeof at load)."""
    _fields_ = [
        ("q", _ptr), ("k", _ptr), ("v", _ptr), ("o", _ptr), ("lse", _ptr),
        ("q_batch_stride", _i64), ("q_row_stride", _i64), ("q_head_stride", _i64),
        ("k_batch_stride", _i64), ("k_row_stride", _i64), ("k_head_stride", _i64),
        ("v_batch_stride", _i64), ("v_row_stride", _i64), ("v_head_stride", _i64),
        ("o_batch_stride", _i64), ("o_row_stride", _i64), ("o_head_stride", _i64),
        ("lse_batch_stride", _i64), ("lse_head_stride", _i64),
        ("dout", _ptr), ("dq", _ptr), ("dk", _ptr), ("dv", _ptr), ("softmax_d", _ptr),
        ("do_batch_stride", _i64), ("do_row_stride", _i64), ("do_head_stride", _i64),
        ("dq_batch_stride", _i64), ("dq_row_stride", _i64), ("dq_head_stride", _i64),
        ("dk_batch_stride", _i64), ("dk_row_stride", _i64), ("dk_head_stride", _i64),
        ("dv_batch_stride", _i64), ("dv_row_stride", _i64), ("dv_head_stride", _i64),
        ("batch", _i32), ("nheads_q", _i32), ("nheads_k", _i32), ("seqlen_q", _i32),
        ("seqlen_k", _i32), ("head_dim", _i32), ("dtype", _i32), ("kv_dtype", _i32),
        ("softmax_scale", _f32), ("softcap", _f32),
        ("is_causal", _i32), ("window_left", _i32), ("window_right", _i32),
        ("alibi_slopes", _ptr), ("alibi_batch_stride", _i64),
        ("p_dropout", _f32), ("philox_seed", _u64), ("philox_offset", _u64), ("dmask", _ptr),
        ("cu_seqlens_q", _ptr), ("cu_seqlens_k", _ptr), ("seqused_k", _ptr),
        ("total_q", _i32), ("total_k", _i32),
        ("block_table", _ptr), ("block_table_batch_stride", _i64),
        ("page_block_size", _i32), ("head_dim_v", _i32),
        ("cache_seqlens", _ptr), ("cache_batch_idx", _ptr), ("cache_leftpad", _ptr),
        ("k_new", _ptr), ("v_new", _ptr),
        ("knew_batch_stride", _i64), ("knew_row_stride", _i64), ("knew_head_stride", _i64),
        ("vnew_batch_stride", _i64), ("vnew_row_stride", _i64), ("vnew_head_stride", _i64),
        ("seqlen_new", _i32), ("rotary_dim", _i32),
        ("rotary_cos", _ptr), ("rotary_sin", _ptr),
        ("rotary_interleaved", _i32), ("seqlen_ro", _i32),
        ("k_descale", _f32), ("v_descale", _f32),
        ("num_splits", _i32), ("flags", _i32),
        ("workspace", _ptr), ("workspace_bytes", ctypes.c_size_t),
        ("q_descale", _f32), ("o_dtype", _i32),                      # ABI 4: fp8-e4m3 q, k, v
    ]


class FaExtParams(ctypes.Structure):
    """Mirror of `struct fa_ext_params` (include/fa_mi355.h): the extension block of the *_ext entry points
    (attention sinks).  struct_size must be set to sizeof(FaExtParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("sinks", _ptr),                 # [nheads_q] fp32, NULL = none
        ("dsinks", _ptr),                # backward: [nheads_q] fp32 gradient (written), NULL = not wanted
    ]


def ext_params(sinks=None, dsinks=None):
    """an FaExtParams with struct_size filled in; sinks / dsinks: fp32 GPU tensors or None"""
    e = FaExtParams()
    e.struct_size = ctypes.sizeof(FaExtParams)
    e.sinks = None if sinks is None else sinks.data_ptr()
    e.dsinks = None if dsinks is None else dsinks.data_ptr()
    return e


class FaTreeParams(ctypes.Structure):
    """Mirror of `struct fa_tree_params` (include/fa_mi355.h): the tree-mask block of fa_fwd_kvcache_tree.
    struct_size must be set to sizeof(FaTreeParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("mask", _ptr),                  # uint32 [B, T_q, W] / [T_q, W] visibility words, NULL = no tree
        ("mask_batch_stride", _i64),     # in words, 0 = one tree for the whole batch
        ("mask_words", _i32),            # W = ceil(T_q / 32)
        ("depths", _ptr),                # int32 [B, T_q] / [T_q] node depths, NULL = none
        ("depths_batch_stride", _i64),   # in elements, 0 = shared
    ]


def tree_params(mask=None, depths=None):
    """an FaTreeParams with struct_size filled in; mask: packed int32 [B, T, W] / [T, W] GPU tensor, depths: int32 [B, T] / [T]"""
    t = FaTreeParams()
    t.struct_size = ctypes.sizeof(FaTreeParams)
    if mask is not None:
        t.mask = mask.data_ptr()
        t.mask_words = mask.shape[-1]
        t.mask_batch_stride = mask.stride(0) if mask.dim() == 3 else 0
    if depths is not None:
        t.depths = depths.data_ptr()
        t.depths_batch_stride = depths.stride(0) if depths.dim() == 2 else 0
    return t


FA_MERGE_MAX_PARTS = 8


class FaMergeState(ctypes.Structure):
    """Mirror of `struct fa_merge_state` (include/fa_mi355.h): one (o, lse) pair of fa_merge_states, strides in elements."""
    _fields_ = [
        ("o", _ptr), ("lse", _ptr),
        ("o_batch_stride", _i64), ("o_row_stride", _i64), ("o_head_stride", _i64),
        ("lse_batch_stride", _i64), ("lse_head_stride", _i64), ("lse_row_stride", _i64),
    ]


class FaMergeParams(ctypes.Structure):
    """Mirror of `struct fa_merge_params` (include/fa_mi355.h).  struct_size must be set to sizeof(FaMergeParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("n_parts", _i32), ("batch", _i32), ("seqlen", _i32), ("nheads", _i32), ("head_dim", _i32), ("dtype", _i32),
        ("parts", FaMergeState * FA_MERGE_MAX_PARTS),
        ("out", FaMergeState),
    ]


def merge_state(st, o, lse):
    """fill an FaMergeState from o [B, S, H, D] (last dimension contiguous) and fp32 lse [B, H, S], both taken as strided views"""
    st.o, st.lse = o.data_ptr(), lse.data_ptr()
    st.o_batch_stride, st.o_row_stride, st.o_head_stride = o.stride(0), o.stride(1), o.stride(2)
    st.lse_batch_stride, st.lse_head_stride, st.lse_row_stride = lse.stride(0), lse.stride(1), lse.stride(2)


class FaRotaryParams(ctypes.Structure):
    """Mirror of `struct fa_rotary_params` (include/fa_mi355.h): the standalone rotary embedding fa_rotary.
    struct_size must be set to sizeof(FaRotaryParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("x", _ptr), ("out", _ptr),
        ("x_batch_stride", _i64), ("x_row_stride", _i64), ("x_head_stride", _i64),
        ("o_batch_stride", _i64), ("o_row_stride", _i64), ("o_head_stride", _i64),
        ("batch", _i32), ("seqlen", _i32), ("nheads", _i32), ("head_dim", _i32),
        ("rotary_dim", _i32), ("dtype", _i32),
        ("cos", _ptr), ("sin", _ptr),
        ("cos_sin_fp32", _i32), ("seqlen_ro", _i32), ("interleaved", _i32), ("conjugate", _i32),
        ("seqlen_offset", _i32), ("total_rows", _i32),
        ("seqlen_offsets", _ptr),        # int32 [batch] on the device, NULL = none
        ("cu_seqlens", _ptr),            # int32 [batch + 1] on the device, NULL = dense
    ]


class FaKvStoreParams(ctypes.Structure):
    """Mirror of `struct fa_kv_store_params` (include/fa_mi355.h): fa_kv_store, a ragged packed batch of K / V rows into a KV
    cache.  struct_size must be set to sizeof(FaKvStoreParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("k", _ptr), ("v", _ptr),
        ("k_row_stride", _i64), ("k_head_stride", _i64), ("v_row_stride", _i64), ("v_head_stride", _i64),
        ("k_cache", _ptr), ("v_cache", _ptr),
        ("kc_batch_stride", _i64), ("kc_row_stride", _i64), ("kc_head_stride", _i64),
        ("vc_batch_stride", _i64), ("vc_row_stride", _i64), ("vc_head_stride", _i64),
        ("total_rows", _i32), ("nheads", _i32), ("head_dim", _i32), ("dtype", _i32), ("cache_dtype", _i32),
        ("paged", _i32), ("num_blocks", _i32), ("page_block_size", _i32),
        ("slot_mapping", _ptr),          # int64 [total_rows] on the device: slot mode
        ("cu_seqlens", _ptr),            # int32 [batch + 1] on the device: sequence mode
        ("cache_seqlens", _ptr),         # int32 [batch], NULL = zeros
        ("block_table", _ptr), ("block_table_batch_stride", _i64),
        ("cache_batch_idx", _ptr),
        ("batch", _i32), ("max_blocks", _i32),
        ("k_descale", _f32), ("v_descale", _f32),
        ("rotary_dim", _i32), ("rotary_interleaved", _i32),
        ("rotary_cos", _ptr), ("rotary_sin", _ptr),
        ("seqlen_ro", _i32), ("reserved", _i32),
    ]


class FaKvGatherParams(ctypes.Structure):
    """Mirror of `struct fa_kv_gather_params` (include/fa_mi355.h): fa_kv_gather, ragged K / V rows out of a KV cache into a packed
    pair.  struct_size must be set to sizeof(FaKvGatherParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("k_cache", _ptr), ("v_cache", _ptr),
        ("kc_batch_stride", _i64), ("kc_row_stride", _i64), ("kc_head_stride", _i64),
        ("vc_batch_stride", _i64), ("vc_row_stride", _i64), ("vc_head_stride", _i64),
        ("k", _ptr), ("v", _ptr),
        ("k_row_stride", _i64), ("k_head_stride", _i64), ("v_row_stride", _i64), ("v_head_stride", _i64),
        ("total_rows", _i32), ("nheads", _i32), ("head_dim", _i32), ("dtype", _i32), ("cache_dtype", _i32),
        ("paged", _i32), ("num_blocks", _i32), ("page_block_size", _i32),
        ("slot_mapping", _ptr),          # int64 [total_rows] on the device: slot mode
        ("cu_seqlens", _ptr),            # int32 [batch + 1] on the device: sequence mode
        ("seq_offsets", _ptr),           # int32 [batch]: first position read, NULL = zeros
        ("block_table", _ptr), ("block_table_batch_stride", _i64),
        ("cache_batch_idx", _ptr),
        ("batch", _i32), ("max_blocks", _i32),
        ("k_descale", _f32), ("v_descale", _f32),
    ]


class FaRopeStoreParams(ctypes.Structure):
    """Mirror of `struct fa_rope_store_params` (include/fa_mi355.h): fa_rope_store, q / k rotated at per-token positions and K / V
    stored into a KV cache by slot, one launch.  struct_size must be set to sizeof(FaRopeStoreParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("q", _ptr), ("k", _ptr), ("v", _ptr),               # q NULL: K / V only; v NULL: rotate only
        ("q_row_stride", _i64), ("q_head_stride", _i64), ("k_row_stride", _i64), ("k_head_stride", _i64),
        ("v_row_stride", _i64), ("v_head_stride", _i64),
        ("q_out", _ptr), ("k_out", _ptr),                     # may equal q / k (in place); k_out NULL: K is only cached
        ("qo_row_stride", _i64), ("qo_head_stride", _i64), ("ko_row_stride", _i64), ("ko_head_stride", _i64),
        ("positions", _ptr),             # int64 [total_rows] on the device
        ("rotary_cos", _ptr), ("rotary_sin", _ptr),
        ("rotary_dim", _i32), ("seqlen_ro", _i32), ("rotary_interleaved", _i32),
        ("total_rows", _i32), ("nheads_q", _i32), ("nheads_k", _i32), ("head_dim", _i32), ("dtype", _i32), ("cache_dtype", _i32),
        ("reserved", _i32),
        ("k_cache", _ptr), ("v_cache", _ptr),                 # both NULL: rotate only
        ("kc_batch_stride", _i64), ("kc_row_stride", _i64), ("kc_head_stride", _i64),
        ("vc_batch_stride", _i64), ("vc_row_stride", _i64), ("vc_head_stride", _i64),
        ("num_blocks", _i32), ("page_block_size", _i32),
        ("slot_mapping", _ptr),          # int64 [total_rows] on the device
        ("k_descale", _f32), ("v_descale", _f32),
    ]


class FaQkNormRopeStoreParams(ctypes.Structure):
    """Mirror of `struct fa_qk_norm_rope_store_params` (include/fa_mi355.h): fa_qk_norm_rope_store, fa_rope_store with a per-head
    RMSNorm of q and k in front of the rotation - FaRopeStoreParams' fields, then the norm's.  struct_size must be set to
    sizeof(FaQkNormRopeStoreParams)."""
    _fields_ = FaRopeStoreParams._fields_ + [
        ("q_weight", _ptr), ("k_weight", _ptr),               # [head_dim] of weight_dtype; NULL: that tensor is not normalised
        ("weight_dtype", _i32),          # the q / k dtype, or FA_FP32
        ("eps", _f32), ("weight_offset", _f32),
        ("reserved1", _i32),
    ]


class FaQkNormRopeBwdParams(ctypes.Structure):
    """Mirror of `struct fa_qk_norm_rope_bwd_params` (include/fa_mi355.h): fa_qk_norm_rope_bwd, the backward of the norm + rotation
    of fa_qk_norm_rope_store - dq / dk from the gradients of q_out / k_out and the saved pre-norm q / k, and the two weight
    gradients.  struct_size must be set to sizeof(FaQkNormRopeBwdParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("dq_out", _ptr), ("dk_out", _ptr),                   # the incoming gradients
        ("dqo_row_stride", _i64), ("dqo_head_stride", _i64), ("dko_row_stride", _i64), ("dko_head_stride", _i64),
        ("q", _ptr), ("k", _ptr),                             # the saved pre-norm inputs; q NULL: no q heads
        ("q_row_stride", _i64), ("q_head_stride", _i64), ("k_row_stride", _i64), ("k_head_stride", _i64),
        ("dq", _ptr), ("dk", _ptr),                           # outputs; may equal dq_out / dk_out (in place); NULL: skipped
        ("dq_row_stride", _i64), ("dq_head_stride", _i64), ("dk_row_stride", _i64), ("dk_head_stride", _i64),
        ("positions", _ptr),             # int64 [total_rows] on the device
        ("rotary_cos", _ptr), ("rotary_sin", _ptr),
        ("rotary_dim", _i32), ("seqlen_ro", _i32), ("rotary_interleaved", _i32),
        ("total_rows", _i32), ("nheads_q", _i32), ("nheads_k", _i32), ("head_dim", _i32), ("dtype", _i32),
        ("q_weight", _ptr), ("k_weight", _ptr),
        ("weight_dtype", _i32), ("eps", _f32), ("weight_offset", _f32), ("reserved", _i32),
        ("dq_weight", _ptr), ("dk_weight", _ptr),             # [head_dim] of weight_dtype; NULL: skipped
        ("workspace", _ptr), ("workspace_bytes", ctypes.c_size_t),
        ("reserved1", _i64 * 2),
    ]


class FaAddNormParams(ctypes.Structure):
    """Mirror of `struct fa_add_norm_params` (include/fa_mi355.h): fa_add_norm, residual add + RMSNorm / LayerNorm over the whole
    hidden size.  struct_size must be set to sizeof(FaAddNormParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("x", _ptr), ("residual", _ptr),                      # residual NULL: none
        ("out", _ptr), ("residual_out", _ptr),                # may equal x / residual (in place); residual_out NULL: not written
        ("x_row_stride", _i64), ("residual_row_stride", _i64), ("out_row_stride", _i64), ("residual_out_row_stride", _i64),
        ("weight", _ptr), ("bias", _ptr),                     # [n] of weight_dtype; bias NULL: none
        ("rows", _i64),
        ("n", _i32), ("dtype", _i32), ("residual_dtype", _i32), ("residual_out_dtype", _i32), ("weight_dtype", _i32),
        ("is_rms_norm", _i32),
        ("eps", _f32), ("weight_offset", _f32),
        ("reserved", _i64 * 2),
    ]


class FaAddNormBwdParams(ctypes.Structure):
    """Mirror of `struct fa_add_norm_bwd_params` (include/fa_mi355.h): fa_add_norm_bwd, the backward of fa_add_norm - dx / dres
    from dy, the saved z and an optional dres_out, and dweight / dbias.  struct_size must be set to sizeof(FaAddNormBwdParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("dy", _ptr), ("z", _ptr), ("dres_out", _ptr),        # dres_out NULL: none
        ("dx", _ptr), ("dres", _ptr),                         # outputs; dx may equal dy (in place); NULL: skipped
        ("dy_row_stride", _i64), ("z_row_stride", _i64), ("dres_out_row_stride", _i64), ("dx_row_stride", _i64),
        ("dres_row_stride", _i64),
        ("weight", _ptr), ("dweight", _ptr), ("dbias", _ptr),  # [n] of weight_dtype; dweight / dbias NULL: skipped
        ("workspace", _ptr), ("workspace_bytes", ctypes.c_size_t),
        ("rows", _i64),
        ("n", _i32), ("dtype", _i32), ("z_dtype", _i32), ("dres_dtype", _i32), ("weight_dtype", _i32), ("is_rms_norm", _i32),
        ("eps", _f32), ("weight_offset", _f32),
        ("reserved", _i64 * 2),
    ]


class FaCrossEntropyParams(ctypes.Structure):
    """Mirror of `struct fa_cross_entropy_params` (include/fa_mi355.h): fa_cross_entropy, the softmax cross-entropy loss over the
    vocabulary - losses, z_losses and lse of [rows, vocab] logits.  struct_size must be set to sizeof(FaCrossEntropyParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("logits", _ptr), ("labels", _ptr),                   # [rows, vocab] of dtype; int64 [rows]
        ("losses", _ptr), ("z_losses", _ptr), ("lse", _ptr),  # fp32 [rows], written
        ("workspace", _ptr), ("workspace_bytes", ctypes.c_size_t),
        ("logits_row_stride", _i64),
        ("rows", _i64), ("ignore_index", _i64),
        ("vocab", _i32), ("dtype", _i32),
        ("label_smoothing", _f32), ("logit_scale", _f32), ("lse_square_scale", _f32),
        ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


class FaCrossEntropyBwdParams(ctypes.Structure):
    """Mirror of `struct fa_cross_entropy_bwd_params` (include/fa_mi355.h): fa_cross_entropy_bwd, dlogits from dlosses, the logits,
    the labels and the forward's lse.  struct_size must be set to sizeof(FaCrossEntropyBwdParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("dlosses", _ptr), ("logits", _ptr), ("labels", _ptr), ("lse", _ptr),
        ("dlogits", _ptr),                                    # may equal logits (in place)
        ("dlosses_stride", _i64), ("logits_row_stride", _i64), ("dlogits_row_stride", _i64),
        ("rows", _i64), ("ignore_index", _i64),
        ("vocab", _i32), ("dtype", _i32),
        ("label_smoothing", _f32), ("logit_scale", _f32), ("lse_square_scale", _f32),
        ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


class FaSampleParams(ctypes.Structure):
    """Mirror of `struct fa_sample_params` (include/fa_mi355.h): fa_sample, temperature / top-k / min-p / top-p token sampling from
    [rows, vocab] logits with one caller-supplied uniform number per row.  struct_size must be set to sizeof(FaSampleParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("logits", _ptr), ("u", _ptr),                        # [rows, vocab] of dtype; fp32 [rows]
        ("temperature", _ptr), ("top_k", _ptr), ("top_p", _ptr), ("min_p", _ptr),   # [rows] arrays, or NULL: the *_value
        ("ids", _ptr), ("n_kept", _ptr), ("lse", _ptr), ("filtered", _ptr),         # written; NULL: skipped
        ("workspace", _ptr), ("workspace_bytes", ctypes.c_size_t),
        ("logits_row_stride", _i64), ("filtered_row_stride", _i64),
        ("rows", _i64),
        ("vocab", _i32), ("dtype", _i32),
        ("temperature_value", _f32), ("top_k_value", _i32), ("top_p_value", _f32), ("min_p_value", _f32),
        ("reserved", _i64 * 4),
    ]


class FaSpecAcceptParams(ctypes.Structure):
    """Mirror of `struct fa_spec_accept_params` (include/fa_mi355.h): fa_spec_accept, the rejection-sampling decision of every
    draft node of a speculative-decoding step.  struct_size must be set to sizeof(FaSpecAcceptParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("target_logits", _ptr), ("draft_probs", _ptr),       # [batch x nodes, vocab] of dtype / probs_dtype
        ("draft_ids", _ptr), ("parents", _ptr),               # int32 [batch, nodes]; int32 or NULL: the chain
        ("u_accept", _ptr), ("u_recover", _ptr),              # fp32 [batch x nodes]
        ("temperature", _ptr),                                # fp32 [batch], or NULL: temperature_value
        ("accept", _ptr), ("recovered", _ptr),                # int32 [batch x nodes], written
        ("workspace", _ptr), ("workspace_bytes", ctypes.c_size_t),
        ("logits_row_stride", _i64), ("probs_row_stride", _i64), ("parents_batch_stride", _i64),
        ("batch", _i64),
        ("nodes", _i32), ("vocab", _i32), ("dtype", _i32), ("probs_dtype", _i32),
        ("temperature_value", _f32), ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


class FaSpecWalkParams(ctypes.Structure):
    """Mirror of `struct fa_spec_walk_params` (include/fa_mi355.h): fa_spec_walk, the walk over a request's draft tree that
    emits the tokens and the accepted path.  struct_size must be set to sizeof(FaSpecWalkParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("parents", _ptr), ("draft_ids", _ptr), ("target_ids", _ptr),
        ("accept", _ptr), ("recovered", _ptr),                # fa_spec_accept's outputs, or both NULL: deterministic drafts
        ("out_tokens", _ptr), ("num_out", _ptr), ("path_nodes", _ptr),   # written
        ("parents_batch_stride", _i64), ("target_ids_batch_stride", _i64), ("target_ids_node_stride", _i64),
        ("batch", _i64),
        ("nodes", _i32), ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


class FaActMulParams(ctypes.Structure):
    """Mirror of `struct fa_act_mul_params` (include/fa_mi355.h): fa_act_mul, the gated activation act(gate) * up of the MLP
    (up NULL: act(gate)).  struct_size must be set to sizeof(FaActMulParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("gate", _ptr), ("up", _ptr),                         # [rows, n] of dtype; up NULL: ungated
        ("out", _ptr),                                        # may equal gate or up (in place)
        ("gate_row_stride", _i64), ("up_row_stride", _i64), ("out_row_stride", _i64),
        ("rows", _i64),
        ("n", _i32), ("dtype", _i32), ("activation", _i32),
        ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


class FaActMulBwdParams(ctypes.Structure):
    """Mirror of `struct fa_act_mul_bwd_params` (include/fa_mi355.h): fa_act_mul_bwd, dgate and dup from dout, gate and up.
    struct_size must be set to sizeof(FaActMulBwdParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("dout", _ptr), ("gate", _ptr), ("up", _ptr),
        ("dgate", _ptr), ("dup", _ptr),                       # may equal gate / up (in place); dup NULL exactly where up is
        ("dout_row_stride", _i64), ("gate_row_stride", _i64), ("up_row_stride", _i64), ("dgate_row_stride", _i64),
        ("dup_row_stride", _i64),
        ("rows", _i64),
        ("n", _i32), ("dtype", _i32), ("activation", _i32),
        ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


class FaQuantFp8Params(ctypes.Structure):
    """Mirror of `struct fa_quant_fp8_params` (include/fa_mi355.h): fa_quant_fp8, dynamic fp8-e4m3 quantisation of [rows, n]
    fp16 / bf16 - codes and fp32 scales.  struct_size must be set to sizeof(FaQuantFp8Params)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("x", _ptr),
        ("codes", _ptr), ("scales", _ptr),                    # [rows, n] bytes; fp32 [rows] / [rows, n / 128] / NULL (static)
        ("x_row_stride", _i64), ("codes_row_stride", _i64),
        ("rows", _i64),
        ("n", _i32), ("dtype", _i32), ("mode", _i32), ("has_scale_ub", _i32),
        ("scale", _f32), ("scale_ub", _f32),
        ("reserved", _i64 * 4),
    ]


class FaAddNormQuantParams(ctypes.Structure):
    """Mirror of `struct fa_add_norm_quant_params` (include/fa_mi355.h): fa_add_norm_quant, fa_add_norm's forward with fp8 codes
    and scales in the place of `out` (norm.out NULL).  struct_size and norm.struct_size must both be set."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("norm", FaAddNormParams),
        ("codes", _ptr), ("scales", _ptr),
        ("codes_row_stride", _i64),
        ("mode", _i32), ("has_scale_ub", _i32),
        ("scale", _f32), ("scale_ub", _f32),
        ("reserved", _i64 * 4),
    ]


class FaActMulQuantParams(ctypes.Structure):
    """Mirror of `struct fa_act_mul_quant_params` (include/fa_mi355.h): fa_act_mul_quant, act(gate) * up (up NULL: act(gate))
    as fp8 codes and scales.  struct_size must be set to sizeof(FaActMulQuantParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("gate", _ptr), ("up", _ptr),
        ("codes", _ptr), ("scales", _ptr),
        ("gate_row_stride", _i64), ("up_row_stride", _i64), ("codes_row_stride", _i64),
        ("rows", _i64),
        ("n", _i32), ("dtype", _i32), ("activation", _i32), ("mode", _i32), ("has_scale_ub", _i32),
        ("scale", _f32), ("scale_ub", _f32),
        ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


class FaMoeRouteParams(ctypes.Structure):
    """Mirror of `struct fa_moe_route_params` (include/fa_mi355.h): fa_moe_route, top-k routing of [tokens, num_experts] logits -
    fp32 weights and int32 ids.  struct_size must be set to sizeof(FaMoeRouteParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("logits", _ptr), ("bias", _ptr),                     # [tokens, num_experts] of dtype; fp32 [num_experts] or NULL
        ("weights", _ptr), ("ids", _ptr),                     # fp32 / int32 [tokens, top_k], written
        ("logits_row_stride", _i64),
        ("tokens", _i64),
        ("num_experts", _i32), ("top_k", _i32), ("dtype", _i32), ("scoring", _i32), ("renormalize", _i32),
        ("scale", _f32),
        ("reserved", _i64 * 4),
    ]


class FaMoeRouteBwdParams(ctypes.Structure):
    """Mirror of `struct fa_moe_route_bwd_params` (include/fa_mi355.h): fa_moe_route_bwd, dlogits from dweights, the logits and
    the ids.  struct_size must be set to sizeof(FaMoeRouteBwdParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("dweights", _ptr), ("logits", _ptr), ("ids", _ptr),
        ("dlogits", _ptr),
        ("logits_row_stride", _i64), ("dlogits_row_stride", _i64),
        ("tokens", _i64),
        ("num_experts", _i32), ("top_k", _i32), ("dtype", _i32), ("scoring", _i32), ("renormalize", _i32),
        ("scale", _f32),
        ("reserved", _i64 * 4),
    ]


class FaMoeSortParams(ctypes.Structure):
    """Mirror of `struct fa_moe_sort_params` (include/fa_mi355.h): fa_moe_sort, the stable counting sort of the (token, k) slots
    by expert.  struct_size must be set to sizeof(FaMoeSortParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("ids", _ptr),
        ("sorted_slot", _ptr), ("pos", _ptr), ("expert_offsets", _ptr),
        ("workspace", _ptr), ("workspace_bytes", ctypes.c_size_t),
        ("tokens", _i64),
        ("num_experts", _i32), ("top_k", _i32), ("align", _i32), ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


class FaMoePermuteParams(ctypes.Structure):
    """Mirror of `struct fa_moe_permute_params` (include/fa_mi355.h): fa_moe_permute, the rows of x in sorted order, optionally
    scaled per slot.  struct_size must be set to sizeof(FaMoePermuteParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("x", _ptr), ("sorted_slot", _ptr), ("slot_scale", _ptr),
        ("out", _ptr),
        ("x_row_stride", _i64), ("out_row_stride", _i64),
        ("rows", _i64), ("tokens", _i64),
        ("top_k", _i32), ("n", _i32), ("dtype", _i32), ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


class FaMoeCombineParams(ctypes.Structure):
    """Mirror of `struct fa_moe_combine_params` (include/fa_mi355.h): fa_moe_combine, the weighted sum of a token's expert rows.
    struct_size must be set to sizeof(FaMoeCombineParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("y", _ptr), ("weights", _ptr), ("pos", _ptr),
        ("out", _ptr),
        ("y_row_stride", _i64), ("out_row_stride", _i64),
        ("rows", _i64), ("tokens", _i64),
        ("top_k", _i32), ("n", _i32), ("dtype", _i32), ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


class FaMoeCombineBwdParams(ctypes.Structure):
    """Mirror of `struct fa_moe_combine_bwd_params` (include/fa_mi355.h): fa_moe_combine_bwd, dy and dw of fa_moe_combine.
    struct_size must be set to sizeof(FaMoeCombineBwdParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("dout", _ptr), ("y", _ptr), ("weights", _ptr), ("pos", _ptr),
        ("dy", _ptr), ("dw", _ptr),                            # NULL: skipped
        ("dout_row_stride", _i64), ("y_row_stride", _i64), ("dy_row_stride", _i64),
        ("rows", _i64), ("tokens", _i64),
        ("top_k", _i32), ("n", _i32), ("dtype", _i32), ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


class FaMoeGemmParams(ctypes.Structure):
    """Mirror of `struct fa_moe_gemm_params` (include/fa_mi355.h): fa_moe_gemm, the grouped expert GEMM over the segments of
    expert_offsets.  struct_size must be set to sizeof(FaMoeGemmParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("x", _ptr), ("w", _ptr), ("bias", _ptr), ("expert_offsets", _ptr), ("sorted_slot", _ptr),
        ("out", _ptr),
        ("x_row_stride", _i64), ("out_row_stride", _i64), ("w_expert_stride", _i64),
        ("rows", _i64), ("tokens", _i64),
        ("num_experts", _i32), ("top_k", _i32), ("n", _i32), ("k", _i32),
        ("dtype", _i32), ("bias_dtype", _i32), ("layout", _i32), ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


class FaMoeGemmWgradParams(ctypes.Structure):
    """Mirror of `struct fa_moe_gemm_wgrad_params` (include/fa_mi355.h): fa_moe_gemm_wgrad, the weight and bias gradients of the
    grouped expert GEMM.  struct_size must be set to sizeof(FaMoeGemmWgradParams)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("dy", _ptr), ("x", _ptr), ("expert_offsets", _ptr), ("sorted_slot", _ptr),
        ("dw", _ptr), ("dbias", _ptr),                          # NULL: skipped
        ("dy_row_stride", _i64), ("x_row_stride", _i64), ("dw_expert_stride", _i64),
        ("rows", _i64), ("tokens", _i64),
        ("num_experts", _i32), ("top_k", _i32), ("n", _i32), ("k", _i32),
        ("dtype", _i32), ("dw_dtype", _i32), ("dbias_dtype", _i32), ("layout", _i32),
        ("accumulate", _i32), ("reserved0", _i32),
        ("reserved", _i64 * 4),
    ]


EXT_OPS = ["fa_fwd_ext", "fa_varlen_fwd_ext", "fa_fwd_kvcache_ext", "fa_bwd_ext", "fa_varlen_bwd_ext"]

EXPORTS = ["fa_abi_version", "fa_params_size", "fa_last_error", "fa_build_info",
           "fa_fwd_workspace_bytes", "fa_bwd_workspace_bytes", "fa_fwd_kvcache_workspace_bytes",
           "fa_fwd", "fa_bwd", "fa_varlen_fwd", "fa_varlen_bwd", "fa_fwd_kvcache",
           "fa_gather_rows", "fa_scatter_rows", "fa_fwd_kvcache_tree", "fa_tree_params_size",
           "fa_merge_states", "fa_merge_params_size", "fa_rotary", "fa_rotary_params_size",
           "fa_kv_store", "fa_kv_store_params_size", "fa_kv_gather", "fa_kv_gather_params_size",
           "fa_rope_store", "fa_rope_store_params_size", "fa_qk_norm_rope_store", "fa_qk_norm_rope_store_params_size",
           "fa_qk_norm_rope_bwd", "fa_qk_norm_rope_bwd_workspace_bytes", "fa_qk_norm_rope_bwd_params_size",
           "fa_add_norm", "fa_add_norm_params_size",
           "fa_add_norm_bwd", "fa_add_norm_bwd_workspace_bytes", "fa_add_norm_bwd_params_size",
           "fa_cross_entropy", "fa_cross_entropy_workspace_bytes", "fa_cross_entropy_params_size",
           "fa_cross_entropy_bwd", "fa_cross_entropy_bwd_params_size",
           "fa_sample", "fa_sample_workspace_bytes", "fa_sample_params_size",
           "fa_spec_accept", "fa_spec_accept_workspace_bytes", "fa_spec_accept_params_size",
           "fa_spec_walk", "fa_spec_walk_params_size",
           "fa_act_mul", "fa_act_mul_params_size", "fa_act_mul_plan", "fa_act_mul_bwd", "fa_act_mul_bwd_params_size",
           "fa_quant_fp8", "fa_quant_fp8_params_size", "fa_add_norm_quant", "fa_add_norm_quant_params_size",
           "fa_act_mul_quant", "fa_act_mul_quant_params_size",
           "fa_moe_route", "fa_moe_route_params_size", "fa_moe_route_bwd", "fa_moe_route_bwd_params_size",
           "fa_moe_sort", "fa_moe_sort_params_size", "fa_moe_sort_workspace_bytes", "fa_moe_sort_plan",
           "fa_moe_permute", "fa_moe_permute_params_size", "fa_moe_combine", "fa_moe_combine_params_size",
           "fa_moe_combine_bwd", "fa_moe_combine_bwd_params_size",
           "fa_moe_gemm", "fa_moe_gemm_params_size", "fa_moe_gemm_plan",
           "fa_moe_gemm_wgrad", "fa_moe_gemm_wgrad_params_size", "fa_moe_gemm_wgrad_plan"] + EXT_OPS


# The struct-taking row ops, each declared once: (entry point, struct class, workspace query or None).  The struct's size
# export is `<entry point>_params_size`.  _load() sets restype / argtypes and checks the sizes from this table; the call_* and
# *_workspace_bytes functions below are bound from it.
ROW_OPS = [
    ("fa_rotary", FaRotaryParams, None),
    ("fa_kv_store", FaKvStoreParams, None),
    ("fa_kv_gather", FaKvGatherParams, None),
    ("fa_rope_store", FaRopeStoreParams, None),
    ("fa_qk_norm_rope_store", FaQkNormRopeStoreParams, None),
    ("fa_qk_norm_rope_bwd", FaQkNormRopeBwdParams, "fa_qk_norm_rope_bwd_workspace_bytes"),
    ("fa_add_norm", FaAddNormParams, None),
    ("fa_add_norm_bwd", FaAddNormBwdParams, "fa_add_norm_bwd_workspace_bytes"),
    ("fa_cross_entropy", FaCrossEntropyParams, "fa_cross_entropy_workspace_bytes"),
    ("fa_cross_entropy_bwd", FaCrossEntropyBwdParams, None),
    ("fa_sample", FaSampleParams, "fa_sample_workspace_bytes"),
    ("fa_spec_accept", FaSpecAcceptParams, "fa_spec_accept_workspace_bytes"),
    ("fa_spec_walk", FaSpecWalkParams, None),
    ("fa_act_mul", FaActMulParams, None),
    ("fa_act_mul_bwd", FaActMulBwdParams, None),
    ("fa_quant_fp8", FaQuantFp8Params, None),
    ("fa_add_norm_quant", FaAddNormQuantParams, None),
    ("fa_act_mul_quant", FaActMulQuantParams, None),
    ("fa_moe_route", FaMoeRouteParams, None),
    ("fa_moe_route_bwd", FaMoeRouteBwdParams, None),
    ("fa_moe_sort", FaMoeSortParams, "fa_moe_sort_workspace_bytes"),
    ("fa_moe_permute", FaMoePermuteParams, None),
    ("fa_moe_combine", FaMoeCombineParams, None),
    ("fa_moe_combine_bwd", FaMoeCombineBwdParams, None),
    ("fa_moe_gemm", FaMoeGemmParams, None),
    ("fa_moe_gemm_wgrad", FaMoeGemmWgradParams, None),
]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the gfx950 HIP library is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or flash-attention-v100_amd/build.py). "
            "There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise ImportError(f"libfa_mi355.so does not export {name}")
    lib.fa_abi_version.restype = ctypes.c_int
    lib.fa_params_size.restype = ctypes.c_size_t
    lib.fa_last_error.restype = ctypes.c_char_p
    lib.fa_build_info.restype = ctypes.c_char_p
    for name in ("fa_fwd_workspace_bytes", "fa_bwd_workspace_bytes", "fa_fwd_kvcache_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_size_t
        fn.argtypes = [ctypes.POINTER(FaParams)]
    for name in ("fa_fwd", "fa_bwd", "fa_varlen_fwd", "fa_varlen_bwd", "fa_fwd_kvcache"):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.POINTER(FaParams), ctypes.c_void_p]
    for name in EXT_OPS:
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.POINTER(FaParams), ctypes.POINTER(FaExtParams), ctypes.c_void_p]
    lib.fa_fwd_kvcache_tree.restype = ctypes.c_int
    lib.fa_fwd_kvcache_tree.argtypes = [ctypes.POINTER(FaParams), ctypes.POINTER(FaExtParams), ctypes.POINTER(FaTreeParams),
                                        ctypes.c_void_p]
    lib.fa_tree_params_size.restype = ctypes.c_size_t
    lib.fa_merge_states.restype = ctypes.c_int
    lib.fa_merge_states.argtypes = [ctypes.POINTER(FaMergeParams), ctypes.c_void_p]
    lib.fa_merge_params_size.restype = ctypes.c_size_t
    for entry, struct, query in ROW_OPS:
        fn = getattr(lib, entry)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.POINTER(struct), ctypes.c_void_p]
        getattr(lib, entry + "_params_size").restype = ctypes.c_size_t
        if query:
            getattr(lib, query).restype = ctypes.c_size_t
            getattr(lib, query).argtypes = [ctypes.POINTER(struct)]
    i64 = ctypes.c_int64
    lib.fa_act_mul_plan.restype = ctypes.c_int
    lib.fa_act_mul_plan.argtypes = [i64, ctypes.c_int32] + [ctypes.POINTER(i64)] * 3
    lib.fa_moe_sort_plan.restype = ctypes.c_int
    lib.fa_moe_sort_plan.argtypes = [i64, ctypes.c_int32] + [ctypes.POINTER(i64)] * 3
    lib.fa_moe_gemm_plan.restype = ctypes.c_int
    lib.fa_moe_gemm_plan.argtypes = [i64] + [ctypes.c_int32] * 5 + [ctypes.POINTER(ctypes.c_int32)] * 3 + [ctypes.POINTER(i64)] * 2
    lib.fa_moe_gemm_wgrad_plan.restype = ctypes.c_int
    lib.fa_moe_gemm_wgrad_plan.argtypes = [ctypes.c_int32] * 5 + [ctypes.POINTER(ctypes.c_int32)] * 3 + [ctypes.POINTER(i64)] * 3
    lib.fa_gather_rows.restype = ctypes.c_int
    lib.fa_gather_rows.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, i64, i64, i64, i64, ctypes.c_void_p]
    lib.fa_scatter_rows.restype = ctypes.c_int
    lib.fa_scatter_rows.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, i64, i64, i64, ctypes.c_int, ctypes.c_void_p]
    if lib.fa_abi_version() != FA_ABI_VERSION:
        raise ImportError(f"libfa_mi355.so ABI {lib.fa_abi_version()} != binding {FA_ABI_VERSION}")
    if lib.fa_params_size() != ctypes.sizeof(FaParams):
        raise ImportError(f"fa_params size mismatch: library {lib.fa_params_size()} vs ctypes "
                          f"{ctypes.sizeof(FaParams)}")
    if lib.fa_tree_params_size() != ctypes.sizeof(FaTreeParams):
        raise ImportError(f"fa_tree_params size mismatch: library {lib.fa_tree_params_size()} vs ctypes "
                          f"{ctypes.sizeof(FaTreeParams)}")
    if lib.fa_merge_params_size() != ctypes.sizeof(FaMergeParams):
        raise ImportError(f"fa_merge_params size mismatch: library {lib.fa_merge_params_size()} vs ctypes "
                          f"{ctypes.sizeof(FaMergeParams)}")
    for entry, struct, _ in ROW_OPS:
        size = getattr(lib, entry + "_params_size")()
        if size != ctypes.sizeof(struct):
            raise ImportError(f"{entry}_params size mismatch: library {size} vs ctypes {ctypes.sizeof(struct)}")
    return lib


lib = _load()


def call(name, params, stream):
    """Invoke an op; raise RuntimeError (like TORCH_CHECK -> RuntimeError in the reference,
    kernel/fused_mha_api.cpp) with the library's message on failure."""
    rc = getattr(lib, name)(ctypes.byref(params), ctypes.c_void_p(stream))
    if rc != 0:
        msg = lib.fa_last_error().decode(errors="replace")
        raise RuntimeError(f"{name} failed ({rc}): {msg}")


def call_ext(name, params, ext, stream):
    """call() for the *_ext entry points: `name` is the ABI-4 op; with ext None the ABI-4 op itself runs"""
    if ext is None:
        return call(name, params, stream)
    rc = getattr(lib, name + "_ext")(ctypes.byref(params), ctypes.byref(ext), ctypes.c_void_p(stream))
    if rc != 0:
        msg = lib.fa_last_error().decode(errors="replace")
        raise RuntimeError(f"{name}_ext failed ({rc}): {msg}")


def call_tree(params, ext, tree, stream):
    """fa_fwd_kvcache_tree: the kv-cache op with an optional extension block and an optional tree block (None: NULL)"""
    rc = lib.fa_fwd_kvcache_tree(ctypes.byref(params), None if ext is None else ctypes.byref(ext),
                                 None if tree is None else ctypes.byref(tree), ctypes.c_void_p(stream))
    if rc != 0:
        msg = lib.fa_last_error().decode(errors="replace")
        raise RuntimeError(f"fa_fwd_kvcache_tree failed ({rc}): {msg}")


def _struct_call(entry):
    """the call_* function of a (params, stream) entry point: raises RuntimeError with the library's message on failure"""
    fn = getattr(lib, entry)

    def call_op(params, stream):
        rc = fn(ctypes.byref(params), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"{entry} failed ({rc}): {lib.fa_last_error().decode(errors='replace')}")
    call_op.__name__ = call_op.__qualname__ = "call_" + entry[len("fa_"):]
    call_op.__doc__ = entry
    return call_op


def _workspace_query(query):
    """the *_workspace_bytes function of a workspace query: needs no device"""
    fn = getattr(lib, query)

    def workspace_bytes(params):
        return int(fn(ctypes.byref(params)))
    workspace_bytes.__name__ = workspace_bytes.__qualname__ = query[len("fa_"):]
    workspace_bytes.__doc__ = query + ": needs no device"
    return workspace_bytes


call_merge = _struct_call("fa_merge_states")
# call_rotary, call_kv_store, call_kv_gather, call_rope_store, call_qk_norm_rope_store, call_qk_norm_rope_bwd, call_add_norm,
# call_add_norm_bwd, call_cross_entropy, call_cross_entropy_bwd, call_act_mul, call_act_mul_bwd, call_quant_fp8, call_add_norm_quant,
# call_act_mul_quant, call_moe_route, call_moe_route_bwd, call_moe_sort, call_moe_permute, call_moe_combine, call_moe_combine_bwd,
# call_moe_gemm, call_moe_gemm_wgrad,
# call_sample, call_spec_accept, call_spec_walk; qk_norm_rope_bwd_workspace_bytes, add_norm_bwd_workspace_bytes,
# cross_entropy_workspace_bytes, sample_workspace_bytes, spec_accept_workspace_bytes, moe_sort_workspace_bytes
for _entry, _struct, _query in ROW_OPS:
    globals()["call_" + _entry[len("fa_"):]] = _struct_call(_entry)
    if _query:
        globals()[_query[len("fa_"):]] = _workspace_query(_query)
del _entry, _struct, _query


def call_rows(name, *args):
    """fa_gather_rows / fa_scatter_rows (plain-argument entry points)."""
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {lib.fa_last_error().decode(errors='replace')}")


def act_mul_plan(rows, n):
    """fa_act_mul_plan: (run_columns, items, grid) of fa_act_mul / fa_act_mul_bwd, a function of (rows, n) alone; needs no device"""
    out = [ctypes.c_int64() for _ in range(3)]
    rc = lib.fa_act_mul_plan(rows, n, *(ctypes.byref(o) for o in out))
    if rc != 0:
        raise RuntimeError(f"fa_act_mul_plan failed ({rc}): {lib.fa_last_error().decode(errors='replace')}")
    return tuple(o.value for o in out)


def moe_sort_plan(slots, num_experts):
    """fa_moe_sort_plan: (chunk_slots, chunks, workspace_bytes) of fa_moe_sort, a function of (slots = tokens x top_k,
    num_experts) alone; needs no device"""
    out = [ctypes.c_int64() for _ in range(3)]
    rc = lib.fa_moe_sort_plan(slots, num_experts, *(ctypes.byref(o) for o in out))
    if rc != 0:
        raise RuntimeError(f"fa_moe_sort_plan failed ({rc}): {lib.fa_last_error().decode(errors='replace')}")
    return tuple(o.value for o in out)


def moe_gemm_plan(rows, n, k, num_experts, layout, dtype):
    """fa_moe_gemm_plan: (block_m, block_n, block_k, grid_m, grid_n) of fa_moe_gemm, a function of its arguments alone; needs
    no device"""
    blk = [ctypes.c_int32() for _ in range(3)]
    grid = [ctypes.c_int64() for _ in range(2)]
    rc = lib.fa_moe_gemm_plan(rows, n, k, num_experts, layout, dtype, *(ctypes.byref(o) for o in blk + grid))
    if rc != 0:
        raise RuntimeError(f"fa_moe_gemm_plan failed ({rc}): {lib.fa_last_error().decode(errors='replace')}")
    return tuple(o.value for o in blk + grid)


def moe_gemm_wgrad_plan(n, k, num_experts, layout, dtype):
    """fa_moe_gemm_wgrad_plan: (block_n, block_k, block_rows, grid_n, grid_k, grid_e) of fa_moe_gemm_wgrad, a function of the
    shapes alone; needs no device"""
    blk = [ctypes.c_int32() for _ in range(3)]
    grid = [ctypes.c_int64() for _ in range(3)]
    rc = lib.fa_moe_gemm_wgrad_plan(n, k, num_experts, layout, dtype, *(ctypes.byref(o) for o in blk + grid))
    if rc != 0:
        raise RuntimeError(f"fa_moe_gemm_wgrad_plan failed ({rc}): {lib.fa_last_error().decode(errors='replace')}")
    return tuple(o.value for o in blk + grid)
