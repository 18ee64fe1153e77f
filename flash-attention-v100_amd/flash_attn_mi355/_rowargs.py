"""What the wrappers of the row ops share (rope_store, qk_norm, kv_store, kv_gather, add_norm, cross_entropy, act_mul, sample): the
validators of their common arguments and the fillers of the parameter-block fields that go with them.  Every validator takes `op`,
the prefix of the wrapper's messages ("rope_store", "qk_norm", "kv_store", "kv_gather", "add_norm", "cross_entropy", "act_mul"), and
raises RuntimeError; a filler writes
into any block that has the fields (the blocks share their names, include/fa_mi355.h).  Private: nothing here is API."""
import ctypes

import torch

from . import _lib
from . import flash_attn_interface as _fi


def ids(op, t, T, name):
    """an id vector (positions, slot_mapping) as the kernels take it: int64 (T,), contiguous"""
    dtype = t.dtype
    if dtype not in (torch.int64, torch.int32) or tuple(t.shape) != (T,):
        raise RuntimeError(f"{op}: {name} must be an int64 (or int32) tensor of shape ({T},)")
    return (t if dtype == torch.int64 else t.to(torch.int64)).contiguous()


def view(op, x, D, inplace, name):
    """the tensor as the kernel takes it: a view with 16-byte friendly strides as it is; anything else is copied - which in place
    would change the copy, so there it is an error"""
    p = _fi._prep(x, D)
    if inplace and p is not x:
        raise RuntimeError(f"{op}: in place needs a 16-byte aligned {name} whose strides are multiples of 8 elements "
                           f"(got strides {tuple(x.stride())}); pass inplace=False")
    return p


def i32(op, t, shape, name):
    """an int32 side table of the given shape, contiguous"""
    if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{op}: {name} must be an int32 tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def weight(op, w, n, dtype, name, of="k", dim="headdim"):
    """a norm weight (or bias): (n,) of `dtype` or float32, contiguous and 16-byte aligned (a copy where it is not).  of / dim:
    how the messages name the tensor that sets the dtype and the length"""
    if w.dtype not in (dtype, torch.float32):
        raise RuntimeError(f"{op}: {name} must have {of}'s dtype ({dtype}) or float32, got {w.dtype}")
    if tuple(w.shape) != (n,):
        raise RuntimeError(f"{op}: {name} must have shape ({dim},) = ({n},), got {tuple(w.shape)}")
    w = w.contiguous()
    return w if w.data_ptr() % 16 == 0 else w.clone()


def scalars(op, eps, weight_offset):
    """(eps, weight_offset) as floats: eps finite and >= 0, weight_offset finite"""
    eps, weight_offset = float(eps), float(weight_offset)
    if not (0.0 <= eps < float("inf")):
        raise RuntimeError(f"{op}: eps must be finite and >= 0, got {eps}")
    if not (abs(weight_offset) < float("inf")):
        raise RuntimeError(f"{op}: weight_offset must be finite, got {weight_offset}")
    return eps, weight_offset


def loss_scalars(op, label_smoothing, logit_scale, lse_square_scale, ignore_index):
    """(label_smoothing, logit_scale, lse_square_scale, ignore_index): label_smoothing in [0, 1), logit_scale finite,
    lse_square_scale finite and >= 0, ignore_index an int64"""
    label_smoothing, logit_scale, lse_square_scale = float(label_smoothing), float(logit_scale), float(lse_square_scale)
    if not (0.0 <= label_smoothing < 1.0):
        raise RuntimeError(f"{op}: label_smoothing must be in [0, 1), got {label_smoothing}")
    if not (abs(logit_scale) < float("inf")):
        raise RuntimeError(f"{op}: logit_scale must be finite, got {logit_scale}")
    if not (0.0 <= lse_square_scale < float("inf")):
        raise RuntimeError(f"{op}: lse_square_scale must be finite and >= 0, got {lse_square_scale}")
    ignore_index = int(ignore_index)
    if not (-2 ** 63 <= ignore_index < 2 ** 63):
        raise RuntimeError(f"{op}: ignore_index must fit an int64, got {ignore_index}")
    return label_smoothing, logit_scale, lse_square_scale, ignore_index


def row_param(op, value, rows, dtype, name):
    """a per-row parameter (sample): a number for every row, or a tensor of `rows` values (any shape that flattens to it; cast to
    `dtype`, made contiguous).  Returns (tensor or None, number or None) - exactly one is set"""
    if isinstance(value, torch.Tensor):
        if value.numel() != rows:
            raise RuntimeError(f"{op}: {name} must be a number or a tensor of one value per row ({rows}), got {tuple(value.shape)}")
        if value.is_floating_point() != dtype.is_floating_point or value.dtype == torch.bool:
            raise RuntimeError(f"{op}: {name} must be {'a floating-point' if dtype.is_floating_point else 'an integer'} tensor, "
                               f"got {value.dtype}")
        return value.reshape(-1).to(dtype).contiguous(), None
    try:
        return None, (float(value) if dtype.is_floating_point else int(value))
    except (TypeError, ValueError):
        raise RuntimeError(f"{op}: {name} must be a number or a tensor of one value per row, got {type(value).__name__}") from None


def same_device(op, tensors, ref, whose):
    """every tensor (None: skipped) on a GPU of this library, and on ref's"""
    _fi._check_device(*tensors)
    dev = ref.device                                      # (read once: every `.device` builds a new object)
    if any(t is not None and t.device != dev for t in tensors):
        raise RuntimeError(f"{op}: every tensor must be on {whose} device")


# ---- q / k of the per-token ops

def k_shape(op, k):
    """k (total_rows, nheads_k, headdim) fp16 / bf16 -> (T, Hk, D)"""
    if k.dtype not in _fi._DTYPES:
        raise RuntimeError(f"{op}: k must be fp16 or bf16, got {k.dtype}")
    if k.dim() != 3:
        raise RuntimeError(f"{op}: k must be (total_rows, nheads_k, headdim), got {tuple(k.shape)}")
    return k.shape


def q_like_k(op, q, k, T, D):
    """q (total_rows, nheads_q, headdim) = (T, *, D) of k's dtype"""
    if q.dtype != k.dtype:
        raise RuntimeError(f"{op}: q must have k's dtype ({k.dtype}), got {q.dtype}")
    if q.dim() != 3 or q.shape[0] != T or q.shape[2] != D:
        raise RuntimeError(f"{op}: q must be (total_rows, nheads_q, headdim) = ({T}, *, {D}), got {tuple(q.shape)}")


def head_dim(op, D):
    if D % 8 != 0 or D > 256:
        raise RuntimeError(f"{op}: head dimension must be a multiple of 8 and <= 256, got {D}")


# ---- the cache pair

def cache_shape(op, k_cache, v_cache):
    if k_cache.dim() != 4 or tuple(k_cache.shape) != tuple(v_cache.shape):
        raise RuntimeError(f"{op}: k_cache and v_cache must have the same 4-D shape, got {tuple(k_cache.shape)} / {tuple(v_cache.shape)}")


def cache_pair(op, k, Hk, D, k_cache, v_cache):
    """the caches against k (total_rows, Hk, D): k's dtype or float8_e4m3fn, 4-D, k's last two dimensions.  Returns fp8"""
    fp8 = k_cache.dtype == _fi._FP8
    if v_cache.dtype != k_cache.dtype or not (fp8 or k_cache.dtype == k.dtype):
        raise RuntimeError(f"{op}: k_cache / v_cache must both have k's dtype ({k.dtype}) or both be float8_e4m3fn, "
                           f"got {k_cache.dtype} / {v_cache.dtype}")
    cache_shape(op, k_cache, v_cache)
    if tuple(k_cache.shape[2:]) != (Hk, D):
        raise RuntimeError(f"{op}: the cache's last two dimensions must be k's (nheads_k, headdim) = {(Hk, D)}, got {tuple(k_cache.shape[2:])}")
    return fp8


def cache_last_dim(op, k_cache, v_cache):
    if k_cache.stride(-1) != 1 or v_cache.stride(-1) != 1:
        raise RuntimeError(f"{op}: k_cache / v_cache must have a contiguous last dimension (a cache is never copied)")


def descales_need_fp8(op, fp8, k_descale, v_descale):
    if not fp8 and (k_descale is not None or v_descale is not None):
        raise RuntimeError(f"{op}: k_descale / v_descale go with a float8_e4m3fn cache")


def fill_cache(s, k_cache, v_cache, fp8, k_descale, v_descale):
    """the cache fields of a block whose `dtype` is set: pointers, strides, num_blocks / page_block_size, cache_dtype, descales"""
    s.k_cache, s.v_cache = k_cache.data_ptr(), v_cache.data_ptr()
    s.kc_batch_stride, s.kc_row_stride, s.kc_head_stride = k_cache.stride(0), k_cache.stride(1), k_cache.stride(2)
    s.vc_batch_stride, s.vc_row_stride, s.vc_head_stride = v_cache.stride(0), v_cache.stride(1), v_cache.stride(2)
    s.num_blocks, s.page_block_size = k_cache.shape[0], k_cache.shape[1]
    s.cache_dtype = _lib.FA_FP8_E4M3 if fp8 else s.dtype
    if fp8:
        s.k_descale = 1.0 if k_descale is None else float(k_descale)
        s.v_descale = 1.0 if v_descale is None else float(v_descale)


# ---- the rotary table pair of the per-token ops

def rope_tables(op, rotary_cos, rotary_sin, dtype, D, hint=""):
    """rotary_cos / rotary_sin (seqlen_ro, rotary_dim / 2) of `dtype`, rotary_dim a positive multiple of 16 and <= D.
    Returns rotary_dim"""
    if rotary_cos.dtype != dtype or rotary_sin.dtype != dtype:
        raise RuntimeError(f"{op}: rotary_cos / rotary_sin must have k's dtype ({dtype}), got {rotary_cos.dtype} / {rotary_sin.dtype}")
    if rotary_cos.dim() != 2 or tuple(rotary_cos.shape) != tuple(rotary_sin.shape):
        raise RuntimeError(f"{op}: rotary_cos and rotary_sin must have the same shape (seqlen_ro, rotary_dim / 2)")
    rotary_dim = 2 * rotary_cos.shape[1]
    if rotary_dim == 0 or rotary_dim % 16 != 0:
        raise RuntimeError(f"{op}: rotary_dim must be a positive multiple of 16, got {rotary_dim}{hint}")
    if rotary_dim > D:
        raise RuntimeError(f"{op}: rotary_dim must be <= headdim ({rotary_dim} > {D})")
    return rotary_dim


def optional_rope(op, positions, rotary_cos, rotary_sin, dtype, T, D):
    """positions / rotary_cos / rotary_sin that may be None together (no rotation).  Returns (rope, rotary_dim, positions):
    rope False where no row is rotated - no tables, or empty ones"""
    given = [positions is not None, rotary_cos is not None, rotary_sin is not None]
    if any(given) and not all(given):
        raise RuntimeError(f"{op}: positions, rotary_cos and rotary_sin go together (all three, or none: no rotation)")
    if not all(given):
        return False, 0, positions
    rotary_dim = rope_tables(op, rotary_cos, rotary_sin, dtype, D)
    return rotary_cos.shape[0] > 0, rotary_dim, ids(op, positions, T, "positions")


def fill_rope(s, positions, rotary_cos, rotary_sin, rotary_dim, interleaved):
    """the rotation fields of a block; returns the contiguous tables, which the caller keeps until the launch is queued"""
    rotary_cos, rotary_sin = rotary_cos.contiguous(), rotary_sin.contiguous()
    s.positions = positions.data_ptr()
    s.rotary_cos, s.rotary_sin = rotary_cos.data_ptr(), rotary_sin.data_ptr()
    s.rotary_dim, s.seqlen_ro, s.rotary_interleaved = rotary_dim, rotary_cos.shape[0], 1 if interleaved else 0
    return rotary_cos, rotary_sin


# ---- the QK-norm weights

def norm_weights(op, q, k, q_weight, k_weight):
    """(q_weight, k_weight) as the kernels take them, None where there is none"""
    if q_weight is not None and q is None:
        raise RuntimeError(f"{op}: q_weight without q")
    if q_weight is not None and k_weight is not None and q_weight.dtype != k_weight.dtype:
        raise RuntimeError(f"{op}: q_weight and k_weight must have the same dtype, got {q_weight.dtype} / {k_weight.dtype}")
    D = k.shape[2]
    qw = None if q_weight is None else weight(op, q_weight, D, k.dtype, "q_weight")
    kw = None if k_weight is None else weight(op, k_weight, D, k.dtype, "k_weight")
    return qw, kw


def fill_norm(s, qw, kw, eps, weight_offset):
    """the norm fields of a block whose `dtype` is set"""
    if qw is not None:
        s.q_weight = qw.data_ptr()
    if kw is not None:
        s.k_weight = kw.data_ptr()
    w = qw if qw is not None else kw
    s.weight_dtype = _lib.FA_FP32 if (w is not None and w.dtype == torch.float32) else s.dtype
    s.eps, s.weight_offset = eps, weight_offset


# ---- slot mode or sequence mode (kv_store, kv_gather).  base / base_name: the op's own per-sequence int32 array of sequence
# mode and its name (cache_seqlens, seq_offsets)

def one_mode(op, slot_mapping, cu_seqlens, base_name):
    if (slot_mapping is None) == (cu_seqlens is None):
        raise RuntimeError(f"{op}: exactly one addressing mode - slot_mapping, or cu_seqlens (with {base_name} and block_table "
                           f"/ cache_batch_idx); {'both' if slot_mapping is not None else 'neither'} given")


def slot_mode(op, base, base_name, block_table, cache_batch_idx):
    if base is not None or block_table is not None or cache_batch_idx is not None:
        raise RuntimeError(f"{op}: slot_mapping takes no {base_name}, block_table or cache_batch_idx")


def sequence_mode(op, k_cache, cu_seqlens, base, base_name, block_table, cache_batch_idx):
    """Returns (B, cu_seqlens, base, block_table, cache_batch_idx) as the kernels take them"""
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1:
        raise RuntimeError(f"{op}: cu_seqlens must be an int32 tensor of shape (batch + 1,)")
    B = cu_seqlens.numel() - 1
    cu_seqlens = cu_seqlens.contiguous()
    if base is not None:
        base = i32(op, base, (B,), base_name)
    if block_table is not None:
        if cache_batch_idx is not None:
            raise RuntimeError(f"{op}: a paged cache (block_table) does not take cache_batch_idx")
        if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B:
            raise RuntimeError(f"{op}: block_table must be an int32 tensor of shape ({B}, max_num_blocks_per_seq)")
        if block_table.stride(1) != 1:
            block_table = block_table.contiguous()
    elif cache_batch_idx is not None:
        cache_batch_idx = i32(op, cache_batch_idx, (B,), "cache_batch_idx")
    elif k_cache.shape[0] < B:
        raise RuntimeError(f"{op}: the cache has {k_cache.shape[0]} batch slots for {B} sequences (pass cache_batch_idx)")
    return B, cu_seqlens, base, block_table, cache_batch_idx


def fill_mode(s, slot_mapping, cu_seqlens, B, base, base_name, block_table, cache_batch_idx):
    """the addressing fields of a block; the op's own array goes into the field of its name"""
    if slot_mapping is not None:
        s.slot_mapping = slot_mapping.data_ptr()
        return
    s.cu_seqlens, s.batch = cu_seqlens.data_ptr(), B
    if base is not None:
        setattr(s, base_name, base.data_ptr())
    if block_table is not None:
        s.paged = 1
        s.block_table, s.block_table_batch_stride = block_table.data_ptr(), block_table.stride(0)
        s.max_blocks = block_table.shape[1]
    elif cache_batch_idx is not None:
        s.cache_batch_idx = cache_batch_idx.data_ptr()


# ---- fa_rope_store and fa_qk_norm_rope_store: one validate / allocate / fill / launch sequence

def rope_and_store(op, params_type, call, norm, rope_optional, hints, q, k, v, positions, rotary_cos, rotary_sin, k_cache, v_cache,
                   slot_mapping, interleaved, inplace, k_out, k_descale, v_descale):
    """`rope_store.rope_and_store_kv` and `qk_norm.qk_norm_rope_and_store_kv`, which say what runs: params_type / call - the
    parameter block and the _lib.call_* of the entry point (two kernels: the plain op is never routed through the norm's);
    norm - None, or (q_weight, k_weight, eps, weight_offset) for a block with the norm fields; rope_optional - positions and
    the tables may be None together; hints - what the plain op's messages add about rotating only: (to "or neither", to "v and
    slot_mapping go with the caches", to the rotary_dim rule).  Returns (q_out, k_out)."""
    T, Hk, D = k_shape(op, k)
    if q is not None:
        q_like_k(op, q, k, T, D)
    Hq = 0 if q is None else q.shape[1]
    head_dim(op, D)
    cached = k_cache is not None or v_cache is not None
    if cached:
        if k_cache is None or v_cache is None:
            raise RuntimeError(f"{op}: k_cache and v_cache must both be given (or neither{hints[0]})")
        if v is None or slot_mapping is None:
            raise RuntimeError(f"{op}: caches need v and slot_mapping")
        if v.dtype != k.dtype:
            raise RuntimeError(f"{op}: v must have k's dtype ({k.dtype}), got {v.dtype}")
        if tuple(v.shape) != tuple(k.shape):
            raise RuntimeError(f"{op}: k and v must have the same shape (total_rows, nheads_k, headdim), got {tuple(k.shape)} / {tuple(v.shape)}")
        fp8 = cache_pair(op, k, Hk, D, k_cache, v_cache)
        cache_last_dim(op, k_cache, v_cache)
    else:
        fp8 = False
        if v is not None or slot_mapping is not None:
            raise RuntimeError(f"{op}: v and slot_mapping go with k_cache / v_cache{hints[1]}")
        if q is None and not k_out:
            raise RuntimeError(f"{op}: nothing to do - no caches, no q and k_out=False")
    descales_need_fp8(op, fp8, k_descale, v_descale)
    if rope_optional:
        rope, rotary_dim, positions = optional_rope(op, positions, rotary_cos, rotary_sin, k.dtype, T, D)
    else:
        rope, rotary_dim = True, rope_tables(op, rotary_cos, rotary_sin, k.dtype, D, hints[2])
        positions = ids(op, positions, T, "positions")
    qw = kw = None
    if norm is not None:
        qw, kw = norm_weights(op, q, k, norm[0], norm[1])
        eps, weight_offset = scalars(op, norm[2], norm[3])
    if cached:
        slot_mapping = ids(op, slot_mapping, T, "slot_mapping")
    same_device(op, [q, k, v, positions, rotary_cos, rotary_sin, k_cache, v_cache, slot_mapping, qw, kw], k, "k's")

    write_k = bool(k_out)
    qi = None if q is None else view(op, q, D, inplace, "q")
    ki = view(op, k, D, inplace and write_k, "k")
    if inplace:
        qo, ko = qi, (ki if write_k else None)
    else:
        qo = None if q is None else torch.empty(q.shape, dtype=q.dtype, device=q.device)
        ko = torch.empty(k.shape, dtype=k.dtype, device=k.device) if write_k else None
    if T == 0 or (Hq == 0 and Hk == 0):
        return qo, ko

    s = params_type()
    s.struct_size = ctypes.sizeof(params_type)
    if qi is not None:
        s.q, s.q_out = qi.data_ptr(), qo.data_ptr()
        s.q_row_stride, s.q_head_stride = qi.stride(0), qi.stride(1)
        s.qo_row_stride, s.qo_head_stride = qo.stride(0), qo.stride(1)
    s.k = ki.data_ptr()
    s.k_row_stride, s.k_head_stride = ki.stride(0), ki.stride(1)
    if ko is not None:
        s.k_out = ko.data_ptr()
        s.ko_row_stride, s.ko_head_stride = ko.stride(0), ko.stride(1)
    if rope:
        rotary_cos, rotary_sin = fill_rope(s, positions, rotary_cos, rotary_sin, rotary_dim, interleaved)
    s.total_rows, s.nheads_q, s.nheads_k, s.head_dim = T, Hq, Hk, D
    s.dtype = s.cache_dtype = _fi._DTYPES[k.dtype]
    if norm is not None:
        fill_norm(s, qw, kw, eps, weight_offset)
    vi = None
    if cached:
        vi = _fi._prep(v, D)
        s.v = vi.data_ptr()
        s.v_row_stride, s.v_head_stride = vi.stride(0), vi.stride(1)
        fill_cache(s, k_cache, v_cache, fp8, k_descale, v_descale)
        s.slot_mapping = slot_mapping.data_ptr()
    with _fi._on_device(k.device):
        call(s, _fi._stream(k.device))                       # (queued: the tensors made here stay referenced until here)
    del qi, ki, vi, positions, slot_mapping, rotary_cos, rotary_sin, qw, kw
    return qo, ko
