"""Speculative-decoding verification on the library's `fa_spec_accept` / `fa_spec_walk` kernels (csrc/fa_spec_verify.hip): which
draft tokens of a chain or tree are accepted, what is emitted, and where the accepted path goes in the cache - the step between
`flash_attn_with_kvcache(..., tree_mask=, tree_depths=)` (the draft scored in one pass), `sample` (ids from logits) and
`move_kv_cache` (the commit).  The rules (include/fa_mi355.h):

    A request has T nodes (1 <= T <= 64), the query tokens of the tree-attention call.  Node 0 is the root, the last accepted
    token; node t >= 1 has parents[t] in [0, t) (tests/tree_ref.py's convention); any other parents[t] marks a PADDING node that
    is never visited (ragged draft lengths in a fixed-shape batch).  parents: int32 [B, T] or [T]; None: the chain t - 1.
    draft_ids: int32 / int64 [B, T], entry 0 ignored.  target_logits [B, T, V] (fp16 / bf16 / fp32, V <= 2^20): row t is the
    target's distribution for the token that FOLLOWS node t; a row may be `top_k_top_p_filter`'s output as it is (that is how
    target-side filters compose - verification itself takes a temperature, per request, and nothing else; !(T > 0) is greedy).

    Mode A, draft_probs None (deterministic drafts: EAGLE / Medusa / n-gram trees): every node's target row is sampled by
    `sample`'s rules (one fa_sample call over the B T rows with u_sample [B, T]); the walk starts at c = 0, emits
    y = target_ids[c] and moves to the child of c of LOWEST index whose draft token is y; none: stop.  Lossless: every emitted
    token is a draw from the target at its node.

    Mode B, draft_probs [B, T, V] (fp32 / bf16 / fp16; row 0 ignored; used as they are, never renormalised): the rule of
    Leviathan et al. per node t >= 1 with the target row P = parents[t] and d = draft_ids[t]:
        p_j = e_j * (1 / s) from sample's masses e_j and fa_lse.h's sum-exp s;  accept = (u_accept * q_d < p_d)
        r_j = max(p_j - q_j, 0),  R_j = floor(r_j 2^40),  R = sum R_j  (R == 0: R_j = floor(e_j 2^40), the target's own masses)
        recovered = the smallest index whose index-order running sum of R_j exceeds min(floor(u_recover R), R - 1)
        a greedy row: accept = (d == j*), recovered = j*;  an empty row: accept = 0, recovered = -1;  d outside [0, V): reject
    The walk looks at the FIRST (lowest-index) child t of c only - its siblings are ignored: accepted - emit d, c = t;
    rejected - emit recovered[t], stop; no child - emit target_ids[c] (the bonus token), stop.  With parents None only the last
    node can be without a child, so only column T - 1 of the target ids is sampled (B rows, a strided view).

    Outputs (int32, every element written): out_tokens [B, T] - the emitted tokens in order, then -1; num_out [B] in 1 .. T;
    path_nodes [B, T] - 0, t_1, t_2, .. (the accepted nodes, root included), then -1.  A target id of -1 (an empty row) is
    emitted and ends the walk.

The kernels hold no RNG: uniform numbers are drawn here with `torch.rand(generator=...)` where the caller passes none - pass them
for a captured graph.  A node's result depends on its rows, d, the temperature and its uniform numbers alone, not on the batch.

Not covered: multi-child trees with draft probabilities (SpecInfer's multi-round rule - only the first child is tried); typical
acceptance; an in-kernel RNG; a fused commit (`commit_slots` + `move_kv_cache` are separate launches).  Nothing here is exported
through the packages' `__all__` lists."""
import ctypes

import torch

from . import _lib
from . import _rowargs as _ra
from . import flash_attn_interface as _fi
from . import sample as _sample

_OP = "spec_decode"
_CODES = _sample._CODES
NODES_MAX = 64


def _shape(target_logits, draft_ids):
    if target_logits.dtype not in _CODES:
        raise RuntimeError(f"{_OP}: target_logits must be fp16, bf16 or fp32, got {target_logits.dtype}")
    if target_logits.dim() != 3:
        raise RuntimeError(f"{_OP}: target_logits must be [B, T, V], got {tuple(target_logits.shape)}")
    B, T, V = target_logits.shape
    if not (1 <= T <= NODES_MAX):
        raise RuntimeError(f"{_OP}: T must be in 1 .. {NODES_MAX}, got {T}")
    if not (1 <= V <= _sample.VOCAB_MAX):
        raise RuntimeError(f"{_OP}: V must be in 1 .. 2^20, got {V}")
    _ids_shape(draft_ids, B, T, "draft_ids")
    return B, T, V


def _ids_shape(t, B, T, name):
    if t.dtype not in (torch.int32, torch.int64) or tuple(t.shape) != (B, T):
        raise RuntimeError(f"{_OP}: {name} must be an int32 or int64 tensor of shape ({B}, {T}), got {t.dtype} {tuple(t.shape)}")


def _draft_ids(draft_ids, V):
    """int32 [B, T], contiguous; an int64 id that is no token (outside [0, V)) becomes -1 before it is narrowed"""
    if draft_ids.dtype == torch.int64:
        draft_ids = torch.where((draft_ids >= 0) & (draft_ids < V), draft_ids, -1).to(torch.int32)
    return draft_ids.contiguous()


def _parents(parents, B, T):
    """(int32 tensor or None, batch stride in elements)"""
    if parents is None:
        return None, 0
    if parents.dtype != torch.int32 or tuple(parents.shape) not in ((B, T), (T,)):
        raise RuntimeError(f"{_OP}: parents must be an int32 tensor of shape ({B}, {T}) or ({T},), got {parents.dtype} "
                           f"{tuple(parents.shape)}")
    parents = parents.contiguous()
    return parents, (T if parents.dim() == 2 else 0)


def _uniform(u, B, T, name):
    if not isinstance(u, torch.Tensor) or u.dtype != torch.float32 or tuple(u.shape) != (B, T):
        raise RuntimeError(f"{_OP}: {name} must be a float32 tensor of shape ({B}, {T})")
    return u.contiguous()


def _i32_out(B, T, dev):
    return torch.empty((B, T), dtype=torch.int32, device=dev)


def accept_forward(target_logits, draft_probs, draft_ids, u_accept, u_recover, *, parents=None, temperature=1.0):
    """fa_spec_accept alone: (accept int32 [B, T], recovered int32 [B, T]) by the rules of mode B at the top of this module; node 0
    and padding nodes get 0 and -1.  u_accept / u_recover: fp32 [B, T] (None only where temperature is a number that is not above
    0).  Three launches on the current stream; the tensors are taken as the views they are where their rows flatten to one
    stride."""
    B, T, V = _shape(target_logits, draft_ids)
    if draft_probs.dtype not in _CODES or tuple(draft_probs.shape) != (B, T, V):
        raise RuntimeError(f"{_OP}: draft_probs must be fp16, bf16 or fp32 of shape {(B, T, V)}, got {draft_probs.dtype} "
                           f"{tuple(draft_probs.shape)}")
    tt, tv = _ra.row_param(_OP, temperature, B, torch.float32, "temperature")
    if u_accept is None and u_recover is None:
        if tt is not None or tv > 0:
            raise RuntimeError(f"{_OP}: u_accept and u_recover are needed unless temperature is a number that is not above 0")
    else:
        u_accept, u_recover = _uniform(u_accept, B, T, "u_accept"), _uniform(u_recover, B, T, "u_recover")
    par, par_bs = _parents(parents, B, T)
    _ra.same_device(_OP, [target_logits, draft_probs, draft_ids, u_accept, u_recover, par, tt], target_logits, "target_logits'")
    dev = target_logits.device
    d = _draft_ids(draft_ids, V)
    accept, recovered = _i32_out(B, T, dev), _i32_out(B, T, dev)
    if B == 0:
        return accept, recovered
    xi, qi = _sample._rows(target_logits, V), _sample._rows(draft_probs, V)
    s = _lib.FaSpecAcceptParams()
    s.struct_size = ctypes.sizeof(_lib.FaSpecAcceptParams)
    s.target_logits, s.logits_row_stride = xi.data_ptr(), xi.stride(0)
    s.draft_probs, s.probs_row_stride = qi.data_ptr(), qi.stride(0)
    s.draft_ids = d.data_ptr()
    if par is not None:
        s.parents, s.parents_batch_stride = par.data_ptr(), par_bs
    if u_accept is not None:
        s.u_accept, s.u_recover = u_accept.data_ptr(), u_recover.data_ptr()
    if tt is not None:
        s.temperature = tt.data_ptr()
    else:
        s.temperature_value = tv
    s.accept, s.recovered = accept.data_ptr(), recovered.data_ptr()
    s.batch, s.nodes, s.vocab = B, T, V
    s.dtype, s.probs_dtype = _CODES[xi.dtype], _CODES[qi.dtype]
    nbytes = _lib.spec_accept_workspace_bytes(s)
    ws = _fi._workspace(nbytes, dev)
    if ws is not None:
        s.workspace, s.workspace_bytes = ws.data_ptr(), nbytes
    with _fi._on_device(dev):
        _lib.call_spec_accept(s, _fi._stream(dev))            # (queued: the tensors made here stay referenced until here)
    del xi, qi, d, par, tt, ws
    return accept, recovered


def walk(draft_ids, target_ids, *, parents=None, accept=None, recovered=None):
    """fa_spec_walk alone: (out_tokens int32 [B, T], num_out int32 [B], path_nodes int32 [B, T]).  target_ids: int32 [B, T], or
    [B] - one id per request, which serves every node (the bonus token of a chain).  accept / recovered (int32 [B, T],
    `accept_forward`'s outputs) select mode B; both None: mode A.  One launch, one wave per request."""
    if draft_ids.dim() != 2:
        raise RuntimeError(f"{_OP}: draft_ids must be [B, T], got {tuple(draft_ids.shape)}")
    B, T = draft_ids.shape
    if not (1 <= T <= NODES_MAX):
        raise RuntimeError(f"{_OP}: T must be in 1 .. {NODES_MAX}, got {T}")
    _ids_shape(draft_ids, B, T, "draft_ids")
    if target_ids.dtype != torch.int32 or tuple(target_ids.shape) not in ((B, T), (B,)):
        raise RuntimeError(f"{_OP}: target_ids must be an int32 tensor of shape ({B}, {T}) or ({B},), got {target_ids.dtype} "
                           f"{tuple(target_ids.shape)}")
    if (accept is None) != (recovered is None):
        raise RuntimeError(f"{_OP}: accept and recovered go together (both, or neither: deterministic drafts)")
    if accept is not None:
        for name, t in (("accept", accept), ("recovered", recovered)):
            if t.dtype != torch.int32 or tuple(t.shape) != (B, T):
                raise RuntimeError(f"{_OP}: {name} must be an int32 tensor of shape ({B}, {T}), got {t.dtype} {tuple(t.shape)}")
        accept, recovered = accept.contiguous(), recovered.contiguous()
    par, par_bs = _parents(parents, B, T)
    _ra.same_device(_OP, [draft_ids, target_ids, par, accept, recovered], draft_ids, "draft_ids'")
    dev = draft_ids.device
    d = _draft_ids(draft_ids, 1 << 31)
    tid = target_ids.contiguous()
    out_tokens, path_nodes = _i32_out(B, T, dev), _i32_out(B, T, dev)
    num_out = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return out_tokens, num_out, path_nodes
    s = _lib.FaSpecWalkParams()
    s.struct_size = ctypes.sizeof(_lib.FaSpecWalkParams)
    s.draft_ids, s.target_ids = d.data_ptr(), tid.data_ptr()
    s.target_ids_batch_stride, s.target_ids_node_stride = (T, 1) if tid.dim() == 2 else (1, 0)
    if par is not None:
        s.parents, s.parents_batch_stride = par.data_ptr(), par_bs
    if accept is not None:
        s.accept, s.recovered = accept.data_ptr(), recovered.data_ptr()
    s.out_tokens, s.num_out, s.path_nodes = out_tokens.data_ptr(), num_out.data_ptr(), path_nodes.data_ptr()
    s.batch, s.nodes = B, T
    with _fi._on_device(dev):
        _lib.call_spec_walk(s, _fi._stream(dev))              # (queued: the tensors made here stay referenced until here)
    del d, tid, par, accept, recovered
    return out_tokens, num_out, path_nodes


def _row_temperature(tt, tv, T):
    """the per-request temperature as fa_sample takes it for B T rows"""
    return tv if tt is None else tt.repeat_interleave(T)


def verify_forward(target_logits, draft_ids, draft_probs, parents, temperature, u_sample, u_accept, u_recover):
    """`verify` with every uniform tensor given (u_accept / u_recover None in mode A): what torch.ops...spec_verify runs"""
    B, T, V = _shape(target_logits, draft_ids)
    tt, tv = _ra.row_param(_OP, temperature, B, torch.float32, "temperature")
    u_sample = _uniform(u_sample, B, T, "u_sample")
    if draft_probs is None:
        ids, _, _ = _sample.sample_forward(target_logits, u_sample, temperature=_row_temperature(tt, tv, T))
        return walk(draft_ids, ids, parents=parents)
    accept, recovered = accept_forward(target_logits, draft_probs, draft_ids, u_accept, u_recover, parents=parents,
                                       temperature=temperature)
    if parents is None:
        # only the last node of a chain can be without a child: sample that column alone, B rows of stride T V
        ids, _, _ = _sample.sample_forward(target_logits[:, T - 1], u_sample[:, T - 1], temperature=temperature)
    else:
        ids, _, _ = _sample.sample_forward(target_logits, u_sample, temperature=_row_temperature(tt, tv, T))
    return walk(draft_ids, ids, parents=parents, accept=accept, recovered=recovered)


def verify(target_logits, draft_ids, *, draft_probs=None, parents=None, temperature=1.0, u_sample=None, u_accept=None,
           u_recover=None, generator=None):
    """(out_tokens, num_out, path_nodes) of a speculative-decoding step by the rules at the top of this module.  draft_probs
    None: mode A; given: mode B.  u_sample / u_accept / u_recover: fp32 [B, T] uniform numbers in [0, 1), each drawn with
    torch.rand(generator=generator) where None (pass them for a captured graph; u_accept / u_recover are mode B's)."""
    B, T, V = _shape(target_logits, draft_ids)
    tt, tv = _ra.row_param(_OP, temperature, B, torch.float32, "temperature")
    if draft_probs is None and (u_accept is not None or u_recover is not None):
        raise RuntimeError(f"{_OP}: u_accept / u_recover go with draft_probs")
    _fi._check_device(target_logits)
    draw = lambda: torch.rand((B, T), dtype=torch.float32, device=target_logits.device, generator=generator)   # noqa: E731
    u_sample = draw() if u_sample is None else u_sample
    if draft_probs is not None:
        u_accept = draw() if u_accept is None else u_accept
        u_recover = draw() if u_recover is None else u_recover
    from . import torch_ops as _ops                            # (registers torch.ops.flash_attn_mi355.spec_verify)
    return _ops.spec_verify(target_logits, draft_ids, draft_probs, parents, tt, 1.0 if tv is None else tv, u_sample, u_accept,
                            u_recover)


def commit_slots(path_nodes, cache_seqlens, *, block_table=None, page_block_size=None, cache_batch_idx=None, seqlen_cache=None):
    """`move_kv_cache`'s (src_slots, dst_slots), int64 [B T], from the accepted path: the tree call appended node t of request b
    at position cache_seqlens[b] + t; path entry i (node t_i) goes to position cache_seqlens[b] + i; the padded entries (-1) get
    slot -1 in both, which the gather and the store skip.  A paged cache: block_table int32 [B, W] and page_block_size; a
    contiguous cache [B', S, H, D]: seqlen_cache = S and optionally cache_batch_idx int32 [B].  Plain torch on path_nodes' device:
    fixed shapes, no host synchronisation - capturable."""
    if path_nodes.dim() != 2 or path_nodes.dtype != torch.int32:
        raise RuntimeError(f"{_OP}: path_nodes must be an int32 tensor [B, T], got {path_nodes.dtype} {tuple(path_nodes.shape)}")
    B, T = path_nodes.shape
    if tuple(cache_seqlens.shape) != (B,):
        raise RuntimeError(f"{_OP}: cache_seqlens must have shape ({B},), got {tuple(cache_seqlens.shape)}")
    if (block_table is None) == (seqlen_cache is None) or (block_table is not None) != (page_block_size is not None):
        raise RuntimeError(f"{_OP}: pass block_table with page_block_size (a paged cache) or seqlen_cache (a contiguous one)")
    dev = path_nodes.device
    keep = path_nodes >= 0
    L = cache_seqlens.to(torch.int64).unsqueeze(1)
    src_pos = L + path_nodes.to(torch.int64).clamp(min=0)
    dst_pos = L + torch.arange(T, dtype=torch.int64, device=dev).unsqueeze(0)
    if block_table is not None:
        if block_table.dim() != 2 or block_table.shape[0] != B:
            raise RuntimeError(f"{_OP}: block_table must be [{B}, max_num_blocks_per_seq], got {tuple(block_table.shape)}")
        page, bt = int(page_block_size), block_table.to(torch.int64)
        slot = lambda pos: bt.gather(1, (pos // page).clamp(0, bt.shape[1] - 1)) * page + pos % page   # noqa: E731
    else:
        if cache_batch_idx is None:
            row = torch.arange(B, dtype=torch.int64, device=dev)
        else:
            row = cache_batch_idx.to(torch.int64)
        S = int(seqlen_cache)
        slot = lambda pos: row.unsqueeze(1) * S + pos        # noqa: E731
    minus = torch.full((), -1, dtype=torch.int64, device=dev)
    src = torch.where(keep, slot(src_pos), minus)
    dst = torch.where(keep, slot(dst_pos), minus)
    return src.reshape(-1), dst.reshape(-1)
