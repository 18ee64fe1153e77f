"""What surrounds the expert GEMMs of a mixture-of-experts block, on the library's `fa_moe_*` kernels (csrc/fa_moe.hip): top-k
routing with its gradient, the stable sort of the (token, k) slots by expert, the permutation of the activations into per-expert
segments and the weighted combine with its backward - and, on csrc/fa_moe_gemm.hip, the forward grouped expert GEMM `moe_gemm`
over the contiguous, `align`-padded segments of `xp` that `expert_offsets` describes, on csrc/fa_moe_gemm_wgrad.hip its weight and
bias gradients `moe_gemm_wgrad`, and on the two of them `moe_linear`, the expert layer autograd differentiates (their docstrings
have their contracts).

    weights, ids = moe_route(logits, k)                         # fp32 [T, K], int32 [T, K]
    sorted_slot, pos, expert_offsets = moe_sort(ids, E, align=16)
    xp = moe_permute(x, sorted_slot, k, pos=pos)                # [M_max, N], M_max = T K + E (align - 1)
    yp = experts(xp, expert_offsets)                            # the grouped GEMMs: moe_gemm(xp, w, expert_offsets), or the
                                                                # first one as moe_gemm(x, w, .., sorted_slot=.., top_k=k) without xp
    out = moe_combine(yp, weights, pos)                         # [T, N]

  training, the experts as differentiable layers (no xp; dx by moe_gemm + moe_combine, dw and dbias by moe_gemm_wgrad):
    h = moe_linear(x, w1, expert_offsets, sorted_slot=sorted_slot, top_k=k, pos=pos)      # gate-up, fused gather
    yp = moe_linear(act_and_mul(h), w2, expert_offsets)                                   # down

No function synchronises with the host, every result is a pure function of its inputs (no ordering depends on an atomic, two calls
give the same bits), all are capturable in a HIP graph.

`moe_route` - fp32 throughout, every operation rounds once, in exactly this order (it depends on (E, K, dtype) alone: a row's bits
do not depend on the batch or on the row's index):

    "softmax"  z_j = float(logit_j), a NaN read as -inf;   selection score c_j = z_j   (exact comparisons, no exp)
    "sigmoid"  s_j = rcp(1 + exp2(-float(logit_j) * log2e))    act_mul's sigmoid: hardware exp2 (v_exp_f32) and reciprocal (v_rcp_f32)
               c_j = s_j + bias_j (bias fp32 [E]; None: c_j = s_j), a NaN read as -inf
    select     K rounds; round k takes the largest c_j not yet taken, the LOWEST index among equals (-0 == +0).  Slot k of a row
               holds the k-th winner, so the ids of a row are distinct and inside [0, E) whatever the logits hold.
    softmax, renormalize=True    m = c_{id_0};  e_k = exp2((c_{id_k} - m) * log2e);  S = e_0 + e_1 + .. (ascending k);  w_k = e_k / S
    softmax, renormalize=False   m = c_{id_0};  e_j = exp2((z_j - m) * log2e) for all E columns;  Z = sum_j e_j: a lane's 8 columns
                                 in column order (a row lies 8 columns per lane in G adjacent lanes, G the smallest power of two
                                 with 8 G >= E; absent columns +0), then a xor butterfly over the G lanes;  w_k = e_{id_k} / Z
    sigmoid                      w_k = s_{id_k}, without the bias;  renormalize: S = w_0 + w_1 + .. (ascending k), w_k = w_k / S
    last                         w_k = w_k * scale   (`routed_scaling_factor`).  The divisions are IEEE divisions.

Special values follow these lines literally; none is a fault, a device assert or a host synchronisation:
    all logits equal             ids 0 .. K - 1 (the lowest indices); softmax renormalised: every weight 1 / K up to the division
    all -inf (softmax)           ids 0 .. K - 1; m = -inf, -inf - -inf = NaN: every weight NaN.  The same for a row of NaNs.
    a +inf logit (softmax)       it is selected first; m = +inf, inf - inf = NaN: every weight of the row NaN
    a NaN logit (softmax)        read as -inf: it loses against every number, and if selected all the same has weight 0
    a NaN logit (sigmoid)        its score is -inf; if it is selected all the same (fewer than K numbers) its weight is NaN, and
                                 under renormalize so is every weight of the row
    +-inf logit (sigmoid)        s = 1 / 0: ordinary values
    a NaN / inf bias             enters c_j alone: NaN -> -inf, +inf wins, -inf loses; the weight never sees the bias

`moe_route_backward` recomputes the selected scores from the logits in the forward's order (nothing but `ids` is saved), treats
the roundings to the io dtype as straight-through, and writes every element of dlogits (unselected columns +0 where the formula
says so: everywhere but softmax without renormalisation, which is dense): with g_k = dW_k * scale and D = fma(g_k, w_k, D) in
ascending k from +0 (sigmoid + renormalize: D = fma(dW_k, w_k, D)),
    softmax, renormalize=False   dl_j = p_j * (([j selected] ? g_j : 0) - D),  p = e / Z
    softmax, renormalize=True    dl_{id_k} = w_k * (g_k - D)
    sigmoid                      ds_k = g_k, or renormalize: ((dW_k - D) * scale) / S;   dl_{id_k} = (ds_k * s_k) * (1 - s_k)
with one rounding to the logits' dtype.  The bias has no gradient here (it is a buffer in DeepSeek-V3).

`moe_sort` is a stable counting sort: slot s = t * K + k; segment e starts at expert_offsets[e] (a multiple of `align`), holds the
slots routed to e in ascending order and is padded to the next multiple of `align` with sorted_slot = -1; expert_offsets[E] is
the padded total and everything behind it, up to M_max = T K + E (align - 1), is -1.  pos[t, k] is the slot's row, -1 for an id
outside [0, E) - a dropped slot (an expert-parallel `expert_map`), which is only ever compared, never an address.

`moe_permute` copies row sorted_slot[r] // K of x to row r bit for bit (padding rows +0); with `scale` (fp32 [T, K]) row r is
round16(scale[slot] * x[slot // K]).  `moe_combine` is out[t] = round16(sum_k w[t, k] * float(y[pos[t, k]])), fma in ascending k
from +0, one rounding; a pos of -1 is skipped and a token with no live slot is +0.  `moe_combine_backward`: dy[pos[t, k]] =
round16(w[t, k] * dout[t]) - the scaled permute, bit for bit - with padding rows +0, and dw[t, k] = sum_n dout[t, n] *
y[pos[t, k], n] in add_norm's fixed row-sum order (dropped slots +0).

Limits (outside them: RuntimeError naming the argument, before any device work): T >= 0, 2 <= E <= 512, 1 <= K <= min(E, 16), N a
multiple of 8 up to 16384 in fp16 / bf16, T K + E (align - 1) < 2^31, 1 <= align <= 256.  CPU tensors raise: there is no fallback.

Not covered: grouped top-k (`n_group` / `topk_group`), capacity factors and token dropping by load, the auxiliary load-balancing
loss, a gradient for the router's bias or for permute's scale, an fp8 / quantised permute, fusing an activation or the combine
into the expert GEMMs, a split over rows in their weight gradient, a gradient through the tables, expert-parallel all-to-all,
E > 512, K > 16, fp32 activations, a double backward.  Nothing here is exported through
the packages' `__all__` lists."""
import ctypes

import torch

from . import _lib
from . import _rowargs as _ra
from . import flash_attn_interface as _fi

MAX_EXPERTS, MAX_TOPK, MAX_ALIGN, MAX_N = 512, 16, 256, 16384
GEMM_MAX_K, GEMM_MAX_N, GEMM_MAX_ROW_STRIDE = 32768, 65536, 2 ** 22
W_LAYOUTS = {"nk": _lib.FA_MOE_W_NK, "kn": _lib.FA_MOE_W_KN}
SCORINGS = {"softmax": _lib.FA_MOE_SOFTMAX, "sigmoid": _lib.FA_MOE_SIGMOID}
_LOGIT_DTYPES = {torch.float16: _lib.FA_FP16, torch.bfloat16: _lib.FA_BF16, torch.float32: _lib.FA_FP32}


def _sizes(op, E, K):
    if not (2 <= E <= MAX_EXPERTS):
        raise RuntimeError(f"{op}: num_experts must be in [2, {MAX_EXPERTS}], got {E}")
    if not (1 <= K <= min(E, MAX_TOPK)):
        raise RuntimeError(f"{op}: k must be in [1, min(num_experts, {MAX_TOPK})] = [1, {min(E, MAX_TOPK)}], got {K}")


def _slots(op, T, K):
    if T * K >= 2 ** 31:
        raise RuntimeError(f"{op}: tokens x k must stay below 2^31, got {T} x {K}")


def _topk(op, K):
    if not (1 <= K <= MAX_TOPK):
        raise RuntimeError(f"{op}: k must be in [1, {MAX_TOPK}], got {K}")


def _route_args(op, logits, k, scoring, bias, scale):
    """(T, E, scoring code, scale) of a router call; everything here needs no device"""
    if scoring not in SCORINGS:
        raise RuntimeError(f"{op}: scoring must be one of {sorted(SCORINGS)}, got {scoring!r}")
    if logits.dtype not in _LOGIT_DTYPES:
        raise RuntimeError(f"{op}: logits must be fp16, bf16 or fp32, got {logits.dtype}")
    if logits.dim() != 2:
        raise RuntimeError(f"{op}: logits must be [tokens, num_experts], got {tuple(logits.shape)}")
    T, E = logits.shape
    k = int(k)
    _sizes(op, E, k)
    _slots(op, T, k)
    if bias is not None:
        if scoring != "sigmoid":
            raise RuntimeError(f"{op}: bias goes with scoring='sigmoid'")
        if bias.dtype != torch.float32 or tuple(bias.shape) != (E,):
            raise RuntimeError(f"{op}: bias must be an fp32 tensor of shape ({E},), got {bias.dtype} {tuple(bias.shape)}")
    scale = float(scale)
    if not (abs(scale) < float("inf")):
        raise RuntimeError(f"{op}: scale must be finite, got {scale}")
    return T, E, k, SCORINGS[scoring], scale


def _logit_rows(t):
    """[T, E] as the kernels take it: any row stride with a contiguous last dimension as it is, anything else copied"""
    return t if (t.stride(1) == 1 or t.shape[1] == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]) else t.contiguous()


def _hidden(op, t, name, rows=None):
    """a [rows, N] fp16 / bf16 activation: N"""
    if t.dtype not in _fi._DTYPES:
        raise RuntimeError(f"{op}: {name} must be fp16 or bf16, got {t.dtype}")
    if t.dim() != 2 or (rows is not None and t.shape[0] != rows):
        raise RuntimeError(f"{op}: {name} must be [{'rows' if rows is None else rows}, N], got {tuple(t.shape)}")
    N = t.shape[1]
    if N < 8 or N > MAX_N or N % 8:
        raise RuntimeError(f"{op}: the hidden size N of {name} must be a multiple of 8 in [8, {MAX_N}], got {N}")
    return N


def _hidden_rows(t):
    """[rows, N] as the piece kernels take it: 16-byte aligned rows (a copy where they are not)"""
    ok = t.stride(1) == 1 and t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])
    if ok:
        return t
    c = t.contiguous()
    return c if c.data_ptr() % 16 == 0 else c.clone()


def _table(op, t, shape, dtype, name):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{op}: {name} must be {str(dtype).replace('torch.', '')} of shape {tuple(shape)}, got "
                           f"{str(t.dtype).replace('torch.', '')} {tuple(t.shape)}")
    return t.contiguous()


def moe_route_forward(logits, k, *, scoring="softmax", renormalize=True, bias=None, scale=1.0, out=None):
    """The router alone, no autograd: (weights fp32 [T, K], ids int32 [T, K]).  out=(weights, ids): contiguous tensors to write."""
    op = "moe_route"
    T, E, k, sc, scale = _route_args(op, logits, k, scoring, bias, scale)
    w = i = None
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise RuntimeError(f"{op}: out must be the pair (weights, ids)")
        w = _table(op, out[0], (T, k), torch.float32, "out[0]")
        i = _table(op, out[1], (T, k), torch.int32, "out[1]")
        if w is not out[0] or i is not out[1]:
            raise RuntimeError(f"{op}: out tensors must be contiguous")
    _ra.same_device(op, [logits, bias, w, i], logits, "logits'")
    dev = logits.device
    if w is None:
        w = torch.empty((T, k), dtype=torch.float32, device=dev)
        i = torch.empty((T, k), dtype=torch.int32, device=dev)
    if T == 0:
        return w, i
    li = _logit_rows(logits)
    bi = None if bias is None else bias.contiguous()
    s = _lib.FaMoeRouteParams()
    s.struct_size = ctypes.sizeof(_lib.FaMoeRouteParams)
    s.logits, s.logits_row_stride = li.data_ptr(), li.stride(0)
    if bi is not None:
        s.bias = bi.data_ptr()
    s.weights, s.ids = w.data_ptr(), i.data_ptr()
    s.tokens, s.num_experts, s.top_k = T, E, k
    s.dtype, s.scoring, s.renormalize, s.scale = _LOGIT_DTYPES[logits.dtype], sc, 1 if renormalize else 0, scale
    with _fi._on_device(dev):
        _lib.call_moe_route(s, _fi._stream(dev))              # (queued: the tensors made here stay referenced until here)
    del li, bi
    return w, i


def moe_route_backward(dweights, logits, ids, *, scoring="softmax", renormalize=True, bias=None, scale=1.0):
    """dlogits [T, E] of the logits' dtype, every element written, from dweights fp32 [T, K], the forward's logits and ids"""
    op = "moe_route_backward"
    if ids.dim() != 2:
        raise RuntimeError(f"{op}: ids must be [tokens, k], got {tuple(ids.shape)}")
    T, E, k, sc, scale = _route_args(op, logits, ids.shape[1], scoring, bias, scale)
    ids = _table(op, ids, (T, k), torch.int32, "ids")
    if dweights.dtype != torch.float32:
        dweights = dweights.float()
    dweights = _table(op, dweights, (T, k), torch.float32, "dweights")
    _ra.same_device(op, [dweights, logits, ids], logits, "logits'")
    dev = logits.device
    dl = torch.empty((T, E), dtype=logits.dtype, device=dev)
    if T == 0:
        return dl
    li = _logit_rows(logits)
    s = _lib.FaMoeRouteBwdParams()
    s.struct_size = ctypes.sizeof(_lib.FaMoeRouteBwdParams)
    s.dweights, s.ids = dweights.data_ptr(), ids.data_ptr()
    s.logits, s.logits_row_stride = li.data_ptr(), li.stride(0)
    s.dlogits, s.dlogits_row_stride = dl.data_ptr(), dl.stride(0)
    s.tokens, s.num_experts, s.top_k = T, E, k
    s.dtype, s.scoring, s.renormalize, s.scale = _LOGIT_DTYPES[logits.dtype], sc, 1 if renormalize else 0, scale
    with _fi._on_device(dev):
        _lib.call_moe_route_bwd(s, _fi._stream(dev))
    del li, dweights, ids
    return dl


def moe_route(logits, k, *, scoring="softmax", renormalize=True, bias=None, scale=1.0):
    """(weights fp32 [T, K], ids int32 [T, K]) with the formulas at the top of this module; the weights are differentiable in
    the logits (`moe_route_backward`), ids is not differentiable; no double backward."""
    _route_args("moe_route", logits, k, scoring, bias, scale)
    _fi._check_device(logits, bias)
    from . import torch_ops as _ops                            # (registers torch.ops.flash_attn_mi355.moe_*)
    return _ops.moe_route(logits, int(k), scoring, bool(renormalize), bias, float(scale))


def sort_max_rows(T, K, num_experts, align):
    """M_max = T K + E (align - 1): the rows of sorted_slot and of the permuted activations, known on the host"""
    return T * K + num_experts * (align - 1)


def moe_sort(ids, num_experts, *, align=1):
    """(sorted_slot int32 [M_max], pos int32 [T, K], expert_offsets int32 [E + 1]) of ids int32 [T, K]: the stable counting sort
    described at the top of this module.  Three launches over a workspace of `_lib.moe_sort_plan(T K, E)[2]` bytes."""
    op = "moe_sort"
    if ids.dtype != torch.int32 or ids.dim() != 2:
        raise RuntimeError(f"{op}: ids must be an int32 tensor [tokens, k], got {ids.dtype} {tuple(ids.shape)}")
    T, K = ids.shape
    E, align = int(num_experts), int(align)
    if not (2 <= E <= MAX_EXPERTS):
        raise RuntimeError(f"{op}: num_experts must be in [2, {MAX_EXPERTS}], got {E}")
    _topk(op, K)
    if not (1 <= align <= MAX_ALIGN):
        raise RuntimeError(f"{op}: align must be in [1, {MAX_ALIGN}], got {align}")
    M = sort_max_rows(T, K, E, align)
    if M >= 2 ** 31:
        raise RuntimeError(f"{op}: tokens x k + num_experts x (align - 1) must stay below 2^31, got {M}")
    _fi._check_device(ids)
    dev = ids.device
    ids = ids.contiguous()
    sorted_slot = torch.empty((M,), dtype=torch.int32, device=dev)
    pos = torch.empty((T, K), dtype=torch.int32, device=dev)
    offsets = torch.empty((E + 1,), dtype=torch.int32, device=dev)
    s = _lib.FaMoeSortParams()
    s.struct_size = ctypes.sizeof(_lib.FaMoeSortParams)
    s.ids, s.sorted_slot, s.pos, s.expert_offsets = ids.data_ptr(), sorted_slot.data_ptr(), pos.data_ptr(), offsets.data_ptr()
    s.tokens, s.num_experts, s.top_k, s.align = T, E, K, align
    with _fi._on_device(dev):
        ws = _fi._workspace(_lib.moe_sort_workspace_bytes(s), dev)
        s.workspace, s.workspace_bytes = ws.data_ptr(), ws.numel()
        _lib.call_moe_sort(s, _fi._stream(dev))
    del ws, ids
    return sorted_slot, pos, offsets


def moe_permute_forward(x, sorted_slot, k, *, scale=None, out=None):
    """xp [M_max, N]: row r is row sorted_slot[r] // k of x (padding rows +0), a bit-exact copy - or, with scale fp32 [T, k],
    round16(scale[slot] * x[slot // k]).  No autograd."""
    op = "moe_permute"
    N = _hidden(op, x, "x")
    T, k = x.shape[0], int(k)
    _topk(op, k)
    _slots(op, T, k)
    if sorted_slot.dtype != torch.int32 or sorted_slot.dim() != 1:
        raise RuntimeError(f"{op}: sorted_slot must be an int32 tensor [M_max], got {sorted_slot.dtype} {tuple(sorted_slot.shape)}")
    M = sorted_slot.shape[0]
    if scale is not None:
        scale = _table(op, scale, (T, k), torch.float32, "scale")
    if out is not None and (out.dtype != x.dtype or tuple(out.shape) != (M, N)):
        raise RuntimeError(f"{op}: out must be {x.dtype} of shape {(M, N)}, got {out.dtype} {tuple(out.shape)}")
    _ra.same_device(op, [x, sorted_slot, scale, out], x, "x's")
    dev = x.device
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=dev)
    elif _hidden_rows(out) is not out:
        raise RuntimeError(f"{op}: out must have 16-byte aligned rows with a contiguous last dimension")
    if M == 0:
        return out
    xi, si = _hidden_rows(x), sorted_slot.contiguous()
    s = _lib.FaMoePermuteParams()
    s.struct_size = ctypes.sizeof(_lib.FaMoePermuteParams)
    s.x, s.x_row_stride = (xi.data_ptr() if T else 0), xi.stride(0)
    s.sorted_slot = si.data_ptr()
    if scale is not None and T:
        s.slot_scale = scale.data_ptr()
    s.out, s.out_row_stride = out.data_ptr(), out.stride(0)
    s.rows, s.tokens, s.top_k, s.n, s.dtype = M, T, k, N, _fi._DTYPES[x.dtype]
    with _fi._on_device(dev):
        _lib.call_moe_permute(s, _fi._stream(dev))
    del xi, si, scale
    return out


def moe_permute(x, sorted_slot, k, *, scale=None, pos=None):
    """`moe_permute_forward`, differentiable in x: the backward is the combine with unit weights (with `scale`: with the scale
    as weights) over `pos`, moe_sort's third result - pass it; without it the backward inverts sorted_slot first."""
    _hidden("moe_permute", x, "x")
    _topk("moe_permute", int(k))
    _fi._check_device(x, sorted_slot, scale, pos)
    from . import torch_ops as _ops
    return _ops.moe_permute(x, sorted_slot, int(k), scale, pos)


def _combine_args(op, y, weights, pos, first, first_name):
    """(T, K, M, N) of a combine call: `first` ([T, N] for the backward: dout) or y sets dtype and N"""
    N = _hidden(op, y if first is None else first, "y" if first is None else first_name)
    if first is not None and (y.dtype != first.dtype or y.dim() != 2 or y.shape[1] != N):
        raise RuntimeError(f"{op}: y must be {first.dtype} [rows, {N}], got {y.dtype} {tuple(y.shape)}")
    if pos.dtype != torch.int32 or pos.dim() != 2:
        raise RuntimeError(f"{op}: pos must be an int32 tensor [tokens, k], got {pos.dtype} {tuple(pos.shape)}")
    T, K = pos.shape
    _topk(op, K)
    _slots(op, T, K)
    if first is not None and first.shape[0] != T:
        raise RuntimeError(f"{op}: {first_name} must have pos' {T} rows, got {tuple(first.shape)}")
    if weights is not None and (weights.dtype != torch.float32 or tuple(weights.shape) != (T, K)):
        raise RuntimeError(f"{op}: weights must be fp32 of pos' shape {(T, K)}, got {weights.dtype} {tuple(weights.shape)}")
    return T, K, y.shape[0], N


def moe_combine_forward(y, weights, pos, *, out=None):
    """out [T, N] = round16(sum_k weights[t, k] * float(y[pos[t, k]])); weights None: ones.  No autograd."""
    op = "moe_combine"
    T, K, M, N = _combine_args(op, y, weights, pos, None, None)
    if out is not None and (out.dtype != y.dtype or tuple(out.shape) != (T, N)):
        raise RuntimeError(f"{op}: out must be {y.dtype} of shape {(T, N)}, got {out.dtype} {tuple(out.shape)}")
    _ra.same_device(op, [y, weights, pos, out], y, "y's")
    dev = y.device
    if out is None:
        out = torch.empty((T, N), dtype=y.dtype, device=dev)
    elif _hidden_rows(out) is not out:
        raise RuntimeError(f"{op}: out must have 16-byte aligned rows with a contiguous last dimension")
    if T == 0:
        return out
    yi, pi = _hidden_rows(y), pos.contiguous()
    wi = None if weights is None else weights.contiguous()
    s = _lib.FaMoeCombineParams()
    s.struct_size = ctypes.sizeof(_lib.FaMoeCombineParams)
    s.y, s.y_row_stride = (yi.data_ptr() if M else 0), yi.stride(0)
    if wi is not None:
        s.weights = wi.data_ptr()
    s.pos = pi.data_ptr()
    s.out, s.out_row_stride = out.data_ptr(), out.stride(0)
    s.rows, s.tokens, s.top_k, s.n, s.dtype = M, T, K, N, _fi._DTYPES[y.dtype]
    with _fi._on_device(dev):
        _lib.call_moe_combine(s, _fi._stream(dev))
    del yi, pi, wi
    return out


def moe_combine_backward(dout, y, weights, pos, *, need_dy=True, need_dw=True):
    """(dy [M_max, N] or None, dw fp32 [T, K] or None) of `moe_combine`: dy is the scaled permute of dout (padding rows +0),
    dw the fixed-order row sums of dout[t] * y[pos[t, k]]"""
    op = "moe_combine_backward"
    T, K, M, N = _combine_args(op, y, weights, pos, dout, "dout")
    if weights is None and need_dy:
        raise RuntimeError(f"{op}: dy needs weights")
    _ra.same_device(op, [dout, y, weights, pos], dout, "dout's")
    dev = dout.device
    dy = torch.empty((M, N), dtype=dout.dtype, device=dev) if need_dy else None
    dw = torch.empty((T, K), dtype=torch.float32, device=dev) if need_dw else None
    if (dy is None or M == 0) and (dw is None or T == 0):
        return dy, dw
    di, yi, pi = _hidden_rows(dout), _hidden_rows(y), pos.contiguous()
    wi = None if weights is None else weights.contiguous()
    s = _lib.FaMoeCombineBwdParams()
    s.struct_size = ctypes.sizeof(_lib.FaMoeCombineBwdParams)
    s.dout, s.dout_row_stride = (di.data_ptr() if T else 0), di.stride(0)
    s.y, s.y_row_stride = (yi.data_ptr() if M else 0), yi.stride(0)
    if wi is not None and T:
        s.weights = wi.data_ptr()
    s.pos = pi.data_ptr() if T else 0
    if dy is not None and M:
        s.dy, s.dy_row_stride = dy.data_ptr(), dy.stride(0)
    if dw is not None and T:
        s.dw = dw.data_ptr()
    s.rows, s.tokens, s.top_k, s.n, s.dtype = M, T, K, N, _fi._DTYPES[dout.dtype]
    with _fi._on_device(dev):
        _lib.call_moe_combine_bwd(s, _fi._stream(dev))
    del di, yi, pi, wi
    return dy, dw


def moe_combine(y, weights, pos):
    """`moe_combine_forward`, differentiable in y and in weights (`moe_combine_backward`); no double backward."""
    _combine_args("moe_combine", y, weights, pos, None, None)
    _fi._check_device(y, weights, pos)
    from . import torch_ops as _ops
    return _ops.moe_combine(y, weights, pos)


def _gemm_dim(op, v, name, most):
    if v < 8 or v > most or v % 8:
        raise RuntimeError(f"{op}: {name} must be a multiple of 8 in [8, {most}], got {v}")


def _gemm_rows(op, t, name):
    """a [rows, cols] operand of the GEMM as the kernel takes it: nothing is copied, a layout it cannot read raises"""
    if t.stride(1) != 1 and t.shape[1] != 1:
        raise RuntimeError(f"{op}: {name} must have a contiguous last dimension, got strides {tuple(t.stride())}")
    if t.data_ptr() % 16 or t.stride(0) % 8 or t.stride(0) > GEMM_MAX_ROW_STRIDE or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise RuntimeError(f"{op}: {name} must be 16-byte aligned with a row stride that is a multiple of 8, at least its row "
                           f"length and at most 2^22, got offset {t.data_ptr() % 16} and stride {t.stride(0)}")


def moe_gemm_plan(M_max, N, K, num_experts, *, w_layout="nk", dtype=torch.bfloat16):
    """(block_m, block_n, block_k, grid_m, grid_n) of `moe_gemm`: a function of these arguments alone, no device"""
    if w_layout not in W_LAYOUTS:
        raise RuntimeError(f"moe_gemm_plan: w_layout must be one of {sorted(W_LAYOUTS)}, got {w_layout!r}")
    if dtype not in _fi._DTYPES:
        raise RuntimeError(f"moe_gemm_plan: dtype must be fp16 or bf16, got {dtype}")
    return _lib.moe_gemm_plan(int(M_max), int(N), int(K), int(num_experts), W_LAYOUTS[w_layout], _fi._DTYPES[dtype])


def moe_gemm(x, w, expert_offsets, *, w_layout="nk", bias=None, sorted_slot=None, top_k=None, out=None):
    """The grouped expert GEMM (csrc/fa_moe_gemm.hip), forward, fp16 / bf16 with fp32 accumulation: out [M_max, N] with

        out[r] = round16(sum_k float(a_r[k]) * float(W_e[k, n]) (+ float(bias[e, n])))    expert_offsets[e] <= r < expert_offsets[e + 1]
        out[r] = +0                                                                       expert_offsets[E] <= r < M_max

    one launch, no workspace, nothing read on the host: `expert_offsets` (int32 [E + 1], moe_sort's) stays on the device, so a
    decode step with its host-known M_max is capturable.  M_max is out.shape[0]; without `sorted_slot` it is x.shape[0] and
    a_r = x[r] (x = moe_permute's output).  With `sorted_slot` (int32 [M_max]) and `top_k`, x is the un-permuted [T, K] and
    a_r = x[sorted_slot[r] // top_k], a slot outside [0, T top_k) - the -1 padding - being a row of +0 that forms no address:
    the bits of moe_gemm(moe_permute(x, sorted_slot, top_k), ...) without the permute launch and the xp buffer.

    w_layout "nk": w [E, N, K] (nn.Linear, vLLM, DeepSeek); "kn": w [E, K, N] (HF gpt-oss) - also the data gradient of an "nk"
    layer, dx = moe_gemm(dy, w, offsets, w_layout="kn"), N and K exchanged.  w may be a view with any expert stride >= N K (a
    multiple of 8) and contiguous experts, 16-byte aligned.  bias [E, N] of the io dtype or fp32.  x and out: 16-byte aligned,
    contiguous last dimension, row strides multiples of 8 (nothing is copied; another layout raises).

    Every output element is one fp32 accumulator chain of v_mfma_f32_32x32x16 over k ascending in steps of 16 from +0, in both
    tile shapes (`moe_gemm_plan`); the bias is added to the finished sum.  A row's bits depend on its source row, W_e, bias[e]
    and K alone.  expert_offsets values are only compared and clamped to [0, M_max]: a malformed table gives wrong rows, never
    an address outside out, x or w.

    Limits: 2 <= E <= 512, K and N multiples of 8 with K <= 32768 and N <= 65536, row strides of x and out at most 2^22 elements,
    M_max >= 0 (0 launches nothing); expert_offsets[0] is 0 (moe_sort's: rows below a positive first offset are not written).  No autograd:
    an input that requires grad raises (`moe_linear` is the differentiable name).  Not covered: fp8 / block-scaled operands, an activation or the
    combine fused into the epilogue, a per-row routing weight, E > 512."""
    op = "moe_gemm"
    if w_layout not in W_LAYOUTS:
        raise RuntimeError(f"{op}: w_layout must be one of {sorted(W_LAYOUTS)}, got {w_layout!r}")
    for name, t in (("x", x), ("w", w), ("bias", bias)):
        if t is not None and t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{op}: {name} requires grad, and moe_gemm has no autograd (detach it, or run under no_grad)")
    if x.dtype not in _fi._DTYPES:
        raise RuntimeError(f"{op}: x must be fp16 or bf16, got {x.dtype}")
    if x.dim() != 2:
        raise RuntimeError(f"{op}: x must be [rows, K], got {tuple(x.shape)}")
    if w.dtype != x.dtype or w.dim() != 3:
        raise RuntimeError(f"{op}: w must be a {x.dtype} tensor [E, N, K] ('nk') or [E, K, N] ('kn'), got {w.dtype} {tuple(w.shape)}")
    K = x.shape[1]
    E = w.shape[0]
    N = w.shape[1] if w_layout == "nk" else w.shape[2]
    if (w.shape[2] if w_layout == "nk" else w.shape[1]) != K:
        raise RuntimeError(f"{op}: w {tuple(w.shape)} in layout {w_layout!r} does not contract with x's K = {K}")
    if not (2 <= E <= MAX_EXPERTS):
        raise RuntimeError(f"{op}: num_experts (w.shape[0]) must be in [2, {MAX_EXPERTS}], got {E}")
    _gemm_dim(op, K, "K", GEMM_MAX_K)
    _gemm_dim(op, N, "N", GEMM_MAX_N)
    if w.stride(2) != 1 or w.stride(1) != w.shape[2] or w.stride(0) < N * K or w.stride(0) % 8 or w.data_ptr() % 16:
        raise RuntimeError(f"{op}: w must be 16-byte aligned with contiguous experts and an expert stride that is a multiple of 8 "
                           f"and at least N K, got strides {tuple(w.stride())}")
    expert_offsets = _table(op, expert_offsets, (E + 1,), torch.int32, "expert_offsets")
    if (sorted_slot is None) != (top_k is None):
        raise RuntimeError(f"{op}: sorted_slot and top_k go together")
    if sorted_slot is not None:
        top_k = int(top_k)
        _topk(op, top_k)
        _slots(op, x.shape[0], top_k)
        if sorted_slot.dtype != torch.int32 or sorted_slot.dim() != 1:
            raise RuntimeError(f"{op}: sorted_slot must be an int32 tensor [M_max], got {sorted_slot.dtype} {tuple(sorted_slot.shape)}")
        M = sorted_slot.shape[0]
        sorted_slot = sorted_slot.contiguous()
    else:
        M = x.shape[0]
    if M >= 2 ** 31:
        raise RuntimeError(f"{op}: M_max must stay below 2^31, got {M}")
    if bias is not None and (bias.dtype not in (x.dtype, torch.float32) or tuple(bias.shape) != (E, N)):
        raise RuntimeError(f"{op}: bias must be {x.dtype} or fp32 of shape {(E, N)}, got {bias.dtype} {tuple(bias.shape)}")
    if out is not None and (out.dtype != x.dtype or tuple(out.shape) != (M, N)):
        raise RuntimeError(f"{op}: out must be {x.dtype} of shape {(M, N)}, got {out.dtype} {tuple(out.shape)}")
    if x.shape[0]:
        _gemm_rows(op, x, "x")
    if out is not None and M:
        _gemm_rows(op, out, "out")
    _ra.same_device(op, [x, w, expert_offsets, bias, sorted_slot, out], x, "x's")
    dev = x.device
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=dev)
    if M == 0:
        return out
    bi = None if bias is None else bias.contiguous()
    s = _lib.FaMoeGemmParams()
    s.struct_size = ctypes.sizeof(_lib.FaMoeGemmParams)
    s.x, s.x_row_stride = (x.data_ptr() if x.shape[0] else 0), x.stride(0)
    s.w, s.w_expert_stride = w.data_ptr(), w.stride(0)
    if bi is not None:
        s.bias, s.bias_dtype = bi.data_ptr(), (_lib.FA_FP32 if bi.dtype == torch.float32 else _fi._DTYPES[bi.dtype])
    s.expert_offsets = expert_offsets.data_ptr()
    if sorted_slot is not None:
        s.sorted_slot, s.tokens, s.top_k = sorted_slot.data_ptr(), x.shape[0], top_k
    s.out, s.out_row_stride = out.data_ptr(), out.stride(0)
    s.rows, s.num_experts, s.n, s.k = M, E, N, K
    s.dtype, s.layout = _fi._DTYPES[x.dtype], W_LAYOUTS[w_layout]
    with _fi._on_device(dev):
        _lib.call_moe_gemm(s, _fi._stream(dev))
    del bi, expert_offsets, sorted_slot
    return out


def moe_gemm_wgrad_plan(N, K, num_experts, *, w_layout="nk", dtype=torch.bfloat16):
    """(block_n, block_k, block_rows, grid_n, grid_k, grid_e) of `moe_gemm_wgrad`: a function of these arguments alone, no device"""
    if w_layout not in W_LAYOUTS:
        raise RuntimeError(f"moe_gemm_wgrad_plan: w_layout must be one of {sorted(W_LAYOUTS)}, got {w_layout!r}")
    if dtype not in _fi._DTYPES:
        raise RuntimeError(f"moe_gemm_wgrad_plan: dtype must be fp16 or bf16, got {dtype}")
    return _lib.moe_gemm_wgrad_plan(int(N), int(K), int(num_experts), W_LAYOUTS[w_layout], _fi._DTYPES[dtype])


def _grad_dtype(op, dtype, io, name):
    """the code of a gradient's dtype: None is the io dtype"""
    dtype = io if dtype is None else dtype
    if dtype not in (io, torch.float32):
        raise RuntimeError(f"{op}: {name} must be {io} or torch.float32, got {dtype}")
    return dtype, (_lib.FA_FP32 if dtype == torch.float32 else _fi._DTYPES[dtype])


def moe_gemm_wgrad(dy, x, expert_offsets, *, w_layout="nk", sorted_slot=None, top_k=None, dw_dtype=None, out=None,
                   accumulate=False, need_dbias=False, dbias_dtype=None, need_dw=True):
    """The weight gradient of `moe_gemm` (csrc/fa_moe_gemm_wgrad.hip): dw [E, N, K] ("nk") or [E, K, N] ("kn") with

        dW_e[n, k]  = round(sum_r float(dy[r, n]) * float(a_r[k]))  (+ the old dw with accumulate)
        dbias[e, n] = round(sum_r float(dy[r, n]))                     over expert_offsets[e] <= r < expert_offsets[e + 1]

    and +0 for an empty expert (with accumulate: its slab is left as it is).  Returns dw, or (dw, dbias) with need_dbias (dbias
    [E, N] of `dbias_dtype`: the io dtype or fp32; need_dw=False: dw is None and only the dbias launch runs).  dy is [M_max, N];
    a_r is x[r] (x [M_max, K]) or, with `sorted_slot` / `top_k`, x[sorted_slot[r] // top_k] (x [T, K]) exactly as in `moe_gemm`:
    the weight gradient of a fused-gather layer needs no permuted copy of x.  E is len(expert_offsets) - 1.

    One launch for dw over a grid known on the host (`moe_gemm_wgrad_plan`), a second small one for dbias; no workspace, no
    atomics, nothing read on the host.  Every element of dw is one fp32 accumulator chain of v_mfma_f32_32x32x16 from +0 over the
    segment's rows, ascending from its first row in steps of 16, rounded once: its bits are a function of the segment's rows of
    dy and a alone - not of the other experts, of E, of where the segment lies or of the rows behind expert_offsets[E].  Rows
    outside the segment are never loaded, so a NaN there stays there.  dbias adds 16 interleaved fp32 partial sums in a fixed
    order that depends on the segment's length alone.

    `dw_dtype` is the io dtype (default) or torch.float32; `out` is written in place of a fresh tensor and may be a view with
    any expert stride >= N K that is a multiple of 8, contiguous experts, 16-byte aligned; `accumulate` (fp32 dw only, with
    `out`) adds to it, one fp32 add.  Nothing is copied: dy and x must be 16-byte aligned with a contiguous last dimension and
    row strides that are multiples of 8 (another layout raises).  Limits as `moe_gemm`; M_max == 0 still writes +0.  No autograd.
    Not covered: a split over rows for very long segments (one chain per tile: an expert that holds most rows is the slow
    case), fp8 operands."""
    op = "moe_gemm_wgrad"
    if w_layout not in W_LAYOUTS:
        raise RuntimeError(f"{op}: w_layout must be one of {sorted(W_LAYOUTS)}, got {w_layout!r}")
    if dy.dtype not in _fi._DTYPES:
        raise RuntimeError(f"{op}: dy must be fp16 or bf16, got {dy.dtype}")
    if dy.dim() != 2:
        raise RuntimeError(f"{op}: dy must be [rows, N], got {tuple(dy.shape)}")
    if x.dtype != dy.dtype or x.dim() != 2:
        raise RuntimeError(f"{op}: x must be a {dy.dtype} tensor [rows, K], got {x.dtype} {tuple(x.shape)}")
    io = dy.dtype
    M, N = dy.shape
    K = x.shape[1]
    _gemm_dim(op, K, "K", GEMM_MAX_K)
    _gemm_dim(op, N, "N", GEMM_MAX_N)
    if expert_offsets.dtype != torch.int32 or expert_offsets.dim() != 1:
        raise RuntimeError(f"{op}: expert_offsets must be an int32 tensor [E + 1], got {expert_offsets.dtype} {tuple(expert_offsets.shape)}")
    E = expert_offsets.shape[0] - 1
    if not (2 <= E <= MAX_EXPERTS):
        raise RuntimeError(f"{op}: num_experts (len(expert_offsets) - 1) must be in [2, {MAX_EXPERTS}], got {E}")
    expert_offsets = expert_offsets.contiguous()
    if (sorted_slot is None) != (top_k is None):
        raise RuntimeError(f"{op}: sorted_slot and top_k go together")
    if sorted_slot is not None:
        top_k = int(top_k)
        _topk(op, top_k)
        _slots(op, x.shape[0], top_k)
        if sorted_slot.dtype != torch.int32 or tuple(sorted_slot.shape) != (M,):
            raise RuntimeError(f"{op}: sorted_slot must be an int32 tensor of dy's {M} rows, got {sorted_slot.dtype} {tuple(sorted_slot.shape)}")
        sorted_slot = sorted_slot.contiguous()
    elif x.shape[0] != M:
        raise RuntimeError(f"{op}: x must have dy's {M} rows, got {tuple(x.shape)}")
    if M >= 2 ** 31:
        raise RuntimeError(f"{op}: M_max must stay below 2^31, got {M}")
    dw_dtype, dw_code = _grad_dtype(op, dw_dtype if out is None or dw_dtype is not None else out.dtype, io, "dw_dtype")
    dbias_dtype, dbias_code = _grad_dtype(op, dbias_dtype, io, "dbias_dtype")
    if accumulate and dw_dtype != torch.float32:
        raise RuntimeError(f"{op}: accumulate needs an fp32 dw (dw_dtype=torch.float32), got {dw_dtype}")
    if accumulate and out is None:
        raise RuntimeError(f"{op}: accumulate needs out, the tensor to add to")
    if (out is not None or accumulate) and not need_dw:
        raise RuntimeError(f"{op}: out and accumulate go with need_dw")
    shape = (E, N, K) if w_layout == "nk" else (E, K, N)
    if out is not None:
        if out.dtype != dw_dtype or tuple(out.shape) != shape:
            raise RuntimeError(f"{op}: out must be {dw_dtype} of shape {shape}, got {out.dtype} {tuple(out.shape)}")
        if out.stride(2) != 1 or out.stride(1) != out.shape[2] or out.stride(0) < N * K or out.stride(0) % 8 or out.data_ptr() % 16:
            raise RuntimeError(f"{op}: out must be 16-byte aligned with contiguous experts and an expert stride that is a multiple "
                               f"of 8 and at least N K, got strides {tuple(out.stride())}")
    if M:
        _gemm_rows(op, dy, "dy")
    if x.shape[0]:
        _gemm_rows(op, x, "x")
    _ra.same_device(op, [dy, x, expert_offsets, sorted_slot, out], dy, "dy's")
    dev = dy.device
    dw = out
    if need_dw and dw is None:
        dw = torch.empty(shape, dtype=dw_dtype, device=dev)
    dbias = torch.empty((E, N), dtype=dbias_dtype, device=dev) if need_dbias else None
    if dw is None and dbias is None:
        return None
    s = _lib.FaMoeGemmWgradParams()
    s.struct_size = ctypes.sizeof(_lib.FaMoeGemmWgradParams)
    s.dy, s.dy_row_stride = (dy.data_ptr() if M else 0), dy.stride(0)
    s.x, s.x_row_stride = (x.data_ptr() if x.shape[0] else 0), x.stride(0)
    s.expert_offsets = expert_offsets.data_ptr()
    if sorted_slot is not None:
        s.sorted_slot, s.tokens, s.top_k = sorted_slot.data_ptr(), x.shape[0], top_k
    if dw is not None:
        s.dw, s.dw_expert_stride = dw.data_ptr(), dw.stride(0)
    if dbias is not None:
        s.dbias = dbias.data_ptr()
    s.rows, s.num_experts, s.n, s.k = M, E, N, K
    s.dtype, s.dw_dtype, s.dbias_dtype, s.layout = _fi._DTYPES[io], dw_code, dbias_code, W_LAYOUTS[w_layout]
    s.accumulate = 1 if accumulate else 0
    with _fi._on_device(dev):
        _lib.call_moe_gemm_wgrad(s, _fi._stream(dev))
    del expert_offsets, sorted_slot
    return (dw, dbias) if need_dbias else dw


def moe_linear(x, w, expert_offsets, *, w_layout="nk", bias=None, sorted_slot=None, top_k=None, pos=None):
    """The differentiable expert layer: the forward is `moe_gemm(x, w, expert_offsets, ...)`, bit for bit, with the same
    arguments and limits.  The backward, from dy made conforming (a copy only where its layout cannot be read):

        dx        moe_gemm(dy, w, expert_offsets, the other layout); in the gather form followed by moe_combine_forward(.., None,
                  pos) - pass `pos`, moe_sort's third result; without it the backward inverts sorted_slot on the device first
        dw, dbias moe_gemm_wgrad(dy, x, expert_offsets, the same layout and gather), in w's and bias' dtypes

    Only the gradients autograd asks for are computed.  The tables have no gradient; no double backward."""
    op = "moe_linear"
    if w_layout not in W_LAYOUTS:
        raise RuntimeError(f"{op}: w_layout must be one of {sorted(W_LAYOUTS)}, got {w_layout!r}")
    if (sorted_slot is None) != (top_k is None):
        raise RuntimeError(f"{op}: sorted_slot and top_k go together")
    if pos is not None and sorted_slot is None:
        raise RuntimeError(f"{op}: pos goes with sorted_slot (the gather form)")
    _fi._check_device(x, w, expert_offsets, bias, sorted_slot, pos)
    from . import torch_ops as _ops
    return _ops.moe_linear(x, w, expert_offsets, w_layout, bias, sorted_slot, None if top_k is None else int(top_k), pos)
