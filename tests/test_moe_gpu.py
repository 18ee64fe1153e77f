"""GPU: the fa_moe_* kernels (csrc/fa_moe.hip) against the fp64 / exact-integer reference of moe_ref.py.

Path boundaries covered (moe_ref.ROUTE_SHAPES for the router):
  route / route_bwd  G = 1, 2, 4, 8, 16, 32, 64 lanes per row (E = 8, 16, 32, 60 / 64, 128, 256, 384 / 512); a ragged last lane
                     (E = 60: element-wise loads and stores) and a ragged last lane group (E = 384: lanes without columns); K = 1,
                     K = E, K = 16; one row, 67 rows (dead groups in the last workgroup at every G) and 300 rows; 16-bit and fp32
                     logits; row strides that break the 16-byte alignment of odd rows
  sort               T K = 0, one chunk (<= 256 slots), a partial last 64-slot step, 2400 slots = 10 chunks; align 1, 16, 128;
                     an empty expert, one expert with everything, dropped ids -1, E and 2^31 - 1
  permute / combine  N = 8 (one piece a row: 256 rows per item), 264 (rows straddle items), 4096, 7168; more items than one trip
                     of four in flight; K = 1, 2, 6 (a partial group of four in the combine), 8, 16; dw: N <= 256 (G lanes),
                     264 (one wave), 4096 (4 waves, 2 pieces), 7168 (4 pieces, absent ones)
Bounds: moe_ref.py's docstring (route weights), route_bwd_ref (dlogits), combine_ref / combine_bwd_ref (out, dw); the exact
parts - ids, sort, permute, dy, unselected gradient columns - are compared bit for bit.  Every test prints the worst share of its
bound that it measured ("share"), which profiles/moe.txt records."""
import numpy as np
import pytest
import torch

import guard
import moe_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
LOGIT_DTYPES = [torch.bfloat16, torch.float16, torch.float32]
COMBOS = [("softmax", True), ("softmax", False), ("sigmoid", True), ("sigmoid", False)]
DEV = "cuda"


def _M():
    from flash_attn_mi355 import moe
    import flash_attn_mi355.torch_ops  # noqa: F401
    return moe


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _same(got, want, name):
    assert got.shape == want.shape and got.dtype == want.dtype, name
    a, b = got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)
    assert torch.equal(a, b), f"{name}: {int((a != b).sum())} bytes differ"


def _share(name, err, bound):
    """assert err <= bound elementwise and print the worst share (NaN positions must agree and are left out)"""
    nan_e, nan_b = np.isnan(err), np.isnan(bound)
    assert (nan_e == nan_b).all(), f"{name}: NaN where the reference has none (or the reverse)"
    ok = ~nan_e
    share = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    print(f"share {name}: {share:.3f}")
    assert share <= 1.0, f"{name}: {share:.3f} of the bound"
    return share


def _logits(T, E, dtype, seed, spread=2.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, E, generator=g) * spread).to(dtype).to(DEV)


def _check_route(M, logits, K, scoring, renorm, bias, scale, name):
    w, ids = M.moe_route_forward(logits, K, scoring=scoring, renormalize=renorm, bias=bias, scale=scale)
    lw, nb = R.widen(logits), None if bias is None else R.widen(bias)
    w_ref, ids_ref, _ = R.route_ref(lw, K, scoring=scoring, renormalize=renorm, bias=nb, scale=scale)
    assert w.dtype == torch.float32 and ids.dtype == torch.int32
    assert (ids.cpu().numpy() == ids_ref).all(), f"{name}: ids differ from the reference"
    bound = R.route_weight_bound(lw, w_ref, ids_ref, scoring=scoring, renormalize=renorm, bias=nb)
    _share(name, np.abs(R.widen(w) - w_ref), np.where(np.isnan(w_ref), np.nan, bound))
    return w, ids


# route -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", LOGIT_DTYPES, ids=_name)
@pytest.mark.parametrize("shape", R.ROUTE_SHAPES, ids=lambda s: "T%d-E%d-K%d" % s)
def test_route_softmax(shape, dtype):
    """the selection is exact (16-bit randn rows are full of ties: the lowest index wins them), the weights are within the
    counted bound, renormalised and over all E"""
    M = _M()
    T, E, K = shape
    logits = _logits(T, E, dtype, R.route_seed(*shape))
    for renorm in (True, False):
        _check_route(M, logits, K, "softmax", renorm, None, 2.5, f"route softmax renorm={renorm} {shape} {_name(dtype)}")


@pytest.mark.parametrize("dtype", LOGIT_DTYPES, ids=_name)
@pytest.mark.parametrize("shape", R.ROUTE_SHAPES, ids=lambda s: "T%d-E%d-K%d" % s)
def test_route_sigmoid_with_bias(shape, dtype):
    """decisive inputs (moe_ref.decisive_logits: test_moe_cpu.py asserts every row's gap): the ids are the reference's bit for
    bit in every row, the weights are the sigmoid WITHOUT the bias within the bound"""
    M = _M()
    T, E, K = shape
    logits, bias = R.decisive_logits(T, E, K, R.route_seed(*shape))
    logits, bias = torch.from_numpy(logits).to(dtype).to(DEV), torch.from_numpy(bias).to(DEV)
    for renorm in (True, False):
        for b in (bias, None):
            _check_route(M, logits, K, "sigmoid", renorm, b, 2.5,
                         f"route sigmoid renorm={renorm} bias={b is not None} {shape} {_name(dtype)}")


def _adversarial(E):
    inf, nan = float("inf"), float("nan")
    rows = [[1.0] * E, [-inf] * E, [nan] * E, [0.0, -0.0] * (E // 2), [inf] + [0.0] * (E - 1),
            [nan, 2.0] * (E // 2), [-inf] * (E - 1) + [3.0], [float(i % 3) for i in range(E)],
            [nan] * (E - 2) + [-inf, -1.0], [inf, nan, -inf, 1.0] * (E // 4)]
    return torch.tensor(rows)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=_name)
@pytest.mark.parametrize("E", [8, 60, 512])
def test_route_adversarial_rows(E, dtype):
    """equal logits, an all-equal row, ties across the K boundary, NaN, -inf and +inf entries: the ids are distinct, inside
    [0, E) and the reference's bit for bit (softmax: exact; sigmoid: these rows hold only values whose sigmoids are far apart
    or exactly equal), the weights are NaN exactly where the formulas give NaN and within the bound elsewhere"""
    M = _M()
    logits = _adversarial(E).to(dtype).to(DEV)
    for K in (1, 2, min(E, 16)):
        for scoring, renorm in COMBOS:
            w, ids = _check_route(M, logits, K, scoring, renorm, None, 1.0, f"adversarial {scoring} renorm={renorm} E={E} K={K}")
            i = ids.cpu().numpy()
            assert i.min() >= 0 and i.max() < E and all(len(set(r)) == K for r in i.tolist())
    w, ids = M.moe_route_forward(logits[:1], 2)
    assert ids.tolist() == [[0, 1]] and w.tolist() == [[0.5, 0.5]]


@pytest.mark.parametrize("dtype", LOGIT_DTYPES, ids=_name)
@pytest.mark.parametrize("E,K", [(8, 2), (60, 6), (384, 8)])
def test_route_is_batch_invariant_and_takes_padded_rows(E, K, dtype):
    """a row alone gives the bits it has inside 67 rows; a [:, :E] view of wider, NaN-padded rows (odd rows off the 16-byte grid)
    gives the bits of the contiguous tensor - forward and backward"""
    M = _M()
    logits = _logits(67, E, dtype, 77)
    dw = torch.randn(67, K, device=DEV)
    for scoring, renorm in COMBOS:
        kw = dict(scoring=scoring, renormalize=renorm, scale=1.5)
        w, ids = M.moe_route_forward(logits, K, **kw)
        dl = M.moe_route_backward(dw, logits, ids, **kw)
        for r in (0, 33, 66):
            w1, i1 = M.moe_route_forward(logits[r:r + 1], K, **kw)
            _same(w1, w[r:r + 1], "weights of a row alone")
            _same(i1, ids[r:r + 1], "ids of a row alone")
            _same(M.moe_route_backward(dw[r:r + 1], logits[r:r + 1], i1, **kw), dl[r:r + 1], "dlogits of a row alone")
        wide = torch.full((67, E + 3), float("nan"), dtype=dtype, device=DEV)
        wide[:, :E] = logits
        wv, iv = M.moe_route_forward(wide[:, :E], K, **kw)
        _same(wv, w, "weights of padded rows")
        _same(iv, ids, "ids of padded rows")
        _same(M.moe_route_backward(dw, wide[:, :E], iv, **kw), dl, "dlogits of padded rows")


@pytest.mark.parametrize("dtype", LOGIT_DTYPES, ids=_name)
@pytest.mark.parametrize("shape", [(3, 8, 2), (67, 60, 6), (300, 128, 8), (67, 384, 8), (67, 512, 16), (67, 16, 16)],
                         ids=lambda s: "T%d-E%d-K%d" % s)
def test_route_backward(shape, dtype):
    """dlogits within route_bwd_ref's bound; unselected columns exactly +0 wherever the formula is sparse; every element
    written (the output starts as NaN)"""
    M = _M()
    T, E, K = shape
    g = torch.Generator().manual_seed(R.route_seed(*shape))
    dw = torch.randn(T, K, generator=g).to(DEV)
    for scoring, renorm in COMBOS:
        if scoring == "sigmoid":
            lg, bias = R.decisive_logits(T, E, K, R.route_seed(*shape))
            logits, bias = torch.from_numpy(lg).to(dtype).to(DEV), torch.from_numpy(bias).to(DEV)
        else:
            logits, bias = _logits(T, E, dtype, R.route_seed(*shape)), None
        kw = dict(scoring=scoring, renormalize=renorm, bias=bias, scale=2.5)
        _, ids = M.moe_route_forward(logits, K, **kw)
        dl = M.moe_route_backward(dw, logits, ids, **kw)
        assert dl.dtype == dtype and dl.shape == (T, E)
        ref, bound = R.route_bwd_ref(R.widen(dw), R.widen(logits), ids.cpu().numpy(), scoring=scoring, renormalize=renorm,
                                     bias=None if bias is None else R.widen(bias), scale=2.5, with_bound=True, io=_name(dtype))
        _share(f"route_bwd {scoring} renorm={renorm} {shape} {_name(dtype)}", np.abs(R.widen(dl) - ref), bound)
        if not (scoring == "softmax" and not renorm):
            sel = torch.zeros(T, E, dtype=torch.bool, device=DEV)
            sel.scatter_(1, ids.long(), True)
            rest = dl[~sel]
            assert not bool(rest.view(torch.int16 if dtype != torch.float32 else torch.int32).any()), "an unselected column is not +0"


@pytest.mark.parametrize("scoring,renorm", COMBOS)
def test_route_autograd_through_torch_ops(scoring, renorm):
    """torch.ops.flash_attn_mi355.moe_route is differentiable in the logits - the direct backward's bits - and ids is not"""
    M = _M()
    T, E, K = 67, 60, 6
    lg, bias = R.decisive_logits(T, E, K, 5)
    logits = torch.from_numpy(lg).to(torch.bfloat16).to(DEV).requires_grad_()
    bias = torch.from_numpy(bias).to(DEV) if scoring == "sigmoid" else None
    w, ids = M.moe_route(logits, K, scoring=scoring, renormalize=renorm, bias=bias, scale=2.5)
    assert w.requires_grad and not ids.requires_grad
    dw = torch.randn(T, K, device=DEV)
    (dl,) = torch.autograd.grad(w, logits, dw)
    _same(dl, M.moe_route_backward(dw, logits.detach(), ids, scoring=scoring, renormalize=renorm, bias=bias, scale=2.5), "autograd")


# sort --------------------------------------------------------------------------------------------------------------------------
def _sort_cases():
    rng = np.random.default_rng(21)
    cases = []
    for T, K, E in ((1, 1, 2), (3, 2, 8), (67, 6, 60), (300, 8, 128), (67, 16, 512), (40, 8, 384)):
        cases.append((f"random T{T} K{K} E{E}", rng.integers(0, E, size=(T, K)), E))
    ids = rng.integers(0, 8, size=(67, 2))
    ids[ids == 3] = 4
    cases.append(("an expert without tokens", ids, 8))
    cases.append(("everything on one expert", np.full((300, 8), 5), 60))
    ids = rng.integers(0, 8, size=(67, 2))
    ids[::3, 0], ids[1::5, 1], ids[2::7, 0] = -1, 8, 2 ** 31 - 1
    cases.append(("dropped ids", ids, 8))
    cases.append(("all dropped", np.full((5, 2), -7), 8))
    cases.append(("no tokens", np.zeros((0, 4), dtype=np.int64), 8))
    return [(n, i.astype(np.int32), E) for n, i, E in cases]


@pytest.mark.parametrize("align", [1, 16, 128])
def test_sort_equals_the_reference_bit_for_bit(align):
    M = _M()
    for name, ids, E in _sort_cases():
        t = torch.from_numpy(ids).to(DEV)
        got = M.moe_sort(t, E, align=align)
        again = M.moe_sort(t, E, align=align)
        want = R.sort_ref(ids, E, align=align)
        for a, b, w, what in zip(got, again, want, ("sorted_slot", "pos", "expert_offsets")):
            assert a.dtype == torch.int32 and tuple(a.shape) == w.shape, (name, what)
            assert (a.cpu().numpy() == w).all(), f"{name}, align {align}: {what} differs from the reference"
            _same(a, b, f"{name}: {what} of a second call")


# permute -----------------------------------------------------------------------------------------------------------------------
def _sorted_case(T, K, E, align, seed, drop=True):
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(T)]).to(torch.int32) if T else torch.zeros(0, K, dtype=torch.int32)
    if drop and T > 2:
        ids[1, 0] = -1
        ids[2] = E                                           # a token with no live slot
    return ids.to(DEV), R.sort_ref(ids.numpy(), E, align=align)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("T,K,E,N,align", [(1, 1, 8, 8, 1), (3, 2, 8, 264, 16), (67, 6, 60, 264, 16), (300, 8, 128, 8, 128),
                                           (67, 2, 8, 4096, 16), (300, 16, 64, 7168, 1)])
def test_permute(T, K, E, N, align, dtype):
    """bit-exact against index_select, padding rows +0; the scaled form bit-exact against an fp32 product followed by a cast"""
    M = _M()
    ids, (sorted_slot, pos, offsets) = _sorted_case(T, K, E, align, 31)
    ss = torch.from_numpy(sorted_slot).to(DEV)
    x = torch.randn(T, N, device=DEV).to(dtype)
    scale = torch.randn(T, K, device=DEV)
    live = ss >= 0
    tok = (ss.clamp(min=0) // K).long()
    want = x.index_select(0, tok) * live[:, None]
    want[~live] = 0.0
    xp = M.moe_permute_forward(x, ss, K)
    _same(xp, want, "permute")
    assert not bool(xp[~live].view(torch.int16).any()), "a padding row is not +0"
    wanted = (scale.reshape(-1)[ss.clamp(min=0).long()][:, None] * x.float().index_select(0, tok)).to(dtype)
    wanted[~live] = 0.0
    xs = M.moe_permute_forward(x, ss, K, scale=scale)
    _same(xs, wanted, "scaled permute")
    assert not bool(xs[~live].view(torch.int16).any())
    # a row-strided x and out=
    wide = torch.randn(T, N + 8, device=DEV).to(dtype)
    out = torch.full((len(sorted_slot), N), float("nan"), dtype=dtype, device=DEV)
    assert M.moe_permute_forward(wide[:, :N], ss, K, out=out) is out
    _same(out, M.moe_permute_forward(wide[:, :N].contiguous(), ss, K), "permute of strided rows")


# combine -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("T,K,E,N,align", [(1, 1, 8, 8, 1), (3, 2, 8, 264, 16), (67, 6, 60, 264, 16), (300, 8, 128, 8, 128),
                                           (67, 2, 8, 4096, 16), (67, 16, 64, 7168, 1)])
def test_combine_and_its_backward(T, K, E, N, align, dtype):
    """out within 0.5 ulp16 + K 2^-24 sum_k |w y|; dropped slots skipped; a token with no live slot +0; dy bit-exact against the
    scaled permute with padding rows +0; dw within the row-sum bound (24 2^-24 sum_n |dout y|), dropped slots +0"""
    M = _M()
    ids, (sorted_slot, pos_np, offsets) = _sorted_case(T, K, E, align, 41)
    ss, pos = torch.from_numpy(sorted_slot).to(DEV), torch.from_numpy(pos_np).to(DEV)
    Mrows = len(sorted_slot)
    y = torch.randn(Mrows, N, device=DEV).to(dtype)
    y[ss < 0] = float("nan")                                  # padding rows are never read
    w = torch.rand(T, K, device=DEV) + 0.25
    dout = torch.randn(T, N, device=DEV).to(dtype)
    out = M.moe_combine_forward(y, w, pos)
    yw = np.nan_to_num(R.widen(y))
    ref, mag = R.combine_ref(yw, R.widen(w), pos_np)
    err32 = K * R.U * mag
    bound = R.half_ulp16(np.abs(ref) + err32, _name(dtype)) + err32 + R.TINY
    _share(f"combine T{T} K{K} N{N} {_name(dtype)}", np.abs(R.widen(out) - ref), bound)
    if T > 2:
        assert not bool(out[2].view(torch.int16).any()), "a token with no live slot is not +0"
    ones = M.moe_combine_forward(y, None, pos)
    _same(ones, M.moe_combine_forward(y, torch.ones_like(w), pos), "unit weights")
    dy, dw = M.moe_combine_backward(dout, y, w, pos)
    _same(dy, M.moe_permute_forward(dout, ss, K, scale=w), "dy")
    assert not bool(dy[ss < 0].view(torch.int16).any())
    _, dw_ref, dmag = R.combine_bwd_ref(R.widen(dout), yw, R.widen(w), pos_np)
    _share(f"combine dw T{T} K{K} N{N} {_name(dtype)}", np.abs(R.widen(dw) - dw_ref), R.DW_DEPTH * R.U * dmag * R.SLACK + R.TINY)
    assert not bool(dw[pos < 0].view(torch.int32).any()), "the dw of a dropped slot is not +0"
    only_dy, none = M.moe_combine_backward(dout, y, w, pos, need_dw=False)
    assert none is None
    _same(only_dy, dy, "dy alone")
    none, only_dw = M.moe_combine_backward(dout, y, w, pos, need_dy=False)
    assert none is None
    _same(only_dw, dw, "dw alone")


def test_permute_and_combine_autograd_through_torch_ops():
    M = _M()
    T, K, E, N, align = 67, 2, 8, 264, 16
    ids, (sorted_slot, pos_np, offsets) = _sorted_case(T, K, E, align, 51)
    ss, pos = torch.from_numpy(sorted_slot).to(DEV), torch.from_numpy(pos_np).to(DEV)
    x = torch.randn(T, N, device=DEV).to(torch.bfloat16).requires_grad_()
    dxp = torch.randn(len(sorted_slot), N, device=DEV).to(torch.bfloat16)
    for p in (pos, None):                                     # (without pos the backward inverts sorted_slot itself)
        xp = M.moe_permute(x, ss, K, pos=p)
        (dx,) = torch.autograd.grad(xp, x, dxp)
        _same(dx, M.moe_combine_forward(dxp, None, pos), "permute's gradient")
    y = torch.randn(len(sorted_slot), N, device=DEV).to(torch.bfloat16).requires_grad_()
    w = torch.rand(T, K, device=DEV).requires_grad_()
    dout = torch.randn(T, N, device=DEV).to(torch.bfloat16)
    dy, dw = torch.autograd.grad(M.moe_combine(y, w, pos), (y, w), dout)
    want = M.moe_combine_backward(dout, y.detach(), w.detach(), pos)
    _same(dy, want[0], "combine's dy")
    _same(dw, want[1], "combine's dw")


# end to end --------------------------------------------------------------------------------------------------------------------
def test_a_tiny_moe_block_end_to_end():
    """T 67, E 8, K 2, N 264, bf16: route -> sort -> permute -> per-segment fp32 matmuls over expert_offsets (read back by the
    test: the ops never synchronise) -> combine, forward and backward, against the dense fp64 definition sum_k w_k
    Expert_{id_k}(x_t) with gradients in x and in the router logits.  The tolerance is the sum of the stage bounds, first order:
      forward   out: sum_k [bw_k |y_k| + |w_k| ey_k] + K u sum_k |w_k y_k| + hu(out), with bw the route bound and
                ey = N u sum_n |x W| + hu(y) the fp32 matmul (N roundings on a sum bounded by sum |x W|) and its rounding to bf16
      backward  dy = round16(w dout): e_dy = bw |dout| + hu;   dxp = round16(dy W^T): e_dxp = e_dy |W|^T + N u |dy| |W|^T + hu;
                dx = sum_k dxp: sum_k e_dxp + K u sum |dxp| + hu
                dw = dout . y: 24 u sum_n |dout y| + |dout| . ey;   dlogits: route_bwd_ref's own bound + its propagation of
                the dw error, |w_j| (e_g_j + sum_k |w_k| e_g_k) with e_g = scale e_dw, + hu
    (u = 2^-24, hu = half an ulp of bf16 at the value)."""
    M = _M()
    T, E, K, N, align, scale = 67, 8, 2, 264, 16, 1.5
    dt, nm = torch.bfloat16, "bfloat16"
    g = torch.Generator().manual_seed(61)
    logits = (torch.randn(T, E, generator=g) * 2).to(dt).to(DEV).requires_grad_()
    x = torch.randn(T, N, generator=g).to(dt).to(DEV).requires_grad_()
    W = (torch.randn(E, N, N, generator=g) / N ** 0.5).to(DEV)                 # fp32 experts
    dout = torch.randn(T, N, generator=g).to(dt).to(DEV)

    w, ids = M.moe_route(logits, K, scale=scale)
    sorted_slot, pos, offsets = M.moe_sort(ids, E, align=align)
    xp = M.moe_permute(x, sorted_slot, K, pos=pos)
    off = offsets.tolist()                                                     # (the test's own read-back)
    yp = torch.cat([(xp[off[e]:off[e + 1]].float() @ W[e]).to(dt) for e in range(E)] + [xp[off[E]:] * 0])
    out = M.moe_combine(yp, w, pos)
    dx, dlogits = torch.autograd.grad(out, (x, logits), dout)

    lw, xw, Ww, dw_ = R.widen(logits), R.widen(x), R.widen(W), R.widen(dout)
    w_ref, ids_ref, _ = R.route_ref(lw, K, scale=scale)
    assert (ids.cpu().numpy() == ids_ref).all()
    bw = R.route_weight_bound(lw, w_ref, ids_ref, scoring="softmax", renormalize=True)
    hu = lambda v: R.half_ulp16(v, nm)                                          # noqa: E731
    u = R.U
    y_ref = np.einsum("tn,tknm->tkm", xw, Ww[ids_ref])                         # [T, K, N]
    y_mag = np.einsum("tn,tknm->tkm", np.abs(xw), np.abs(Ww[ids_ref]))
    ey = N * u * y_mag + hu(np.abs(y_ref) + N * u * y_mag)
    out_ref = (w_ref[:, :, None] * y_ref).sum(1)
    e_out = (bw[:, :, None] * np.abs(y_ref) + np.abs(w_ref)[:, :, None] * ey).sum(1) + K * u * np.abs(w_ref[:, :, None] * y_ref).sum(1)
    e_out = (e_out + hu(np.abs(out_ref) + e_out)) * R.SLACK
    _share("end to end out", np.abs(R.widen(out) - out_ref), e_out)
    # backward, in fp64
    dy_ref = w_ref[:, :, None] * dw_[:, None, :]                               # [T, K, N]
    e_dy = bw[:, :, None] * np.abs(dw_)[:, None, :] + hu(np.abs(dy_ref))
    WT = np.swapaxes(Ww[ids_ref], 2, 3)
    dxp_ref = np.einsum("tkm,tkmn->tkn", dy_ref, WT)
    e_dxp = np.einsum("tkm,tkmn->tkn", e_dy + N * u * np.abs(dy_ref), np.abs(WT))
    e_dxp = e_dxp + hu(np.abs(dxp_ref) + e_dxp)
    dx_ref = dxp_ref.sum(1)
    e_dx = e_dxp.sum(1) + K * u * np.abs(dxp_ref).sum(1)
    e_dx = (e_dx + hu(np.abs(dx_ref) + e_dx)) * R.SLACK
    _share("end to end dx", np.abs(R.widen(dx) - dx_ref), e_dx)
    dwt_ref = np.einsum("tn,tkn->tk", dw_, y_ref)
    e_dw = R.DW_DEPTH * u * np.einsum("tn,tkn->tk", np.abs(dw_), np.abs(y_ref)) + np.einsum("tn,tkn->tk", np.abs(dw_), ey)
    dl_ref, e_dl = R.route_bwd_ref(dwt_ref, lw, ids_ref, scale=scale, with_bound=True, io=nm)
    e_g = scale * e_dw
    prop = np.zeros_like(dl_ref)
    rows = np.arange(T)[:, None]
    wn = w_ref / scale
    prop[rows, ids_ref] = np.abs(wn) * (e_g + (np.abs(wn) * e_g).sum(1, keepdims=True))
    e_dl = (e_dl + prop * (1 + 2.0 ** -8)) * R.SLACK        # (the propagated part is rounded to bf16 too: half an ulp <= 2^-8 of it)
    _share("end to end dlogits", np.abs(R.widen(dlogits) - dl_ref), e_dl)


# guard bands -------------------------------------------------------------------------------------------------------------------
def _fslab(shape, dtype=torch.float32):
    """(buf, view, snap) of an output: NaN-filled, between two bands.  int32 outputs are float32 slabs seen as int32"""
    buf, view = guard.slab(shape, dtype, gaps=False, device=DEV, check_prep=False)
    return buf, view, guard.snapshot(buf)


def test_guard_bands_around_every_output_and_the_workspace(monkeypatch):
    """every output of every op lies in a NaN-filled slab and is written through the C ABI: nothing outside its elements changes,
    every element is written, the inputs stay as they were, the sort's workspace is exactly the queried size between sentinel
    bands, and the results are those of the plain calls"""
    import ctypes
    from flash_attn_mi355 import _lib
    from flash_attn_mi355 import flash_attn_interface as fi
    M = _M()
    T, E, K, N, align, dt = 67, 60, 6, 264, 16, torch.bfloat16
    logits = _logits(T, E, dt, 71)
    want_w, want_ids = M.moe_route_forward(logits, K)
    want_sort = M.moe_sort(want_ids, E, align=align)
    Mrows = want_sort[0].shape[0]
    x = torch.randn(T, N, device=DEV).to(dt)
    dwt = torch.randn(T, K, device=DEV)
    want_xp = M.moe_permute_forward(x, want_sort[0], K)
    want_out = M.moe_combine_forward(want_xp, want_w, want_sort[1])
    want_dl = M.moe_route_backward(dwt, logits, want_ids)
    want_dy, want_dw = M.moe_combine_backward(x, want_xp, want_w, want_sort[1])
    ins = [guard.guarded(t, gaps=True) for t in (logits, x)]
    lv, xv = ins[0][1], ins[1][1]

    checks = []

    def out(shape, dtype=torch.float32):
        s = _fslab(shape, dtype)
        checks.append(s)
        return s[1]
    stream = fi._stream(logits.device)
    # route: out= takes the slabs
    wv, iv = out((T, K)), out((T, K))
    M.moe_route_forward(lv, K, out=(wv, iv.view(torch.int32)))
    # route_bwd, sort, combine_bwd: their outputs are allocated inside the wrappers - through the blocks
    dlv = out((T, E), dt)
    s = _lib.FaMoeRouteBwdParams()
    s.struct_size = ctypes.sizeof(s)
    s.dweights, s.logits, s.ids, s.dlogits = dwt.data_ptr(), lv.data_ptr(), want_ids.data_ptr(), dlv.data_ptr()
    s.logits_row_stride, s.dlogits_row_stride, s.tokens, s.num_experts, s.top_k = lv.stride(0), dlv.stride(0), T, E, K
    s.dtype, s.scoring, s.renormalize, s.scale = _lib.FA_BF16, _lib.FA_MOE_SOFTMAX, 1, 1.0
    _lib.call_moe_route_bwd(s, stream)
    ssv, pv, ov = out((Mrows,)), out((T, K)), out((E + 1,))
    workspace, ws_check = guard.guarded_workspace("ones")
    s = _lib.FaMoeSortParams()
    s.struct_size = ctypes.sizeof(s)
    s.ids, s.sorted_slot, s.pos, s.expert_offsets = want_ids.data_ptr(), ssv.data_ptr(), pv.data_ptr(), ov.data_ptr()
    s.tokens, s.num_experts, s.top_k, s.align = T, E, K, align
    ws = workspace(_lib.moe_sort_workspace_bytes(s), logits.device)
    s.workspace, s.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.call_moe_sort(s, stream)
    xpv, outv = out((Mrows, N), dt), out((T, N), dt)
    M.moe_permute_forward(xv, want_sort[0], K, out=xpv)
    M.moe_combine_forward(want_xp, want_w, want_sort[1], out=outv)
    dyv, dwv = out((Mrows, N), dt), out((T, K))
    s = _lib.FaMoeCombineBwdParams()
    s.struct_size = ctypes.sizeof(s)
    s.dout, s.y, s.weights, s.pos = xv.data_ptr(), want_xp.data_ptr(), want_w.data_ptr(), want_sort[1].data_ptr()
    s.dy, s.dw = dyv.data_ptr(), dwv.data_ptr()
    s.dout_row_stride, s.y_row_stride, s.dy_row_stride = xv.stride(0), want_xp.stride(0), dyv.stride(0)
    s.rows, s.tokens, s.top_k, s.n, s.dtype = Mrows, T, K, N, _lib.FA_BF16
    _lib.call_moe_combine_bwd(s, stream)
    torch.cuda.synchronize()
    info = ws_check()
    assert info["sizes"] == [_lib.moe_sort_plan(T * K, E)[2]]
    for (buf, view, snap), name in zip(ins, ("logits", "x")):
        assert torch.equal(guard.bits(buf), snap), f"{name} was written"
    wants = (want_w, want_ids, want_dl, *want_sort, want_xp, want_out, want_dy, want_dw)
    names = ("weights", "ids", "dlogits", "sorted_slot", "pos", "expert_offsets", "xp", "out", "dy", "dw")
    for (buf, view, snap), want, name in zip(checks, wants, names):
        guard.assert_untouched(buf, view, snap, name)
        got = view.view(torch.int32) if want.dtype == torch.int32 else view
        _same(got, want, name)


# graph -------------------------------------------------------------------------------------------------------------------------
def test_the_forward_chain_replays_in_a_graph():
    """route -> sort -> permute -> combine, one linear chain captured once and replayed on new data: every output equals the
    eager calls bit for bit (nothing in the chain reads a result back)"""
    _M()
    ns = torch.ops.flash_attn_mi355
    T, E, K, N, align, dt = 67, 60, 6, 264, 16, torch.bfloat16

    def run(logits, x):
        w, ids = ns.moe_route(logits, K, "softmax", True, None, 1.0)
        sorted_slot, pos, offsets = ns.moe_sort(ids, E, align)
        xp = ns.moe_permute(x, sorted_slot, K, None, pos)
        return w, ids, sorted_slot, pos, offsets, xp, ns.moe_combine(xp, w, pos)
    sets = [(_logits(T, E, dt, 80 + i), torch.randn(T, N, device=DEV).to(dt)) for i in range(3)]
    ref = [tuple(t.clone() for t in run(*st)) for st in sets]
    st = tuple(t.clone() for t in sets[0])
    run(*st)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(*st)
    for i in (1, 2, 0):
        for t, src in zip(st, sets[i]):
            t.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for got, want, name in zip(outs, ref[i], ("weights", "ids", "sorted_slot", "pos", "expert_offsets", "xp", "out")):
            _same(got, want, f"replay {i} {name}")
    assert not torch.equal(ref[0][1], ref[1][1])


# opcheck -----------------------------------------------------------------------------------------------------------------------
def test_opcheck_on_every_op():
    _M()
    ns = torch.ops.flash_attn_mi355
    T, E, K, N, align, dt = 5, 8, 2, 16, 4, torch.bfloat16
    lg, bias = R.decisive_logits(T, E, K, 9)
    logits = torch.from_numpy(lg).to(dt).to(DEV)
    bias = torch.from_numpy(bias).to(DEV)
    w, ids = ns.moe_route(logits, K, "softmax", True, None, 1.0)
    sorted_slot, pos, offsets = ns.moe_sort(ids, E, align)
    x = torch.randn(T, N, device=DEV).to(dt)
    xp = ns.moe_permute(x, sorted_slot, K, None, pos)
    rg = lambda t: t.clone().requires_grad_()                # noqa: E731
    torch.library.opcheck(ns.moe_route, (rg(logits), K, "softmax", True, None, 1.0))
    torch.library.opcheck(ns.moe_route, (rg(logits), K, "sigmoid", False, bias, 2.5))
    torch.library.opcheck(ns.moe_route_bwd, (w, logits, ids, "softmax", True, None, 1.0))
    torch.library.opcheck(ns.moe_sort, (ids, E, align))
    torch.library.opcheck(ns.moe_permute, (rg(x), sorted_slot, K, None, pos))
    torch.library.opcheck(ns.moe_permute, (rg(x), sorted_slot, K, w, None))
    torch.library.opcheck(ns.moe_combine, (rg(xp), rg(w), pos))
    torch.library.opcheck(ns.moe_combine, (rg(xp), None, pos))
    torch.library.opcheck(ns.moe_combine_bwd, (x, xp, w, pos, True, True))
    torch.library.opcheck(ns.moe_combine_bwd, (x, xp, w, pos, False, True))
