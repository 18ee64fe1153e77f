"""GPU: fa_cross_entropy / fa_cross_entropy_bwd against the fp64 reference (cross_entropy_ref.py) within the bounds derived there,
and everything else bit for bit: ignored rows, in place against out of place, a padded view against its contiguous copy against
a misaligned layout, a row alone against the same row in a batch, two runs, a broadcast dloss against its copy, the special
values, the autograd paths, a captured graph and the guard bands.
Inputs (cross_entropy_ref.inputs): rows of logit magnitude 1e-3, 1 and 30 side by side, every third label ignore_index, labels
on column 0 and V - 1, rows with -inf over a whole piece, a leading run and a whole chunk.  Each case prints its worst
error / bound ratio."""
import ctypes

import pytest
import torch

import cross_entropy_ref as R
import guard

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
SCALARS = [(ls, sc, zs) for ls in (0.0, 0.1) for sc in (1.0, 0.5) for zs in (0.0, 1e-4)]


def _C():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import cross_entropy as C
    return C


def _shapes(dtype):
    """(rows, V): every V of the list with one of the row counts; the three largest V only with rows <= 67"""
    c = R.CHUNK[dtype]
    return [(1031, 1), (67, 7), (3, 8), (1031, 264), (67, 1000), (1031, 1001), (1, 1001), (67, c - 8), (3, c), (67, c + 1),
            (1, 2 * c + 13), (3, 2 * c + 13)]


def _same(got, want, name):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert torch.equal(guard.bits(got), guard.bits(want)), f"{name}: the bits differ"


def _run(C, x, y, dloss, ls, sc, zs, inplace=False):
    losses, z, lse = C.cross_entropy_forward(x, y, label_smoothing=ls, logit_scale=sc, lse_square_scale=zs)
    dx = C.cross_entropy_backward(dloss, x.clone() if inplace else x, y, lse, label_smoothing=ls, logit_scale=sc,
                                  lse_square_scale=zs, inplace=inplace)
    return losses, z, lse, dx


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(12))
def test_against_the_reference_within_the_derived_bounds(case, dtype):
    """lse, losses, z_losses and dlogits within cross_entropy_ref's bounds for all eight classes of (label_smoothing 0 / 0.1,
    logit_scale 1 / 0.5, lse_square_scale 0 / 1e-4); the inputs are unchanged; ignored rows are +0 everywhere; the backward in
    place leaves the out-of-place bits"""
    C = _C()
    rows, V = _shapes(dtype)[case]
    xc, yc, dlc = R.inputs(rows, V, dtype, seed=case)
    x, y, dl = xc.cuda(), yc.cuda(), dlc.cuda()
    x0 = x.clone()
    steps = R.plan(rows, V, dtype)["steps"]
    ign = y == R.IGNORE
    worst = {"lse": 0.0, "loss": 0.0, "z": 0.0, "dx": 0.0}
    for ls, sc, zs in SCALARS:
        losses, z, lse, dx = _run(C, x, y, dl, ls, sc, zs)
        ref = R.forward_ref(x, y, ls, sc, zs)
        rdx, mags = R.backward_ref(dl, x, y, lse, ls, sc, zs)
        w = {"lse": R.worst(lse, ref["lse"], R.lse_bound(ref, steps)),
             "loss": R.worst(losses, ref["loss"], R.loss_bound(ref, steps, ls, zs, V)),
             "z": R.worst(z, ref["z"], R.z_bound(ref, steps, zs)),
             "dx": R.worst(dx, rdx, R.dx_bound(rdx, mags, dtype))}
        for k in w:
            worst[k] = max(worst[k], w[k])
        assert all(v <= 1.0 for v in w.values()), (ls, sc, zs, w)
        _same(x, x0, "logits")
        zero32 = torch.zeros(int(ign.sum()), dtype=torch.float32, device="cuda")
        _same(losses[ign], zero32, "losses of ignored rows")
        _same(z[ign], zero32, "z_losses of ignored rows")
        _same(dx[ign], torch.zeros_like(dx[ign]), "dlogits of ignored rows")
        _same(_run(C, x, y, dl, ls, sc, zs, inplace=True)[3], dx, "in place")
    print(f"cross_entropy rows {rows} V {V} {dtype}: worst error / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_layouts_give_the_same_bits(dtype):
    """V = 1001: a [:, :V] view of a padded buffer == its contiguous copy (every odd row misaligned) == the same rows behind a
    base that is off by one element; two runs are identical; dloss with stride 0 == its materialised copy"""
    C = _C()
    rows, V = 67, 1001
    xc, yc, _ = R.inputs(rows, V, dtype, seed=77)
    y = yc.cuda()
    pad = torch.full((rows, 1024), float("nan"), dtype=dtype, device="cuda")
    pad[:, :V] = xc.cuda()
    view = pad[:, :V]
    cont = view.contiguous()
    shifted = torch.empty(rows * V + 1, dtype=dtype, device="cuda")[1:].view(rows, V)
    shifted.copy_(cont)
    assert view.stride(0) == 1024 and cont.stride(0) == V and shifted.data_ptr() % 16 != 0
    one = torch.full((1,), 0.75, dtype=torch.float32, device="cuda")
    bcast = one.expand(rows)
    assert bcast.stride(0) == 0
    ls, sc, zs = 0.1, 0.5, 1e-4
    want = _run(C, view, y, bcast, ls, sc, zs)
    for name, t in (("contiguous", cont), ("shifted", shifted), ("again", view)):
        got = _run(C, t, y, bcast, ls, sc, zs)
        for g, w, n in zip(got, want, ("losses", "z_losses", "lse", "dlogits")):
            _same(g, w, f"{name} {n}")
    _same(_run(C, view, y, bcast.contiguous(), ls, sc, zs)[3], want[3], "materialised dloss")
    _same(_run(C, view, y, bcast, ls, sc, zs, inplace=True)[3], want[3], "in place on a copy of the view")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("big", [False, True])
def test_a_row_alone_has_the_bits_it_has_in_the_batch(big, dtype):
    """forward and backward: rows of the 1031-row batch at V = 1001 (aligned and misaligned ones, masked ones), and of a 67-row
    batch of more than one chunk"""
    C = _C()
    rows, V = (67, R.CHUNK[dtype] + 1) if big else (1031, 1001)
    xc, yc, dlc = R.inputs(rows, V, dtype, seed=5)
    x, y, dl = xc.cuda(), yc.cuda(), dlc.cuda()
    ls, sc, zs = 0.1, 0.5, 1e-4
    batch = _run(C, x, y, dl, ls, sc, zs)
    for r in (0, 1, 3, 4, 5, rows - 1):
        alone = _run(C, x[r:r + 1].clone(), y[r:r + 1], dl[r:r + 1], ls, sc, zs)
        for a, b, n in zip(alone, batch, ("losses", "z_losses", "lse", "dlogits")):
            _same(a, b[r:r + 1], f"row {r} {n}")


def _nan_like(got, ref):
    g = got.double()
    assert torch.equal(torch.isnan(g), torch.isnan(ref)) and torch.equal(torch.isinf(g), torch.isinf(ref))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [40, 1001, "chunk"])
def test_edge_rows(V, dtype):
    """the all -inf row and the +inf / NaN rows carry the reference's special values; a label outside [0, V) gives a NaN loss
    and a NaN gradient row; the rows between them are untouched (the bits of a batch without the edge rows)"""
    C = _C()
    V = R.CHUNK[dtype] + 1 if V == "chunk" else V
    rows = 9
    xc, _, dlc = R.inputs(rows, V, dtype, seed=9)
    xc = torch.where(torch.isinf(xc), torch.zeros_like(xc), xc)
    yc = torch.arange(rows) % V
    plain = _run(C, xc.cuda(), yc.cuda(), dlc.cuda(), 0.1, 1.0, 1e-4)
    xe, ye = xc.clone(), yc.clone()
    xe[0] = float("-inf")
    xe[2, V - 1] = float("inf")
    xe[4, V // 2] = float("nan")
    xe[5, :V - 1] = float("-inf")                             # (one finite column, the last: an ordinary row)
    ye[5] = V - 1
    ye[6], ye[8] = V, -1
    x, y, dl = xe.cuda(), ye.cuda(), dlc.cuda()
    losses, z, lse, dx = _run(C, x, y, dl, 0.1, 1.0, 1e-4)
    ref = R.forward_ref(x, y, 0.1, 1.0, 1e-4)
    rdx, _ = R.backward_ref(dl, x, y, lse, 0.1, 1.0, 1e-4)
    _nan_like(lse, ref["lse"]); _nan_like(losses, ref["loss"]); _nan_like(z, ref["z"]); _nan_like(dx, rdx)
    assert torch.isnan(lse[[0, 2, 4]]).all() and torch.isnan(losses[[0, 2, 4, 6, 8]]).all() and torch.isnan(dx[[0, 2, 4, 6, 8]]).all()
    assert torch.isfinite(lse[[1, 3, 5, 6, 7, 8]]).all() and float(lse[5]) == float(x[5, V - 1])   # (one live column: lse is its logit)
    for r in (1, 3, 7):
        for a, b, n in zip((losses, z, lse, dx), plain, ("losses", "z_losses", "lse", "dlogits")):
            _same(a[r], b[r], f"neighbour row {r} {n}")
    for r in (6, 8):
        _same(lse[r], plain[2][r], f"lse of the bad-label row {r}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_autograd_paths_equal_the_direct_backward(dtype):
    """torch.ops.flash_attn_mi355.cross_entropy, cross_entropy_loss and CrossEntropyLoss (three reductions, return_z_loss,
    inplace_backward): the gradient is the direct backward call's, bit for bit"""
    C = _C()
    import flash_attn_mi355.torch_ops  # noqa: F401
    from flash_attn.losses.cross_entropy import CrossEntropyLoss
    from flash_attn.ops.triton.cross_entropy import cross_entropy_loss
    B, S, V = 3, 23, 1001
    xc, yc, dlc = R.inputs(B * S, V, dtype, seed=21)
    x = xc.cuda().view(B, S, V)
    y = yc.cuda().view(B, S)
    dl = dlc.cuda().view(B, S)
    ls, sc, zs = 0.1, 0.5, 1e-4
    kw = dict(label_smoothing=ls, logit_scale=sc, lse_square_scale=zs)
    losses, z, lse = C.cross_entropy_forward(x, y, **kw)
    assert losses.shape == y.shape
    want = C.cross_entropy_backward(dl, x, y, lse, **kw)

    xa = x.clone().requires_grad_(True)
    lo, zo, lseo = torch.ops.flash_attn_mi355.cross_entropy(xa, y, ls, sc, zs, -100, False)
    _same(lo.detach(), losses, "op losses"); _same(zo.detach(), z, "op z_losses"); _same(lseo.detach(), lse, "op lse")
    (g,) = torch.autograd.grad(lo, xa, dl)
    _same(g, want, "op gradient")

    xa = x.clone().requires_grad_(True)
    lo, zo = cross_entropy_loss(xa.view(-1, V), y.view(-1), **kw)
    assert lo.requires_grad and not zo.requires_grad          # z_losses carries no gradient
    (g,) = torch.autograd.grad(lo, xa, dl.view(-1))
    _same(g, want, "cross_entropy_loss gradient")

    xa = x.clone().requires_grad_(True)
    xin = xa * 1.0                                            # (a non-leaf: the in-place backward may overwrite it)
    lo, _ = cross_entropy_loss(xin.view(-1, V), y.view(-1), inplace_backward=True, **kw)
    (g,) = torch.autograd.grad(lo, xa, dl.view(-1))
    _same(g, want, "inplace_backward gradient")

    n = (y != -100).sum()
    for reduction in ("none", "sum", "mean"):
        for inplace in (False, True):
            mod = CrossEntropyLoss(reduction=reduction, inplace_backward=inplace, return_z_loss=True, **kw)
            xa = x.clone().requires_grad_(True)
            loss, zl = mod((xa * 1.0).view(-1, V), y.view(-1))
            if reduction == "none":
                _same(loss.detach(), losses.view(-1), "module losses"); _same(zl.detach(), z.view(-1), "module z_losses")
                dloss = dl.view(-1)
                (g,) = torch.autograd.grad(loss, xa, dloss)
            else:
                div = n if reduction == "mean" else 1
                _same(loss.detach(), losses.view(-1).sum() / div, f"module {reduction}")
                _same(zl.detach(), z.view(-1).sum() / div, f"module z {reduction}")
                dloss = (torch.ones((), device="cuda") / div).float().expand(B * S)
                (g,) = torch.autograd.grad(loss, xa)
            _same(g, C.cross_entropy_backward(dloss.view(B, S), x, y, lse, **kw), f"module gradient {reduction} {inplace}")
    assert not isinstance(CrossEntropyLoss()(x.view(-1, V), y.view(-1)), tuple)


def test_forward_and_backward_replay_in_a_graph():
    """forward (two launches, the workspace allocated during capture) + backward captured in one graph; replayed after the
    inputs were overwritten in place: every output equals the eager result bit for bit"""
    C = _C()
    import flash_attn_mi355.torch_ops  # noqa: F401
    ns = torch.ops.flash_attn_mi355
    dtype, rows = torch.bfloat16, 67
    V = R.CHUNK[dtype] + 1
    sets = [tuple(t.cuda() for t in R.inputs(rows, V, dtype, seed=30 + i)) for i in range(3)]
    ls, sc, zs = 0.1, 0.5, 1e-4

    def run(x, y, dl):
        lo, zo, lse = ns.cross_entropy(x, y, ls, sc, zs, -100, False)
        return lo, zo, lse, ns.cross_entropy_bwd(dl, x, y, lse, ls, sc, zs, -100)
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
        for got, want, name in zip(outs, ref[i], ("losses", "z_losses", "lse", "dlogits")):
            _same(got, want, f"replay {i} {name}")
    assert not torch.equal(guard.bits(ref[0][3]), guard.bits(ref[1][3]))


# guard bands -------------------------------------------------------------------------------------------------------------------
_CODES = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 3}
_BAND = 4096


def _guarded_1d(t):
    """(buf, view): the 1-D tensor exactly sized between two bands that hold all-ones bits"""
    buf = torch.full((_BAND + t.numel() + _BAND,), -1, dtype=guard._INT_OF.get(t.dtype, t.dtype), device="cuda").view(t.dtype)
    view = buf[_BAND:_BAND + t.numel()]
    view.copy_(t)
    return buf, view


def _bands_hold(buf, n, name):
    b = buf.view(guard._INT_OF.get(buf.dtype, buf.dtype))
    assert bool((b[:_BAND] == -1).all()) and bool((b[_BAND + n:] == -1).all()), f"{name}: written outside its {n} elements"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["1001", "chunk+1"])
def test_guard_bands(shape, dtype):
    """logits and dlogits are views inside NaN-filled slabs (V = 1001: contiguous rows, so every odd row is misaligned and its
    neighbour's columns are the first thing past it; CHUNK + 1: gaps between the rows), labels, dloss, lse and the three outputs
    sit exactly sized inside guarded buffers, and the workspace has exactly the queried size between sentinel bands (pre-filled
    with 0xFF: a partial read before it is written would show): nothing outside a tensor's elements or the reported workspace
    is written, no NaN of a gap reaches an output, the inputs are unchanged, and the results are the unguarded call's"""
    C = _C()
    from flash_attn_mi355 import _lib
    from flash_attn_mi355 import flash_attn_interface as fi
    rows, V, gaps = (67, 1001, False) if shape == "1001" else (5, R.CHUNK[dtype] + 1, True)
    xc, yc, dlc = R.inputs(rows, V, dtype, seed=41)
    ls, sc, zs = 0.1, 0.5, 1e-4
    want = _run(C, xc.cuda(), yc.cuda(), dlc.cuda(), ls, sc, zs)
    xb, x, xsnap = guard.guarded(xc.cuda(), gaps=gaps)
    assert x.stride(0) > V if gaps else x.stride(0) == V
    (yb, y), (dlb, dl) = _guarded_1d(yc.cuda()), _guarded_1d(dlc.cuda())
    outs = [_guarded_1d(torch.zeros(rows, dtype=torch.float32, device="cuda")) for _ in range(3)]
    workspace, check_ws = guard.guarded_workspace("ones")

    s = _lib.FaCrossEntropyParams()
    s.struct_size = ctypes.sizeof(_lib.FaCrossEntropyParams)
    s.logits, s.logits_row_stride, s.labels = x.data_ptr(), x.stride(0), y.data_ptr()
    s.losses, s.z_losses, s.lse = (o[1].data_ptr() for o in outs)
    s.rows, s.vocab, s.dtype, s.ignore_index = rows, V, _CODES[dtype], -100
    s.label_smoothing, s.logit_scale, s.lse_square_scale = ls, sc, zs
    nbytes = _lib.cross_entropy_workspace_bytes(s)
    assert nbytes == R.plan(rows, V, dtype)["workspace_bytes"]
    ws = workspace(nbytes, x.device)
    if ws is not None:
        s.workspace, s.workspace_bytes = ws.data_ptr(), nbytes
    _lib.call_cross_entropy(s, fi._stream(x.device))
    torch.cuda.synchronize()
    assert check_ws()["sizes"] == [nbytes]
    assert torch.equal(guard.bits(xb), xsnap), "logits were written"
    for (buf, view), w, name in zip(outs, want, ("losses", "z_losses", "lse")):
        _bands_hold(buf, rows, name)
        _same(view, w, name)
    _bands_hold(yb, rows, "labels"); _bands_hold(dlb, rows, "dloss")

    db, dx, dsnap = guard.guarded(shape=(rows, V), dtype=dtype, device="cuda", gaps=gaps)
    b = _lib.FaCrossEntropyBwdParams()
    b.struct_size = ctypes.sizeof(_lib.FaCrossEntropyBwdParams)
    b.dlosses, b.dlosses_stride = dl.data_ptr(), 1
    b.logits, b.logits_row_stride, b.labels, b.lse = x.data_ptr(), x.stride(0), y.data_ptr(), outs[2][1].data_ptr()
    b.dlogits, b.dlogits_row_stride = dx.data_ptr(), dx.stride(0)
    b.rows, b.vocab, b.dtype, b.ignore_index = rows, V, _CODES[dtype], -100
    b.label_smoothing, b.logit_scale, b.lse_square_scale = ls, sc, zs
    _lib.call_cross_entropy_bwd(b, fi._stream(x.device))
    torch.cuda.synchronize()
    guard.assert_untouched(db, dx, dsnap, "dlogits")
    assert torch.equal(guard.bits(xb), xsnap), "logits were written by the backward"
    _bands_hold(outs[2][0], rows, "lse"); _bands_hold(dlb, rows, "dloss"); _bands_hold(yb, rows, "labels")
    _same(dx.contiguous(), want[3], "dlogits")
    # in place inside the slab: the gradient lands on the logits' elements and nowhere else
    b.dlogits, b.dlogits_row_stride = x.data_ptr(), x.stride(0)
    _lib.call_cross_entropy_bwd(b, fi._stream(x.device))
    torch.cuda.synchronize()
    guard.assert_untouched(xb, x, xsnap, "logits rewritten in place")
    _same(x.contiguous(), want[3], "dlogits in place")
