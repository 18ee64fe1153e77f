"""GPU: fa_act_mul / fa_act_mul_bwd against the fp64 reference (act_mul_ref.py) within the bounds derived there, and everything
else bit for bit: the layouts (packed halves, separate tensors, a padded view, [B, S, N], a misaligned row against its aligned
copy), a row alone, the same operands at another column, in place against out of place, the special values, the autograd paths,
a captured graph, the guard bands and a row that starts past 2^31 elements.
Inputs (act_mul_ref.inputs): gates dense over [-12, 12] plus +-30, +-100, +-0 and -1.28, up and dout normal with magnitudes 1e-3,
1 and 37 mixed.  Each reference case prints its worst error / bound ratio."""
import pytest
import torch

import act_mul_ref as R
import guard

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
BIG_ROWS = 67
# (rows, N): one piece; several pieces and a short last wave; the element path with misaligned odd rows; one workgroup step + 8;
# one whole item + 8 (the period of the tiled case below)
SHAPES = [(r, n) for n in (8, 264, 1001, R.STEP + 8) for r in (1, 3, BIG_ROWS)] + [(BIG_ROWS, 4 * R.STEP + 8)]
# .. and - 67 rows only - the N at which the items outnumber the grid, so the kernel's stride loop takes a second trip.  That is
# 8 M columns, half a billion elements: its inputs are the last shape of SHAPES tiled along the columns, and its results must be
# that shape's results - which are held to the bounds - tiled the same way, bit for bit (an element's bits depend on its own
# operands alone), instead of a float64 reference of 4 GB per temporary
SECOND_TRIP = (BIG_ROWS, R.second_trip_n(BIG_ROWS))


def _M():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import act_mul as M
    return M


def _same(got, want, name):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    differ = guard.bits(got) != guard.bits(want)
    assert not bool(differ.any()), f"{name}: the bits of {int(differ.sum())} of {differ.numel()} elements differ"


_INPUTS = {}


def _inputs(rows, N, dtype, seed=0):
    """act_mul_ref.inputs on the GPU, made once per (rows, N, dtype, seed) and never written"""
    key = (rows, N, dtype, seed)
    if key not in _INPUTS:
        _INPUTS[key] = R.inputs(rows, N, dtype, seed=seed, device="cuda")
    return _INPUTS[key]


def _run(M, g, u, d, act, **kw):
    out = M.act_mul_forward(g, u, activation=act)
    dg, dp = M.act_mul_backward(d, g, u, activation=act, **kw)
    return out, dg, dp


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("activation", R.ACTIVATIONS)
def test_against_the_reference_within_the_derived_bounds(activation, gated, dtype):
    """out, dgate and dup within act_mul_ref's bounds on every shape of SHAPES (the reference is float64 on the GPU); the inputs
    are unchanged; and SECOND_TRIP, whose results are the last shape's, tiled"""
    M = _M()
    worst, used = {"out": 0.0, "dgate": 0.0, "dup": 0.0}, {"out": 0.0, "dgate": 0.0, "dup": 0.0}
    for rows, N in SHAPES:
        g, u, d = _inputs(rows, N, dtype)
        u = u if gated else None
        snap = [t.clone() for t in (g, u, d) if t is not None]
        out, dg, dp = _run(M, g, u, d, activation)
        ro, Do = R.forward_ref(g, u, activation)
        rg, rp, Dg, Dp = R.backward_ref(d, g, u, activation)
        w = {"out": R.worst(out, ro, R.bound(ro, Do, dtype), dtype=dtype),
             "dgate": R.worst(dg, rg, R.bound(rg, Dg, dtype), dtype=dtype),
             "dup": R.worst(dp, rp, R.bound(rp, Dp, dtype), dtype=dtype) if gated else 0.0}
        assert (dp is None) == (not gated)
        f32 = {"out": R.used(out, ro, Do, dtype), "dgate": R.used(dg, rg, Dg, dtype), "dup": R.used(dp, rp, Dp, dtype) if gated else 0.0}
        print(f"act_mul {activation} {'gated' if gated else 'ungated'} {dtype} rows {rows} N {N}: worst error / bound "
              + " ".join(f"{k} {v:.3f}" for k, v in w.items()) + "; share of the bound's fp32 part used "
              + " ".join(f"{k} {v:.3f}" for k, v in f32.items()))
        for k in f32:
            used[k] = max(used[k], f32[k])
        assert all(v <= 1.0 for v in w.values()), (rows, N, w)
        for k in w:
            worst[k] = max(worst[k], w[k])
        for t, s, name in zip([t for t in (g, u, d) if t is not None], snap, ("gate", "up", "dout")):
            _same(t, s, name)
        del ro, Do, rg, rp, Dg, Dp, snap
    # the second trip of the stride loop: (g, u, d) and (out, dg, dp) are the last shape's
    rows, N = SECOND_TRIP
    assert R.plan(rows, N)["items"] > R.GRID_CAP and g.shape[0] == rows
    tile = lambda t: None if t is None else t.repeat(1, -(-N // t.shape[1]))[:, :N].contiguous()       # noqa: E731
    bg, bu, bd = tile(g), tile(u), tile(d)
    big = _run(M, bg, bu, bd, activation)
    for got, small, name in zip(big, (out, dg, dp), ("out", "dgate", "dup")):
        if small is not None:
            want = tile(small)
            _same(got, want, f"second trip {name}")
            del want
    del big, bg, bu, bd
    print(f"act_mul {activation} {'gated' if gated else 'ungated'} {dtype}: worst error / bound over all shapes "
          + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + "; share of the bound's fp32 part used "
          + " ".join(f"{k} {v:.3f}" for k, v in used.items()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("activation", ["silu", "gelu"])
def test_layouts_give_the_same_bits(activation, dtype):
    """separate contiguous tensors (N = 1001: every odd row misaligned, taken element by element) against the halves of a packed
    [rows, 2N], a [:, :N] view of rows padded to 1008 (aligned: the vector path), a [B, S, N] input, a row alone, and the same
    operands moved to other columns: the same bits everywhere, forward and backward"""
    M = _M()
    rows, N = 12, 1001
    g, u, d = _inputs(rows, N, dtype, seed=5)
    want = _run(M, g, u, d, activation)
    assert g.is_contiguous() and (g[1].data_ptr() % 16) != 0
    # packed halves, and the gradient written into the halves of one packed tensor
    x = torch.cat([g, u], dim=-1)
    dx = torch.empty_like(x)
    got = _run(M, x[:, :N], x[:, N:], d, activation, out=(dx[:, :N], dx[:, N:]))
    for a, b, name in zip(got, want, ("out", "dgate", "dup")):
        _same(a, b, "packed " + name)
    _same(dx, torch.cat([want[1], want[2]], dim=-1), "packed gradient")
    assert got[1].data_ptr() == dx.data_ptr() and got[2].data_ptr() == dx[:, N:].data_ptr()
    # padded rows: aligned
    pad = [torch.full((rows, 1008), float("nan"), dtype=dtype, device="cuda") for _ in range(3)]
    for p, t in zip(pad, (g, u, d)):
        p[:, :N] = t
    gv, uv, dv = (p[:, :N] for p in pad)
    assert gv.stride(0) == 1008 and gv[1].data_ptr() % 16 == 0
    for a, b, name in zip(_run(M, gv, uv, dv, activation), want, ("out", "dgate", "dup")):
        _same(a, b, "padded view " + name)
    # [B, S, N]
    for a, b, name in zip(_run(M, g.view(3, 4, N), u.view(3, 4, N), d.view(3, 4, N), activation), want, ("out", "dgate", "dup")):
        assert a.shape == (3, 4, N)
        _same(a.view(rows, N), b, "[B, S, N] " + name)
    # a row alone; the ungated form of a row alone
    for r in (0, 5, 11):
        for a, b, name in zip(_run(M, g[r:r + 1], u[r:r + 1], d[r:r + 1], activation), want, ("out", "dgate", "dup")):
            _same(a, b[r:r + 1], f"row {r} alone " + name)
    # the same operands at other columns and rows
    sh = lambda t: torch.roll(t, shifts=(1, 3), dims=(0, 1)).contiguous()       # noqa: E731
    for a, b, name in zip(_run(M, sh(g), sh(u), sh(d), activation), want, ("out", "dgate", "dup")):
        _same(a, sh(b), "rolled " + name)
    # ungated: the same layouts once
    wantu = _run(M, g, None, d, activation)
    for a, b, name in zip(_run(M, gv, None, dv, activation)[:2], wantu, ("out", "dgate")):
        _same(a, b, "ungated padded view " + name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1001, R.STEP + 8])
def test_in_place_equals_out_of_place(N, dtype):
    """forward with out = gate and out = up, backward with inplace=True (dgate over gate, dup over up) - also on the halves of a
    packed tensor - bit for bit against out of place, and nothing is allocated in place"""
    M = _M()
    rows = 7
    g, u, d = _inputs(rows, N, dtype, seed=6)
    for act in ("silu", "gelu_tanh", "relu2"):
        want = _run(M, g, u, d, act)
        wantu = _run(M, g, None, d, act)
        gc = g.clone()
        assert M.act_mul_forward(gc, u, activation=act, out=gc) is gc
        _same(gc, want[0], "out is gate")
        uc = u.clone()
        assert M.act_mul_forward(g, uc, activation=act, out=uc) is uc
        _same(uc, want[0], "out is up")
        gc = g.clone()
        M.act_mul_forward(gc, activation=act, out=gc)
        _same(gc, wantu[0], "ungated out is gate")
        gc, uc = g.clone(), u.clone()
        allocations = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]       # noqa: E731  (a count: frees do not move it)
        before = allocations()
        dg, dp = M.act_mul_backward(d, gc, uc, activation=act, inplace=True)
        assert allocations() == before and dg is gc and dp is uc
        _same(gc, want[1], "dgate in place")
        _same(uc, want[2], "dup in place")
        gc = g.clone()
        dg, dp = M.act_mul_backward(d, gc, activation=act, inplace=True)
        assert dg is gc and dp is None
        _same(gc, wantu[1], "ungated dgate in place")
        x = torch.cat([g, u], dim=-1)
        M.act_mul_backward(d, x[:, :N], x[:, N:], activation=act, inplace=True)
        _same(x, torch.cat([want[1], want[2]], dim=-1), "packed in place")
    with pytest.raises(RuntimeError, match="in place needs gate"):
        M.act_mul_backward(d, g.t().contiguous().t(), u, inplace=True)
    with pytest.raises(RuntimeError, match="out overlaps gate"):
        M.act_mul_forward(g[:-1], u[:-1], out=g[1:])          # one row further: not the exact alias (nothing is launched)


_INF, _NAN = float("inf"), float("nan")
# gate: +0, -0, +inf, -inf, NaN, 100, -100  ->  (act, act') as flash_attn_mi355/act_mul.py documents them
_SPECIAL_G = [0.0, -0.0, _INF, -_INF, _NAN, 100.0, -100.0]
_SPECIAL = {
    "silu": ([0.0, -0.0, _INF, _NAN, _NAN, 100.0, -0.0], [0.5, 0.5, _NAN, _NAN, _NAN, 1.0, -0.0]),
    "gelu_tanh": ([0.0, -0.0, _INF, _NAN, _NAN, 100.0, -0.0], [0.5, 0.5, _NAN, _NAN, _NAN, 1.0, -0.0]),
    "gelu": ([0.0, -0.0, _INF, _NAN, _NAN, 100.0, -0.0], [0.5, 0.5, _NAN, _NAN, _NAN, 1.0, 0.0]),
    "relu": ([0.0, 0.0, _INF, 0.0, _NAN, 100.0, 0.0], [0.0, 0.0, 1.0, 0.0, _NAN, 1.0, 0.0]),
    "relu2": ([0.0, 0.0, _INF, 0.0, _NAN, 1e4, 0.0], [0.0, 0.0, _INF, 0.0, _NAN, 200.0, 0.0]),
}


def _same_values(got, want, name):
    """equal to the wanted values rounded to the io type (relu2(100) = 1e4 is 9984 in bf16), including the sign of zero; NaN
    where NaN is wanted"""
    got, want = got.float().cpu(), torch.tensor(want).to(got.dtype).float()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), (name, got, want)
    assert torch.equal(got[~nan], want[~nan]) and torch.equal(torch.signbit(got[~nan]), torch.signbit(want[~nan])), (name, got, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("activation", R.ACTIVATIONS)
def test_special_values(activation, dtype):
    """+-0, +-inf, NaN and +-100 (e overflows) in the gate give the documented values, with up = dout = 1 so that out = act(g),
    dgate = act'(g) and dup = act(g); the vector path (a row of 16) and the element path (a misaligned row of 7) agree; in bf16
    a gate of +-1e30 (g g overflows in the tanh GELU) too; an infinite up times act = 0 is NaN"""
    M = _M()
    act, dact = _SPECIAL[activation]
    for n, off in ((16, 0), (7, 1)):
        buf = torch.zeros(2, 16, dtype=dtype, device="cuda")
        g = buf.view(-1)[off:off + n].view(1, n)
        vals = (_SPECIAL_G * 3)[:n]
        g.copy_(torch.tensor(vals, dtype=dtype))
        one = torch.ones(1, n, dtype=dtype, device="cuda")
        out, dg, dp = _run(M, g, one, one, activation)
        _same_values(out[0], (act * 3)[:n], "out")
        _same_values(dg[0], (dact * 3)[:n], "dgate")
        _same_values(dp[0], (act * 3)[:n], "dup")
        outu, dgu, _ = _run(M, g, None, one, activation)
        _same(outu, out, "ungated out")
        _same(dgu, dg, "ungated dgate")
    if dtype == torch.bfloat16 and activation in ("silu", "gelu_tanh"):
        g = torch.tensor([[1e30, -1e30]], dtype=dtype, device="cuda")
        one = torch.ones_like(g)
        out, dg, _ = _run(M, g, one, one, activation)
        _same_values(out[0], [float(g[0, 0]), -0.0], "out at +-1e30")
        _same_values(dg[0], [1.0, -0.0] if activation == "silu" else [_NAN, _NAN], "dgate at +-1e30")
    g = torch.tensor([[-100.0, 0.0, 1.0]], dtype=dtype, device="cuda")
    out = M.act_mul_forward(g, torch.full_like(g, _INF), activation=activation)
    assert bool(torch.isnan(out[0, :2]).all()) and float(out[0, 2]) == _INF


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_paths_equal_the_direct_backward(dtype):
    """act_mul, act_and_mul (whose gradient is ONE packed tensor), torch.ops, flash_attn.ops.activations.swiglu and
    inplace_backward: the forward and every gradient equal act_mul_forward / act_mul_backward bit for bit"""
    M = _M()
    import flash_attn.ops.activations as A
    import flash_attn_mi355.torch_ops  # noqa: F401
    ns = torch.ops.flash_attn_mi355
    B, S, N = 3, 5, 264
    g, u, d = (t.view(B, S, N) for t in _inputs(B * S, N, dtype, seed=7))
    for act in ("silu", "gelu", "relu"):
        want = _run(M, g, u, d, act)
        wantu = _run(M, g, None, d, act)

        def grads(fn, *leaves):
            ls = [t.clone().requires_grad_(True) for t in leaves]
            out = fn(*ls)
            out.backward(d)
            return out.detach(), ls
        out, (gl, ul) = grads(lambda a, b: M.act_mul(a, b, activation=act), g, u)
        for a, b, name in zip((out, gl.grad, ul.grad), want, ("out", "dgate", "dup")):
            _same(a, b, f"act_mul {act} {name}")
        out, (gl,) = grads(lambda a: M.act_mul(a, activation=act), g)
        _same(out, wantu[0], "ungated out")
        _same(gl.grad, wantu[1], "ungated dgate")
        out, (gl, ul) = grads(lambda a, b: ns.act_mul(a, b, act, False), g, u)
        for a, b, name in zip((out, gl.grad, ul.grad), want, ("out", "dgate", "dup")):
            _same(a, b, f"torch.ops act_mul {act} {name}")
        dgo, dpo = ns.act_mul_bwd(d, g, u, act)
        _same(dgo, want[1], "torch.ops act_mul_bwd dgate")
        _same(dpo, want[2], "torch.ops act_mul_bwd dup")
        dgo, dpo = ns.act_mul_bwd(d, g, None, act)
        _same(dgo, wantu[1], "torch.ops ungated dgate")
        assert tuple(dpo.shape) == (0,)
        # packed: one [.., 2N] gradient
        x = torch.cat([g, u], dim=-1)
        out, (xl,) = grads(lambda a: M.act_and_mul(a, activation=act), x)
        _same(out, want[0], "act_and_mul out")
        assert xl.grad.shape == x.shape and xl.grad.is_contiguous()
        _same(xl.grad, torch.cat([want[1], want[2]], dim=-1), "act_and_mul gradient")
        _same(ns.act_and_mul_bwd(d, x, act), xl.grad, "torch.ops act_and_mul_bwd")
        # in place: the gradients ARE the inputs' storage
        gl, ul = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
        gi, ui = gl.clone(), ul.clone()                       # (non-leaves with the leaves' bits: the in-place backward may
                                                              #  overwrite them, and a clone's backward hands the gradient on as it is)
        out = M.act_mul(gi, ui, activation=act, inplace_backward=True)
        out.backward(d)
        _same(gl.grad, want[1], "inplace_backward dgate")
        _same(ul.grad, want[2], "inplace_backward dup")
        _same(gi.detach(), want[1], "inplace_backward: gate holds dgate")
        xl = x.clone().requires_grad_(True)
        xi = xl.clone()
        M.act_and_mul(xi, activation=act, inplace_backward=True).backward(d)
        _same(xl.grad, torch.cat([want[1], want[2]], dim=-1), "act_and_mul inplace_backward")
        _same(xi.detach(), xl.grad, "act_and_mul inplace_backward: x holds its gradient")
    out, (gl, ul) = grads(A.swiglu, g, u)
    want = _run(M, g, u, d, "silu")
    for a, b, name in zip((out, gl.grad, ul.grad), want, ("out", "dx", "dy")):
        _same(a, b, "swiglu " + name)
    _same(A.swiglu_fwd(g, u), want[0], "swiglu_fwd")
    for a, b in zip(A.swiglu_bwd(g, u, d), want[1:]):
        _same(a, b, "swiglu_bwd")
    _same(A.gelu_fwd(g), M.act_mul_forward(g, activation="gelu_tanh"), "gelu_fwd")
    _same(A.gelu_bwd(d, g), M.act_mul_backward(d, g, activation="gelu_tanh")[0], "gelu_bwd")
    _same(A.sqrelu_fwd(g), M.act_mul_forward(g, activation="relu2"), "sqrelu_fwd")
    _same(A.sqrelu_bwd(d, g), M.act_mul_backward(d, g, activation="relu2")[0], "sqrelu_bwd")
    _same(A.relu_bwd(d, g), M.act_mul_backward(d, g, activation="relu")[0], "relu_bwd")
    out, (gl,) = grads(A.fast_gelu_impl, g)
    _same(gl.grad, A.gelu_bwd(d, g), "fast_gelu_impl gradient")


def test_forward_and_backward_replay_in_a_graph():
    """forward + backward (separate and packed) captured in one graph; replayed after the inputs were overwritten in place: every
    output equals the eager result bit for bit"""
    _M()
    import flash_attn_mi355.torch_ops  # noqa: F401
    ns = torch.ops.flash_attn_mi355
    dtype, rows, N = torch.bfloat16, 67, R.STEP + 8
    sets = [_inputs(rows, N, dtype, seed=30 + i) for i in range(3)]

    def run(g, u, d):
        out = ns.act_mul(g, u, "silu", False)
        dg, dp = ns.act_mul_bwd(d, g, u, "silu")
        x = torch.cat([g, u], dim=-1)
        return out, dg, dp, ns.act_and_mul(x, "gelu_tanh", False), ns.act_and_mul_bwd(d, x, "gelu_tanh")
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
        for got, want, name in zip(outs, ref[i], ("out", "dgate", "dup", "packed out", "packed gradient")):
            _same(got, want, f"replay {i} {name}")
    assert not torch.equal(guard.bits(ref[0][1]), guard.bits(ref[1][1]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1001, R.STEP + 8])
@pytest.mark.parametrize("gaps", [False, True])
def test_guard_bands(gaps, N, dtype):
    """every tensor is a view inside a NaN-filled slab (gaps=False at N = 1001: contiguous rows, every odd row misaligned and its
    neighbour's columns the first thing past it; gaps=True: NaN between the rows): nothing outside an output's elements is
    written, the inputs are unchanged, no NaN of a gap or a band reaches an output, and the results are the unguarded call's -
    out of place, then the backward in place"""
    M = _M()
    rows = 5
    g, u, d = _inputs(rows, N, dtype, seed=8)
    for act, up in (("silu", u), ("gelu", None)):
        want = _run(M, g, up, d, act)
        ins = [guard.guarded(t, gaps=gaps) for t in (g, up, d) if t is not None]
        gv, uv, dv = (ins[0][1], ins[1][1] if up is not None else None, ins[-1][1])
        assert gv.stride(0) > N if gaps else gv.stride(0) == N
        outs = [guard.guarded(shape=(rows, N), dtype=dtype, device="cuda", gaps=gaps) for _ in range(3 if up is not None else 2)]
        M.act_mul_forward(gv, uv, activation=act, out=outs[0][1])
        M.act_mul_backward(dv, gv, uv, activation=act, out=(outs[1][1], outs[2][1] if up is not None else None))
        torch.cuda.synchronize()
        for (buf, view, snap), name in zip(ins, ("gate", "up", "dout") if up is not None else ("gate", "dout")):
            assert torch.equal(guard.bits(buf), snap), f"{name} was written"
        for (buf, view, snap), w, name in zip(outs, want, ("out", "dgate", "dup")):
            guard.assert_untouched(buf, view, snap, name)
            assert not bool(torch.isnan(view).any()), f"{name}: a NaN from outside an input"
            _same(view, w, name)
        # in place: the inputs' own slabs are the outputs
        M.act_mul_backward(dv, gv, uv, activation=act, inplace=True)
        torch.cuda.synchronize()
        guard.assert_untouched(ins[0][0], gv, ins[0][2], "dgate in place")
        _same(gv, want[1], "dgate in place")
        if up is not None:
            guard.assert_untouched(ins[1][0], uv, ins[1][2], "dup in place")
            _same(uv, want[2], "dup in place")
        assert torch.equal(guard.bits(ins[-1][0]), ins[-1][2]), "dout was written"


def test_rows_that_start_past_2_31_elements():
    """3 rows of N = 264 as a view with row stride 2^30 + 8 over an uninitialised allocation - the last row starts 2^31 + 16
    elements in; only the rows are touched - against the same rows held contiguously, bit for bit: forward, then the backward in
    place over gate and up"""
    M = _M()
    dtype, rows, N, rs = torch.bfloat16, 3, 264, 2 ** 30 + 8
    g, u, d = _inputs(rows, N, dtype, seed=9)
    want = _run(M, g, u, d, "silu")
    bufs = [torch.empty((rows - 1) * rs + N, dtype=dtype, device="cuda") for _ in range(3)]
    gv, uv, ov = (b.as_strided((rows, N), (rs, 1)) for b in bufs)
    assert (rows - 1) * rs > 2 ** 31 and gv[rows - 1].data_ptr() - gv.data_ptr() > 2 ** 32
    gv.copy_(g)
    uv.copy_(u)
    ov.fill_(0)
    assert M.act_mul_forward(gv, uv, activation="silu", out=ov) is ov
    _same(ov.contiguous(), want[0], "out")
    ov.copy_(d)
    dg, dp = M.act_mul_backward(ov, gv, uv, activation="silu", inplace=True)
    assert dg is gv and dp is uv
    _same(gv.contiguous(), want[1], "dgate")
    _same(uv.contiguous(), want[2], "dup")
    _same(ov.contiguous(), d, "dout")
    del bufs, gv, uv, ov
    torch.cuda.empty_cache()
