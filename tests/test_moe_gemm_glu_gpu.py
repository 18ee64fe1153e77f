"""GPU: fa_moe_gemm_glu (the GLU instantiations of csrc/fa_moe_gemm.hip) - the gate-up grouped GEMM with the gated activation
in its epilogue - and moe_glu_linear, the differentiable layer on it.

The contract is bit equality with moe_gemm followed by act_mul_forward; the witness data of moe_gemm_ref.py make both
accumulator chains exact, so the fused output is also compared bit for bit against fp64 (relu: round16(relu(g16) * u16), a
product of two 16-bit values being exact in fp32).  Plans: block_m 128 over moe_gemm_ref.PATTERN, block_m 32 over DECODE.
Argument errors (Python and the C ABI, on host pointers: each returns before any launch) are in test_moe_gemm_glu_cpu.py."""
import pytest
import torch

import act_mul_ref as A
import guard
import moe_gemm_ref as G
from test_moe_gemm_glu_cpu import LIPSCHITZ, glu_share

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DEV = "cuda"
DECODE = [5, 0, 9, 16, 1, 0, 3]                              # with align 16 and a +0 tail: 96 + 11 rows <= 32 x 7
PLANS = {128: dict(lengths=G.PATTERN, align=1, tail=0), 32: dict(lengths=DECODE, align=16, tail=11)}
SORTS = {128: (67, 6, 7, 16), 32: (5, 2, 7, 1)}              # (T, top_k, E, align) whose moe_sort tables reach each plan


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


def _dev(a, dtype):
    return torch.from_numpy(a).to(dtype).to(DEV)


def _sorted(M, T, topk, E, align, seed):
    """moe_sort's own tables, with dropped ids (-1 and E) and, with align > 1, padding slots"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32)
    ids[1, 0], ids[T - 1, topk - 1] = -1, E
    return M.moe_sort(ids.to(DEV), E, align=align)


def _random(rows, K, I, E, layout, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g).to(dtype).to(DEV)
    w = (torch.randn((E, 2 * I, K) if layout == "nk" else (E, K, 2 * I), generator=g) / K ** 0.5).to(dtype).to(DEV)
    return x, w, torch.randn(E, 2 * I, generator=g).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("block_m", [128, 32])
def test_witness_bit_for_bit_against_fp64(block_m, layout, dtype):
    """relu on witness data, every K x I, into a strided out between guard bands; the bias (none, io dtype, fp32) cycles over
    the shapes.  A gate paired with the wrong up column, a tail masked on one half only or a wrong "kn" upper-half lane map
    changes bits here."""
    M, p = _M(), PLANS[block_m]
    E = len(p["lengths"])
    off = G.offsets_of(p["lengths"], p["align"])
    rows = int(off[E]) + p["tail"]
    for i, (K, I) in enumerate((K, I) for K in (8, 24, 264) for I in (8, 40, 72, 136)):
        assert M.moe_gemm_glu_plan(rows, I, K, E, w_layout=layout, dtype=dtype)[:2] == (block_m, 64)
        x, w, bias = G.witness(rows, K, 2 * I, E, layout, 1000 + i, i % 3 != 0)
        buf, view = guard.slab((rows, I), dtype, gaps=True, device=DEV, check_prep=False)
        snap = guard.snapshot(buf)
        bt = None if bias is None else _dev(bias, torch.float32 if i % 3 == 2 else dtype)
        got = M.moe_gemm_glu(_dev(x, dtype), _dev(w, dtype), torch.from_numpy(off).to(DEV), activation="relu", w_layout=layout,
                             bias=bt, out=view)
        torch.cuda.synchronize()
        assert got is view
        guard.assert_untouched(buf, view, snap, "out")
        h16 = torch.from_numpy(G.expected(x, w, off, _name(dtype), layout=layout, bias=bias)).float()
        g16, u16 = h16[:, :I], h16[:, I:]
        want = (torch.where(g16 <= 0, torch.zeros_like(g16), g16) * u16).to(dtype)       # fp32: exact, then ONE rounding
        _same(view.cpu(), want, f"witness block_m {block_m} K {K} I {I} {layout} {_name(dtype)} bias {i % 3}")


def _fused_equals_composed(M, block_m, K, I, activation, layout, dtype):
    from flash_attn_mi355 import act_mul
    T, topk, E, align = SORTS[block_m]
    sorted_slot, pos, offsets = _sorted(M, T, topk, E, align, 2000 + block_m)
    assert bool((sorted_slot < 0).any())
    x, w, bias = _random(T, K, I, E, layout, dtype, 2100 + K)
    assert M.moe_gemm_glu_plan(sorted_slot.shape[0], I, K, E, w_layout=layout, dtype=dtype)[0] == block_m
    xp = M.moe_permute_forward(x, sorted_slot, topk)
    for kw in (dict(sorted_slot=sorted_slot, top_k=topk), dict()):
        xa = x if kw else xp
        h = M.moe_gemm(xa, w, offsets, w_layout=layout, bias=bias, **kw)
        want = act_mul.act_mul_forward(h[:, :I], h[:, I:], activation=activation)
        got = M.moe_gemm_glu(xa, w, offsets, activation=activation, w_layout=layout, bias=bias, **kw)
        _same(got, want, f"{activation} {layout} {_name(dtype)} block_m {block_m} {'gather' if kw else 'plain'}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("block_m", [128, 32])
@pytest.mark.parametrize("activation", A.ACTIVATIONS)
def test_fused_equals_moe_gemm_then_act_mul(activation, block_m, layout, dtype):
    """random data, bias, plain and gathered through moe_sort's tables: the contract, bit for bit"""
    _fused_equals_composed(_M(), block_m, 264, 136, activation, layout, dtype)


def test_fused_equals_composed_at_2880():
    _fused_equals_composed(_M(), 128, 2880, 264, "silu", "kn", torch.bfloat16)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("activation", sorted(LIPSCHITZ))
def test_against_the_plain_fp64_definition(activation, layout, dtype):
    """act(g) * u without intermediate rounding; the bound is test_moe_gemm_glu_cpu.py's (derived, not measured)"""
    M = _M()
    for block_m, p in PLANS.items():
        off = G.offsets_of(p["lengths"], p["align"])
        x, w, bias = _random(int(off[-1]), 264, 136, len(p["lengths"]), layout, dtype, 3000 + block_m)
        got = M.moe_gemm_glu(x, w, torch.from_numpy(off).to(DEV), activation=activation, w_layout=layout, bias=bias)
        share = glu_share(got, x, w, off, bias, activation, layout, dtype)
        print(f"share moe_gemm_glu {activation} {layout} {_name(dtype)} block_m {block_m}: {share:.3f}")
        assert share <= 1.0, f"{share:.3f} of the bound"


@pytest.mark.parametrize("layout", ["nk", "kn"])
def test_a_row_has_the_same_bits_alone_and_in_a_batch(layout):
    M = _M()
    dtype, K, I, E = torch.bfloat16, 264, 136, 7
    x, w, bias = _random(226, K, I, E, layout, dtype, 77)
    off = torch.from_numpy(G.offsets_of(G.PATTERN)).to(DEV)
    r0, r1 = 97 + 3, 97 + 128                                # expert 6 owns rows 97 .. 225: its first and second tile
    x[r1] = x[r0]
    big = M.moe_gemm_glu(x, w, off, w_layout=layout, bias=bias)
    _same(big[r0], big[r1], "a row at two places of its segment")
    lone_off = torch.tensor([0] * 7 + [1], dtype=torch.int32, device=DEV)
    assert M.moe_gemm_glu_plan(1, I, K, E)[0] == 32 and M.moe_gemm_glu_plan(226, I, K, E)[0] == 128
    lone = M.moe_gemm_glu(x[r0:r0 + 1], w, lone_off, w_layout=layout, bias=bias)
    _same(lone[0], big[r0], "a row alone against the row in a batch")


def test_replays_in_a_graph_after_the_tables_were_rewritten():
    M = _M()
    ns = torch.ops.flash_attn_mi355
    dtype, (T, topk, E, align), K, I = torch.bfloat16, (67, 2, 8, 16), 264, 136     # (segment lengths differ between the seeds)
    tables = [_sorted(M, T, topk, E, align, 700 + i) for i in range(3)]
    assert not torch.equal(tables[0][2], tables[1][2])
    x, w, bias = _random(T, K, I, E, "nk", dtype, 710)
    ref = [ns.moe_gemm_glu(x, w, t[2], "gelu_tanh", "nk", bias, t[0], topk).clone() for t in tables]
    ss, off = tables[0][0].clone(), tables[0][2].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ns.moe_gemm_glu(x, w, off, "gelu_tanh", "nk", bias, ss, topk)
    for i in (1, 2, 0):
        ss.copy_(tables[i][0])
        off.copy_(tables[i][2])
        graph.replay()
        torch.cuda.synchronize()
        _same(out, ref[i], f"replay {i}")


def test_opcheck():
    M = _M()
    ns = torch.ops.flash_attn_mi355
    dtype, T, topk, E, K, I = torch.bfloat16, 5, 2, 8, 16, 24
    g = torch.Generator().manual_seed(950)
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32)
    ss, pos, off = M.moe_sort(ids.to(DEV), E, align=4)
    x, w, bias = _random(T, K, I, E, "nk", dtype, 951)
    xp, wkn = M.moe_permute_forward(x, ss, topk), w.transpose(1, 2).contiguous()
    torch.library.opcheck(ns.moe_gemm_glu, (x, w, off, "silu", "nk", bias, ss, topk))
    torch.library.opcheck(ns.moe_gemm_glu, (xp, wkn, off, "gelu", "kn", None, None, None))
    req = lambda t, r=True: t.clone().requires_grad_(r)          # noqa: E731
    torch.library.opcheck(ns.moe_glu_linear, (req(x), req(w), off, "silu", "nk", req(bias), ss, topk, pos))
    torch.library.opcheck(ns.moe_glu_linear, (req(xp), req(wkn, False), off, "relu2", "kn", None, None, None, None))


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "gather"])
@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("activation", ["silu", "gelu_tanh"])
def test_moe_glu_linear_has_the_gradients_of_the_two_layers(activation, layout, gather):
    """forward and dx, dw, dbias bit-identical to autograd through act_and_mul(moe_linear(...))"""
    from flash_attn_mi355 import act_mul
    M = _M()
    dtype, K, I, E = torch.bfloat16, 264, 136, 7
    kw = {}
    if gather:
        T, topk, _, align = SORTS[128]
        ss, pos, off = _sorted(M, T, topk, E, align, 4000)
        rows, kw = T, dict(sorted_slot=ss, top_k=topk, pos=pos)
    else:
        off = torch.from_numpy(G.offsets_of(G.PATTERN)).to(DEV)
        rows = int(off[-1])
    x, w, bias = _random(rows, K, I, E, layout, dtype, 4100)
    dy = torch.randn(ss.shape[0] if gather else rows, I, generator=torch.Generator().manual_seed(4200)).to(dtype).to(DEV)
    res = []
    for fused in (True, False):
        ins = [t.clone().requires_grad_() for t in (x, w, bias)]
        if fused:
            y = M.moe_glu_linear(ins[0], ins[1], off, activation=activation, w_layout=layout, bias=ins[2], **kw)
        else:
            y = act_mul.act_and_mul(M.moe_linear(ins[0], ins[1], off, w_layout=layout, bias=ins[2], **kw), activation=activation)
        res.append((y,) + torch.autograd.grad(y, ins, dy))
    for name, a, b in zip(("out", "dx", "dw", "dbias"), *res):
        _same(a.detach(), b.detach(), f"{name} {activation} {layout}")
