"""GPU: fa_moe_gemm_mxfp4_dgrad (csrc/fa_moe_gemm_mxfp4_dgrad.hip) bit for bit against fp64 and against fa_moe_gemm's "kn" form on
dequantised weights, and moe_linear_mxfp4 against moe_linear on them.

Witness data: every code, scale bytes 126 ... 128 that differ from weight row to row and from block to block, dy integers in
[-3, 3]: a product is a multiple of 1/4 of magnitude <= 36, so any partial sum at N <= 264 is below 2^24 quarter units and exact
in fp32 in any order; dx must be round_bf16(exact).  N runs over half an MFMA step, tails inside a 64-row stage and more than four
stages; K over tails of the 128-wide tile with scale blocks that differ inside it."""
import numpy as np
import pytest
import torch

import guard
import moe_gemm_ref as G
import mx_quant_ref as Q

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
# segment lengths by (plan, E): 0 / 1 / 31 / 32 / 33 / 129 rows at unaligned starts; (rows + tail <= 32 E) picks block_m 32
LENGTHS = {(128, 7): G.PATTERN, (32, 7): [0, 1, 31, 32, 0, 129, 3], (128, 2): [129, 33], (32, 2): [33, 31]}
NS, KS = [8, 40, 72, 264], [32, 96, 160, 288]


def _M():
    from flash_attn_mi355 import moe
    import flash_attn_mi355.torch_ops  # noqa: F401
    return moe


def _same(got, want, name):
    assert got.shape == want.shape and got.dtype == want.dtype, name
    a, b = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    assert torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ"


def _case(block_m, E, N, K, seed, ints=True):
    """one problem on the device.  ints: witness data; else N(0, 1) dy and weights made by the quantiser from N(0, 1) * 2^[-4, 4]"""
    g = np.random.default_rng(seed)
    off = G.offsets_of(LENGTHS[block_m, E])
    rows = int(off[E]) + (0 if (block_m, E) == (32, 2) else 5)
    c = dict(off=off, rows=rows, E=E)
    if ints:
        c["blocks"] = g.integers(0, 256, (E, N, K // 2), dtype=np.uint8)
        c["scales"] = g.integers(126, 129, (E, N, K // 32)).astype(np.uint8)
        dy = g.integers(-3, 4, (rows, N)).astype(np.float64)
    else:
        c["blocks"], c["scales"] = Q.quant(g.standard_normal((E, N, K)) * np.exp2(g.integers(-4, 5, (E, N, 1))))
        dy = g.standard_normal((rows, N))
    c["dy"] = torch.from_numpy(dy).to(BF).to(DEV)
    c["b"], c["s"], c["o"] = (torch.from_numpy(c[k]).to(DEV) for k in ("blocks", "scales", "off"))
    assert _M().moe_gemm_mxfp4_dgrad_plan(rows, N, K, E)[0] == block_m == _M().moe_gemm_plan(rows, K, N, E, w_layout="kn")[0]
    return c


def _kn(c):
    """the parent's path: moe_gemm's "kn" form on the dequantised [E, N, K] weights"""
    from flash_attn_mi355 import quant
    return _M().moe_gemm(c["dy"], quant.dequant_mxfp4(c["b"], c["s"]), c["o"], w_layout="kn")


@pytest.mark.parametrize("block_m", [32, 128])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_witness_bit_for_bit(N, K, block_m):
    """nibble and byte order, the scale of (n, k / 32), N and K tails, segment edges, the +0 tail; E rotates over the shapes"""
    c = _case(block_m, (2, 7)[(NS.index(N) + KS.index(K)) % 2], N, K, 100 + N + K)
    want = G.expected(c["dy"].double().cpu().numpy(), Q.dequant(c["blocks"], c["scales"]), c["off"], "bfloat16", layout="kn")
    got = _M().moe_gemm_mxfp4_dgrad(c["dy"], c["b"], c["s"], c["o"])
    _same(got, torch.from_numpy(want).to(BF).to(DEV), f"witness N {N} K {K} block_m {block_m}")    # (bits: the tail is +0)


@pytest.mark.parametrize("block_m", [32, 128])
@pytest.mark.parametrize("N,K,E", [(264, 288, 7), (2880, 2880, 2)])
def test_equals_kn_gemm_on_dequantised_weights(N, K, E, block_m):
    """random bf16 dy: inexact sums, so the bits hold only with every operand in moe_gemm's slot and chain order"""
    c = _case(block_m, E, N, K, 200 + N, ints=False)
    _same(_M().moe_gemm_mxfp4_dgrad(c["dy"], c["b"], c["s"], c["o"]), _kn(c), f"N {N} K {K} E {E} block_m {block_m}")


def _strided_experts(t):
    """`t` [E, ...] as a view whose experts lie 48 bytes further apart than they need, between bands of 0xFF"""
    E, n = t.shape[0], t[0].numel()
    buf = torch.full((64 + E * (n + 48),), 0xFF, dtype=torch.uint8, device=DEV)
    view = buf[64:].as_strided(t.shape, (n + 48,) + tuple(t[0].stride()))
    view.copy_(t)
    return buf, view


@pytest.mark.parametrize("block_m", [32, 128])
def test_isolation_batch_and_plan_invariance(block_m):
    """N and K tails next to 0xFF bands (scale 0xFF is NaN even with a zero code), dx between guard bands; every other expert's
    slabs 0xFF; a row alone (the decode plan) is the row in the batch"""
    c = _case(block_m, 7, 264, 288, 400 + block_m, ints=False)
    M, E, off = _M(), 7, c["off"]
    (bbuf, blocks), (sbuf, scales) = _strided_experts(c["b"]), _strided_experts(c["s"])
    obuf, out = guard.slab((c["rows"], 288), BF, gaps=True, device=DEV, check_prep=False)
    snap = guard.snapshot(obuf)
    assert M.moe_gemm_mxfp4_dgrad(c["dy"], blocks, scales, c["o"], out=out) is out
    torch.cuda.synchronize()
    guard.assert_untouched(obuf, out, snap, "dx")
    _same(out, _kn(c), "strided dx and expert-strided weights")
    assert not out.isnan().any()
    for e in (1, 3, 6):
        r = int(off[e + 1]) - 1
        alone = torch.tensor([0] * (e + 1) + [1] * (E - e), dtype=torch.int32, device=DEV)
        _same(M.moe_gemm_mxfp4_dgrad(c["dy"][r:r + 1], blocks, scales, alone), out[r:r + 1], f"row {r} alone")
        b2 = torch.full_like(bbuf, 0xFF)[64:].as_strided(blocks.shape, blocks.stride())
        s2 = torch.full_like(sbuf, 0xFF)[64:].as_strided(scales.shape, scales.stride())
        b2[e], s2[e] = blocks[e], scales[e]
        only = M.moe_gemm_mxfp4_dgrad(c["dy"], b2, s2, c["o"])
        _same(only[int(off[e]):int(off[e + 1])], out[int(off[e]):int(off[e + 1])], f"expert {e} among 0xFF experts")
        assert not only[int(off[E]):].isnan().any()


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "gather"])
def test_moe_linear_mxfp4_equals_moe_linear_on_dequantised_weights(gather):
    """out, dx and dbias under autograd, through moe_sort's tables in the gather form; the weights get no gradient"""
    from flash_attn_mi355 import quant
    M, g, E, N, K, T, topk = _M(), torch.Generator().manual_seed(7), 7, 136, 288, 67, 2
    blocks, scales = (torch.from_numpy(t).to(DEV) for t in Q.quant(np.random.default_rng(5).standard_normal((E, N, K))))
    ss, pos, off = M.moe_sort(torch.randint(0, E, (T, topk), generator=g).to(torch.int32).to(DEV), E, align=16)
    x0 = torch.randn(T if gather else ss.shape[0], K, generator=g).to(BF).to(DEV)
    b0, dy = torch.randn(E, N, generator=g).to(DEV), torch.randn(ss.shape[0], N, generator=g).to(BF).to(DEV)
    kw = dict(sorted_slot=ss, top_k=topk, pos=pos) if gather else {}
    res = []
    for f, w in ((M.moe_linear_mxfp4, (blocks, scales)), (M.moe_linear, (quant.dequant_mxfp4(blocks, scales),))):
        x, b = x0.clone().requires_grad_(), b0.clone().requires_grad_()
        out = f(x, *w, off, bias=b, **kw)
        res.append((out, *torch.autograd.grad(out, (x, b), dy)))
    for name, got, want in zip(("out", "dx", "dbias"), *res):
        assert got.dtype == want.dtype and torch.equal(guard.bits(got), guard.bits(want)), name


def test_graph_replay_and_opcheck():
    c = _case(32, 7, 72, 160, 500, ints=False)
    ns = torch.ops.flash_attn_mi355
    tables = [c["o"].clone(), torch.from_numpy(G.offsets_of([9, 0, 50, 1, 64, 3, 2])).to(DEV)]
    eager = [ns.moe_gemm_mxfp4_dgrad(c["dy"], c["b"], c["s"], off) for off in tables]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ns.moe_gemm_mxfp4_dgrad(c["dy"], c["b"], c["s"], c["o"])
    for i in (1, 0, 1):
        c["o"].copy_(tables[i])
        graph.replay()
        torch.cuda.synchronize()
        _same(out, eager[i], f"replay with table {i}")
    torch.library.opcheck(ns.moe_gemm_mxfp4_dgrad, (c["dy"], c["b"], c["s"], c["o"]))
    ss, pos, off = _M().moe_sort(torch.arange(40 * 2, dtype=torch.int32, device=DEV).view(40, 2) % 7, 7)   # 80 rows
    req = lambda t: t.clone().requires_grad_()                                                 # noqa: E731
    x, xp, bias = torch.randn(40, 160, device=DEV).to(BF), torch.randn(80, 160, device=DEV).to(BF), torch.randn(7, 72, device=DEV)
    torch.library.opcheck(ns.moe_linear_mxfp4, (req(x), c["b"], c["s"], off, req(bias), ss, 2, pos))
    torch.library.opcheck(ns.moe_linear_mxfp4, (req(xp), c["b"], c["s"], off, None, None, None, None))
