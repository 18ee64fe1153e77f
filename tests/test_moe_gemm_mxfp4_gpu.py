"""GPU: fa_moe_gemm_mxfp4 (csrc/fa_moe_gemm_mxfp4.hip) bit for bit against fp64 and against fa_moe_gemm on dequantised weights.

The fp64 reference is E2M1 and ldexp below.  Witness data: every code, scale bytes 126 ... 128, x integers in [-3, 3], bias in
[-8, 8]: a product is a multiple of 1/4 of magnitude <= 36, so any partial sum at K <= 288 is below 2^24 quarter units and exact
in fp32 in any order; out must be round_bf16(exact).  Plans: block_m 32 where rows <= 32 E (block_k 256), else 128 (block_k 128);
K runs over both steps' edges and 288 (9 scale bytes a row), N over a tile's tail."""
import numpy as np
import pytest
import torch

import guard
import moe_gemm_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])
# segment lengths by (plan, E): 0 / 1 / 31 / 32 / 33 / 129 rows at unaligned starts; (rows + tail <= 32 E) picks block_m 32
LENGTHS = {(128, 7): G.PATTERN, (32, 7): [0, 1, 31, 32, 0, 129, 3], (128, 2): [129, 33], (32, 2): [33, 31]}


def _M():
    from flash_attn_mi355 import moe
    import flash_attn_mi355.torch_ops  # noqa: F401
    return moe


def dequant(blocks, scales):
    """uint8 [E, N, K / 2], [E, N, K / 32] -> float64 [E, N, K]: element k in byte k // 2, low nibble for even k"""
    codes = np.stack([blocks & 15, blocks >> 4], axis=-1).reshape(*blocks.shape[:2], -1)
    return np.ldexp(E2M1[codes], np.repeat(scales.astype(np.int64) - 127, 32, axis=-1))


def _same(got, want, name):
    assert got.shape == want.shape and got.dtype == want.dtype, name
    a, b = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    assert torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ"


def _case(block_m, E, K, N, seed, scales=(126, 128), ints=True, bias=None, gather=False):
    """numpy inputs and device tensors of one problem; gather: x [40, K] read through sorted_slot with a -1 and an out-of-range slot"""
    g = np.random.default_rng(seed)
    off = G.offsets_of(LENGTHS[block_m, E])
    rows = int(off[E]) + (0 if (block_m, E) == (32, 2) else 5)
    c = dict(off=off, rows=rows, blocks=g.integers(0, 256, (E, N, K // 2), dtype=np.uint8),
             scales=g.integers(scales[0], scales[1] + 1, (E, N, K // 32)).astype(np.uint8), ss=None, topk=None)
    nx = 40 if gather else rows
    x = g.integers(-3, 4, (nx, K)).astype(np.float64) if ints else g.standard_normal((nx, K))
    c["x"] = torch.from_numpy(x).to(BF)
    c["a"] = c["x"].double().numpy()
    if gather:
        c["topk"] = 2
        ss = g.integers(0, 80, rows).astype(np.int32)
        ss[[0, rows // 2]] = -1, 80
        ok = (ss >= 0) & (ss < 80)
        c["a"] = np.where(ok[:, None], c["a"][np.where(ok, ss, 0) // 2], 0.0)
        c["ss"] = torch.from_numpy(ss).to(DEV)
    c["bias"] = None if bias is None else g.integers(-8, 9, (E, N)).astype(np.float64)
    c["t"] = dict(x=c["x"].to(DEV), blocks=torch.from_numpy(c["blocks"]).to(DEV), scales=torch.from_numpy(c["scales"]).to(DEV),
                  off=torch.from_numpy(off).to(DEV), bias=None if bias is None else torch.from_numpy(c["bias"]).to(bias).to(DEV))
    assert _M().moe_gemm_mxfp4_plan(rows, N, K, E)[0] == block_m
    return c


def _run(c, **kw):
    t = c["t"]
    return _M().moe_gemm_mxfp4(t["x"], t["blocks"], t["scales"], t["off"], bias=t["bias"], sorted_slot=c["ss"], top_k=c["topk"], **kw)


def _want64(c):
    want = G.expected(c["a"], dequant(c["blocks"], c["scales"]), c["off"], "bfloat16", bias=c["bias"])
    return torch.from_numpy(want).to(BF).to(DEV)


KS = [32, 96, 128, 160, 224, 256, 288]                        # block_k - 32, block_k, block_k + 32 of both plans


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("block_m", [32, 128])
@pytest.mark.parametrize("N", [8, 40, 264])
@pytest.mark.parametrize("K", KS)
def test_witness_bit_for_bit(K, N, block_m, gather):
    """nibble and byte order, scale indexing, K and N tails, segment edges; E and the bias kind rotate over the shapes"""
    i = KS.index(K) + [8, 40, 264].index(N) + gather
    c = _case(block_m, (2, 7)[i % 2], K, N, 100 + i, bias=(None, BF, torch.float32)[i % 3], gather=gather)
    _same(_run(c), _want64(c), f"witness K {K} N {N} block_m {block_m} gather {gather}")


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("block_m", [32, 128])
@pytest.mark.parametrize("K,N,E", [(96, 40, 2), (288, 264, 7), (2880, 264, 7)])
def test_equals_moe_gemm_on_dequantised_weights(K, N, E, block_m, gather):
    c = _case(block_m, E, K, N, 200 + K, scales=(117, 137), ints=False, bias=torch.float32, gather=gather)
    t = c["t"]
    w = torch.from_numpy(dequant(c["blocks"], c["scales"])).to(BF).to(DEV)              # exact in bf16
    want = _M().moe_gemm(t["x"], w, t["off"], bias=t["bias"], sorted_slot=c["ss"], top_k=c["topk"])
    _same(_run(c), want, f"K {K} N {N} E {E} block_m {block_m} gather {gather}")


@pytest.mark.parametrize("block_m", [32, 128])
def test_scale_range(block_m):
    """scale bytes 2 and 252 on alternate weight rows, one activation of +-1 per row: out is a weight, exact in bf16"""
    c = _case(block_m, 2, 64, 8, 300)
    c["scales"][:, 0::2], c["scales"][:, 1::2] = 2, 252
    c["a"] = np.zeros_like(c["a"])
    r = np.arange(c["rows"])
    c["a"][r, r % 64] = np.where(r % 3, 1.0, -1.0)
    c["t"]["x"], c["t"]["scales"] = torch.from_numpy(c["a"]).to(BF).to(DEV), torch.from_numpy(c["scales"]).to(DEV)
    _same(_run(c), _want64(c), f"scale bytes 2 and 252, block_m {block_m}")


def _strided_experts(t, fill=0xFF):
    """(buf, view): `t` [E, ...] as a view whose experts lie 48 bytes further apart than they need, between bands of 0xFF"""
    E, n = t.shape[0], t[0].numel()
    buf = torch.full((64 + E * (n + 48),), fill, dtype=torch.uint8, device=DEV)
    view = buf[64:].as_strided(t.shape, (n + 48,) + tuple(t[0].stride()))
    view.copy_(t)
    return buf, view


def test_isolation():
    c = _case(128, 7, 288, 264, 400, scales=(117, 137), ints=False, bias=BF)
    t, M, E, rows, off = c["t"], _M(), 7, c["rows"], c["off"]
    (bbuf, blocks), (sbuf, scales) = _strided_experts(t["blocks"]), _strided_experts(t["scales"])
    obuf, out = guard.slab((rows, 264), BF, gaps=True, device=DEV, check_prep=False)
    snap = guard.snapshot(obuf)
    got = M.moe_gemm_mxfp4(t["x"], blocks, scales, t["off"], bias=t["bias"], out=out)
    torch.cuda.synchronize()
    assert got is out
    guard.assert_untouched(obuf, out, snap, "out")
    _same(out, _run(c), "strided out and expert-strided weights against contiguous ones")
    _same(out, _run(c), "two runs")
    assert (out[int(off[E]):].view(torch.int16) == 0).all()                      # the tail is +0
    for e in (1, 2, 4, 6):                                                       # a row alone (block_m 32) is the row in the batch
        r = int(off[e + 1]) - 1
        alone = torch.tensor([0] * (e + 1) + [1] * (E - e), dtype=torch.int32, device=DEV)
        _same(M.moe_gemm_mxfp4(t["x"][r:r + 1], blocks, scales, alone, bias=t["bias"]), out[r:r + 1], f"row {r} alone")
        bbuf2, sbuf2 = torch.full_like(bbuf, 0xFF), torch.full_like(sbuf, 0xFF)  # every other expert: codes and scales 0xFF
        b2, s2 = bbuf2[64:].as_strided(blocks.shape, blocks.stride()), sbuf2[64:].as_strided(scales.shape, scales.stride())
        b2[e], s2[e] = blocks[e], scales[e]
        only = M.moe_gemm_mxfp4(t["x"], b2, s2, t["off"], bias=t["bias"])
        _same(only[int(off[e]):int(off[e + 1])], out[int(off[e]):int(off[e + 1])], f"expert {e} among 0xFF experts")


def test_graph_replay_and_opcheck():
    c = _case(32, 7, 288, 40, 500, scales=(117, 137), ints=False, bias=torch.float32, gather=True)
    t, ns = c["t"], torch.ops.flash_attn_mi355
    args = (t["x"], t["blocks"], t["scales"], t["off"], t["bias"], c["ss"], 2)
    tables = [(c["ss"].clone(), t["off"].clone()), (c["ss"].flip(0).contiguous(), torch.from_numpy(G.offsets_of([9, 0, 50, 1, 64, 3, 2])).to(DEV))]
    eager = []
    for ss, off in tables:
        eager.append(ns.moe_gemm_mxfp4(t["x"], t["blocks"], t["scales"], off, t["bias"], ss, 2))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ns.moe_gemm_mxfp4(*args)
    for i in (1, 0, 1):
        c["ss"].copy_(tables[i][0])
        t["off"].copy_(tables[i][1])
        graph.replay()
        torch.cuda.synchronize()
        _same(out, eager[i], f"replay with tables {i}")
    torch.library.opcheck(ns.moe_gemm_mxfp4, args)
    torch.library.opcheck(ns.moe_gemm_mxfp4, (t["x"], t["blocks"], t["scales"], t["off"], None, None, None))   # plain: 40 rows
