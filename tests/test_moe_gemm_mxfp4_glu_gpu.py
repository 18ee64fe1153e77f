"""GPU: fa_moe_gemm_mxfp4_glu (csrc/fa_moe_gemm_mxfp4.hip, the GLU kernels).  K 96 and 288 lie below and across block_k of both plans;
I = 8 is a 16-row weight image, 40 a partial tile, 72 a tile and a tail, 136 two tiles and a tail.  Witness data: x integers in [-3, 3],
scale bytes 126 ... 128, integer bias: h = round_bf16(exact) and relu(g) * u is exact in fp32 - out is its one rounding, bit for bit."""
import numpy as np
import pytest
import torch

import guard
import moe_gemm_ref as G
from test_moe_gemm_mxfp4_gpu import LENGTHS, dequant

pytestmark = pytest.mark.gpu

DEV, BF = "cuda", torch.bfloat16
KS, IS, ORDERS = [96, 288], [8, 40, 72, 136], ["interleaved", "packed"]
shapes = pytest.mark.parametrize("K,I", [(K, I) for K in KS for I in IS])
forms = pytest.mark.parametrize("block_m,gate_up,gather", [(b, o, g) for b in (32, 128) for o in ORDERS for g in (False, True)])


def _M():
    from flash_attn_mi355 import moe
    import flash_attn_mi355.torch_ops  # noqa: F401
    return moe


def _case(block_m, E, K, I, seed, scales=(126, 128), ints=True, bias=None, gather=False):
    """one problem whose weights hold 2 I rows; gather: x [40, K] read through sorted_slot with a -1 and an out-of-range slot"""
    g = np.random.default_rng(seed)
    off = G.offsets_of(LENGTHS[block_m, E])
    rows = int(off[E]) + (0 if (block_m, E) == (32, 2) else 5)
    c = dict(off=off, rows=rows, E=E, I=I, ss=None, topk=None, blocks=g.integers(0, 256, (E, 2 * I, K // 2), dtype=np.uint8),
             scales=g.integers(scales[0], scales[1] + 1, (E, 2 * I, K // 32)).astype(np.uint8))
    c["x"] = (torch.from_numpy(g.integers(-3, 4, (rows, K)).astype(np.float64) if ints else g.standard_normal((rows, K))).to(BF))[:40 if gather else rows]
    if gather:
        ss = g.integers(0, 80, rows).astype(np.int32)
        ss[[0, rows // 2]] = -1, 80
        c["ss"], c["topk"], c["ok"], c["src"] = torch.from_numpy(ss).to(DEV), 2, (ss >= 0) & (ss < 80), np.clip(ss, 0, 79) // 2
    c["bias"] = None if bias is None else torch.from_numpy(g.integers(-8, 9, (E, 2 * I)).astype(np.float64)).to(bias)
    assert _M().moe_gemm_mxfp4_glu_plan(rows, I, K, E)[0] == block_m
    return c


def _dev(c):
    return (c["x"].to(DEV),) + tuple(torch.from_numpy(c[k]).to(DEV) for k in ("blocks", "scales", "off"))


def _run(c, **kw):
    return _M().moe_gemm_mxfp4_glu(*_dev(c), bias=None if c["bias"] is None else c["bias"].to(DEV), sorted_slot=c["ss"],
                                   top_k=c["topk"], **kw)


def _halves(h, gate_up):                                          # the gate and up columns of h [.., 2 I] (numpy or torch)
    return (h[..., 0::2], h[..., 1::2]) if gate_up == "interleaved" else (h[..., :h.shape[-1] // 2], h[..., h.shape[-1] // 2:])


def _same(got, want, name):
    a, b = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    assert got.dtype == want.dtype and a.shape == b.shape and torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ"


@pytest.mark.parametrize("activation", ["relu", "silu"])
@forms
@shapes
def test_bit_for_bit(K, I, block_m, gate_up, gather, activation):
    """relu, witness data against fp64: the gate - up pairing, a tail masked on one half only or a wrong scale row (packed) change
    bits; E and the bias kind rotate.  silu, random data against moe_gemm_glu on the dequantised (exact in bf16) weights with rows
    and bias columns in packed order: also interleaved(w) == packed(w re-ordered)"""
    i, name = KS.index(K) + IS.index(I) + gather, f"{activation} K {K} I {I} block_m {block_m} {gate_up} gather {gather}"
    if activation == "relu":
        c = _case(block_m, (2, 7)[i % 2], K, I, 100 + i, bias=(None, BF, torch.float32)[i % 3], gather=gather)
        a = c["x"].double().numpy()
        a = np.where(c["ok"][:, None], a[c["src"]], 0.0) if gather else a
        g, u = _halves(G.expected(a, dequant(c["blocks"], c["scales"]), c["off"], "bfloat16",
                                  bias=None if c["bias"] is None else c["bias"].double().numpy()), gate_up)
        want = torch.from_numpy(np.where(g <= 0, 0.0, g) * u).to(torch.float32).to(BF).to(DEV)
    else:
        c = _case(block_m, (7, 2)[i % 2], K, I, 200 + K + I, scales=(117, 137), ints=False, bias=torch.float32, gather=gather)
        w = torch.cat(_halves(torch.from_numpy(dequant(c["blocks"], c["scales"])).to(BF).transpose(1, 2), gate_up), dim=2)
        want = _M().moe_gemm_glu(c["x"].to(DEV), w.transpose(1, 2).contiguous().to(DEV), torch.from_numpy(c["off"]).to(DEV), activation="silu",
                                 bias=torch.cat(_halves(c["bias"], gate_up), dim=1).to(DEV), sorted_slot=c["ss"], top_k=c["topk"])
    _same(_run(c, activation=activation, gate_up=gate_up), want, name)


def _ordered(t):                                                  # bf16 -> integers in the values' order: neighbours differ by 1
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7fff), b)


@pytest.mark.parametrize("alpha,limit,sd", [(None, None, 5.0), (1.0, 2.5, 2.5 * 5 / 7)])
@pytest.mark.parametrize("block_m,gate_up,gather", [(32, "interleaved", True), (32, "packed", False), (128, "interleaved", False), (128, "packed", True)])
@pytest.mark.parametrize("K,I", [(96, 40), (288, 136)])
def test_swiglu_oai_within_one_ulp_of_fp64(K, I, block_m, gate_up, gather, alpha, limit, sd):
    """h from moe_gemm_mxfp4 on the device (bit-identical by contract), the formula in fp64, one rounding.  fp32 and the hardware exp2 /
    reciprocal err by about 2^-17, far below half a bf16 ulp: the reference's rounding or its neighbour.  h's spread is limit / 1.4."""
    c = _case(block_m, 7, K, I, 300 + K, scales=(124, 130), ints=False, bias=torch.float32, gather=gather)
    c["bias"] = c["bias"] / 8                                                           # in [-1, 1]: it leaves h's spread alone
    M, t, bias = _M(), _dev(c), c["bias"].to(DEV)
    h0 = M.moe_gemm_mxfp4(*t, sorted_slot=c["ss"], top_k=c["topk"])[:int(c["off"][-1])].double()
    c["x"] = (c["x"].double() * (sd / float(h0.std()))).to(BF)
    t = _dev(c)
    kw = {} if alpha is None else dict(alpha=alpha, limit=limit)
    alpha, limit = float(np.float32(alpha or 1.702)), limit or 7.0
    g, u = _halves(M.moe_gemm_mxfp4(*t, bias=bias, sorted_slot=c["ss"], top_k=c["topk"]).double(), gate_up)
    assert float(torch.maximum(g.abs(), u.abs()).max()) <= 40
    hi_g, out_u = g[:int(c["off"][-1])] > limit, u[:int(c["off"][-1])].abs() > limit
    assert hi_g.double().mean() >= 0.05 and out_u.double().mean() >= 0.05 and (~hi_g & ~out_u).double().mean() >= 0.5
    gc = g.clamp(max=limit)
    want = ((u.clamp(-limit, limit) + 1) * (gc * torch.sigmoid(alpha * gc))).to(torch.float32).to(BF)
    err = (_ordered(_run(c, gate_up=gate_up, **kw)) - _ordered(want)).abs()
    print(f"swiglu_oai K {K} I {I} block_m {block_m} {gate_up}: {int((err == 1).sum())} of {err.numel()} one ulp off, max {int(err.max())}")
    assert int(err.max()) <= 1


def _strided_experts(t):                                          # a view of uint8 [E, ...] with 48 bytes of 0xFF between experts
    buf = torch.full((t.shape[0], t[0].numel() + 48), 0xFF, dtype=torch.uint8, device=DEV)
    return buf[:, :t[0].numel()].unflatten(1, t.shape[1:]).copy_(t)


@pytest.mark.parametrize("gate_up", ORDERS)
def test_isolation_graph_replay_and_opcheck(gate_up):
    c = _case(128, 7, 288, 136, 400, scales=(117, 137), ints=False, bias=BF)
    M, (x, blocks, scales, off), bias, end = _M(), _dev(c), c["bias"].to(DEV), int(c["off"][-1])
    bv, sv = _strided_experts(blocks), _strided_experts(scales)
    obuf, out = guard.slab((c["rows"], 136), BF, gaps=True, device=DEV, check_prep=False)
    snap = guard.snapshot(obuf)
    assert M.moe_gemm_mxfp4_glu(x, bv, sv, off, gate_up=gate_up, bias=bias, out=out) is out
    torch.cuda.synchronize()
    guard.assert_untouched(obuf, out, snap, "out")
    _same(out, _run(c, gate_up=gate_up), "strided out and expert-strided weights against contiguous ones")
    _same(out, _run(c, gate_up=gate_up), "two runs")
    assert (out[end:].view(torch.int16) == 0).all()                                 # the tail is +0; below: graph replay, opcheck
    c = _case(32, 7, 288, 40, 500, scales=(117, 137), ints=False, bias=torch.float32, gather=True)
    (x, blocks, scales, off), bias, ns = _dev(c), c["bias"].to(DEV), torch.ops.flash_attn_mi355
    args = (x, blocks, scales, off, "swiglu_oai", gate_up, 1.702, 7.0, bias, c["ss"], 2)
    tables = [(c["ss"].clone(), off.clone()), (c["ss"].flip(0).contiguous(), torch.from_numpy(G.offsets_of([9, 0, 50, 1, 64, 3, 2])).to(DEV))]
    eager = [ns.moe_gemm_mxfp4_glu(*args[:3], o, *args[4:9], ss, 2) for ss, o in tables]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ns.moe_gemm_mxfp4_glu(*args)
    for i in (1, 0, 1):
        c["ss"].copy_(tables[i][0]), off.copy_(tables[i][1])
        graph.replay()
        torch.cuda.synchronize()
        _same(res, eager[i], f"replay with tables {i}")
    torch.library.opcheck(ns.moe_gemm_mxfp4_glu, args)
    torch.library.opcheck(ns.moe_gemm_mxfp4_glu, args[:8] + (None, None, None))     # plain: 40 rows
