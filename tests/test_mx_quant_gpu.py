"""GPU: fa_mx_quant / fa_mx_dequant (csrc/fa_mx_quant.hip) bit for bit against tests/mx_quant_ref.py.

_blocks is a fixed table of 32-element blocks, values times 2^s: every tie point with its two neighbours in the dtype beside an
amax of 6; an amax of exactly 1.5 2^e and its two neighbours (the "rceil" edge); values in (6, 8); zeros of both signs; blocks around
2^-126 (the clamp at 2) and below 2^-14 (fp16 subnormals); bf16's largest value; one NaN; one inf.  Block j of row r is entry
3 r + j, so the NaN blocks have finite neighbours; every fourth row is N(0, 1) times a power of two."""
import numpy as np
import pytest
import torch

import guard
import mx_quant_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
SHAPES = [(32, 8), (96, 40), (288, 264)]                   # K, N: one block / 3 scale bytes a row / tails of both "kn" tile sides


def _Q():
    from flash_attn_mi355 import quant
    import flash_attn_mi355.torch_ops  # noqa: F401
    return quant


def _blocks(dtype):
    """the table as a float64 array [B, 32] of values exact in `dtype`"""
    t = torch.tensor(TIES, dtype=dtype)
    near = torch.stack([t, (t.view(torch.int16) - 1).view(dtype), (t.view(torch.int16) + 1).view(dtype)]).double().flatten().tolist()
    ties = near + [6.0] + [0.0] * 10
    edge = lambda a: [a] + [a * f / 32 * (-1) ** f for f in range(31)]        # a is the block's amax
    one5 = torch.tensor([1.5], dtype=dtype).view(torch.int16)
    rows = [[v * 2.0 ** s * (-1) ** i for i, v in enumerate(ties)] for s in (-3, 0, 5)]
    rows += [edge(float((one5 + d).view(dtype)) * 2.0 ** s) for d in (-1, 0, 1) for s in (-9, 2)]
    rows += [[(6.0 + 2 * i / 32) * 2.0 ** s * (-1) ** i for i in range(32)] for s in (-1, 4)]
    rows += [[0.0, -0.0] * 16]
    rows += [[2.0 ** -126 * f / 8 * (-1) ** f for f in range(32)], [2.0 ** -126 * f / 64 for f in range(32)]]
    rows += [[2.0 ** -24 * f * (-1) ** f for f in range(32)], [2.0 ** -24 * (f % 3) for f in range(32)]]      # fp16 subnormals
    rows += [[3.3895313892515355e38 * f / 31 for f in range(32)]]
    rows += [[1.0] * 7 + [float("nan")] + [-2.0] * 24, [3.0] * 30 + [float("-inf"), 0.5]]
    return torch.tensor(rows, dtype=torch.float64).to(dtype).double().numpy()


def _weights(E, N, K, dtype):
    """[E, N, K] of `dtype` on the device, "nk\""""
    tab = _blocks(dtype)
    r = np.arange(E * N)[:, None]
    w = tab[(3 * r + np.arange(K // 32)) % len(tab)].reshape(E * N, K)
    g = np.random.default_rng(N + K)
    w[3::4] = g.standard_normal(w[3::4].shape) * 2.0 ** (r[3::4] % 7 - 3)
    return torch.from_numpy(w.reshape(E, N, K)).to(dtype).to(DEV)


def _strided(t, pad=48):
    """(buf, view): `t` [E, ...] as a view whose experts lie `pad` elements further apart than they need, between 0xA5 bands"""
    E, n = t.shape[0], t[0].numel()
    buf = torch.full(((64 + E * (n + pad)) * t.element_size(),), guard.WS_SENTINEL, dtype=torch.uint8, device=DEV).view(t.dtype)
    view = buf[64:].as_strided(t.shape, (n + pad,) + tuple(t[0].stride()))
    view.copy_(t)
    return buf, view


def _eq(got, want, name):
    assert got.shape == want.shape and got.dtype == want.dtype, name
    a, b = guard.bits(got.contiguous()), guard.bits(want.contiguous())
    assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} elements differ"


def _want(w, rule):
    b, s = R.quant(w.double().cpu().numpy(), rule)
    return torch.from_numpy(b).to(DEV), torch.from_numpy(s).to(DEV)


@pytest.mark.parametrize("N", [8, 40, 264])
@pytest.mark.parametrize("K", [32, 96, 288])
@pytest.mark.parametrize("rule", ["floor", "rceil"])
@pytest.mark.parametrize("dtype", [BF, torch.float16])
@pytest.mark.parametrize("layout", ["nk", "kn"])
def test_quant_bit_for_bit(layout, dtype, rule, K, N):
    E = 1 if (K // 96 + N // 40 + (rule == "rceil") + (layout == "kn") + (dtype is BF)) % 2 else 3   # 2-D | an expert-strided view
    w = _weights(E, N, K, dtype)
    arg = w if layout == "nk" else w.transpose(1, 2).contiguous()
    arg = arg[0] if E == 1 else _strided(arg)[1]
    blocks, scales = _Q().quant_mxfp4(arg, w_layout=layout, scale_rule=rule)
    wb, ws = _want(w, rule)
    _eq(scales, ws[0] if E == 1 else ws, f"scales {layout} {dtype} {rule} K {K} N {N}")
    _eq(blocks, wb[0] if E == 1 else wb, f"blocks {layout} {dtype} {rule} K {K} N {N}")


@pytest.mark.parametrize("K,N", SHAPES + [(2880, 72)])
def test_kn_equals_nk_of_the_transposed_weights(K, N):
    w = _weights(2, N, K, BF)
    for got, want in zip(_Q().quant_mxfp4(w.transpose(1, 2).contiguous(), w_layout="kn"), _Q().quant_mxfp4(w)):
        _eq(got, want, f"K {K} N {N}")


def _codes(E, N, K, bytes_):
    """every code beside every one of `bytes_`: (blocks [E, N, K / 2], scales [E, N, K / 32]) as numpy"""
    n, j = np.arange(E * N)[:, None], np.arange(K // 2)
    blocks = ((j + n) % 16 | ((j * 7 + n + 3) % 16) << 4).astype(np.uint8).reshape(E, N, K // 2)
    scales = np.array(bytes_, dtype=np.uint8)[(n + np.arange(K // 32)) % len(bytes_)].reshape(E, N, K // 32)
    return blocks, scales


@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("layout", ["nk", "kn"])
def test_dequant_bit_for_bit(layout, K, N):
    """all 16 codes under the bytes of the contract's edges, 255 (NaN) and the four bytes outside the contract"""
    blocks, scales = _codes(2, N, K, [2, 126, 127, 128, 252, 255, 0, 1, 253, 254])
    want = torch.from_numpy(R.dequant(blocks, scales)).to(BF).to(DEV)
    got = _Q().dequant_mxfp4(_strided(torch.from_numpy(blocks).to(DEV))[1], _strided(torch.from_numpy(scales).to(DEV), 5)[1], w_layout=layout)
    want = torch.where(want.isnan(), torch.tensor([0x7FC0], dtype=torch.int16, device=DEV).view(BF), want)   # the NaN the header names
    _eq(got, want if layout == "nk" else want.transpose(1, 2), f"{layout} K {K} N {N}")


@pytest.mark.parametrize("rule", ["floor", "rceil"])
@pytest.mark.parametrize("layout", ["nk", "kn"])
def test_round_trip(layout, rule):
    """blocks whose largest magnitude is 4 or 6 are fixed points of quant(dequant(.)) under both rules"""
    blocks, scales = _codes(2, 40, 96, list(range(100, 150)))
    codes = np.stack([blocks & 15, blocks >> 4], -1).reshape(2, 40, 3, 32)
    four = (np.arange(2 * 40 * 3).reshape(2, 40, 3) % 2 == 0)[..., None]              # these blocks: no 6, and a 4 in front
    codes = np.where(four & (codes % 8 == 7), codes - 2, codes)
    codes[..., 0] = np.where(four[..., 0], 6, 15)
    codes = codes.reshape(2, 40, 96)
    b = torch.from_numpy((codes[..., 0::2] | codes[..., 1::2] << 4).astype(np.uint8)).to(DEV)
    s = torch.from_numpy(scales).to(DEV)
    b2, s2 = _Q().quant_mxfp4(_Q().dequant_mxfp4(b, s, w_layout=layout), w_layout=layout, scale_rule=rule)
    _eq(s2, s, "scales")
    _eq(b2, b, "blocks")


@pytest.mark.parametrize("rows", [40, 200])                    # block_m 32 and 128
def test_the_gemm_reads_what_the_quantiser_writes(rows):
    from flash_attn_mi355 import moe
    g = torch.Generator(device=DEV).manual_seed(rows)
    w = torch.randn(2, 40, 96, device=DEV, dtype=BF, generator=g)
    x = torch.randn(rows, 96, device=DEV, dtype=BF, generator=g)
    off = torch.tensor([0, rows // 2 - 3, rows], dtype=torch.int32, device=DEV)
    assert moe.moe_gemm_mxfp4_plan(rows, 40, 96, 2)[0] == (32 if rows == 40 else 128)
    b, s = _Q().quant_mxfp4(w)
    _eq(moe.moe_gemm_mxfp4(x, b, s, off), moe.moe_gemm(x, _Q().dequant_mxfp4(b, s), off), f"rows {rows}")


@pytest.mark.parametrize("layout", ["nk", "kn"])
def test_outputs_stay_in_place(layout):
    """strided out views between guard bands; a captured graph replayed after w was rewritten; opcheck"""
    Q, ns = _Q(), torch.ops.flash_attn_mi355
    w = [_weights(3, 40, 96, BF), _weights(3, 40, 96, BF).flip(1).contiguous()]
    if layout == "kn":
        w = [t.transpose(1, 2).contiguous() for t in w]
    want = [Q.quant_mxfp4(t, w_layout=layout) for t in w]
    (bbuf, bv), (sbuf, sv) = _strided(torch.zeros_like(want[0][0])), _strided(torch.zeros_like(want[0][1]), 5)
    obuf, ov = _strided(torch.zeros_like(w[0]), 8)
    snaps = [guard.snapshot(t) for t in (bbuf, sbuf, obuf)]
    assert Q.quant_mxfp4(w[0], w_layout=layout, out=(bv, sv))[0] is bv and Q.dequant_mxfp4(bv, sv, w_layout=layout, out=ov) is ov
    torch.cuda.synchronize()
    for buf, view, snap, name in zip((bbuf, sbuf, obuf), (bv, sv, ov), snaps, ("blocks", "scales", "out")):
        guard.assert_untouched(buf, view, snap, name)
    _eq(bv, want[0][0], "blocks into a view")
    _eq(sv, want[0][1], "scales into a view")
    _eq(ov, Q.dequant_mxfp4(*want[0], w_layout=layout), "out into a view")
    src = w[0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b, s = ns.quant_mxfp4(src, layout, "floor")
        o = ns.dequant_mxfp4(b, s, layout)
    for i in (1, 0, 1):
        src.copy_(w[i])
        graph.replay()
        torch.cuda.synchronize()
        _eq(b, want[i][0], f"replay {i}: blocks")
        _eq(s, want[i][1], f"replay {i}: scales")
        _eq(o, Q.dequant_mxfp4(*want[i], w_layout=layout), f"replay {i}: out")
    torch.library.opcheck(ns.quant_mxfp4, (w[0], layout, "rceil"))
    finite = [torch.from_numpy(t).to(DEV) for t in _codes(3, 40, 96, [2, 127, 252])]        # (opcheck compares values: no NaN block)
    torch.library.opcheck(ns.dequant_mxfp4, (*finite, layout))
