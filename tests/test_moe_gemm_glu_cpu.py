"""CPU: the host side of fa_moe_gemm_glu - the plan, the C ABI's and the wrapper's argument errors, the fake implementations of
the two torch ops - and the bound its GPU test holds it to against the plain fp64 definition act(g) * u (`glu_share`, shared
with tests/test_moe_gemm_glu_gpu.py), shown here on an fp32 emulation of the op's contract.  Nothing here needs a GPU.

The bound.  With g, u the exact sums, g', u' the rounded 16-bit values the kernel forms (|g' - g| <= Bg, |u' - u| <= Bu:
moe_gemm_ref.bound, which includes the rounding) and L the activation's Lipschitz constant:
    |act(g') u' - act(g) u| <= |act(g') - act(g)| |u'| + |act(g)| |u' - u| <= L Bg (|u| + Bu) + |act(g)| Bu
and the epilogue's own fp32 arithmetic and final rounding add act_mul_ref.bound.  L = sup |act'|: 1 for relu; silu' peaks at
1.0998 (g = 2.3994), gelu' at 1.1289 (g = 1.4142) and gelu_tanh' at 1.1290: 1.10, 1.13, 1.13.  relu2's slope is unbounded: it
is left to the bit-for-bit tests."""
import ctypes

import numpy as np
import pytest
import torch

import act_mul_ref as A
import moe_gemm_ref as G
import moe_ref as R

LIPSCHITZ = {"relu": 1.0, "silu": 1.10, "gelu": 1.13, "gelu_tanh": 1.13}


def glu_share(got, x, w, off, bias, activation, layout, dtype):
    """max |got - act(g) u| / bound over the elements, g and u the fp64 sums of the 16-bit inputs without any rounding"""
    nm = str(dtype).replace("torch.", "")
    ref, mag = G.gemm_ref(R.widen(x), R.widen(w), off, layout=layout, bias=None if bias is None else R.widen(bias), with_mag=True)
    B = G.bound(ref, mag, x.shape[1], nm, bias is not None)[0]
    I = ref.shape[1] // 2
    g, u, Bg, Bu = (torch.from_numpy(np.ascontiguousarray(t)) for t in (ref[:, :I], ref[:, I:], B[:, :I], B[:, I:]))
    out, D = A.forward_ref(g, u, activation)
    bnd = LIPSCHITZ[activation] * Bg * (u.abs() + Bu) + A.act_ref(g, activation)[0].abs() * Bu + A.bound(out, D, dtype)
    return float(((got.detach().double().cpu() - out).abs() / bnd).max())


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


def test_plan_values(lib):
    from flash_attn_mi355 import moe
    assert lib.lib.fa_moe_gemm_glu_params_size() == ctypes.sizeof(lib.FaMoeGemmGluParams) and lib.lib.fa_abi_version() == 4
    for M, I, E in ((226, 136, 7), (224, 136, 7), (225, 8, 7), (80, 72, 7), (1, 2880, 512), (0, 64, 2), (16416, 32768, 512)):
        for layout in ("nk", "kn"):
            bm, bn, bk, grid_m, grid_n = moe.moe_gemm_glu_plan(M, I, 264, E, w_layout=layout, dtype=torch.float16)
            assert bm == (32 if M <= 32 * E else 128) == moe.moe_gemm_plan(M, 2 * I, 264, E)[0]
            assert (bn, bk) == (64, 64) and grid_n == -(-I // 64) and grid_m == (M // bm + E + 1 if M else 0)
    for bad in (dict(I=12), dict(I=32776), dict(E=1), dict(K=12)):
        a = dict(dict(I=64, K=64, E=4), **bad)
        with pytest.raises(RuntimeError, match=r"\(-2\)"):
            moe.moe_gemm_glu_plan(64, a["I"], a["K"], a["E"])
    with pytest.raises(RuntimeError, match="w_layout"):
        moe.moe_gemm_glu_plan(64, 64, 64, 4, w_layout="xx")


@pytest.mark.parametrize("match,code,kw", [
    ("struct_size", "(-1)", dict(struct_size=8)), ("unknown activation", "(-1)", dict(activation=5)),
    ("unknown activation", "(-1)", dict(activation=-1)), ("reserved", "(-1)", dict(reserved0=1)), ("reserved", "(-1)", dict(reserved1=1)),
    (": n must", "(-2)", dict(n=12)), (": n must", "(-2)", dict(n=32776, w_expert_stride=2 * 32776 * 64)),
    ("w_expert_stride", "(-2)", dict(w_expert_stride=64 * 32)), ("out rows must not overlap", "(-1)", dict(out_row_stride=24)),
    ("num_experts", "(-2)", dict(num_experts=513)), ("overlaps", "(-1)", dict(out=0x10000))])
def test_c_abi_rejects_before_any_device_work(lib, match, code, kw):
    """host pointers: every one of these returns before a launch (FA_ERR_INVALID_ARGUMENT -1, FA_ERR_UNSUPPORTED -2)"""
    buf = (ctypes.c_char * (0x60000 + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaMoeGemmGluParams()
    s.struct_size = ctypes.sizeof(s)
    s.x, s.w, s.expert_offsets, s.out = base, base + 0x10000, base + 0x30000, base + 0x40000
    s.x_row_stride, s.out_row_stride, s.w_expert_stride = 64, 32, 2 * 64 * 32
    s.rows, s.num_experts, s.n, s.k, s.dtype, s.layout, s.activation = 16, 4, 32, 64, lib.FA_BF16, lib.FA_MOE_W_NK, lib.FA_ACT_GELU
    for k, v in kw.items():
        setattr(s, k, base + v if k == "out" else v)
    with pytest.raises(RuntimeError, match=match) as e:
        lib.call_moe_gemm_glu(s, 0)
    assert code in str(e.value), str(e.value)


def test_wrapper_rejects_by_name_without_a_device(lib):
    from flash_attn_mi355 import moe
    bf = torch.bfloat16
    x, w, off = torch.zeros(16, 64, dtype=bf), torch.zeros(4, 64, 64, dtype=bf), torch.zeros(5, dtype=torch.int32)

    def bad(match, *a, fn=moe.moe_gemm_glu, **kw):
        with pytest.raises(RuntimeError, match=match):
            fn(*a, **kw)
    bad("activation must be one of", x, w, off, activation="swish")
    bad("multiple of 16", x, w[:, :24], off)                                 # I = 12: an odd count of 8-column pieces
    bad("2 I must be a multiple of 8", x[:, :8], torch.zeros(2, 65552, 8, dtype=bf), off[:3])
    bad("does not contract", x, w[:, :, :32], off)
    bad("bias must be", x, w, off, bias=torch.zeros(4, 32, dtype=bf))       # the bias is [E, 2 I]
    bad("out must be", x, w, off, out=torch.zeros(16, 64, dtype=bf))        # out is [M, I]
    bad("w requires grad, and moe_gemm_glu has no autograd", x, w.clone().requires_grad_(), off)
    bad("no CPU fallback", x, w, off, bias=torch.zeros(4, 64), out=torch.zeros(16, 32, dtype=bf))
    bad("activation must be one of", x, w, off, activation="swish", fn=moe.moe_glu_linear)
    bad("pos goes with sorted_slot", x, w, off, pos=torch.zeros(16, 1, dtype=torch.int32), fn=moe.moe_glu_linear)


def test_fake_implementations(lib):
    import flash_attn_mi355.torch_ops  # noqa: F401
    ns = torch.ops.flash_attn_mi355
    assert not ns.moe_gemm_glu.default._schema.is_mutable and not ns.moe_glu_linear.default._schema.is_mutable
    bf = torch.bfloat16
    x, off = torch.empty(5, 64, dtype=bf, device="meta"), torch.empty(9, dtype=torch.int32, device="meta")
    nk, kn = torch.empty(8, 48, 64, dtype=bf, device="meta"), torch.empty(8, 64, 48, dtype=bf, device="meta")
    ss = torch.empty(70, dtype=torch.int32, device="meta")
    for out in (ns.moe_gemm_glu(x, nk, off, "silu", "nk", None, None, None), ns.moe_glu_linear(x, kn, off, "relu", "kn", None, None, None, None)):
        assert out.shape == (5, 24) and out.stride() == (24, 1) and out.dtype == bf
    for out in (ns.moe_gemm_glu(x, kn, off, "gelu", "kn", None, ss, 2), ns.moe_glu_linear(x, nk, off, "silu", "nk", None, ss, 2, None)):
        assert out.shape == (70, 24) and out.stride() == (24, 1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
@pytest.mark.parametrize("activation", sorted(LIPSCHITZ))
def test_an_fp32_emulation_of_the_contract_stays_inside_the_bound(activation, dtype):
    """torch fp32 matmul, + bias, round, the activation in fp32, one multiply, round: a correct implementation's share is <= 1"""
    K, I, layout = 264, 136, "nk"
    off = G.offsets_of(G.PATTERN)
    E, rows = len(G.PATTERN), int(off[-1])
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(rows, K, generator=gen).to(dtype)
    w = (torch.randn(E, 2 * I, K, generator=gen) / K ** 0.5).to(dtype)
    bias = torch.randn(E, 2 * I, generator=gen)
    h = torch.zeros(rows, 2 * I, dtype=dtype)
    for e in range(E):
        h[off[e]:off[e + 1]] = (x[off[e]:off[e + 1]].float() @ w[e].float().t() + bias[e]).to(dtype)
    g, u = h[:, :I].float(), h[:, I:].float()
    act = {"relu": torch.relu, "silu": torch.nn.functional.silu, "gelu": torch.nn.functional.gelu,
           "gelu_tanh": lambda t: torch.nn.functional.gelu(t, approximate="tanh")}[activation]
    share = glu_share((act(g) * u).to(dtype), x, w, off, bias, activation, layout, dtype)
    print(f"share moe_gemm_glu emulation {activation} {dtype}: {share:.3f}")
    assert share <= 1.0
