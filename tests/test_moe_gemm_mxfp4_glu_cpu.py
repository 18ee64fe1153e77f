"""CPU: the host side of fa_moe_gemm_mxfp4_glu - exports, struct, plan, refused arguments, the new kernels' registers.  No GPU."""
import ctypes
import json
import os

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


def test_exports_struct_and_kernels(lib):
    assert {"fa_moe_gemm_mxfp4_glu", "fa_moe_gemm_mxfp4_glu_params_size", "fa_moe_gemm_mxfp4_glu_plan"} <= set(lib.EXPORTS)
    assert {"activation", "gate_up", "alpha", "limit"} <= {f[0] for f in lib.FaMoeGemmMxfp4GluParams._fields_}
    assert lib.lib.fa_moe_gemm_mxfp4_glu_params_size() == ctypes.sizeof(lib.FaMoeGemmMxfp4GluParams) and lib.lib.fa_abi_version() == 4
    res = json.load(open(os.path.join(os.path.dirname(lib.__file__), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if "moe_mxfp4_glu_kernel" in k}
    assert len(mine) == 8                                                    # block_m 32 / 128 x plain / gather x interleaved / packed
    assert all(v["spill"] == 0 and v["scratch"] == 0 and v["vgpr"] <= 256 for v in mine.values()), mine


@pytest.mark.parametrize("M,I,E", [(226, 136, 7), (224, 136, 7), (225, 8, 7), (1, 2880, 512), (0, 64, 2), (16416, 32768, 512)])
def test_plan_values(lib, M, I, E):
    from flash_attn_mi355 import moe
    bm, bn, bk, grid_m, grid_n = moe.moe_gemm_mxfp4_glu_plan(M, I, 2880, E)
    assert (bm, bk) == moe.moe_gemm_mxfp4_plan(M, 2 * I, 2880, E)[0:3:2] and bm == (32 if M <= 32 * E else 128)
    assert bn == 64 and grid_n == -(-I // 64) and grid_m == (M // bm + E + 1 if M else 0)


@pytest.mark.parametrize("match,code,kw", [
    ("struct_size", "(-1)", dict(struct_size=8)), ("reserved", "(-1)", dict(reserved0=1)),
    (": n must", "(-2)", dict(n=12)), (": n must", "(-2)", dict(n=32776)), (": k must", "(-2)", dict(k=48)),
    ("unknown activation", "(-1)", dict(activation=1)), ("unknown activation", "(-1)", dict(activation=6)),
    ("unknown gate_up", "(-1)", dict(gate_up=2)), ("limit must be positive", "(-1)", dict(limit=0.0)),
    ("limit must be positive", "(-1)", dict(limit=-7.0)), ("limit must be positive", "(-1)", dict(limit=float("nan"))),
    ("alpha must be finite", "(-1)", dict(alpha=float("inf"))), ("alpha must be finite", "(-1)", dict(alpha=float("nan"))),
    ("dtype must be bf16", "(-2)", dict(dtype=0)), ("layout must be", "(-2)", dict(layout=1)),
    ("w_blocks_expert_stride", "(-2)", dict(w_blocks_expert_stride=32 * 32 - 16)),
    ("out rows must not overlap", "(-1)", dict(out_row_stride=8)), ("overlaps w_scales", "(-1)", dict(out=0x20000))])
def test_c_abi_rejects_before_any_device_work(lib, match, code, kw):
    """host pointers: every one returns before a launch (-1 invalid argument, -2 unsupported); 2 n = 32 weight rows of k = 64"""
    buf = (ctypes.c_char * (0x60000 + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaMoeGemmMxfp4GluParams()
    s.struct_size = ctypes.sizeof(s)
    s.x, s.w_blocks, s.w_scales, s.expert_offsets, s.out = base, base + 0x10000, base + 0x20000, base + 0x30000, base + 0x40000
    s.x_row_stride, s.out_row_stride, s.w_blocks_expert_stride, s.w_scales_expert_stride = 64, 16, 32 * 32, 64
    s.rows, s.num_experts, s.n, s.k, s.dtype, s.layout = 16, 4, 16, 64, lib.FA_BF16, lib.FA_MOE_W_NK
    s.activation, s.gate_up, s.alpha, s.limit = lib.FA_ACT_SWIGLU_OAI, lib.FA_MOE_GLU_INTERLEAVED, 1.702, 7.0
    for k, v in kw.items():
        setattr(s, k, base + v if k == "out" else v)
    with pytest.raises(RuntimeError, match=match) as e:
        lib.call_moe_gemm_mxfp4_glu(s, 0)
    assert code in str(e.value), str(e.value)


def test_wrapper_rejects_by_name_without_a_device(lib):
    from flash_attn_mi355 import act_mul, moe
    bf, u8 = torch.bfloat16, torch.uint8
    x, b, sc, off = torch.zeros(16, 64, dtype=bf), torch.zeros(4, 32, 32, dtype=u8), torch.zeros(4, 32, 2, dtype=u8), torch.zeros(5, dtype=torch.int32)

    def bad(match, *a, **kw):
        with pytest.raises(RuntimeError, match=match):
            moe.moe_gemm_mxfp4_glu(*a, **kw)
    bad("activation must be one of", x, b, sc, off, activation="gelu")
    bad("gate_up must be one of", x, b, sc, off, gate_up="split")
    bad("alpha must be finite and limit positive", x, b, sc, off, limit=float("nan"))
    bad("x must be a bf16", x.half(), b, sc, off)
    bad("rows must be a multiple of 16, got 17", x, torch.zeros(4, 17, 32, dtype=u8), torch.zeros(4, 17, 2, dtype=u8), off)
    bad(r"bias must be torch.bfloat16 or fp32 of shape \(4, 32\)", x, b, sc, off, bias=torch.zeros(4, 16, dtype=bf))
    bad(r"out must be torch.bfloat16 of shape \(16, 16\)", x, b, sc, off, out=torch.zeros(16, 32, dtype=bf))
    bad("x requires grad, and moe_gemm_mxfp4_glu has no autograd", x.clone().requires_grad_(), b, sc, off)
    bad("no CPU fallback", x, b.view(4, 32, 2, 16), sc, off, activation="silu", limit=-1.0)   # silu ignores limit; all checks pass
    assert "swiglu_oai" not in act_mul.ACTIVATIONS and lib.FA_ACT_SWIGLU_OAI not in act_mul.ACTIVATIONS.values()
    with pytest.raises(RuntimeError, match="activation must be one of"):
        moe.moe_gemm_glu(x, torch.zeros(4, 32, 64, dtype=bf), off, activation="swiglu_oai")
