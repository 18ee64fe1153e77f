"""CPU: the host side of fa_moe_gemm_mxfp4_dgrad - exports, struct layout, the plan, the limits refused before any device work by
the C ABI and by the wrapper, the build list and the kernels' registers.  Nothing here needs a GPU."""
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


def test_exports_struct_and_build(lib):
    import build
    from flash_attn_mi355 import moe, torch_ops
    assert {"fa_moe_gemm_mxfp4_dgrad", "fa_moe_gemm_mxfp4_dgrad_params_size", "fa_moe_gemm_mxfp4_dgrad_plan"} <= set(lib.EXPORTS)
    fields = [f[0] for f in lib.FaMoeGemmMxfp4DgradParams._fields_]
    assert fields[0] == "struct_size" and fields[-1] == "reserved" and {"dy", "dx", "w_blocks_expert_stride", "w_scales_expert_stride"} <= set(fields)
    assert lib.lib.fa_moe_gemm_mxfp4_dgrad_params_size() == ctypes.sizeof(lib.FaMoeGemmMxfp4DgradParams) and lib.lib.fa_abi_version() == 4
    assert "fa_moe_gemm_mxfp4_dgrad.hip" in build.SOURCES
    for name in ("moe_gemm_mxfp4_dgrad", "moe_linear_mxfp4"):
        assert hasattr(torch_ops, name) and name not in torch_ops.__all__
    assert callable(moe.moe_linear_mxfp4) and callable(moe.moe_gemm_mxfp4_dgrad)
    res = json.load(open(os.path.join(os.path.dirname(lib.__file__), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if "moe_mxfp4_dgrad_kernel" in k}
    assert len(mine) == 2                                                    # block_m 32 / 128
    assert all(v["spill"] == 0 and v["scratch"] == 0 for v in mine.values()), mine
    count = lambda s: sum(s in k for k in res)                               # noqa: E731
    assert (count("moe_mxfp4_kernel"), count("moe_mxfp4_glu_kernel"), count("moe_gemm_kernel")) == (4, 8, 16)


@pytest.mark.parametrize("M,N,K,E", [(226, 136, 288, 7), (224, 136, 2880, 7), (225, 8, 32, 7), (1, 2880, 2880, 512), (0, 64, 64, 2),
                                     (16416, 32768, 32768, 512)])
def test_plan_is_the_kn_plan_with_the_roles_exchanged(lib, M, N, K, E):
    from flash_attn_mi355 import moe
    plan = moe.moe_gemm_mxfp4_dgrad_plan(M, N, K, E)
    assert plan == moe.moe_gemm_plan(M, K, N, E, w_layout="kn")
    assert plan == (32 if M <= 32 * E else 128, 128, 64, (M // plan[0] + E + 1 if M else 0), -(-K // 128))


@pytest.mark.parametrize("match,code,kw", [
    ("struct_size", "(-1)", dict(struct_size=8)), ("reserved", "(-1)", dict(reserved0=1)),
    (": n must", "(-2)", dict(n=12)), (": n must", "(-2)", dict(n=32776)), (": k must", "(-2)", dict(k=48)),
    (": k must", "(-2)", dict(k=32800)), ("num_experts", "(-2)", dict(num_experts=513)), ("num_experts", "(-2)", dict(num_experts=1)),
    ("dtype must be bf16", "(-2)", dict(dtype=0)), ("layout .* must be", "(-2)", dict(layout=1)),
    ("w_blocks_expert_stride", "(-2)", dict(w_blocks_expert_stride=32 * 32 - 16)), ("w_blocks_expert_stride", "(-2)", dict(w_blocks_expert_stride=32 * 32 + 8)),
    ("w_scales_expert_stride", "(-2)", dict(w_scales_expert_stride=63)), ("x_row_stride", "(-2)", dict(dy_row_stride=2 ** 22 + 8)),
    ("out_row_stride", "(-2)", dict(dx_row_stride=2 ** 22 + 8)), ("out rows must not overlap", "(-1)", dict(dx_row_stride=24)),
    ("overlaps w_scales", "(-1)", dict(dx=0x20000)), ("overlaps w_blocks", "(-1)", dict(dx=0x10000))])
def test_c_abi_rejects_before_any_device_work(lib, match, code, kw):
    """host pointers: every one of these returns before a launch (-1 / -2); the shared checks name dy as x and dx as out"""
    buf = (ctypes.c_char * (0x60000 + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaMoeGemmMxfp4DgradParams()
    s.struct_size = ctypes.sizeof(s)
    s.dy, s.w_blocks, s.w_scales, s.expert_offsets, s.dx = base, base + 0x10000, base + 0x20000, base + 0x30000, base + 0x40000
    s.dy_row_stride, s.dx_row_stride, s.w_blocks_expert_stride, s.w_scales_expert_stride = 32, 64, 32 * 32, 64
    s.rows, s.num_experts, s.n, s.k, s.dtype, s.layout = 16, 4, 32, 64, lib.FA_BF16, lib.FA_MOE_W_NK
    for k, v in kw.items():
        setattr(s, k, base + v if k == "dx" else v)
    with pytest.raises(RuntimeError, match=match) as e:
        lib.call_moe_gemm_mxfp4_dgrad(s, 0)
    assert code in str(e.value), str(e.value)


def test_wrapper_rejects_by_name_without_a_device(lib):
    from flash_attn_mi355 import moe
    bf, u8 = torch.bfloat16, torch.uint8
    dy, b, sc, off = torch.zeros(16, 32, dtype=bf), torch.zeros(4, 32, 32, dtype=u8), torch.zeros(4, 32, 2, dtype=u8), torch.zeros(5, dtype=torch.int32)

    def bad(match, *a, **kw):
        with pytest.raises(RuntimeError, match=match):
            moe.moe_gemm_mxfp4_dgrad(*a, **kw)
    bad("dy must be a bf16", dy.half(), b, sc, off)
    bad("with dy's N = 32 rows", dy, b[:, :24], sc[:, :24], off)
    bad("K must be a multiple of 32", dy, b[:, :, :24], sc, off)
    bad("w_scales must be uint8 of shape", dy, b, sc[:, :, :1], off)
    bad("N must be a multiple of 8", dy[:, :12], b[:, :12], sc[:, :12], off)
    bad("num_experts", dy, b[:1], sc[:1], off[:2])
    bad("w_blocks must be 16-byte aligned", dy, b.transpose(1, 2).contiguous().transpose(1, 2), sc, off)
    bad("expert_offsets must be int32 of shape", dy, b, sc, off[:4])
    bad("out must be", dy, b, sc, off, out=torch.zeros(16, 32, dtype=bf))
    z = lambda *shape: torch.zeros(*shape, dtype=u8)                         # noqa: E731
    bad(r"N must be a multiple of 8 in \[8, 32768\], got 32776", torch.zeros(2, 32776, dtype=bf), z(2, 32776, 16), z(2, 32776, 1), off[:3])
    bad(r"K must be a multiple of 32 in \[32, 32768\], got 32800", dy[:, :8], z(2, 8, 16400), z(2, 8, 1025), off[:3])
    bad("dy must be 16-byte aligned", torch.zeros(16, 40, dtype=bf)[:, 4:36], b, sc, off)
    bad("dy requires grad, and moe_gemm_mxfp4_dgrad has no autograd", dy.clone().requires_grad_(), b, sc, off)
    bad("no CPU fallback", dy, b.view(4, 32, 2, 16), sc, off)                # the [E, N, K / 32, 16] form passes the checks
    with pytest.raises(RuntimeError, match="pos goes with sorted_slot"):
        moe.moe_linear_mxfp4(torch.zeros(16, 64, dtype=bf), b, sc, off, pos=torch.zeros(16, 1, dtype=torch.int32))
