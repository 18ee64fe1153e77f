"""CPU: the host side of fa_moe_gemm_mxfp4 - exports, struct layout, the plan, the limits refused before any device work by the
C ABI and by the wrapper, the build list and the kernels' registers.  Nothing here needs a GPU."""
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
    from flash_attn_mi355 import moe
    assert {"fa_moe_gemm_mxfp4", "fa_moe_gemm_mxfp4_params_size", "fa_moe_gemm_mxfp4_plan"} <= set(lib.EXPORTS)
    fields = [f[0] for f in lib.FaMoeGemmMxfp4Params._fields_]
    assert fields[0] == "struct_size" and fields[-1] == "reserved" and {"w_blocks_expert_stride", "w_scales_expert_stride"} <= set(fields)
    assert lib.lib.fa_moe_gemm_mxfp4_params_size() == ctypes.sizeof(lib.FaMoeGemmMxfp4Params) and lib.lib.fa_abi_version() == 4
    assert "fa_moe_gemm_mxfp4.hip" in build.SOURCES
    assert not hasattr(moe, "__all__") or "moe_gemm_mxfp4" not in moe.__all__
    res = json.load(open(os.path.join(os.path.dirname(lib.__file__), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if "moe_mxfp4_kernel" in k}
    assert len(mine) == 4                                                    # block_m 32 / 128 x plain / gather
    assert all(v["spill"] == 0 and v["scratch"] == 0 for v in mine.values()), mine
    assert sum("moe_gemm_kernel" in k for k in res) == 16                    # fa_moe_gemm's kernels keep their names


@pytest.mark.parametrize("M,N,E", [(226, 136, 7), (224, 136, 7), (225, 8, 7), (1, 2880, 512), (0, 64, 2), (16416, 65536, 512)])
def test_plan_values(lib, M, N, E):
    from flash_attn_mi355 import moe
    bm, bn, bk, grid_m, grid_n = moe.moe_gemm_mxfp4_plan(M, N, 2880, E)
    assert bm == (32 if M <= 32 * E else 128) == moe.moe_gemm_plan(M, N, 2880, E)[0]
    assert (bn, bk) == (128, 256 if bm == 32 else 128) and grid_n == -(-N // 128) and grid_m == (M // bm + E + 1 if M else 0)


@pytest.mark.parametrize("kw", [dict(N=12), dict(N=65544), dict(E=1), dict(E=513), dict(K=48), dict(K=0), dict(K=32800),
                                dict(layout=1), dict(dtype=0)])
def test_plan_refuses_outside_the_limits(lib, kw):
    a = dict(dict(N=64, K=64, E=4, layout=lib.FA_MOE_W_NK, dtype=lib.FA_BF16), **kw)
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        lib.moe_gemm_plan(64, a["N"], a["K"], a["E"], a["layout"], a["dtype"], entry="fa_moe_gemm_mxfp4_plan")


@pytest.mark.parametrize("match,code,kw", [
    ("struct_size", "(-1)", dict(struct_size=8)), ("reserved", "(-1)", dict(reserved0=1)),
    (": n must", "(-2)", dict(n=12)), (": n must", "(-2)", dict(n=65544)), (": k must", "(-2)", dict(k=48)),
    (": k must", "(-2)", dict(k=32800)), ("num_experts", "(-2)", dict(num_experts=513)), ("num_experts", "(-2)", dict(num_experts=1)),
    ("dtype must be bf16", "(-2)", dict(dtype=0)), ("layout must be", "(-2)", dict(layout=1)),
    ("w_blocks_expert_stride", "(-2)", dict(w_blocks_expert_stride=32 * 32 - 16)), ("w_blocks_expert_stride", "(-2)", dict(w_blocks_expert_stride=32 * 32 + 8)),
    ("w_scales_expert_stride", "(-2)", dict(w_scales_expert_stride=63)), ("x_row_stride", "(-2)", dict(x_row_stride=2 ** 22 + 8)),
    ("out_row_stride", "(-2)", dict(out_row_stride=2 ** 22 + 8)), ("out rows must not overlap", "(-1)", dict(out_row_stride=24)),
    ("overlaps w_scales", "(-1)", dict(out=0x20000)), ("overlaps w_blocks", "(-1)", dict(out=0x10000))])
def test_c_abi_rejects_before_any_device_work(lib, match, code, kw):
    """host pointers: every one of these returns before a launch (FA_ERR_INVALID_ARGUMENT -1, FA_ERR_UNSUPPORTED -2)"""
    buf = (ctypes.c_char * (0x60000 + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaMoeGemmMxfp4Params()
    s.struct_size = ctypes.sizeof(s)
    s.x, s.w_blocks, s.w_scales, s.expert_offsets, s.out = base, base + 0x10000, base + 0x20000, base + 0x30000, base + 0x40000
    s.x_row_stride, s.out_row_stride, s.w_blocks_expert_stride, s.w_scales_expert_stride = 64, 32, 32 * 32, 64
    s.rows, s.num_experts, s.n, s.k, s.dtype, s.layout = 16, 4, 32, 64, lib.FA_BF16, lib.FA_MOE_W_NK
    for k, v in kw.items():
        setattr(s, k, base + v if k == "out" else v)
    with pytest.raises(RuntimeError, match=match) as e:
        lib.call_moe_gemm_mxfp4(s, 0)
    assert code in str(e.value), str(e.value)


def test_wrapper_rejects_by_name_without_a_device(lib):
    from flash_attn_mi355 import moe
    bf, u8 = torch.bfloat16, torch.uint8
    x, b, sc, off = torch.zeros(16, 64, dtype=bf), torch.zeros(4, 32, 32, dtype=u8), torch.zeros(4, 32, 2, dtype=u8), torch.zeros(5, dtype=torch.int32)

    def bad(match, *a, **kw):
        with pytest.raises(RuntimeError, match=match):
            moe.moe_gemm_mxfp4(*a, **kw)
    bad("x must be a bf16", x.half(), b, sc, off)
    bad("K must be a multiple of 32", x[:, :48], b[:, :, :24], sc, off)
    bad("w_blocks must be a uint8", x, b.to(torch.int8), sc, off)
    bad("does not contract", x, b[:, :, :16], sc, off)
    bad("w_scales must be uint8 of shape", x, b, sc[:, :, :1], off)
    bad("N must be a multiple of 8", x, b[:, :12], sc[:, :12], off)
    bad("num_experts", x, b[:1], sc[:1], off[:2])
    bad("w_blocks must be 16-byte aligned", x, b.transpose(1, 2).contiguous().transpose(1, 2), sc, off)
    bad("w_scales must have contiguous experts", x, b, sc.transpose(1, 2).contiguous().transpose(1, 2), off)
    bad("bias must be", x, b, sc, off, bias=torch.zeros(4, 16, dtype=bf))
    bad("out must be", x, b, sc, off, out=torch.zeros(16, 64, dtype=bf))
    bad("sorted_slot and top_k go together", x, b, sc, off, top_k=2)
    # the upper limits, by name
    z = lambda *shape: torch.zeros(*shape, dtype=u8)                         # noqa: E731
    bad(r"num_experts \(w_blocks.shape\[0\]\) must be in \[2, 512\], got 513", x[:, :32], z(513, 8, 16), z(513, 8, 1), torch.zeros(514, dtype=torch.int32))
    bad(r"N must be a multiple of 8 in \[8, 65536\], got 65544", x[:, :32], z(2, 65544, 16), z(2, 65544, 1), off[:3])
    bad(r"K must be a multiple of 32 in \[32, 32768\], got 32800", torch.zeros(16, 32800, dtype=bf), z(2, 8, 16400), z(2, 8, 1025), off[:3])
    far = torch.zeros(2 ** 22 + 8 + 64, dtype=bf)                            # two rows 2^22 + 8 elements apart
    bad(r"x must be 16-byte aligned with a row stride .* at most 2\^22", far.as_strided((2, 64), (2 ** 22 + 8, 1)), b, sc, off)
    bad(r"out must be 16-byte aligned with a row stride .* at most 2\^22", x[:2], b, sc, off, out=far.as_strided((2, 32), (2 ** 22 + 8, 1)))
    bad("x must be 16-byte aligned", torch.zeros(16, 72, dtype=bf)[:, 4:68], b, sc, off)
    for k in (0, 17):
        bad(rf"k must be in \[1, 16\], got {k}", x, b, sc, off, sorted_slot=torch.zeros(16, dtype=torch.int32), top_k=k)
    bad(r"tokens x k must stay below 2\^31", x.as_strided((2 ** 28, 64), (0, 1)), b, sc, off, sorted_slot=torch.zeros(16, dtype=torch.int32), top_k=8)
    bad("x requires grad, and moe_gemm_mxfp4 has no autograd", x.clone().requires_grad_(), b, sc, off)
    bad("no CPU fallback", x, b.view(4, 32, 2, 16), sc, off)                 # the [E, N, K / 32, 16] form passes the checks
