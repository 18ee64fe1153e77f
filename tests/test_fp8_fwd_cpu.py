"""CPU: the fp8-e4m3 q / k / v forward (csrc/fa_fwd_fp8.hip) - ABI 4 fields, its argument checks through the C ABI (no device
work happens before them), the compiled code (block-scaled K = 64 MFMAs only, no spill, no scratch) and the fake op."""
import ctypes
import json
import os
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


def test_abi_4_appends_q_descale_and_o_dtype(lib):
    assert lib.lib.fa_abi_version() == 4 == lib.FA_ABI_VERSION
    assert lib.lib.fa_params_size() == ctypes.sizeof(lib.FaParams)
    names = [f[0] for f in lib.FaParams._fields_]
    assert names[-3:] == ["workspace_bytes", "q_descale", "o_dtype"]
    # appended: every ABI 3 field keeps its offset
    assert lib.FaParams.q_descale.offset >= lib.FaParams.workspace_bytes.offset + ctypes.sizeof(ctypes.c_size_t)


def _fp8_params(lib, buf):
    p = lib.FaParams()
    addr = (ctypes.addressof(buf) + 15) & ~15
    p.q = p.k = p.v = p.o = p.lse = addr
    p.batch, p.nheads_q, p.nheads_k, p.head_dim, p.seqlen_q, p.seqlen_k = 1, 2, 2, 128, 4, 4
    p.q_row_stride = p.k_row_stride = p.v_row_stride = p.o_row_stride = 256
    p.q_head_stride = p.k_head_stride = p.v_head_stride = p.o_head_stride = 128
    p.dtype = p.kv_dtype = lib.FA_FP8_E4M3
    p.o_dtype = lib.FA_BF16
    p.softmax_scale = 0.125
    p.window_left = p.window_right = -1
    return p


def test_fp8_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * 65536)()
    addr = (ctypes.addressof(buf) + 15) & ~15

    def fails(p, match, op="fa_fwd"):
        with pytest.raises(RuntimeError, match=match):
            lib.call(op, p, 0)

    p = _fp8_params(lib, buf)
    p.kv_dtype = lib.FA_FP16
    fails(p, "fp8-e4m3 k and v")
    p = _fp8_params(lib, buf)
    p.alibi_slopes = addr
    fails(p, r"failed \(-2\).*ALiBi")
    p = _fp8_params(lib, buf)
    p.softcap = 30.0
    fails(p, r"failed \(-2\).*softcap")
    p = _fp8_params(lib, buf)
    p.p_dropout = 0.1
    fails(p, r"failed \(-2\).*dropout")
    p = _fp8_params(lib, buf)
    p.head_dim = 256
    fails(p, r"failed \(-2\).*head dimension 256")
    p = _fp8_params(lib, buf)
    p.o_dtype = lib.FA_FP8_E4M3
    fails(p, r"failed \(-1\).*o_dtype")
    for name in ("q_descale", "k_descale", "v_descale"):
        for bad in (-1.0, float("inf"), float("nan")):
            p = _fp8_params(lib, buf)
            setattr(p, name, bad)
            fails(p, r"failed \(-1\).*descale")
    p = _fp8_params(lib, buf)
    p.head_dim_v = 72
    fails(p, "multiple of 16")
    # varlen: paged K/V with fp8 q
    cu = (ctypes.c_int32 * 2)(0, 4)
    p = _fp8_params(lib, buf)
    p.cu_seqlens_q = p.cu_seqlens_k = ctypes.addressof(cu)
    p.total_q, p.total_k = 4, 4
    p.block_table, p.page_block_size = addr, 16
    fails(p, r"failed \(-2\).*paged", op="fa_varlen_fwd")
    # the other ops reject fp8 q exactly as before (the 16-bit message)
    p = _fp8_params(lib, buf)
    p.dout = p.softmax_d = addr
    fails(p, "q must be fp16 or bf16", op="fa_bwd")
    p = _fp8_params(lib, buf)
    fails(p, "q must be fp16 or bf16", op="fa_fwd_kvcache")
    # an unknown dtype still names the 16-bit types on the forward ops too
    p = _fp8_params(lib, buf)
    p.dtype = 7
    fails(p, "fp16 or bf16")


def test_fp8_needs_no_workspace(lib):
    buf = (ctypes.c_char * 65536)()
    p = _fp8_params(lib, buf)
    p.is_causal = 1
    p.flags = lib.FA_FLAG_FWD_KEY_SPLIT
    assert lib.lib.fa_fwd_workspace_bytes(ctypes.byref(p)) == 0


def _disassemble(obj, wd):
    llvm = "/opt/rocm/lib/llvm/bin"
    fat, co = os.path.join(wd, "f.fat"), os.path.join(wd, "f.co")
    subprocess.run([f"{llvm}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj], check=True)
    subprocess.run([f"{llvm}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fat}", f"--output={co}", "--unbundle"], check=True)
    return subprocess.run([f"{llvm}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout


def test_fp8_kernel_runs_on_the_block_scaled_mfma(lib):
    import build
    obj = os.path.join(build.CSRC, "build", "fa_fwd_fp8.o")
    assert "fa_fwd_fp8.hip" in build.SOURCES and os.path.exists(obj)
    with tempfile.TemporaryDirectory() as wd:
        txt = _disassemble(obj, wd)
    assert txt.count("v_mfma_scale_f32_32x32x64_f8f6f4") >= 4 * 2 * 6        # four kernels, two unrolled stages, >= 6 each
    for other in ("v_mfma_f32_32x32x16_bf16", "v_mfma_f32_32x32x16_f16", "v_mfma_f32_32x32x16_fp8_fp8"):
        assert other not in txt, other


def test_fp8_kernels_do_not_spill(lib):
    import build
    res = json.load(open(build.RESOURCES))
    fp8 = {n: r for n, r in res.items() if "fa_fwd_fp8_kernel" in n}
    assert len(fp8) == 4, sorted(fp8)                                        # {bf16, fp16 out} x {64, 128}
    for n, r in fp8.items():
        assert r.get("spill", 0) == 0 and r.get("scratch", 0) == 0, (n, r)
    budget = json.load(open(os.path.join(build.CSRC, "spill_budget.json")))["spill"]
    assert not [n for n in budget if "fa_fwd_fp8_kernel" in n]


def test_fake_ops_give_bf16_out_for_fp8_q():
    import flash_attn_mi355.torch_ops  # noqa: F401
    B, S, H, Hk, D = 2, 96, 4, 2, 128
    q = torch.empty(B, S, H, D, dtype=torch.float8_e4m3fn, device="meta")
    k = torch.empty(B, S + 32, Hk, D, dtype=torch.float8_e4m3fn, device="meta")
    out, lse, dmask, rng = torch.ops.flash_attn_mi355.fwd(q, k, k.clone(), None, 0.0, 0.125, True, -1, -1, 0.0, False)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert lse.shape == (B, H, S) and lse.dtype == torch.float32
    T = 300
    q = torch.empty(T, H, D, dtype=torch.float8_e4m3fn, device="meta")
    cu = torch.empty(4, dtype=torch.int32, device="meta")
    out, lse, _, _ = torch.ops.flash_attn_mi355.varlen_fwd(q, q, q, cu, cu, None, None, 128, 128, 0.0, 0.1, True,
                                                           -1, -1, 0.0, False)
    assert out.shape == (T, H, D) and out.dtype == torch.bfloat16 and lse.shape == (H, T)


def test_python_rejections_before_launch():
    """mixed dtypes and the uncovered options raise in Python, before any tensor reaches the device (CPU tensors here:
    the device check would fire only after them)"""
    import flash_attn_mi355 as fa
    q8 = torch.zeros(1, 16, 2, 64, dtype=torch.float8_e4m3fn)
    q16 = torch.zeros(1, 16, 2, 64, dtype=torch.bfloat16)
    from flash_attn_mi355 import flash_attn_interface as fi
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        fi._is_fp8_qkv(q8, q16, q16)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        fi._is_fp8_qkv(q16, q8, q8)
    assert fi._is_fp8_qkv(q8, q8, q8) and not fi._is_fp8_qkv(q16, q16, q16)
    for kw, match in ((dict(head_size_og=256), "head dimension"), (dict(dropout_p=0.1), "dropout"),
                      (dict(softcap=5.0), "softcap"), (dict(alibi_slopes=torch.zeros(2)), "ALiBi"),
                      (dict(paged=True), "paged")):
        args = dict(head_size_og=64, dropout_p=0.0, softcap=0.0, alibi_slopes=None)
        args.update(kw)
        with pytest.raises(RuntimeError, match=match):
            fi._check_fp8_options(**args)
    assert "q_descale" in __import__("inspect").signature(fa.flash_attn_varlen_func).parameters
