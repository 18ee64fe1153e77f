"""CPU: the standalone rotary embedding's host side - the C ABI's fa_rotary argument checks on host pointers, the ctypes mirror,
the flash_attn.layers.rotary surface, the Python-level argument errors, the fake implementations of the torch.library ops and
RotaryEmbedding's cos / sin cache.  No compute calls: nothing here needs a GPU."""
import ctypes
import inspect
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


def test_library_exports_and_struct_size(lib):
    assert hasattr(lib.lib, "fa_rotary") and hasattr(lib.lib, "fa_rotary_params_size")
    assert lib.lib.fa_rotary_params_size() == ctypes.sizeof(lib.FaRotaryParams)


def _block(lib, buf):
    """a valid block over host memory: x [2, 4, 2, 64] fp16 contiguous, out behind it, cos / sin [8, 32]"""
    base = (ctypes.addressof(buf) + 15) & ~15
    r = lib.FaRotaryParams()
    r.struct_size = ctypes.sizeof(lib.FaRotaryParams)
    r.batch, r.seqlen, r.nheads, r.head_dim, r.rotary_dim, r.seqlen_ro = 2, 4, 2, 64, 64, 8
    r.dtype = lib.FA_FP16
    n = 2 * 4 * 2 * 64 * 2
    r.x, r.out = base, base + n
    r.x_batch_stride = r.o_batch_stride = 4 * 2 * 64
    r.x_row_stride = r.o_row_stride = 2 * 64
    r.x_head_stride = r.o_head_stride = 64
    r.cos, r.sin = base + 2 * n, base + 2 * n + 1024
    return r, base, n


def test_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_rotary fires before any device work"""
    buf = (ctypes.c_char * 16384)()

    def bad(match, **kw):
        r, base, n = _block(lib, buf)
        for k, v in kw.items():
            setattr(r, k, v(base, n) if callable(v) else v)
        with pytest.raises(RuntimeError, match=match):
            lib.call_rotary(r, 0)

    bad("struct_size", struct_size=8)
    for name in ("x", "out", "cos", "sin"):
        bad("must not be NULL", **{name: None})
    bad("fp16 or bf16", dtype=lib.FA_FP8_E4M3)
    bad("fp16 or bf16", dtype=7)
    bad("even", rotary_dim=31)
    bad("<= head_dim", rotary_dim=66)
    bad("positive", rotary_dim=0)
    bad("positive", rotary_dim=-2)
    for name in ("batch", "seqlen", "nheads", "head_dim", "seqlen_ro", "total_rows", "seqlen_offset"):
        bad("non-negative", **{name: -1})
    bad("strides", x_row_stride=-128)
    bad("cos / sin", cos=lambda b, n: b + 2 * n + 1)
    bad("cos / sin", sin=lambda b, n: b + 2 * n + 1024 + 2, cos_sin_fp32=1)
    bad("4-byte", seqlen_offsets=lambda b, n: b + 2 * n + 2048 + 2)
    bad("4-byte", cu_seqlens=lambda b, n: b + 2 * n + 2048 + 1, total_rows=8)
    bad("2-byte", x=lambda b, n: b + 1)
    # overlap: out inside x's range but not x itself; x's base with other strides
    bad("overlaps", out=lambda b, n: b + 16)
    bad("overlaps", out=lambda b, n: b + n - 2)
    bad("strides", out=lambda b, n: b, o_row_stride=2 * 64 + 8)
    bad("overlaps", out=lambda b, n: b + 64, cu_seqlens=lambda b, n: b + 2 * n + 2048, total_rows=8)


def test_empty_problem_is_ok_without_launch(lib):
    buf = (ctypes.c_char * 16384)()
    for kw in ({"batch": 0}, {"seqlen": 0}, {"nheads": 0}):
        r, base, n = _block(lib, buf)
        for k, v in kw.items():
            setattr(r, k, v)
        lib.call_rotary(r, 0)                              # FA_OK: nothing is launched (there is no device here)
    r, base, n = _block(lib, buf)
    r.cu_seqlens, r.total_rows = base + 2 * n + 2048, 0
    lib.call_rotary(r, 0)


def test_layers_rotary_surface():
    """upstream's module path, names, parameter lists and defaults; flash_attn.__all__ is what it was"""
    import flash_attn
    from flash_attn.layers import rotary as R

    def params(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items()]

    E = inspect.Parameter.empty
    assert params(R.apply_rotary_emb) == [("x", E), ("cos", E), ("sin", E), ("interleaved", False), ("inplace", False),
                                          ("seqlen_offsets", 0), ("cu_seqlens", None), ("max_seqlen", None)]
    assert R.apply_rotary_emb_func is R.apply_rotary_emb
    assert params(R.apply_rotary_emb_qkv_) == [("qkv", E), ("cos", E), ("sin", E), ("cos_k", None), ("sin_k", None),
                                               ("interleaved", False), ("seqlen_offsets", 0), ("num_heads_q", None)]
    assert params(R.apply_rotary_emb_kv_) == [("kv", E), ("cos", E), ("sin", E), ("interleaved", False), ("seqlen_offsets", 0)]
    assert params(R.RotaryEmbedding.__init__)[1:] == [("dim", E), ("base", 10000.0), ("interleaved", False), ("scale_base", None),
                                                      ("pos_idx_in_fp32", True), ("device", None)]
    assert params(R.RotaryEmbedding.forward)[1:] == [("qkv", E), ("kv", None), ("seqlen_offset", 0), ("max_seqlen", None),
                                                     ("num_heads_q", None)]
    assert flash_attn.__all__ == ["flash_attn_func", "flash_attn_gpu", "flash_attn_varlen_func", "flash_attn_varlen_gpu",
                                  "flash_attn_with_kvcache", "flash_attn_with_kvcache_gpu", "flash_attn_qkvpacked_func",
                                  "flash_attn_kvpacked_func", "flash_attn_varlen_qkvpacked_func",
                                  "flash_attn_varlen_kvpacked_func", "__version__"]
    with pytest.raises(NotImplementedError):
        R.RotaryEmbedding(64, scale_base=512)


def test_python_argument_errors_on_cpu_tensors():
    from flash_attn.layers.rotary import apply_rotary_emb, apply_rotary_emb_kv_, apply_rotary_emb_qkv_
    x = torch.zeros(2, 8, 2, 64, dtype=torch.float16)
    cos = torch.zeros(16, 32, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="fp16 or bf16"):
        apply_rotary_emb(x.float(), cos.float(), cos.float())
    with pytest.raises(RuntimeError, match="fp16 or bf16"):
        apply_rotary_emb(x.to(torch.float8_e4m3fn), cos, cos)
    with pytest.raises(RuntimeError, match="dtype"):
        apply_rotary_emb(x, cos.bfloat16(), cos.bfloat16())
    with pytest.raises(RuntimeError, match="dtype"):
        apply_rotary_emb(x, cos, cos.float())
    with pytest.raises(RuntimeError, match="same shape"):
        apply_rotary_emb(x, cos, cos[:, :16])
    with pytest.raises(RuntimeError, match="<= headdim"):
        apply_rotary_emb(x, torch.zeros(16, 40, dtype=torch.float16), torch.zeros(16, 40, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="seqlen_ro"):
        apply_rotary_emb(x, cos, cos, seqlen_offsets=9)
    with pytest.raises(RuntimeError, match="max_seqlen"):
        apply_rotary_emb(x[0], cos, cos, cu_seqlens=torch.tensor([0, 8], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="seqlen_offsets"):
        apply_rotary_emb(x, cos, cos, seqlen_offsets=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="contiguous"):
        apply_rotary_emb(x.transpose(2, 3), cos[:, :1], cos[:, :1])
    # everything else in order: the CPU tensor itself is the error
    with pytest.raises(RuntimeError, match="GPU"):
        apply_rotary_emb(x, cos, cos)
    with pytest.raises(RuntimeError, match="GPU"):
        apply_rotary_emb_qkv_(torch.zeros(2, 8, 3, 2, 64, dtype=torch.float16), cos, cos)
    with pytest.raises(RuntimeError, match="GPU"):
        apply_rotary_emb_kv_(torch.zeros(2, 8, 2, 2, 64, dtype=torch.float16), cos, cos)
    with pytest.raises(RuntimeError, match="num_heads_q"):
        apply_rotary_emb_qkv_(torch.zeros(2, 8, 8, 64, dtype=torch.float16), cos, cos)


def test_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import flash_attn_mi355.torch_ops  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        base = torch.empty(2, 9, 3, 4, 64, dtype=torch.bfloat16, device="cuda")
        x = base[:, :, 0]                                  # a strided view
        cos = torch.empty(16, 32, dtype=torch.bfloat16, device="cuda")
        out = torch.ops.flash_attn_mi355.rotary(x, cos, cos, None, None, 0, 0, False, False)
        assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous() and out.device == x.device
        assert torch.ops.flash_attn_mi355.rotary_(x, cos, cos, None, None, 0, 0, False, False) is None
        xv = torch.empty(41, 2, 64, dtype=torch.float16, device="cuda")
        cu = torch.empty(5, dtype=torch.int32, device="cuda")
        offs = torch.empty(4, dtype=torch.int32, device="cuda")
        out = torch.ops.flash_attn_mi355.rotary(xv, cos.half(), cos.half(), offs, cu, 0, 37, True, True)
        assert out.shape == xv.shape and out.dtype == torch.float16 and out.stride() == (128, 64, 1)


def test_rotary_embedding_cache_is_the_closed_form():
    from flash_attn.layers.rotary import RotaryEmbedding
    dim, base, n = 64, 10000.0, 50
    m = RotaryEmbedding(dim, base=base)
    m._update_cos_sin_cache(n, device=torch.device("cpu"), dtype=torch.float32)
    inv = torch.tensor([1.0 / base ** (2 * t / dim) for t in range(dim // 2)], dtype=torch.float64)
    ang = torch.arange(n, dtype=torch.float64)[:, None] * inv[None, :]
    assert m._cos_cached.shape == (n, dim // 2) and m._cos_cached.dtype == torch.float32
    # fp32: inv_freq (a power and a division, <= 1) carries a few ulp, the product with a position < n one more rounding -
    # the angle is off by < n x 8 x 2^-24; cos / sin are 1-Lipschitz and their own evaluation adds an ulp
    tol = n * 2.0 ** -21 + 2.0 ** -23
    assert (m._cos_cached.double() - torch.cos(ang)).abs().max() < tol
    assert (m._sin_cached.double() - torch.sin(ang)).abs().max() < tol
    assert m._cos_cached[0].eq(1).all() and m._sin_cached[0].eq(0).all()
    assert math.isclose(float(m.inv_freq[1]), base ** (-2 / dim), rel_tol=1e-6)
    # the cache is kept in the dtype of the tensors it rotates and grows on demand
    m._update_cos_sin_cache(n + 10, device=torch.device("cpu"), dtype=torch.bfloat16)
    assert m._cos_cached.shape == (n + 10, dim // 2) and m._cos_cached.dtype == torch.bfloat16
