"""CPU: fa_kv_store's host side - the C ABI's argument checks on host pointers, the ctypes mirror, the Python-level argument
errors of kv_store.store_kv_cache, the torch.library op's schema and fake implementation, and the test reference itself
(kv_store_ref) against the oracle's cache append.  No compute calls: nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard  # noqa: E402
import kv_store_ref as R  # noqa: E402

FP8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


def test_library_exports_and_struct_size(lib):
    assert hasattr(lib.lib, "fa_kv_store") and hasattr(lib.lib, "fa_kv_store_params_size")
    assert lib.lib.fa_kv_store_params_size() == ctypes.sizeof(lib.FaKvStoreParams)


def test_ctypes_mirror_matches_the_header(lib):
    """field names and order of FaKvStoreParams are the header's"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "fa_mi355.h")).read(), flags=re.S)
    body = re.search(r"typedef struct fa_kv_store_params \{(.*?)\} fa_kv_store_params;", src, flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        if stmt.strip():
            names = stmt.strip().split(",")
            fields.append(names[0].split()[-1].lstrip("*"))
            fields += [n.strip().lstrip("*") for n in names[1:]]
    assert [f[0] for f in lib.FaKvStoreParams._fields_] == fields


# layout of the host buffer behind a valid block: k, v [8, 2, 64] fp16; caches [4, 16, 2, 64]; side arrays; cos / sin [64, 32]
_KV = 8 * 2 * 64 * 2
_CACHE = 4 * 16 * 2 * 64 * 2
_SIDE = 2 * _KV + 2 * _CACHE


def _block(lib, buf, mode):
    """a valid block over host memory, slot mode or sequence mode on a paged cache"""
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaKvStoreParams()
    s.struct_size = ctypes.sizeof(lib.FaKvStoreParams)
    s.k, s.v = base, base + _KV
    s.k_row_stride = s.v_row_stride = 2 * 64
    s.k_head_stride = s.v_head_stride = 64
    s.k_cache, s.v_cache = base + 2 * _KV, base + 2 * _KV + _CACHE
    s.kc_batch_stride = s.vc_batch_stride = 16 * 2 * 64
    s.kc_row_stride = s.vc_row_stride = 2 * 64
    s.kc_head_stride = s.vc_head_stride = 64
    s.total_rows, s.nheads, s.head_dim = 8, 2, 64
    s.dtype = s.cache_dtype = lib.FA_FP16
    s.num_blocks, s.page_block_size = 4, 16
    if mode == "slot":
        s.slot_mapping = base + _SIDE
    else:
        s.cu_seqlens, s.cache_seqlens = base + _SIDE + 256, base + _SIDE + 512
        s.block_table, s.block_table_batch_stride, s.max_blocks = base + _SIDE + 768, 2, 2
        s.batch, s.paged = 2, 1
    return s, base


def test_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_kv_store fires before any device work"""
    buf = (ctypes.c_char * (_SIDE + 16384))()
    cos = lambda b: b + _SIDE + 2048                        # noqa: E731
    sin = lambda b: b + _SIDE + 2048 + 4096                 # noqa: E731

    def bad(match, mode="seq", **kw):
        s, base = _block(lib, buf, mode)
        for k, v in kw.items():
            setattr(s, k, v(base) if callable(v) else v)
        with pytest.raises(RuntimeError, match=match) as e:
            lib.call_kv_store(s, 0)
        assert "(-1)" in str(e.value)                      # FA_ERR_INVALID_ARGUMENT

    for mode in ("slot", "seq"):
        bad("struct_size", mode, struct_size=8)
        for name in ("k", "v", "k_cache", "v_cache"):
            bad("must not be NULL", mode, **{name: None})
        bad("fp16 or bf16", mode, dtype=lib.FA_FP8_E4M3, cache_dtype=lib.FA_FP8_E4M3)
        bad("fp16 or bf16", mode, dtype=7)
        bad("cache dtype", mode, cache_dtype=lib.FA_BF16)
        bad("cache dtype", mode, cache_dtype=9)
        bad("multiple of 8", mode, head_dim=60)
        bad("<= 256", mode, head_dim=264)
        for name in ("total_rows", "nheads", "head_dim", "num_blocks", "batch", "max_blocks", "seqlen_ro", "rotary_dim"):
            bad("non-negative", mode, **{name: -1})
        for name in ("k_row_stride", "k_head_stride", "v_row_stride", "v_head_stride", "kc_batch_stride", "kc_row_stride",
                     "kc_head_stride", "vc_batch_stride", "vc_row_stride", "vc_head_stride", "block_table_batch_stride"):
            bad("strides must be non-negative", mode, **{name: -64})
        bad("page_block_size", mode, page_block_size=0)
        bad("page_block_size", mode, page_block_size=-16)
        # misaligned bases and strides: k / v 16 bytes; 16-bit caches 16 bytes, fp8 caches 8 bytes
        bad("k / v base", mode, k=lambda b: b + 8)
        bad("k / v base", mode, v=lambda b: b + _KV + 2)
        bad("k / v base", mode, k_row_stride=2 * 64 + 4)
        bad("k / v base", mode, v_head_stride=64 + 2)
        bad("multiples of 16 bytes", mode, k_cache=lambda b: b + 2 * _KV + 8)
        bad("multiples of 16 bytes", mode, vc_row_stride=2 * 64 + 4)
        bad("multiples of 8 bytes", mode, cache_dtype=lib.FA_FP8_E4M3, v_cache=lambda b: b + 2 * _KV + _CACHE + 4)
        bad("multiples of 8 bytes", mode, cache_dtype=lib.FA_FP8_E4M3, kc_head_stride=64 + 4)
        for name in ("k_descale", "v_descale"):
            bad("descales", mode, cache_dtype=lib.FA_FP8_E4M3, **{name: -0.5})
            bad("descales", mode, cache_dtype=lib.FA_FP8_E4M3, **{name: float("inf")})
            bad("descales", mode, cache_dtype=lib.FA_FP8_E4M3, **{name: float("nan")})
    # the addressing modes
    bad("both given", "slot", cu_seqlens=lambda b: b + _SIDE + 256)
    bad("neither given", "slot", slot_mapping=None)
    bad("exclude each other", "seq", cache_batch_idx=lambda b: b + _SIDE + 1024)
    bad("needs a block_table", "seq", block_table=None)
    bad("needs paged", "seq", paged=0)
    bad("batch slots", "seq", paged=0, block_table=None, batch=5)
    bad("slot mode takes no", "slot", cache_seqlens=lambda b: b + _SIDE + 512)
    bad("slot mode takes no", "slot", block_table=lambda b: b + _SIDE + 768)
    bad("slot mode takes no", "slot", cache_batch_idx=lambda b: b + _SIDE + 1024)
    bad("8-byte", "slot", slot_mapping=lambda b: b + _SIDE + 4)
    for name in ("cu_seqlens", "cache_seqlens", "block_table"):
        bad("4-byte", "seq", **{name: lambda b: b + _SIDE + 1280 + 2})
    bad("4-byte", "seq", paged=0, block_table=None, cache_batch_idx=lambda b: b + _SIDE + 1024 + 1)
    # rotary: sequence mode only, fa_fwd_kvcache's constraints
    bad("rotary needs sequence mode", "slot", rotary_cos=cos, rotary_sin=sin, rotary_dim=64, seqlen_ro=64)
    bad("rotary needs sequence mode", "slot", rotary_dim=64)
    bad("both be given", "seq", rotary_cos=cos, rotary_dim=64, seqlen_ro=64)
    bad("both be given", "seq", rotary_dim=64, seqlen_ro=64)
    bad("rotary_dim > 0", "seq", rotary_cos=cos, rotary_sin=sin, seqlen_ro=64)
    bad("<= headdim", "seq", rotary_cos=cos, rotary_sin=sin, rotary_dim=80, seqlen_ro=64)
    bad("divisible by 16", "seq", rotary_cos=cos, rotary_sin=sin, rotary_dim=24, seqlen_ro=64)
    bad("16-byte aligned", "seq", rotary_cos=lambda b: cos(b) + 8, rotary_sin=sin, rotary_dim=64, seqlen_ro=64)
    with pytest.raises(RuntimeError, match="must not be NULL"):
        lib.lib.fa_kv_store.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        try:
            if lib.lib.fa_kv_store(None, None) != 0:
                raise RuntimeError(lib.lib.fa_last_error().decode())
        finally:
            lib.lib.fa_kv_store.argtypes = [ctypes.POINTER(lib.FaKvStoreParams), ctypes.c_void_p]


def test_empty_problems_are_ok_without_launch(lib):
    buf = (ctypes.c_char * (_SIDE + 16384))()
    for mode, kw in (("slot", {"total_rows": 0}), ("slot", {"nheads": 0}), ("seq", {"total_rows": 0}), ("seq", {"nheads": 0}),
                     ("seq", {"batch": 0})):
        s, base = _block(lib, buf, mode)
        for k, v in kw.items():
            setattr(s, k, v)
        lib.call_kv_store(s, 0)                            # FA_OK: nothing is launched (there is no device here)


def test_python_argument_errors_on_cpu_tensors():
    from flash_attn_mi355.kv_store import store_kv_cache
    k = torch.zeros(8, 2, 64, dtype=torch.float16)
    kc = torch.zeros(4, 16, 2, 64, dtype=torch.float16)
    slots = torch.arange(8)
    cu = torch.tensor([0, 3, 8], dtype=torch.int32)
    bt = torch.zeros(2, 2, dtype=torch.int32)
    cos = torch.zeros(32, 32, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="fp16 or bf16"):
        store_kv_cache(k.float(), k.float(), kc, kc, slot_mapping=slots)
    with pytest.raises(RuntimeError, match="k's dtype"):
        store_kv_cache(k, k.bfloat16(), kc, kc, slot_mapping=slots)
    with pytest.raises(RuntimeError, match="same shape"):
        store_kv_cache(k, k[:7], kc, kc, slot_mapping=slots)
    with pytest.raises(RuntimeError, match="same shape"):
        store_kv_cache(k[None], k[None], kc, kc, slot_mapping=slots)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        store_kv_cache(k, k, kc.bfloat16(), kc.bfloat16(), slot_mapping=slots)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        store_kv_cache(k, k, kc, kc.to(FP8), slot_mapping=slots)
    with pytest.raises(RuntimeError, match="4-D shape"):
        store_kv_cache(k, k, kc, kc[:3], slot_mapping=slots)
    with pytest.raises(RuntimeError, match="last two dimensions"):
        store_kv_cache(k, k, kc[:, :, :1], kc[:, :, :1], slot_mapping=slots)
    with pytest.raises(RuntimeError, match="last two dimensions"):
        store_kv_cache(k, k, torch.zeros(4, 16, 2, 128, dtype=torch.float16), torch.zeros(4, 16, 2, 128, dtype=torch.float16),
                       slot_mapping=slots)
    k60, kc60 = torch.zeros(8, 2, 60, dtype=torch.float16), torch.zeros(4, 16, 2, 60, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        store_kv_cache(k60, k60, kc60, kc60, slot_mapping=slots)
    with pytest.raises(RuntimeError, match="float8_e4m3fn cache"):
        store_kv_cache(k, k, kc, kc, slot_mapping=slots, k_descale=0.5)
    with pytest.raises(RuntimeError, match="float8_e4m3fn cache"):
        store_kv_cache(k, k, kc, kc, slot_mapping=slots, v_descale=0.5)
    with pytest.raises(RuntimeError, match="both given"):
        store_kv_cache(k, k, kc, kc, slot_mapping=slots, cu_seqlens=cu, block_table=bt)
    with pytest.raises(RuntimeError, match="neither given"):
        store_kv_cache(k, k, kc, kc)
    with pytest.raises(RuntimeError, match="slot_mapping takes no"):
        store_kv_cache(k, k, kc, kc, slot_mapping=slots, block_table=bt)
    with pytest.raises(RuntimeError, match="slot_mapping must be"):
        store_kv_cache(k, k, kc, kc, slot_mapping=slots[:5])
    with pytest.raises(RuntimeError, match="slot_mapping must be"):
        store_kv_cache(k, k, kc, kc, slot_mapping=slots.float())
    with pytest.raises(RuntimeError, match="rotary needs cu_seqlens"):
        store_kv_cache(k, k, kc, kc, slot_mapping=slots, rotary_cos=cos, rotary_sin=cos)
    with pytest.raises(RuntimeError, match="both be given"):
        store_kv_cache(k, k, kc, kc, cu_seqlens=cu, block_table=bt, rotary_cos=cos)
    with pytest.raises(RuntimeError, match="k's dtype"):
        store_kv_cache(k, k, kc, kc, cu_seqlens=cu, block_table=bt, rotary_cos=cos.float(), rotary_sin=cos.float())
    with pytest.raises(RuntimeError, match="<= headdim"):
        big = torch.zeros(32, 40, dtype=torch.float16)
        store_kv_cache(k, k, kc, kc, cu_seqlens=cu, block_table=bt, rotary_cos=big, rotary_sin=big)
    with pytest.raises(RuntimeError, match="cu_seqlens must be"):
        store_kv_cache(k, k, kc, kc, cu_seqlens=cu.long(), block_table=bt)
    with pytest.raises(RuntimeError, match="cache_seqlens must be"):
        store_kv_cache(k, k, kc, kc, cu_seqlens=cu, block_table=bt, cache_seqlens=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="block_table must be"):
        store_kv_cache(k, k, kc, kc, cu_seqlens=cu, block_table=bt[:1])
    with pytest.raises(RuntimeError, match="does not take cache_batch_idx"):
        store_kv_cache(k, k, kc, kc, cu_seqlens=cu, block_table=bt, cache_batch_idx=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="batch slots"):
        store_kv_cache(k, k, kc[:1], kc[:1], cu_seqlens=cu)
    with pytest.raises(RuntimeError, match="contiguous last dimension"):
        t = torch.zeros(4, 16, 64, 2, dtype=torch.float16).transpose(2, 3)
        store_kv_cache(k, k, t, t, slot_mapping=slots)
    # everything else in order: the CPU tensor itself is the error
    with pytest.raises(RuntimeError, match="GPU"):
        store_kv_cache(k, k, kc, kc, slot_mapping=slots)
    with pytest.raises(RuntimeError, match="GPU"):
        store_kv_cache(k, k, kc.to(FP8), kc.to(FP8), cu_seqlens=cu, block_table=bt, k_descale=0.5, v_descale=0.25)


def test_torch_op_schema_and_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import flash_attn_mi355.torch_ops as T
    schema = torch.ops.flash_attn_mi355.kv_store.default._schema
    mutated = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
    assert mutated == ["k_cache", "v_cache"]
    assert len(schema.returns) == 0
    with FakeTensorMode():
        qkv = torch.empty(200, 8, 64, dtype=torch.bfloat16, device="cuda")
        k, v = qkv[:, 4:6], qkv[:, 6:8]
        kc = torch.empty(20, 16, 2, 64, dtype=torch.bfloat16, device="cuda")
        slots = torch.empty(200, dtype=torch.int64, device="cuda")
        assert torch.ops.flash_attn_mi355.kv_store(k, v, kc, kc.clone(), slots, None, None, None, None, None, None, True, 1.0, 1.0) is None
        cu = torch.empty(4, dtype=torch.int32, device="cuda")
        bt = torch.empty(3, 9, dtype=torch.int32, device="cuda")
        cos = torch.empty(64, 32, dtype=torch.bfloat16, device="cuda")
        kc8 = torch.empty(20, 16, 2, 64, dtype=FP8, device="cuda")
        assert torch.ops.flash_attn_mi355.kv_store(k, v, kc8, kc8.clone(), None, cu, cu[:3], bt, None, cos, cos, False, 0.05, 0.04) is None
    assert "kv_store" in T.__all__


def test_public_name_lists_are_unchanged():
    import flash_attn
    import flash_attn_mi355
    import flash_attn_mi355.torch_ops as T
    assert flash_attn.__all__ == ["flash_attn_func", "flash_attn_gpu", "flash_attn_varlen_func", "flash_attn_varlen_gpu",
                                  "flash_attn_with_kvcache", "flash_attn_with_kvcache_gpu", "flash_attn_qkvpacked_func",
                                  "flash_attn_kvpacked_func", "flash_attn_varlen_qkvpacked_func",
                                  "flash_attn_varlen_kvpacked_func", "__version__"]
    assert "store_kv_cache" not in flash_attn.__all__ and "store_kv_cache" not in flash_attn_mi355.__all__
    assert "kv_store" not in flash_attn_mi355.__all__
    assert T.__all__[:12] == ["fwd", "bwd", "varlen_fwd", "varlen_bwd", "fwd_kvcache", "fwd_kvcache_tree", "fwd_out",
                              "varlen_fwd_out", "bwd_out", "merge_states", "rotary", "rotary_"]
    assert T.__all__[12:] == ["kv_store"]


def test_reference_cast_is_round_to_nearest_even_and_saturates():
    f = lambda x: float(torch.tensor(x, dtype=torch.float32).to(FP8).float())     # noqa: E731
    assert f(17.0) == 16.0 and f(19.0) == 20.0             # ties between 16, 18, 20: to the even mantissa
    assert f(2.0 ** -10) == 0.0                            # half the smallest subnormal (2^-9): tie to even = 0
    z = torch.tensor(-0.0).to(FP8)
    assert int(z.view(torch.uint8)) == 0x80                # -0 keeps its sign
    assert np.isnan(f(465.0)) and f(464.0) == 448.0        # no clamp: NaN above 464
    q = R.quantise(torch.tensor([1000.0, -1000.0, 465.0]), 1.0).float().tolist()
    assert q == [448.0, -448.0, 448.0]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_reference_quantiser_agrees_with_the_oracle(dtype):
    """kv_store_ref.quantise (fp32: x * (1 / d)) == oracle.kvcache.round_e4m3 (fp64: x / d) code for code on random data"""
    from oracle.kvcache import round_e4m3
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(400000, generator=g) * 3.0).to(dtype)
    for d in (0.0625, 0.03125, 0.05, 0.04, 0.013):
        got = R.quantise(x, d).float().double().numpy()
        want = round_e4m3(x.double().numpy() / d)
        assert np.array_equal(got, want), d


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("paged", [False, True])
def test_reference_leaves_the_cache_the_oracle_append_leaves(paged, fp8):
    """uniform batch B 3, T_new 3, Hk 2, D 64, cache_seqlens crossing a page-16 boundary: kv_store_ref == oracle.kvcache_fwd's
    append (a dummy one-token q), contiguous and paged, 16-bit and fp8 with power-of-two descales"""
    import oracle
    B, Tn, Hk, D, page = 3, 3, 2, 64, 16
    dt = torch.bfloat16
    L = [14, 0, 31]                                        # 14..16 and 31..33 cross a page boundary
    g = torch.Generator().manual_seed(11)
    knew = torch.randn(B, Tn, Hk, D, generator=g).to(dt)
    vnew = torch.randn(B, Tn, Hk, D, generator=g).to(dt)
    kd, vd = (0.0625, 0.03125) if fp8 else (None, None)
    if paged:
        bt, nblk, _ = guard.paged_table([l + Tn for l in L], page, seed=3)
        shape = (nblk, page, Hk, D)
    else:
        bt, shape = None, (B, 48, Hk, D)
    kc = torch.randn(shape, generator=g).to(dt)
    vc = torch.randn(shape, generator=g).to(dt)
    if fp8:
        kc, vc = kc.to(FP8), vc.to(FP8)
    cu = [0, 3, 6, 9]
    got_k, got_v = R.kv_store_ref(knew.reshape(-1, Hk, D), vnew.reshape(-1, Hk, D), kc, vc, cu_seqlens=cu, cache_seqlens=L,
                                  block_table=bt, k_descale=kd, v_descale=vd)
    assert got_k.dtype == kc.dtype and not R.same_bits(got_k, kc)
    ok, ov = kc.float().double().numpy().copy(), vc.float().double().numpy().copy()
    q = np.zeros((B, 1, Hk, D))
    oracle.kvcache_fwd(q, ok, ov, k=knew.double().numpy(), v=vnew.double().numpy(), cache_seqlens=np.asarray(L),
                       block_table=None if bt is None else bt.numpy(), io_dtype="bf16", k_descale=kd, v_descale=vd)
    assert np.array_equal(got_k.float().double().numpy(), ok)
    assert np.array_equal(got_v.float().double().numpy(), ov)


def test_reference_addressing_rules():
    """slot mode, dropped rows, cache_batch_idx and rows behind cu_seqlens[-1] in the reference itself"""
    dest, _ = R.destinations(5, (3, 4), slot_mapping=[0, 5, -1, 12, 11])
    assert dest == [(0, 0), (1, 1), None, None, (2, 3)]
    dest, pos = R.destinations(9, (4, 8), cu_seqlens=[0, 0, 3, 7], cache_seqlens=[2, 6, 0], cache_batch_idx=[3, 1, 0])
    assert dest == [(1, 6), (1, 7), None, (0, 0), (0, 1), (0, 2), (0, 3), None, None]
    assert pos == [6, 7, 8, 0, 1, 2, 3, -1, -1]
    bt = torch.tensor([[2, 0]], dtype=torch.int32)
    dest, _ = R.destinations(4, (3, 2), cu_seqlens=[0, 4], cache_seqlens=[1], block_table=bt)
    assert dest == [(2, 1), (0, 0), (0, 1), None]
