"""CPU: fa_kv_gather's host side - the C ABI's argument checks on host pointers, the ctypes mirror, the Python-level argument
errors of kv_gather.gather_kv_cache / move_kv_cache, the torch.library ops' schemas and fake implementations, and the test
reference itself (kv_gather_ref): the inverse of kv_store_ref, and the e4m3 round trip.  No compute calls: nothing here needs a
GPU."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard  # noqa: E402
import kv_gather_ref as G  # noqa: E402
import kv_store_ref as R  # noqa: E402

FP8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


def test_library_exports_and_struct_size(lib):
    assert hasattr(lib.lib, "fa_kv_gather") and hasattr(lib.lib, "fa_kv_gather_params_size")
    assert "fa_kv_gather" in lib.EXPORTS and "fa_kv_gather_params_size" in lib.EXPORTS
    assert lib.lib.fa_kv_gather_params_size() == ctypes.sizeof(lib.FaKvGatherParams)


def test_ctypes_mirror_matches_the_header(lib):
    """field names and order of FaKvGatherParams are the header's"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "fa_mi355.h")).read(), flags=re.S)
    body = re.search(r"typedef struct fa_kv_gather_params \{(.*?)\} fa_kv_gather_params;", src, flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        if stmt.strip():
            names = stmt.strip().split(",")
            fields.append(names[0].split()[-1].lstrip("*"))
            fields += [n.strip().lstrip("*") for n in names[1:]]
    assert [f[0] for f in lib.FaKvGatherParams._fields_] == fields


# layout of the host buffer behind a valid block: caches [4, 16, 2, 64] fp16; k, v [8, 2, 64]; side arrays
_KV = 8 * 2 * 64 * 2
_CACHE = 4 * 16 * 2 * 64 * 2
_SIDE = 2 * _KV + 2 * _CACHE


def _block(lib, buf, mode):
    """a valid block over host memory, slot mode or sequence mode on a paged cache"""
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaKvGatherParams()
    s.struct_size = ctypes.sizeof(lib.FaKvGatherParams)
    s.k_cache, s.v_cache = base, base + _CACHE
    s.kc_batch_stride = s.vc_batch_stride = 16 * 2 * 64
    s.kc_row_stride = s.vc_row_stride = 2 * 64
    s.kc_head_stride = s.vc_head_stride = 64
    s.k, s.v = base + 2 * _CACHE, base + 2 * _CACHE + _KV
    s.k_row_stride = s.v_row_stride = 2 * 64
    s.k_head_stride = s.v_head_stride = 64
    s.total_rows, s.nheads, s.head_dim = 8, 2, 64
    s.dtype = s.cache_dtype = lib.FA_FP16
    s.num_blocks, s.page_block_size = 4, 16
    if mode == "slot":
        s.slot_mapping = base + _SIDE
    else:
        s.cu_seqlens, s.seq_offsets = base + _SIDE + 256, base + _SIDE + 512
        s.block_table, s.block_table_batch_stride, s.max_blocks = base + _SIDE + 768, 2, 2
        s.batch, s.paged = 2, 1
    return s, base


def test_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_kv_gather fires before any device work"""
    buf = (ctypes.c_char * (_SIDE + 16384))()

    def bad(match, mode="seq", **kw):
        s, base = _block(lib, buf, mode)
        for k, v in kw.items():
            setattr(s, k, v(base) if callable(v) else v)
        with pytest.raises(RuntimeError, match=match) as e:
            lib.call_kv_gather(s, 0)
        assert "(-1)" in str(e.value)                      # FA_ERR_INVALID_ARGUMENT

    for mode in ("slot", "seq"):
        bad("struct_size", mode, struct_size=8)
        for name in ("k", "v", "k_cache", "v_cache"):
            bad("must not be NULL", mode, **{name: None})
        bad("fp16 or bf16", mode, dtype=lib.FA_FP8_E4M3, cache_dtype=lib.FA_FP8_E4M3)
        bad("fp16 or bf16", mode, dtype=7)
        bad("cache dtype", mode, cache_dtype=lib.FA_BF16)  # a 16-bit cache of the other 16-bit type
        bad("cache dtype", mode, cache_dtype=9)
        bad("multiple of 8", mode, head_dim=60)
        bad("<= 256", mode, head_dim=264)
        for name in ("total_rows", "nheads", "head_dim", "num_blocks", "batch", "max_blocks"):
            bad("non-negative", mode, **{name: -1})
        for name in ("k_row_stride", "k_head_stride", "v_row_stride", "v_head_stride", "kc_batch_stride", "kc_row_stride",
                     "kc_head_stride", "vc_batch_stride", "vc_row_stride", "vc_head_stride", "block_table_batch_stride"):
            bad("strides must be non-negative", mode, **{name: -64})
        bad("page_block_size", mode, page_block_size=0)
        bad("page_block_size", mode, page_block_size=-16)
        # misaligned bases and strides: k / v 16 bytes; 16-bit caches 16 bytes, fp8 caches 8 bytes
        bad("k / v base", mode, k=lambda b: b + 2 * _CACHE + 8)
        bad("k / v base", mode, v=lambda b: b + 2 * _CACHE + _KV + 2)
        bad("k / v base", mode, k_row_stride=2 * 64 + 4)
        bad("k / v base", mode, v_head_stride=64 + 2)
        bad("multiples of 16 bytes", mode, k_cache=lambda b: b + 8)
        bad("multiples of 16 bytes", mode, vc_row_stride=2 * 64 + 4)
        bad("multiples of 8 bytes", mode, cache_dtype=lib.FA_FP8_E4M3, v_cache=lambda b: b + _CACHE + 4)
        bad("multiples of 8 bytes", mode, cache_dtype=lib.FA_FP8_E4M3, kc_head_stride=64 + 4)
        for name in ("k_descale", "v_descale"):
            bad("descales", mode, cache_dtype=lib.FA_FP8_E4M3, **{name: -0.5})
            bad("descales", mode, cache_dtype=lib.FA_FP8_E4M3, **{name: float("inf")})
            bad("descales", mode, cache_dtype=lib.FA_FP8_E4M3, **{name: float("nan")})
        # the output inside what is read: k on k_cache's last row, v one row into v_cache, k_cache ending inside v
        bad("k overlaps k_cache", mode, k=lambda b: b + _CACHE - 256)
        bad("v overlaps v_cache", mode, v=lambda b: b + _CACHE + 256)
        bad("k overlaps v_cache", mode, k=lambda b: b + _CACHE)
        bad("v overlaps k_cache", mode, v=lambda b: b)
    # the addressing modes
    bad("both given", "slot", cu_seqlens=lambda b: b + _SIDE + 256)
    bad("neither given", "slot", slot_mapping=None)
    bad("exclude each other", "seq", cache_batch_idx=lambda b: b + _SIDE + 1024)
    bad("needs a block_table", "seq", block_table=None)
    bad("needs paged", "seq", paged=0)
    bad("batch slots", "seq", paged=0, block_table=None, batch=5)
    bad("slot mode takes no", "slot", seq_offsets=lambda b: b + _SIDE + 512)
    bad("slot mode takes no", "slot", block_table=lambda b: b + _SIDE + 768)
    bad("slot mode takes no", "slot", cache_batch_idx=lambda b: b + _SIDE + 1024)
    bad("8-byte", "slot", slot_mapping=lambda b: b + _SIDE + 4)
    for name in ("cu_seqlens", "seq_offsets", "block_table"):
        bad("4-byte", "seq", **{name: lambda b: b + _SIDE + 1280 + 2})
    bad("4-byte", "seq", paged=0, block_table=None, cache_batch_idx=lambda b: b + _SIDE + 1024 + 1)
    with pytest.raises(RuntimeError, match="must not be NULL"):
        lib.lib.fa_kv_gather.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        try:
            if lib.lib.fa_kv_gather(None, None) != 0:
                raise RuntimeError(lib.lib.fa_last_error().decode())
        finally:
            lib.lib.fa_kv_gather.argtypes = [ctypes.POINTER(lib.FaKvGatherParams), ctypes.c_void_p]


def test_empty_problems_are_ok_without_launch(lib):
    buf = (ctypes.c_char * (_SIDE + 16384))()
    for mode, kw in (("slot", {"total_rows": 0}), ("slot", {"nheads": 0}), ("seq", {"total_rows": 0}), ("seq", {"nheads": 0}),
                     ("seq", {"total_rows": 0, "batch": 0})):
        s, base = _block(lib, buf, mode)
        for k, v in kw.items():
            setattr(s, k, v)
        lib.call_kv_gather(s, 0)                           # FA_OK: nothing is launched (there is no device here)


def test_python_argument_errors_on_cpu_tensors():
    from flash_attn_mi355.kv_gather import gather_kv_cache, move_kv_cache
    kc = torch.zeros(4, 16, 2, 64, dtype=torch.float16)
    kc8 = kc.to(FP8)
    slots = torch.arange(8)
    cu = torch.tensor([0, 3, 8], dtype=torch.int32)
    bt = torch.zeros(2, 2, dtype=torch.int32)
    out = (torch.zeros(8, 2, 64, dtype=torch.float16), torch.zeros(8, 2, 64, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="fp16, bf16 or float8_e4m3fn"):
        gather_kv_cache(kc.float(), kc.float(), slot_mapping=slots)
    with pytest.raises(RuntimeError, match="fp16, bf16 or float8_e4m3fn"):
        gather_kv_cache(kc, kc8, slot_mapping=slots)
    with pytest.raises(RuntimeError, match="4-D shape"):
        gather_kv_cache(kc, kc[:3], slot_mapping=slots)
    with pytest.raises(RuntimeError, match="4-D shape"):
        gather_kv_cache(kc[0], kc[0], slot_mapping=slots)
    kc60 = torch.zeros(4, 16, 2, 60, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        gather_kv_cache(kc60, kc60, slot_mapping=slots)
    with pytest.raises(RuntimeError, match="needs dtype="):                       # dtype missing for fp8
        gather_kv_cache(kc8, kc8, slot_mapping=slots)
    with pytest.raises(RuntimeError, match="dtype must be fp16 or bf16"):
        gather_kv_cache(kc8, kc8, slot_mapping=slots, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="bit for bit"):
        gather_kv_cache(kc, kc, slot_mapping=slots, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="float8_e4m3fn cache"):
        gather_kv_cache(kc, kc, slot_mapping=slots, k_descale=0.5)
    with pytest.raises(RuntimeError, match="float8_e4m3fn cache"):
        gather_kv_cache(kc, kc, slot_mapping=slots, v_descale=0.5)
    with pytest.raises(RuntimeError, match="both given"):
        gather_kv_cache(kc, kc, slot_mapping=slots, cu_seqlens=cu, block_table=bt)
    with pytest.raises(RuntimeError, match="neither given"):
        gather_kv_cache(kc, kc)
    with pytest.raises(RuntimeError, match="contiguous last dimension"):
        t = torch.zeros(4, 16, 64, 2, dtype=torch.float16).transpose(2, 3)
        gather_kv_cache(t, t, slot_mapping=slots)
    with pytest.raises(RuntimeError, match="slot_mapping takes no"):
        gather_kv_cache(kc, kc, slot_mapping=slots, block_table=bt)
    with pytest.raises(RuntimeError, match="slot_mapping takes no"):
        gather_kv_cache(kc, kc, slot_mapping=slots, seq_offsets=cu[:2])
    with pytest.raises(RuntimeError, match="slot_mapping must be"):
        gather_kv_cache(kc, kc, slot_mapping=slots.float())
    with pytest.raises(RuntimeError, match="slot_mapping must be"):
        gather_kv_cache(kc, kc, slot_mapping=slots[None])
    with pytest.raises(RuntimeError, match="slot_mapping's length"):
        gather_kv_cache(kc, kc, slot_mapping=slots, total_rows=5)
    with pytest.raises(RuntimeError, match="cu_seqlens must be"):
        gather_kv_cache(kc, kc, cu_seqlens=cu.long(), block_table=bt, total_rows=8)
    with pytest.raises(RuntimeError, match="seq_offsets must be"):
        gather_kv_cache(kc, kc, cu_seqlens=cu, block_table=bt, seq_offsets=torch.zeros(3, dtype=torch.int32), total_rows=8)
    with pytest.raises(RuntimeError, match="block_table must be"):
        gather_kv_cache(kc, kc, cu_seqlens=cu, block_table=bt[:1], total_rows=8)
    with pytest.raises(RuntimeError, match="does not take cache_batch_idx"):
        gather_kv_cache(kc, kc, cu_seqlens=cu, block_table=bt, cache_batch_idx=torch.zeros(2, dtype=torch.int32), total_rows=8)
    with pytest.raises(RuntimeError, match="batch slots"):
        gather_kv_cache(kc[:1], kc[:1], cu_seqlens=cu, total_rows=8)
    with pytest.raises(RuntimeError, match="needs total_rows="):                  # total_rows missing in sequence mode
        gather_kv_cache(kc, kc, cu_seqlens=cu, block_table=bt)
    with pytest.raises(RuntimeError, match="total_rows must be >= 0"):
        gather_kv_cache(kc, kc, cu_seqlens=cu, block_table=bt, total_rows=-1)
    # out=: a pair of [T, Hk, D] tensors of the output dtype that the kernel can write where they lie
    with pytest.raises(RuntimeError, match="must be a pair"):
        gather_kv_cache(kc, kc, slot_mapping=slots, out=out[0])
    with pytest.raises(RuntimeError, match="k_out must be a"):
        gather_kv_cache(kc, kc, slot_mapping=slots, out=(out[0][:7], out[1]))
    with pytest.raises(RuntimeError, match="v_out must be a"):
        gather_kv_cache(kc, kc, slot_mapping=slots, out=(out[0], out[1].bfloat16()))
    with pytest.raises(RuntimeError, match="k_out must be a"):
        gather_kv_cache(kc8, kc8, slot_mapping=slots, dtype=torch.bfloat16, out=out)
    with pytest.raises(RuntimeError, match="never copied"):                       # a non-viewable out: last dimension strided
        t = torch.zeros(8, 64, 2, dtype=torch.float16).transpose(1, 2)
        gather_kv_cache(kc, kc, slot_mapping=slots, out=(t, out[1]))
    with pytest.raises(RuntimeError, match="never copied"):                       # head stride of 68 elements: not whole 16 bytes
        t = torch.zeros(8, 2, 68, dtype=torch.float16)[:, :, :64]
        gather_kv_cache(kc, kc, slot_mapping=slots, out=(out[0], t))
    with pytest.raises(RuntimeError, match="never copied"):                       # base 8 bytes off
        t = torch.zeros(8 * 2 * 64 + 8, dtype=torch.float16)[4:4 + 8 * 2 * 64].view(8, 2, 64)
        gather_kv_cache(kc, kc, slot_mapping=slots, out=(t, out[1]))
    with pytest.raises(RuntimeError, match="one length"):
        move_kv_cache(kc, kc.clone(), slots, slots[:5])
    # everything else in order: the CPU tensor itself is the error
    with pytest.raises(RuntimeError, match="GPU"):
        gather_kv_cache(kc, kc, slot_mapping=slots)
    with pytest.raises(RuntimeError, match="GPU"):
        gather_kv_cache(kc, kc, slot_mapping=slots, out=out)
    with pytest.raises(RuntimeError, match="GPU"):
        gather_kv_cache(kc8, kc8, cu_seqlens=cu, block_table=bt, total_rows=8, dtype=torch.bfloat16, k_descale=0.5, v_descale=0.25)
    with pytest.raises(RuntimeError, match="GPU"):
        move_kv_cache(kc, kc.clone(), slots, slots + 8)


def test_torch_op_schemas_and_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import flash_attn_mi355.torch_ops  # noqa: F401  (registers the ops)
    schema = torch.ops.flash_attn_mi355.kv_gather.default._schema
    assert [a.name for a in schema.arguments if a.alias_info is not None] == []       # functional
    assert len(schema.returns) == 2
    schema = torch.ops.flash_attn_mi355.kv_move.default._schema
    assert [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write] == ["k_cache", "v_cache"]
    assert len(schema.returns) == 0
    with FakeTensorMode():
        kc = torch.empty(20, 16, 2, 64, dtype=torch.float16, device="cuda")
        slots = torch.empty(200, dtype=torch.int64, device="cuda")
        k, v = torch.ops.flash_attn_mi355.kv_gather(kc, kc.clone(), slots, None, None, None, None, 200, torch.float16, 1.0, 1.0)
        assert k.shape == v.shape == (200, 2, 64) and k.dtype == v.dtype == torch.float16 and k.is_contiguous()
        cu = torch.empty(4, dtype=torch.int32, device="cuda")
        bt = torch.empty(3, 9, dtype=torch.int32, device="cuda")
        kc8 = torch.empty(20, 16, 2, 128, dtype=FP8, device="cuda")
        k, v = torch.ops.flash_attn_mi355.kv_gather(kc8, kc8.clone(), None, cu, cu[:3], bt, None, 77, torch.bfloat16, 0.05, 0.04)
        assert k.shape == v.shape == (77, 2, 128) and k.dtype == v.dtype == torch.bfloat16 and k.device == kc8.device
        assert torch.ops.flash_attn_mi355.kv_move(kc, kc.clone(), slots, slots.clone()) is None


def test_the_name_lists_are_what_they_were():
    import flash_attn
    import flash_attn_mi355
    import flash_attn_mi355.torch_ops as T
    assert T.__all__ == ["fwd", "bwd", "varlen_fwd", "varlen_bwd", "fwd_kvcache", "fwd_kvcache_tree", "fwd_out", "varlen_fwd_out",
                         "bwd_out", "merge_states", "rotary", "rotary_", "kv_store"]
    assert hasattr(T, "kv_gather") and hasattr(T, "kv_move")
    for name in ("gather_kv_cache", "move_kv_cache", "kv_gather", "kv_move"):
        assert name not in flash_attn.__all__ and name not in flash_attn_mi355.__all__


# the reference ---------------------------------------------------------------------------------------------------------------
def _rand(shape, dt, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dt)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_reference_inverts_the_store_reference(dt):
    """(a) 16-bit caches: kv_gather_ref of what kv_store_ref stored returns the stored rows bit for bit - sequence mode (paged
    and contiguous) and slot mode; -0 and a NaN payload among the rows"""
    Hk, D, page = 2, 64, 16
    lens, L = [0, 1, 37, 30], [5, 15, 0, 20]
    T = sum(lens)
    cu = [0, 0, 1, 38, 68]
    k, v = _rand((T, Hk, D), dt, 1), _rand((T, Hk, D), dt, 2)
    k[3, 0, 0] = -0.0
    k.view(torch.int16)[5, 1, 7] = 0x7FC1
    bt, nblk, nanp = guard.paged_table([a + b for a, b in zip(lens, L)], page, seed=1)
    for shape, addr in (((nblk, page, Hk, D), dict(block_table=bt)), ((6, 64, Hk, D), dict(cache_batch_idx=[4, 0, 2, 5])),
                        ((6, 64, Hk, D), {})):
        kc, vc = _rand(shape, dt, 3), _rand(shape, dt, 4)
        kc2, vc2 = R.kv_store_ref(k, v, kc, vc, cu_seqlens=cu, cache_seqlens=L, **addr)
        gk, gv = G.kv_gather_ref(kc2, vc2, cu_seqlens=cu, seq_offsets=L, total_rows=T, **addr)
        G.diff_report(gk, k, "k")
        G.diff_report(gv, v, "v")
        assert not G.same_bits(G.kv_gather_ref(kc, vc, cu_seqlens=cu, seq_offsets=L, total_rows=T, **addr)[0], k)
    slots = torch.randperm(nblk * page, generator=torch.Generator().manual_seed(5))[:T]
    kc, vc = _rand((nblk, page, Hk, D), dt, 3), _rand((nblk, page, Hk, D), dt, 4)
    kc2, vc2 = R.kv_store_ref(k, v, kc, vc, slot_mapping=slots)
    gk, gv = G.kv_gather_ref(kc2, vc2, slot_mapping=slots)
    G.diff_report(gk, k, "k by slot")
    G.diff_report(gv, v, "v by slot")


def test_reference_zero_rows():
    """rows that name nothing are +0: slots out of range, positions past the capacity, rows behind cu_seqlens[-1]"""
    kc = torch.full((3, 4, 1, 8), 2.0, dtype=torch.bfloat16)
    gk, gv = G.kv_gather_ref(kc, -kc, slot_mapping=[0, -1, 12, 11, 99])
    assert gk[:, 0, 0].tolist() == [2.0, 0.0, 0.0, 2.0, 0.0] and gv[:, 0, 0].tolist() == [-2.0, 0.0, 0.0, -2.0, 0.0]
    assert gk.view(torch.int16)[1].eq(0).all() and gv.view(torch.int16)[2].eq(0).all()
    gk, _ = G.kv_gather_ref(kc, kc, cu_seqlens=[0, 3, 5], seq_offsets=[2, 0], cache_batch_idx=[2, 0], total_rows=7)
    assert gk[:, 0, 0].tolist() == [2.0, 2.0, 0.0, 2.0, 2.0, 0.0, 0.0]
    assert G.sources(7, (3, 4), cu_seqlens=[0, 3, 5], seq_offsets=[2, 0], cache_batch_idx=[2, 0]) == \
        [(2, 2), (2, 3), None, (0, 0), (0, 1), None, None]


_FINITE = [c for c in range(256) if c not in (0x7F, 0xFF)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_the_round_trip_keeps_every_finite_code(dtype):
    """(b) quantise(dequantise(code, d, dtype), d) == code for all 254 finite e4m3 codes.  The NaN codes are left out (the
    writer's clamp turns NaN into -448); fp16 at 200.0 is left out because 448 x 200 overflows fp16 (65504)"""
    codes = torch.tensor(_FINITE, dtype=torch.uint8).view(FP8)
    assert codes.numel() == 254 and bool(torch.isfinite(codes.float()).all())
    ds = [1.0, 0.0625, 0.05, 0.04, 0.013, 3.7, 1e-3, 100.0] + ([200.0] if dtype == torch.bfloat16 else [])
    for d in ds:
        x = G.dequantise(codes, d, dtype)
        assert x.dtype == dtype and bool(torch.isfinite(x.float()).all()), d
        back = R.quantise(x, d)
        bad = torch.nonzero(back.view(torch.uint8) != codes.view(torch.uint8)).flatten().tolist()
        assert not bad, (d, [hex(_FINITE[i]) for i in bad])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_power_of_two_descales_are_exact(dtype):
    """(c) with power-of-two descales the reference equals code x descale computed in fp64 (both sides exact; other descales are
    not compared: an fp64 product rounds differently in rare cases)"""
    codes = torch.tensor(_FINITE, dtype=torch.uint8).view(FP8)
    for d in (1.0, 0.0625, 0.03125, 2.0 ** -8, 4.0, 64.0):
        got = G.dequantise(codes, d, dtype)
        want = (codes.double() * d).to(dtype)
        assert G.same_bits(got, want), d
        # (4 significant bits, 2^-17 <= |value| <= 28672: exact in fp16 and bf16, nothing was rounded at all)
        assert torch.equal(got.double(), codes.double() * d), d
