"""CPU: fa_qk_norm_rope_store's host side - the C ABI's argument checks on host pointers, the ctypes mirror, the Python-level
argument errors of qk_norm.qk_norm_rope_and_store_kv / qk_rms_norm, the torch.library op's schema and fake implementation.  No
compute calls: nothing here needs a GPU."""
import ctypes
import os
import re

import pytest
import torch

FP8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


def test_library_exports_and_struct_size(lib):
    assert hasattr(lib.lib, "fa_qk_norm_rope_store") and hasattr(lib.lib, "fa_qk_norm_rope_store_params_size")
    assert "fa_qk_norm_rope_store" in lib.EXPORTS and "fa_qk_norm_rope_store_params_size" in lib.EXPORTS
    assert lib.lib.fa_qk_norm_rope_store_params_size() == ctypes.sizeof(lib.FaQkNormRopeStoreParams)


def _header_fields(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "fa_mi355.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        if stmt.strip():
            names = stmt.strip().split(",")
            fields.append(names[0].split()[-1].lstrip("*"))
            fields += [n.strip().lstrip("*") for n in names[1:]]
    return fields


def test_ctypes_mirror_matches_the_header(lib):
    """field names and order of FaQkNormRopeStoreParams are the header's, and the block begins with fa_rope_store_params"""
    fields = _header_fields("fa_qk_norm_rope_store_params")
    assert [f[0] for f in lib.FaQkNormRopeStoreParams._fields_] == fields
    assert fields[0] == "struct_size"
    base = _header_fields("fa_rope_store_params")
    assert fields[:len(base)] == base
    assert fields[len(base):] == ["q_weight", "k_weight", "weight_dtype", "eps", "weight_offset", "reserved1"]
    for name, _ in lib.FaRopeStoreParams._fields_:
        assert getattr(lib.FaQkNormRopeStoreParams, name).offset == getattr(lib.FaRopeStoreParams, name).offset, name
    assert lib.FaQkNormRopeStoreParams.q_weight.offset == ctypes.sizeof(lib.FaRopeStoreParams)
    assert lib.FA_FP32 == 3


# layout of the host buffer behind a valid block: q [8, 4, 64], k, v [8, 2, 64] fp16; q_out, k_out of the same sizes; caches
# [4, 16, 2, 64]; positions, slot_mapping [8] int64; cos / sin [64, 32]; q_weight, k_weight [64] (room for fp32)
_Q = 8 * 4 * 64 * 2
_KV = 8 * 2 * 64 * 2
_CACHE = 4 * 16 * 2 * 64 * 2
_TAB = 64 * 32 * 2
_W = 64 * 4
_OFF = {}
_o = 0
for _n, _sz in (("q", _Q), ("k", _KV), ("v", _KV), ("q_out", _Q), ("k_out", _KV), ("k_cache", _CACHE), ("v_cache", _CACHE),
                ("positions", 64), ("slot_mapping", 64), ("rotary_cos", _TAB), ("rotary_sin", _TAB), ("q_weight", _W),
                ("k_weight", _W)):
    _OFF[_n] = _o
    _o += _sz
_TOTAL = _o + 64


def _block(lib, buf, form):
    """a valid block over host memory.  form: 'store' (q, k, v, caches, out of place), 'inplace' (the same, q_out = q and
    k_out = k), 'rotate' (no caches, no v, no slot_mapping), 'norm' (no caches and no rotation: seqlen_ro 0, no tables)"""
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaQkNormRopeStoreParams()
    s.struct_size = ctypes.sizeof(lib.FaQkNormRopeStoreParams)
    s.q, s.k = base + _OFF["q"], base + _OFF["k"]
    s.q_out, s.k_out = (s.q, s.k) if form == "inplace" else (base + _OFF["q_out"], base + _OFF["k_out"])
    s.q_row_stride = s.qo_row_stride = 4 * 64
    s.k_row_stride = s.ko_row_stride = s.v_row_stride = 2 * 64
    s.q_head_stride = s.qo_head_stride = s.k_head_stride = s.ko_head_stride = s.v_head_stride = 64
    if form != "norm":
        s.positions = base + _OFF["positions"]
        s.rotary_cos, s.rotary_sin = base + _OFF["rotary_cos"], base + _OFF["rotary_sin"]
        s.rotary_dim, s.seqlen_ro = 64, 64
    s.total_rows, s.nheads_q, s.nheads_k, s.head_dim = 8, 4, 2, 64
    s.dtype = s.cache_dtype = s.weight_dtype = lib.FA_FP16
    s.q_weight, s.k_weight = base + _OFF["q_weight"], base + _OFF["k_weight"]
    s.eps = 1e-6
    if form in ("store", "inplace"):
        s.v = base + _OFF["v"]
        s.k_cache, s.v_cache = base + _OFF["k_cache"], base + _OFF["v_cache"]
        s.kc_batch_stride = s.vc_batch_stride = 16 * 2 * 64
        s.kc_row_stride = s.vc_row_stride = 2 * 64
        s.kc_head_stride = s.vc_head_stride = 64
        s.num_blocks, s.page_block_size = 4, 16
        s.slot_mapping = base + _OFF["slot_mapping"]
    return s, base


def test_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_qk_norm_rope_store fires before any device work"""
    buf = (ctypes.c_char * _TOTAL)()
    at = lambda name, add=0: (lambda b: b + _OFF[name] + add)      # noqa: E731

    def bad(match, form="store", **kw):
        s, base = _block(lib, buf, form)
        for k, v in kw.items():
            setattr(s, k, v(base) if callable(v) else v)
        with pytest.raises(RuntimeError, match=match) as e:
            lib.call_qk_norm_rope_store(s, 0)
        assert "(-1)" in str(e.value)                      # FA_ERR_INVALID_ARGUMENT
        assert "qk_norm_rope_store" in str(e.value)

    for form in ("store", "inplace", "rotate", "norm"):
        bad("struct_size", form, struct_size=8)
        bad("struct_size", form, struct_size=ctypes.sizeof(lib.FaRopeStoreParams))
        bad("must not be NULL", form, k=None)
        bad("q without q_out", form, q_out=None)
        bad("q_out without q", form, q=None)
        bad("fp16 or bf16", form, dtype=7, weight_dtype=lib.FA_FP32)
        bad("multiple of 8", form, head_dim=60, rotary_dim=32)
        bad("<= 256", form, head_dim=264)
        for name in ("total_rows", "nheads_q", "nheads_k", "head_dim", "seqlen_ro", "num_blocks"):
            bad("non-negative", form, **{name: -1})
        for name in ("q_row_stride", "q_head_stride", "k_row_stride", "k_head_stride", "v_row_stride", "v_head_stride",
                     "qo_row_stride", "qo_head_stride", "ko_row_stride", "ko_head_stride", "kc_batch_stride", "kc_row_stride",
                     "kc_head_stride", "vc_batch_stride", "vc_row_stride", "vc_head_stride"):
            bad("strides must be non-negative", form, **{name: -64})
        bad("q / k / v / q_out / k_out base", form, k=at("k", 8), k_out=at("k_out", 0))
        bad("q / k / v / q_out / k_out base", form, q_out=at("q_out", 8))
        for name in ("q_row_stride", "k_head_stride", "qo_head_stride", "ko_row_stride"):
            bad("q / k / v / q_out / k_out base", form, **{name: 2 * 64 + 4})
        for name in ("k_descale", "v_descale"):
            bad("descales", form, **{name: -0.5})
            bad("descales", form, **{name: float("nan")})
        # the norm's own fields
        bad("weight_dtype", form, weight_dtype=lib.FA_BF16)
        bad("weight_dtype", form, weight_dtype=lib.FA_FP8_E4M3)
        bad("weight_dtype", form, weight_dtype=9)
        bad("weight_dtype", form, weight_dtype=lib.FA_BF16, q_weight=None)
        bad("16-byte aligned", form, q_weight=at("q_weight", 8))
        bad("16-byte aligned", form, k_weight=at("k_weight", 2))
        bad("eps", form, eps=-1e-6)
        bad("eps", form, eps=float("inf"))
        bad("eps", form, eps=float("nan"))
        bad("weight_offset", form, weight_offset=float("inf"))
        bad("weight_offset", form, weight_offset=float("nan"))
    for form in ("store", "inplace", "rotate"):
        # with a table (seqlen_ro > 0) the rotation's pointers and rotary_dim are checked as in fa_rope_store
        for name in ("positions", "rotary_cos", "rotary_sin"):
            bad("NULL only where seqlen_ro == 0", form, **{name: None})
        bad("divisible by 16", form, rotary_dim=0)
        bad("divisible by 16", form, rotary_dim=24)
        bad("<= head_dim", form, rotary_dim=80)
        bad("8-byte", form, positions=at("positions", 4))
        bad("16-byte aligned", form, rotary_cos=at("rotary_cos", 8))
    for form in ("store", "inplace"):
        bad("go together", form, k_cache=None)
        bad("go together", form, v_cache=None)
        bad("caches need v and slot_mapping", form, v=None)
        bad("caches need v and slot_mapping", form, slot_mapping=None)
        bad("cache dtype", form, cache_dtype=lib.FA_BF16)
        bad("page_block_size", form, page_block_size=0)
        bad("multiples of 16 bytes", form, k_cache=at("k_cache", 8))
        bad("multiples of 8 bytes", form, cache_dtype=lib.FA_FP8_E4M3, v_cache=at("v_cache", 4))
        bad("8-byte", form, slot_mapping=at("slot_mapping", 4))
    for form in ("rotate", "norm"):
        bad("need caches", form, v=at("v"))
        bad("need caches", form, slot_mapping=at("slot_mapping"))
        bad("needs q or k_out", form, q=None, q_out=None, k_out=None)
    bad("q_out shares q's base", "inplace", qo_row_stride=8 * 64)
    bad("k_out shares k's base", "inplace", ko_head_stride=128)
    for form in ("store", "rotate", "norm"):
        bad("q_out overlaps q", form, q_out=at("q", 16))
        bad("k_out overlaps k", form, k_out=at("k", 128))
        bad("q_out overlaps q_weight", form, q_out=at("q_weight", 0))
        bad("k_out overlaps k_weight", form, k_out=at("k_weight", 0))
        bad("k_out overlaps q_weight", form, k_out=at("q_weight", 256 - 16), weight_dtype=lib.FA_FP32)
    bad("k_out overlaps rotary_cos", "rotate", k_out=at("rotary_cos", 32))
    bad("q_out overlaps v_cache", "store", q_out=at("v_cache", 0))
    with pytest.raises(RuntimeError, match="must not be NULL"):
        lib.lib.fa_qk_norm_rope_store.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        try:
            if lib.lib.fa_qk_norm_rope_store(None, None) != 0:
                raise RuntimeError(lib.lib.fa_last_error().decode())
        finally:
            lib.lib.fa_qk_norm_rope_store.argtypes = [ctypes.POINTER(lib.FaQkNormRopeStoreParams), ctypes.c_void_p]


def test_empty_problems_are_ok_without_launch(lib):
    buf = (ctypes.c_char * _TOTAL)()
    for form in ("store", "inplace", "rotate", "norm"):
        for kw in ({"total_rows": 0}, {"nheads_q": 0, "nheads_k": 0}, {"total_rows": 0, "nheads_k": 0},
                   {"total_rows": 0, "q_weight": None, "k_weight": None, "weight_dtype": 9},
                   {"total_rows": 0, "weight_dtype": lib.FA_FP32, "weight_offset": 1.0, "eps": 0.0}):
            s, base = _block(lib, buf, form)
            for k, v in kw.items():
                setattr(s, k, v)
            lib.call_qk_norm_rope_store(s, 0)              # FA_OK: nothing is launched (there is no device here)
    # q == NULL counts as no q heads; without a table rotary_dim and the table pointers are not read
    s, base = _block(lib, buf, "store")
    s.q = s.q_out = None
    s.nheads_k = 0
    lib.call_qk_norm_rope_store(s, 0)
    s, base = _block(lib, buf, "norm")
    s.total_rows, s.rotary_dim, s.positions = 0, 24, base + _OFF["positions"] + 4
    lib.call_qk_norm_rope_store(s, 0)


def test_python_argument_errors_on_cpu_tensors():
    from flash_attn_mi355.qk_norm import qk_norm_rope_and_store_kv as f, qk_rms_norm as n
    q = torch.zeros(8, 4, 64, dtype=torch.float16)
    k = torch.zeros(8, 2, 64, dtype=torch.float16)
    kc = torch.zeros(4, 16, 2, 64, dtype=torch.float16)
    pos, slots = torch.arange(8), torch.arange(8)
    cos = torch.zeros(32, 32, dtype=torch.float16)
    w = torch.ones(64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="fp16 or bf16"):
        f(q.float(), k.float(), k.float(), pos, cos, cos, kc, kc, slots)
    with pytest.raises(RuntimeError, match=r"k must be \(total_rows"):
        f(q, k[None], k, pos, cos, cos, kc, kc, slots)
    with pytest.raises(RuntimeError, match="q must have k's dtype"):
        f(q.bfloat16(), k, k, pos, cos, cos, kc, kc, slots)
    with pytest.raises(RuntimeError, match=r"q must be \(total_rows"):
        f(q[:7], k, k, pos, cos, cos, kc, kc, slots)
    k60, kc60 = torch.zeros(8, 2, 60, dtype=torch.float16), torch.zeros(4, 16, 2, 60, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        f(None, k60, k60, pos, cos[:, :16], cos[:, :16], kc60, kc60, slots)
    with pytest.raises(RuntimeError, match="must both be given"):
        f(q, k, k, pos, cos, cos, kc, None, slots)
    with pytest.raises(RuntimeError, match="caches need v and slot_mapping"):
        f(q, k, None, pos, cos, cos, kc, kc, slots)
    with pytest.raises(RuntimeError, match="v must have k's dtype"):
        f(q, k, k.bfloat16(), pos, cos, cos, kc, kc, slots)
    with pytest.raises(RuntimeError, match="same shape"):
        f(q, k, k[:, :1], pos, cos, cos, kc, kc, slots)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        f(q, k, k, pos, cos, cos, kc, kc.to(FP8), slots)
    with pytest.raises(RuntimeError, match="4-D shape"):
        f(q, k, k, pos, cos, cos, kc, kc[:3], slots)
    with pytest.raises(RuntimeError, match="last two dimensions"):
        f(q, k, k, pos, cos, cos, kc[:, :, :1], kc[:, :, :1], slots)
    with pytest.raises(RuntimeError, match="contiguous last dimension"):
        t = torch.zeros(4, 16, 64, 2, dtype=torch.float16).transpose(2, 3)
        f(q, k, k, pos, cos, cos, t, t, slots)
    with pytest.raises(RuntimeError, match="go with k_cache"):
        f(q, k, k, pos, cos, cos)
    with pytest.raises(RuntimeError, match="nothing to do"):
        f(None, k, None, pos, cos, cos, k_out=False)
    with pytest.raises(RuntimeError, match="float8_e4m3fn cache"):
        f(q, k, k, pos, cos, cos, kc, kc, slots, k_descale=0.5)
    with pytest.raises(RuntimeError, match="go together"):
        f(q, k, None, None, cos, cos)
    with pytest.raises(RuntimeError, match="go together"):
        f(q, k, None, pos, cos, None)
    with pytest.raises(RuntimeError, match="k's dtype"):
        f(q, k, k, pos, cos.float(), cos.float(), kc, kc, slots)
    with pytest.raises(RuntimeError, match="same shape"):
        f(q, k, k, pos, cos, cos[:16], kc, kc, slots)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        f(q, k, k, pos, cos[:, :12], cos[:, :12], kc, kc, slots)
    with pytest.raises(RuntimeError, match="<= headdim"):
        big = torch.zeros(32, 40, dtype=torch.float16)
        f(q, k, k, pos, big, big, kc, kc, slots)
    with pytest.raises(RuntimeError, match="positions must be"):
        f(q, k, k, pos[:5], cos, cos, kc, kc, slots)
    with pytest.raises(RuntimeError, match="slot_mapping must be"):
        f(q, k, k, pos, cos, cos, kc, kc, slots.float())
    # the norm's own arguments
    with pytest.raises(RuntimeError, match="q_weight must have k's dtype"):
        f(q, k, k, pos, cos, cos, kc, kc, slots, q_weight=w.bfloat16())
    with pytest.raises(RuntimeError, match="k_weight must have k's dtype"):
        n(q, k, None, w.double())
    with pytest.raises(RuntimeError, match=r"k_weight must have shape \(headdim,\)"):
        n(q, k, w, w[:32])
    with pytest.raises(RuntimeError, match=r"q_weight must have shape \(headdim,\)"):
        n(q, k, w[None], w)
    with pytest.raises(RuntimeError, match="same dtype"):
        n(q, k, w, w.float())
    with pytest.raises(RuntimeError, match="q_weight without q"):
        n(None, k, w, w)
    with pytest.raises(RuntimeError, match="eps must be finite"):
        n(q, k, w, w, eps=-1.0)
    with pytest.raises(RuntimeError, match="eps must be finite"):
        n(q, k, w, w, eps=float("nan"))
    with pytest.raises(RuntimeError, match="weight_offset must be finite"):
        n(q, k, w, w, weight_offset=float("inf"))
    # everything else in order: the CPU tensor itself is the error
    with pytest.raises(RuntimeError, match="GPU"):
        f(q, k, k, pos, cos, cos, kc, kc, slots, q_weight=w, k_weight=w)
    with pytest.raises(RuntimeError, match="GPU"):
        f(None, k, k, pos.int(), cos, cos, kc.to(FP8), kc.to(FP8), slots.int(), k_weight=w.float(), weight_offset=1.0,
          interleaved=True, inplace=False, k_out=False, k_descale=0.5, v_descale=0.25)
    with pytest.raises(RuntimeError, match="GPU"):
        n(q, k, w, None)
    with pytest.raises(RuntimeError, match="GPU"):
        f(q, k, k, None, None, None, kc, kc, slots, q_weight=w.float(), k_weight=w.float())


def test_torch_op_schema_and_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import flash_attn_mi355.torch_ops as T
    schema = torch.ops.flash_attn_mi355.qk_norm_rope_store_.default._schema
    mutated = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
    assert mutated == ["q", "k", "k_cache", "v_cache"]
    assert len(schema.returns) == 0
    assert [a.name for a in schema.arguments] == ["q", "k", "v", "positions", "rotary_cos", "rotary_sin", "k_cache", "v_cache",
                                                  "slot_mapping", "q_weight", "k_weight", "eps", "weight_offset", "interleaved",
                                                  "k_descale", "v_descale"]
    with FakeTensorMode():
        qkv = torch.empty(200, 8, 64, dtype=torch.bfloat16, device="cuda")
        q, k, v = qkv[:, :4], qkv[:, 4:6], qkv[:, 6:8]
        kc = torch.empty(20, 16, 2, 64, dtype=torch.bfloat16, device="cuda")
        ids = torch.empty(200, dtype=torch.int64, device="cuda")
        cos = torch.empty(64, 32, dtype=torch.bfloat16, device="cuda")
        w = torch.empty(64, dtype=torch.float32, device="cuda")
        op = torch.ops.flash_attn_mi355.qk_norm_rope_store_
        assert op(q, k, v, ids, cos, cos, kc, kc.clone(), ids, w, w, 1e-6, 0.0, False, 1.0, 1.0) is None
        kc8 = torch.empty(20, 16, 2, 64, dtype=FP8, device="cuda")
        assert op(q, k, v, ids, cos, cos, kc8, kc8.clone(), ids, None, w, 1e-5, 1.0, True, 0.05, 0.04) is None
    assert "qk_norm_rope_store_" not in T.__all__          # registered, reached through torch.ops only


def test_public_name_lists_are_unchanged_and_abi_version(lib):
    import flash_attn
    import flash_attn_mi355
    for name in ("qk_norm_rope_and_store_kv", "qk_rms_norm", "qk_norm"):
        assert name not in flash_attn.__all__ and name not in flash_attn_mi355.__all__
    assert lib.FA_ABI_VERSION == 4 and lib.lib.fa_abi_version() == 4
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert re.search(r"#define FA_ABI_VERSION 4\b", open(os.path.join(root, "include", "fa_mi355.h")).read())
