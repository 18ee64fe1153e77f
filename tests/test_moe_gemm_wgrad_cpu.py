"""CPU: the host side of fa_moe_gemm_wgrad and moe_linear - the C ABI's block, its limits on host pointers, the launch plan, the
Python wrapper's argument errors, the torch.library schemas and fake implementations, the fp64 yardstick of the GPU tests
(moe_gemm_wgrad_ref.py) told apart from the wrong variants it must catch, and the exactness of the witness data.  Nothing here
needs a GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import moe_gemm_ref as G
import moe_gemm_wgrad_ref as W
import moe_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "fa_mi355.h")).read(), flags=re.S)


def test_library_exports_struct_size_and_mirror(lib):
    for name in ("fa_moe_gemm_wgrad", "fa_moe_gemm_wgrad_params_size", "fa_moe_gemm_wgrad_plan"):
        assert hasattr(lib.lib, name) and name in lib.EXPORTS
    assert lib.lib.fa_moe_gemm_wgrad_params_size() == ctypes.sizeof(lib.FaMoeGemmWgradParams)
    rows = {e: (s, q) for e, s, q in lib.ROW_OPS}
    assert rows["fa_moe_gemm_wgrad"] == (lib.FaMoeGemmWgradParams, None) and callable(lib.call_moe_gemm_wgrad)
    assert lib.FA_ABI_VERSION == 4 and lib.lib.fa_abi_version() == 4            # additive: the ABI version stays
    body = re.search(r"typedef struct fa_moe_gemm_wgrad_params \{(.*?)\} fa_moe_gemm_wgrad_params;", _header(), flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        if stmt.strip():
            names = stmt.strip().split(",")
            fields.append(names[0].split()[-1].lstrip("*"))
            fields += [n.strip().lstrip("*") for n in names[1:]]
    fields = [f.split("[")[0] for f in fields]
    assert [f[0] for f in lib.FaMoeGemmWgradParams._fields_] == fields
    assert fields[0] == "struct_size" and fields[-1] == "reserved"
    import build
    assert "fa_moe_gemm_wgrad.hip" in build.SOURCES


def test_no_spill_no_scratch_and_the_budget_is_unchanged(lib):
    import build
    budget = json.load(open(os.path.join(build.CSRC, "spill_budget.json")))["spill"]
    res = json.load(open(build.RESOURCES))
    mine = [n for n in res if "moe_gemm_wgrad_kernel" in n or "moe_dbias_kernel" in n]
    assert len(mine) == 16 + 2                              # 2 dtypes x 2 layouts x plain / gather x 16-bit / fp32 dw; dbias per dtype
    assert not any("wgrad" in n or "dbias" in n for n in budget)
    assert all(res[n]["spill"] == 0 and res[n]["scratch"] == 0 for n in mine)


def _block(lib, base, **kw):
    s = lib.FaMoeGemmWgradParams()
    s.struct_size = ctypes.sizeof(s)
    s.dy, s.x, s.expert_offsets, s.dw = base, base + 0x10000, base + 0x30000, base + 0x40000
    s.dy_row_stride, s.x_row_stride, s.dw_expert_stride = 32, 64, 64 * 32
    s.rows, s.num_experts, s.n, s.k = 16, 4, 32, 64
    s.dtype = s.dw_dtype = s.dbias_dtype = lib.FA_BF16
    s.layout = lib.FA_MOE_W_NK
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_limits_and_stride_rules_fire_before_any_device_work(lib):
    """FA_ERR_UNSUPPORTED (-2) for the limits, FA_ERR_INVALID_ARGUMENT (-1) for the argument rules, each naming its argument"""
    buf = (ctypes.c_char * (0x80000 + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15

    def bad(match, code="(-1)", **kw):
        with pytest.raises(RuntimeError, match=match) as e:
            lib.call_moe_gemm_wgrad(_block(lib, base, **kw), 0)
        assert code in str(e.value) and "moe_gemm_wgrad" in str(e.value), str(e.value)
    bad("struct_size", struct_size=8)
    bad("reserved", reserved=(ctypes.c_int64 * 4)(0, 0, 1, 0))
    bad("reserved", reserved0=1)
    bad("num_experts", "(-2)", num_experts=1)
    bad("num_experts", "(-2)", num_experts=513)
    bad(": n must", "(-2)", n=36)
    bad(": n must", "(-2)", n=65544)
    bad(": k must", "(-2)", k=4)
    bad(": k must", "(-2)", k=32776)
    bad("rows", rows=-1)
    bad("rows", "(-2)", rows=2 ** 31)
    bad("dtype", dtype=lib.FA_FP32)
    bad("layout", layout=2)
    bad("dw_dtype", "(-2)", dw_dtype=lib.FA_FP16)
    bad("accumulate", "(-2)", accumulate=1)
    bad("dbias_dtype", "(-2)", dbias=base + 0x60000, dbias_dtype=lib.FA_FP8_E4M3)
    bad("dw_expert_stride", "(-2)", dw_expert_stride=64 * 32 - 8)
    bad("dw_expert_stride", "(-2)", dw_expert_stride=64 * 32 + 4)
    bad("dy_row_stride", "(-2)", dy_row_stride=36)
    bad("dy_row_stride", "(-2)", dy_row_stride=2 ** 22 + 8)
    bad("x_row_stride", "(-2)", x_row_stride=68)
    bad("dy_row_stride must be at least n", dy_row_stride=24)
    bad("x_row_stride must be at least k", x_row_stride=56)
    bad("must not be NULL", dy=None)
    bad("must not be NULL", x=None)
    bad("must not be NULL", expert_offsets=None)
    bad("16-byte aligned", dw=base + 0x40000 + 8)
    bad("16-byte aligned", dy=base + 2)
    bad("aligned to their elements", expert_offsets=base + 0x30000 + 2)
    bad("top_k", "(-2)", sorted_slot=base + 0x38000, tokens=4, top_k=0)
    bad("top_k", "(-2)", sorted_slot=base + 0x38000, tokens=4, top_k=17)
    bad("2\\^31", "(-2)", sorted_slot=base + 0x38000, tokens=2 ** 30, top_k=2)
    bad("overlaps", dw=base + 0x10000)
    bad("overlaps", dw=base)
    bad("overlaps", dbias=base + 0x40000)
    # nothing to compute launches nothing and needs no device: FA_OK on any machine
    lib.call_moe_gemm_wgrad(_block(lib, base, dw=None), 0)
    # fp32 dw with accumulate passes the argument checks: the same call without dw reaches FA_OK
    lib.call_moe_gemm_wgrad(_block(lib, base, dw=None, dw_dtype=lib.FA_FP32, accumulate=1), 0)
    with pytest.raises(RuntimeError, match=r"\(-2\).*num_experts"):
        lib.moe_gemm_wgrad_plan(32, 64, 1, lib.FA_MOE_W_NK, lib.FA_BF16)
    with pytest.raises(RuntimeError, match=r"\(-2\).*k must"):
        lib.moe_gemm_wgrad_plan(32, 12, 8, lib.FA_MOE_W_NK, lib.FA_BF16)


def test_the_plan_is_a_function_of_the_shapes(lib):
    from flash_attn_mi355 import moe
    for N, K, E in ((8, 8, 2), (40, 264, 7), (264, 264, 7), (2880, 40, 7), (40, 48, 512), (65536, 32768, 512), (128, 136, 3)):
        for layout in ("nk", "kn"):
            for dt in (torch.bfloat16, torch.float16):
                assert moe.moe_gemm_wgrad_plan(N, K, E, w_layout=layout, dtype=dt) == (128, 128, 64, -(-N // 128), -(-K // 128), E)
    assert moe.moe_gemm_wgrad_plan(64, 32, 8) == lib.moe_gemm_wgrad_plan(64, 32, 8, lib.FA_MOE_W_NK, lib.FA_BF16)
    with pytest.raises(RuntimeError, match="w_layout"):
        moe.moe_gemm_wgrad_plan(64, 32, 8, w_layout="xx")
    with pytest.raises(RuntimeError, match="dtype"):
        moe.moe_gemm_wgrad_plan(64, 32, 8, dtype=torch.float32)


def test_wrapper_rejects_by_name_without_a_device(lib):
    from flash_attn_mi355 import moe
    bf = torch.bfloat16
    dy, x, off = torch.zeros(16, 32, dtype=bf), torch.zeros(16, 64, dtype=bf), torch.zeros(5, dtype=torch.int32)

    def bad(match, *a, **kw):
        with pytest.raises(RuntimeError, match=match):
            moe.moe_gemm_wgrad(*a, **kw)
    bad("w_layout", dy, x, off, w_layout="kn ")
    bad("dy must be fp16 or bf16", dy.float(), x, off)
    bad(r"dy must be \[rows, N\]", dy[0], x, off)
    bad("x must be a", dy, x.half(), off)
    bad("x must have dy's", dy, x[:15], off)
    bad("num_experts", dy, x, off[:2])
    bad("num_experts", dy, x, torch.zeros(514, dtype=torch.int32))
    bad("K must be a multiple of 8", dy, x[:, :60], off)
    bad("N must be a multiple of 8", dy[:, :28], x, off)
    bad("expert_offsets", dy, x, off.long())
    bad("go together", dy, x, off, top_k=2)                                   # sorted_slot without top_k and the reverse
    bad("go together", dy, x, off, sorted_slot=torch.zeros(16, dtype=torch.int32))
    bad("k must be", dy, x, off, sorted_slot=torch.zeros(16, dtype=torch.int32), top_k=17)
    bad("sorted_slot must be an int32", dy, x, off, sorted_slot=torch.zeros(16, dtype=torch.int64), top_k=2)
    bad("sorted_slot must be an int32", dy, x, off, sorted_slot=torch.zeros(15, dtype=torch.int32), top_k=2)
    bad("dw_dtype", dy, x, off, dw_dtype=torch.float16)
    bad("dbias_dtype", dy, x, off, need_dbias=True, dbias_dtype=torch.float64)
    bad("accumulate needs an fp32 dw", dy, x, off, accumulate=True, out=torch.zeros(4, 32, 64, dtype=bf))
    bad("accumulate needs an fp32 dw", dy, x, off, accumulate=True)
    bad("accumulate needs out", dy, x, off, accumulate=True, dw_dtype=torch.float32)
    bad("out must be", dy, x, off, out=torch.zeros(4, 64, 32, dtype=bf))
    bad("out must be", dy, x, off, out=torch.zeros(4, 32, 64), dw_dtype=bf)
    bad("expert stride", dy, x, off, out=torch.zeros(4, 32, 72, dtype=bf)[:, :, :64])
    bad("expert stride", dy, x, off, out=torch.zeros(4, 32 * 64 + 4, dtype=bf)[:, :32 * 64].view(4, 32, 64))
    bad("dy must have a contiguous last", torch.zeros(32, 16, dtype=bf).t(), x, off)
    bad("dy must be 16-byte aligned", torch.zeros(16, 40, dtype=bf)[:, 4:36], x, off)
    bad("x must be 16-byte aligned", dy, torch.zeros(16, 68, dtype=bf)[:, :64], off)
    bad("no CPU fallback|must be on", dy, x, off)                              # every check passed: only the device is missing
    bad("no CPU fallback|must be on", dy, x, off, w_layout="kn", dw_dtype=torch.float32, out=torch.zeros(4, 64, 32), accumulate=True,
        need_dbias=True, dbias_dtype=torch.float32)
    assert "moe_gemm_wgrad" not in getattr(moe, "__all__", ()) and "moe_linear" not in getattr(moe, "__all__", ())


def test_moe_linear_on_cpu_and_moe_gemm_still_has_no_autograd(lib):
    from flash_attn_mi355 import moe
    bf = torch.bfloat16
    x, w, off = torch.zeros(16, 64, dtype=bf), torch.zeros(4, 32, 64, dtype=bf), torch.zeros(5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        moe.moe_linear(x.clone().requires_grad_(), w.clone().requires_grad_(), off)
    with pytest.raises(RuntimeError, match="w_layout"):
        moe.moe_linear(x, w, off, w_layout="xx")
    with pytest.raises(RuntimeError, match="go together"):
        moe.moe_linear(x, w, off, top_k=2)
    with pytest.raises(RuntimeError, match="pos goes with sorted_slot"):
        moe.moe_linear(x, w, off, pos=torch.zeros(8, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="x requires grad"):
        moe.moe_gemm(x.clone().requires_grad_(), w, off)
    with pytest.raises(RuntimeError, match="w requires grad"):
        moe.moe_gemm(x, w.clone().requires_grad_(), off)
    with pytest.raises(RuntimeError, match="bias requires grad"):
        moe.moe_gemm(x, w, off, bias=torch.zeros(4, 32, dtype=bf, requires_grad=True))


def test_torch_op_schemas_and_fakes(lib):
    import flash_attn_mi355.torch_ops as ops
    ns = torch.ops.flash_attn_mi355
    sw, sl = str(ns.moe_gemm_wgrad.default._schema), str(ns.moe_linear.default._schema)
    assert "Tensor dy, Tensor x, Tensor expert_offsets, str w_layout, Tensor? sorted_slot" in sw and "-> (Tensor, Tensor)" in sw
    assert "bool need_dw, bool need_dbias, bool dw_fp32, bool dbias_fp32" in sw
    assert "Tensor x, Tensor w, Tensor expert_offsets, str w_layout, Tensor? bias, Tensor? sorted_slot" in sl and "Tensor? pos) -> Tensor" in sl
    assert not ns.moe_gemm_wgrad.default._schema.is_mutable and not ns.moe_linear.default._schema.is_mutable
    assert not any(n in getattr(ops, "__all__", ()) for n in ("moe_gemm_wgrad", "moe_linear"))
    bf = torch.bfloat16
    dy, x = torch.empty(70, 24, dtype=bf, device="meta"), torch.empty(70, 64, dtype=bf, device="meta")
    xt, ss = torch.empty(5, 64, dtype=bf, device="meta"), torch.empty(70, dtype=torch.int32, device="meta")
    off = torch.empty(9, dtype=torch.int32, device="meta")
    dw, db = ns.moe_gemm_wgrad(dy, x, off, "nk", None, None, True, True, False, True)
    assert dw.shape == (8, 24, 64) and dw.dtype == bf and db.shape == (8, 24) and db.dtype == torch.float32
    dw, db = ns.moe_gemm_wgrad(dy, xt, off, "kn", ss, 2, True, False, True, False)
    assert dw.shape == (8, 64, 24) and dw.dtype == torch.float32 and db.shape == (0,) and db.dtype == bf
    dw, db = ns.moe_gemm_wgrad(dy, x, off, "nk", None, None, False, True, False, False)
    assert dw.shape == (0,) and db.shape == (8, 24)
    nk, kn = torch.empty(8, 24, 64, dtype=bf, device="meta"), torch.empty(8, 64, 24, dtype=bf, device="meta")
    assert ns.moe_linear(x, nk, off, "nk", None, None, None, None).shape == (70, 24)
    out = ns.moe_linear(xt, kn, off, "kn", torch.empty(8, 24, device="meta"), ss, 2, torch.empty(5, 2, dtype=torch.int32, device="meta"))
    assert out.shape == (70, 24) and out.dtype == bf


# the yardstick ---------------------------------------------------------------------------------------------------------------
def _case(N=40, K=264, seed=3, head=5, tail=5):
    """W.PATTERN behind `head` unowned rows (every segment starts at an unaligned row) and before `tail` rows behind offsets[E]"""
    off = W.offsets_of(W.PATTERN) + head
    dy, x = W.witness(int(off[-1]) + tail, N, K, seed)
    return dy, x, off


def test_reference_is_the_plain_definition():
    dy, x, off = _case()
    for layout in ("nk", "kn"):
        dw, db = W.wgrad_ref(dy, x, off, layout=layout)
        assert dw.shape == ((9, 40, 264) if layout == "nk" else (9, 264, 40)) and db.shape == (9, 40)
        for e in range(len(W.PATTERN)):
            de, xe = torch.from_numpy(dy[off[e]:off[e + 1]]), torch.from_numpy(x[off[e]:off[e + 1]])
            want = de.t() @ xe
            assert (dw[e] == (want if layout == "nk" else want.t()).numpy()).all()
            assert (db[e] == de.sum(0).numpy()).all()
        assert (dw[0] == 0).all() and (db[0] == 0).all()                      # the empty expert
    old = np.arange(9 * 40 * 264, dtype=np.float64).reshape(9, 40, 264)
    acc, _ = W.wgrad_ref(dy, x, off, old=old)
    assert (acc == W.wgrad_ref(dy, x, off)[0] + old).all() and (acc[0] == old[0]).all()
    # clamping: offsets beyond the rows and below zero own what is left inside [0, rows]
    bad = np.array([-5, 3, 10 ** 6], dtype=np.int64)
    assert W.segments(bad, 20) == [(0, 3), (3, 20)]
    assert W.segments(np.array([4, 2, 9]), 20) == [(4, 4), (2, 9)]            # a decreasing pair: empty


@pytest.mark.parametrize("out_name", ["bfloat16", "float16", "float32"])
def test_witness_data_tell_the_wrong_variants_apart(out_name):
    """each wrong variant changes bits of the expected dw in an expert the right one owns, so a kernel with that defect fails the
    bit-for-bit comparison"""
    dy, x, off = _case()
    assert W.witness_is_exact(dy, x, off, out_name)
    for layout in ("nk", "kn"):
        good, good_b = W.expected(dy, x, off, out_name, layout=layout)
        lens = W.seg_lengths(off, len(dy))
        for variant, hit in (("read_past_end", lens % 16 != 0), ("drop_row_tail", lens % 64 != 0), ("start_rounded_down", lens > 0)):
            wrong, wrong_b = W.expected(dy, x, off, out_name, layout=layout, variant=variant)
            differs = (wrong != good).reshape(len(lens), -1).any(1)
            assert (differs == hit).all(), (variant, differs, hit)
            assert ((wrong_b != good_b).any(1) == hit).all(), variant
    # "kn" written as "nk": a square expert, both readings have a shape
    dy2, x2, off2 = _case(N=40, K=40)
    g2, _ = W.expected(dy2, x2, off2, out_name, layout="kn")
    w2, _ = W.expected(dy2, x2, off2, out_name, layout="kn", variant="kn_as_nk")
    assert w2.shape == g2.shape and (w2[1:] != g2[1:]).mean() > 0.5
    # accumulate ignored
    if out_name == "float32":
        old = np.random.default_rng(1).integers(-50, 50, size=(9, 40, 264)).astype(np.float64)
        assert W.witness_is_exact(dy, x, off, out_name, old=old)
        g3, _ = W.expected(dy, x, off, out_name, old=old)
        w3, _ = W.expected(dy, x, off, out_name, old=old, variant="no_accumulate")
        assert (g3 != w3).mean() > 0.9 and (g3[0] == old[0]).all()
    # a padding slot read as token 0: the padding rows stop being rows of +0
    rng = np.random.default_rng(9)
    ids = np.stack([rng.permutation(7)[:2] for _ in range(20)]).astype(np.int32)
    ss, pos, so = R.sort_ref(ids, 7, align=16)
    dyg, xg = W.witness(len(ss), 40, 264, 11)
    xg = xg[:20]
    assert (ss[:so[-1]] < 0).any()
    good, _ = W.expected(dyg, W.gather_ref(xg, ss, 2), so, out_name)
    wrong, _ = W.expected(dyg, W.gather_ref(xg, ss, 2, variant="pad_as_token0"), so, out_name)
    padded = np.array([(ss[so[e]:so[e + 1]] < 0).any() for e in range(7)])
    assert padded.any() and ((wrong != good).reshape(7, -1).any(1) == padded).all()


def test_the_one_rounding_shows_in_the_witness_data():
    """the positive columns carry sums past the integers the 16-bit types hold exactly: 256 in bf16 at L = 129, 2048 in fp16 at
    L = 2880 (dbias, whose sums grow like 2 L: at L = 2880 in both)"""
    dy, x, off = _case()
    dw, db = W.wgrad_ref(dy, x, off)
    assert dw[8, :4, :4].min() > 256 and (W.round_out(dw, "bfloat16") != dw).any()
    off2 = np.array([3, 3, 2883], dtype=np.int32)
    dy2, x2 = W.witness(2890, 8, 8, 5)
    assert W.witness_is_exact(dy2, x2, off2, "float16")
    dw2, db2 = W.wgrad_ref(dy2, x2, off2)
    assert dw2[1, :4, :4].min() > 2048 and (W.round_out(dw2, "float16") != dw2).any() and np.abs(dw2).max() < 65504
    assert db2[1, :4].min() > 2048 and all((W.round_out(db2, t) != db2).any() for t in ("bfloat16", "float16"))


def test_witness_construction_is_exact():
    """integers exact in both io dtypes; fp32 accumulation in two very different orders gives the fp64 answer"""
    dy, x, off = _case(N=16, K=24)
    for dt in (torch.bfloat16, torch.float16):
        for t in (dy, x):
            assert (torch.from_numpy(t).to(dt).double().numpy() == t).all()
    ref, refb = W.wgrad_ref(dy, x, off)
    d32, x32 = dy.astype(np.float32), x.astype(np.float32)
    for e, (lo, hi) in enumerate(W.segments(off, len(dy))):
        fwd, rev = np.zeros((16, 24), dtype=np.float32), np.zeros((16, 24), dtype=np.float32)
        for r in range(lo, hi):
            fwd += d32[r][:, None] * x32[r][None, :]
            rev += d32[hi - 1 - (r - lo)][:, None] * x32[hi - 1 - (r - lo)][None, :]
        assert (fwd == ref[e]).all() and (rev == ref[e]).all()
    assert not W.witness_is_exact(dy * 0.5, x, off, "float32")
    assert not W.witness_is_exact(np.full((8000, 8), 3.0), np.full((8000, 8), 3.0), np.array([0, 0, 8000]), "bfloat16")
    assert W.witness_is_exact(np.full((8000, 8), 3.0), np.full((8000, 8), 3.0), np.array([0, 0, 8000]), "float32")


def test_bounds_are_the_stated_ones():
    ref, mag = np.array([[[1.0, -300.0]], [[0.0, 0.0]]]), np.array([[[4.0, 900.0]], [[0.0, 0.0]]])
    b, e32 = W.bound(ref, mag, [129, 0], "bfloat16")
    assert np.allclose(e32[0], 131 * 2.0 ** -23 * mag[0]) and np.allclose(b[0], e32[0] + np.array([2.0 ** -8, 2.0 ** 0]))
    b, e32 = W.bound(ref, mag, [129, 0], "float32")
    assert np.allclose(b[0], e32[0] + (np.abs(ref[0]) + e32[0]) * 2.0 ** -24)
    rb, mb = np.array([[2.0, -300.0]]), np.array([[6.0, 500.0]])
    b, e = W.dbias_bound(rb, mb, [65], "float16")
    assert np.allclose(e, 65 * 2.0 ** -24 * mb) and np.allclose(b, e + np.array([2.0 ** -10, 2.0 ** -3]))
