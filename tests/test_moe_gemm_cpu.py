"""CPU: the host side of fa_moe_gemm - the C ABI's block, its limits and stride rules on host pointers, the launch plan against
every segmentation it has to serve, the Python wrapper's argument errors, the torch.library schema and fake implementation, the
fp64 yardstick of the GPU tests (moe_gemm_ref.py) told apart from the wrong variants it must catch, and the exactness of the
witness data.  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import moe_gemm_ref as G
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
    for name in ("fa_moe_gemm", "fa_moe_gemm_params_size", "fa_moe_gemm_plan"):
        assert hasattr(lib.lib, name) and name in lib.EXPORTS
    assert lib.lib.fa_moe_gemm_params_size() == ctypes.sizeof(lib.FaMoeGemmParams)
    rows = {e: (s, q) for e, s, q in lib.ROW_OPS}
    assert rows["fa_moe_gemm"] == (lib.FaMoeGemmParams, None) and callable(lib.call_moe_gemm)
    assert lib.FA_ABI_VERSION == 4 and lib.lib.fa_abi_version() == 4            # additive: the ABI version stays
    body = re.search(r"typedef struct fa_moe_gemm_params \{(.*?)\} fa_moe_gemm_params;", _header(), flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        if stmt.strip():
            names = stmt.strip().split(",")
            fields.append(names[0].split()[-1].lstrip("*"))
            fields += [n.strip().lstrip("*") for n in names[1:]]
    fields = [f.split("[")[0] for f in fields]
    assert [f[0] for f in lib.FaMoeGemmParams._fields_] == fields
    assert fields[0] == "struct_size" and fields[-1] == "reserved" and ctypes.sizeof(dict(lib.FaMoeGemmParams._fields_)["reserved"]) == 32
    body = re.search(r"typedef enum fa_moe_w_layout \{(.*?)\} fa_moe_w_layout;", _header(), flags=re.S).group(1)
    assert {k: int(v) for k, v in re.findall(r"(FA_MOE_W_\w+)\s*=\s*(\d+)", body)} == {"FA_MOE_W_NK": 0, "FA_MOE_W_KN": 1}
    from flash_attn_mi355 import moe
    assert moe.W_LAYOUTS == {"nk": lib.FA_MOE_W_NK, "kn": lib.FA_MOE_W_KN}
    import build
    assert "fa_moe_gemm.hip" in build.SOURCES
    assert json_budget_unchanged()


def json_budget_unchanged():
    """csrc/spill_budget.json lists no kernel of the new source: the budget test holds them to zero spills"""
    import json
    import build
    budget = json.load(open(os.path.join(build.CSRC, "spill_budget.json")))["spill"]
    res = json.load(open(build.RESOURCES))
    mine = [n for n in res if "moe_gemm_kernel" in n]
    assert len(mine) == 16                                                   # 2 dtypes x 2 tile shapes x 2 layouts x plain / gather
    return not any("moe_gemm" in n for n in budget) and all(res[n]["spill"] == 0 and res[n]["scratch"] == 0 for n in mine)


def _block(lib, base, **kw):
    s = lib.FaMoeGemmParams()
    s.struct_size = ctypes.sizeof(s)
    s.x, s.w, s.expert_offsets, s.out = base, base + 0x10000, base + 0x30000, base + 0x40000
    s.x_row_stride, s.out_row_stride, s.w_expert_stride = 64, 32, 64 * 32
    s.rows, s.num_experts, s.n, s.k, s.dtype, s.layout = 16, 4, 32, 64, lib.FA_BF16, lib.FA_MOE_W_NK
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_limits_and_stride_rules_fire_before_any_device_work(lib):
    """FA_ERR_UNSUPPORTED (-2) for the limits, FA_ERR_INVALID_ARGUMENT (-1) for the argument rules, each naming its argument"""
    buf = (ctypes.c_char * (0x60000 + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15

    def bad(match, code="(-1)", **kw):
        with pytest.raises(RuntimeError, match=match) as e:
            lib.call_moe_gemm(_block(lib, base, **kw), 0)
        assert code in str(e.value), str(e.value)
    bad("struct_size", struct_size=8)
    bad("reserved", reserved=(ctypes.c_int64 * 4)(0, 0, 1, 0))
    bad("reserved", reserved0=1)
    bad("num_experts", "(-2)", num_experts=1)
    bad("num_experts", "(-2)", num_experts=513)
    bad(": n must", "(-2)", n=36)
    bad(": n must", "(-2)", n=65544, w_expert_stride=65544 * 64)
    bad(": k must", "(-2)", k=4)
    bad(": k must", "(-2)", k=32776, w_expert_stride=32776 * 32, x_row_stride=32776)
    bad("rows", rows=-1)
    bad("rows", "(-2)", rows=2 ** 31)
    bad("dtype", dtype=lib.FA_FP32)
    bad("layout", layout=2)
    bad("w_expert_stride", "(-2)", w_expert_stride=64 * 32 - 8)
    bad("w_expert_stride", "(-2)", w_expert_stride=64 * 32 + 4)
    bad("x_row_stride", "(-2)", x_row_stride=68)
    bad("x_row_stride", "(-2)", x_row_stride=2 ** 22 + 8)
    bad("out_row_stride", "(-2)", out_row_stride=36)
    bad("out rows must not overlap", out_row_stride=24)
    bad("x_row_stride must be at least k", x_row_stride=56)
    bad("must not be NULL", w=None)
    bad("must not be NULL", expert_offsets=None)
    bad("16-byte aligned", out=base + 0x40000 + 8)
    bad("16-byte aligned", w=base + 0x10000 + 2)
    bad("aligned to their elements", expert_offsets=base + 0x30000 + 2)
    bad("bias_dtype", "(-2)", bias=base + 0x50000, bias_dtype=lib.FA_FP8_E4M3)
    bad("top_k", "(-2)", sorted_slot=base + 0x38000, tokens=4, top_k=0)
    bad("top_k", "(-2)", sorted_slot=base + 0x38000, tokens=4, top_k=17)
    bad("2\\^31", "(-2)", sorted_slot=base + 0x38000, tokens=2 ** 30, top_k=2)
    bad("overlaps", out=base + 0x10000)
    bad("overlaps", out=base)
    # rows == 0 launches nothing and needs no device: FA_OK on any machine
    lib.call_moe_gemm(_block(lib, base, rows=0), 0)
    # the plan's own checks
    with pytest.raises(RuntimeError, match=r"\(-2\).*num_experts"):
        lib.moe_gemm_plan(64, 32, 64, 1, lib.FA_MOE_W_NK, lib.FA_BF16)
    with pytest.raises(RuntimeError, match=r"\(-2\).*k must"):
        lib.moe_gemm_plan(64, 32, 12, 8, lib.FA_MOE_W_NK, lib.FA_BF16)
    with pytest.raises(RuntimeError, match=r"\(-1\).*rows"):
        lib.moe_gemm_plan(-1, 32, 64, 8, lib.FA_MOE_W_NK, lib.FA_BF16)


def _tiles(lengths, tail, bm):
    return sum(-(-n // bm) for n in lengths) + -(-tail // bm)


def test_plan_serves_every_segmentation_and_depends_on_its_arguments_alone(lib):
    """for random and adversarial cuts of M_max rows into E segments and a +0 tail, the tiles of block_m rows the segments (and
    the tail) need never exceed grid_m; block_m is 32 where M_max <= 32 E and 128 above; the same arguments give the same plan"""
    rng = np.random.default_rng(5)
    for E in (2, 7, 8, 128, 512):
        for T, K in ((1, 1), (1, 8), (8, 8), (67, 2), (128, 8), (300, 6), (8192, 8)):
            if K > E:
                continue
            for align in (1, 16, 128):
                m_max = T * K + E * (align - 1)
                for layout in (lib.FA_MOE_W_NK, lib.FA_MOE_W_KN):
                    plan = lib.moe_gemm_plan(m_max, 2880, 2880, E, layout, lib.FA_BF16)
                    assert plan == lib.moe_gemm_plan(m_max, 2880, 2880, E, layout, lib.FA_BF16)
                    bm, bn, bk, grid_m, grid_n = plan
                    assert bm == (32 if m_max <= 32 * E else 128) and (bn, bk) == (128, 64) and grid_n == -(-2880 // 128)
                    assert grid_m == m_max // bm + E + 1
                slots = T * K
                cuts = [[slots] + [0] * (E - 1), [0] * (E - 1) + [slots],                         # all rows in one expert
                        [1] * min(slots, E) + [0] * (E - min(slots, E)),                          # one row per expert
                        list(rng.multinomial(slots, rng.dirichlet(np.ones(E) * 0.3))),            # skewed, empty experts
                        list(rng.multinomial(slots, np.ones(E) / E))]
                for cut in cuts:
                    cut = [int(c) for c in cut]
                    padded = [-(-c // align) * align for c in cut]
                    assert sum(padded) <= m_max
                    assert _tiles(padded, m_max - sum(padded), bm) <= grid_m, (E, T, K, align, cut[:8])
    # the worst case is reached: every piece one row over a multiple of block_m
    bm, _, _, grid_m, _ = lib.moe_gemm_plan(7 * 129 + 129, 8, 8, 7, 0, lib.FA_FP16)
    assert bm == 128 and _tiles([129] * 7, 129, bm) == grid_m == 16
    assert lib.moe_gemm_plan(0, 8, 8, 2, 0, lib.FA_FP16)[3] == 0
    # the GPU tests' shapes go where their docstring says
    assert lib.moe_gemm_plan(226, 264, 264, 7, 0, lib.FA_BF16)[0] == 128 and lib.moe_gemm_plan(200, 264, 264, 7, 0, lib.FA_BF16)[0] == 32
    assert lib.moe_gemm_plan(86, 40, 48, 512, 0, lib.FA_BF16)[0] == 32 and lib.moe_gemm_plan(16409, 8, 8, 512, 0, lib.FA_BF16)[0] == 128


def test_wrapper_rejects_by_name_without_a_device(lib):
    from flash_attn_mi355 import moe
    bf = torch.bfloat16
    x, w, off = torch.zeros(16, 64, dtype=bf), torch.zeros(4, 32, 64, dtype=bf), torch.zeros(5, dtype=torch.int32)

    def bad(match, *a, **kw):
        with pytest.raises(RuntimeError, match=match):
            moe.moe_gemm(*a, **kw)
    bad("w_layout", x, w, off, w_layout="kn ")
    bad("x must be fp16 or bf16", x.float(), w, off)
    bad(r"x must be \[rows, K\]", x[0], w, off)
    bad("w must be a", x, w.half(), off)
    bad("does not contract", x, w, off, w_layout="kn")
    bad("num_experts", x, w[:1], off[:2])
    bad("num_experts", x, torch.zeros(513, 8, 64, dtype=bf), torch.zeros(514, dtype=torch.int32))
    bad("K must be a multiple of 8", x[:, :60], w[:, :, :60], off)
    bad("N must be a multiple of 8", x, w[:, :28], off)
    bad("N must be a multiple of 8", x[:, :8], torch.zeros(2, 65544, 8, dtype=bf), off[:3])
    bad("expert stride", x[:, :32], w[:, :, :32], off)                      # rows of an expert are not contiguous
    bad("expert_offsets", x, w, off.long())
    bad("expert_offsets", x, w, off[:4])
    bad("go together", x, w, off, top_k=2)
    bad("go together", x, w, off, sorted_slot=torch.zeros(8, dtype=torch.int32))
    bad("k must be", x, w, off, sorted_slot=torch.zeros(8, dtype=torch.int32), top_k=17)
    bad("sorted_slot must be an int32", x, w, off, sorted_slot=torch.zeros(8, dtype=torch.int64), top_k=2)
    bad("bias must be", x, w, off, bias=torch.zeros(4, 32, dtype=torch.float16))
    bad("bias must be", x, w, off, bias=torch.zeros(4, 16))
    bad("out must be", x, w, off, out=torch.zeros(16, 32))
    bad("out must be", x, w, off, out=torch.zeros(15, 32, dtype=bf))
    bad("x must have a contiguous last", torch.zeros(64, 16, dtype=bf).t(), w, off)
    bad("x must be 16-byte aligned", torch.zeros(16, 72, dtype=bf)[:, 4:68], w, off)
    bad("out must be 16-byte aligned", x, w, off, out=torch.zeros(16, 36, dtype=bf)[:, :32])
    bad("x requires grad", x.clone().requires_grad_(), w, off)
    bad("w requires grad", x, w.clone().requires_grad_(), off)
    bad("no CPU fallback", x, w, off)                                        # every check passed: only the device is missing
    with pytest.raises(RuntimeError, match="w_layout"):
        moe.moe_gemm_plan(64, 32, 64, 8, w_layout="xx")
    assert moe.moe_gemm_plan(64, 32, 64, 8) == lib.moe_gemm_plan(64, 32, 64, 8, lib.FA_MOE_W_NK, lib.FA_BF16)
    assert "moe_gemm" not in getattr(moe, "__all__", ())


def test_torch_op_schema_and_fake(lib):
    import flash_attn_mi355.torch_ops  # noqa: F401
    op = torch.ops.flash_attn_mi355.moe_gemm.default
    assert "Tensor x, Tensor w, Tensor expert_offsets, str w_layout, Tensor? bias, Tensor? sorted_slot, SymInt? top_k" in str(op._schema) \
        or "int? top_k" in str(op._schema)
    assert not op._schema.is_mutable
    bf = torch.bfloat16
    x, off = torch.empty(5, 64, dtype=bf, device="meta"), torch.empty(9, dtype=torch.int32, device="meta")
    nk, kn = torch.empty(8, 24, 64, dtype=bf, device="meta"), torch.empty(8, 64, 24, dtype=bf, device="meta")
    assert op(x, nk, off, "nk", None, None, None).shape == (5, 24)
    assert op(x, kn, off, "kn", None, None, None).shape == (5, 24)
    out = op(x, nk, off, "nk", None, torch.empty(70, dtype=torch.int32, device="meta"), 2)
    assert out.shape == (70, 24) and out.dtype == bf


# the yardstick ---------------------------------------------------------------------------------------------------------------
def _case(layout, with_bias, K=264, N=40, seed=3):
    off = G.offsets_of(G.PATTERN)
    x, w, bias = G.witness(int(off[-1]) + 5, K, N, len(G.PATTERN), layout, seed, with_bias)
    return x, w, bias, off


def test_reference_is_the_plain_definition():
    for layout in ("nk", "kn"):
        x, w, bias, off = _case(layout, True)
        got = G.gemm_ref(x, w, off, layout=layout, bias=bias)
        for e in range(len(G.PATTERN)):
            We = torch.from_numpy(w[e]).t() if layout == "nk" else torch.from_numpy(w[e])
            want = torch.from_numpy(x[off[e]:off[e + 1]]) @ We + torch.from_numpy(bias[e])
            assert (got[off[e]:off[e + 1]] == want.numpy()).all()
        assert (got[off[-1]:] == 0).all() and got.shape == (231, 40)


@pytest.mark.parametrize("dtype_name", ["bfloat16", "float16"])
def test_witness_data_tell_the_wrong_variants_apart(dtype_name):
    """each wrong variant changes bits of the expected output - in rows the right one owns - so a kernel with that defect fails
    the bit-for-bit comparison"""
    for layout in ("nk", "kn"):
        x, w, bias, off = _case(layout, True)
        good = G.expected(x, w, off, dtype_name, layout=layout, bias=bias)
        xl, wl, bl, _ = _case(layout, True, K=2880, N=8)                 # (fp16 holds integers up to 2048: the long contraction)
        late = [G.expected(xl, wl, off, dtype_name, layout=layout, bias=bl, variant=v) for v in (None, "bias_late")]
        assert (late[0] != late[1]).any(), "bias_late"
        for variant in ("leak_row", "drop_k_tail") + (("kn_as_nk",) if layout == "kn" else ()):
            kw = dict(layout=layout, bias=bias, variant=variant)
            if variant == "kn_as_nk":
                x2, w2, b2, _ = _case("kn", True, K=40, N=40)                # (a square expert: both readings have a shape)
                g2 = G.expected(x2, w2, off, dtype_name, layout="kn", bias=b2)
                wrong = G.expected(x2, w2, off, dtype_name, layout="kn", bias=b2, variant=variant)
                assert (wrong != g2).mean() > 0.5, variant
                continue
            wrong = G.expected(x, w, off, dtype_name, **kw)
            assert wrong.shape == good.shape and (wrong != good).any(), variant
        leak = G.expected(x, w, off, dtype_name, layout=layout, bias=bias, variant="leak_row")
        rows = np.nonzero((leak != good).any(1))[0]
        assert set(rows) <= {int(off[e]) for e in range(len(G.PATTERN))} and len(rows) >= 3     # first rows of segments
        assert (G.expected(x, w, off, dtype_name, layout=layout, bias=bias, variant="drop_k_tail") != good).mean() > 0.5
    # a padding slot read as token 0: the gather's padding rows stop being +0 rows (their output stops being round16(bias))
    rng = np.random.default_rng(9)
    ids = np.stack([rng.permutation(7)[:2] for _ in range(20)]).astype(np.int32)
    ss, pos, off = R.sort_ref(ids, 7, align=16)
    x, w, bias = G.witness(20, 264, 40, 7, "nk", 11, True)
    good = G.expected(G.gather_ref(x, ss, 2), w, off, dtype_name, bias=bias)
    wrong = G.expected(G.gather_ref(x, ss, 2, variant="pad_as_token0"), w, off, dtype_name, bias=bias)
    pad = (ss < 0) & (np.arange(len(ss)) < off[-1])
    assert pad.any() and (wrong[pad] != good[pad]).any() and (wrong[~pad] == good[~pad]).all()


def test_witness_construction_is_exact():
    """integers; every partial sum, in any order, is an integer below 2^24 (the sum of the magnitudes is); results below 65504"""
    for K in (8, 16, 24, 48, 264, 2880):
        for layout in ("nk", "kn"):
            x, w, bias = G.witness(9, K, 16, 3, layout, K, True)
            assert G.witness_is_exact(x, w, bias, layout)
            off = G.offsets_of([4, 0, 5])
            _, mag = G.gemm_ref(x, w, off, layout=layout, bias=bias, with_mag=True)
            assert mag.max() < 2 ** 24 and mag.max() < 65504
            for dt in (torch.bfloat16, torch.float16):
                for t in (x, w, bias):
                    assert (torch.from_numpy(t).to(dt).double().numpy() == t).all()           # exact in both io dtypes
            # fp32 accumulation in two very different orders gives the fp64 answer
            ref = G.gemm_ref(x, w, off, layout=layout)
            a32 = x.astype(np.float32)
            for e, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
                We = G.w_of(w, e, layout).astype(np.float32)
                fwd = np.zeros((hi - lo, 16), dtype=np.float32)
                rev = np.zeros((hi - lo, 16), dtype=np.float32)
                for k in range(K):
                    fwd += a32[lo:hi, k:k + 1] * We[k:k + 1]
                    rev += a32[lo:hi, K - 1 - k:K - k] * We[K - 1 - k:K - k]
                assert (fwd == ref[lo:hi]).all() and (rev == ref[lo:hi]).all()
    assert not G.witness_is_exact(np.full((1, 8), 0.5), np.ones((2, 8, 8)), None, "nk")
    assert not G.witness_is_exact(np.full((1, 2880), 3.0), np.full((2, 8, 2880), 2 ** 12), None, "nk")


def test_bound_is_the_stated_one():
    # the magnitude the GPU tests feed it is sum |a w| alone: a bias enters through 2^-24 |ref| and nowhere else
    x, w, bias = G.witness(9, 24, 16, 3, "nk", 5, True)
    off = G.offsets_of([4, 0, 5])
    _, mag0 = G.gemm_ref(x, w, off, with_mag=True)
    ref1, mag1 = G.gemm_ref(x, w, off, bias=bias * 100, with_mag=True)
    assert (mag0 == mag1).all() and (mag1[:4] == np.abs(x[:4]) @ np.abs(w[0]).T).all()
    b1, e1 = G.bound(ref1, mag1, 24, "float16", True)
    assert np.allclose(e1, 26 * 2.0 ** -23 * mag0 + 2.0 ** -24 * np.abs(ref1))
    ref, mag = np.array([[1.0, -300.0]]), np.array([[4.0, 900.0]])
    b, e32 = G.bound(ref, mag, 264, "bfloat16", False)
    assert np.allclose(e32, 266 * 2.0 ** -23 * mag) and np.allclose(b, e32 + np.array([2.0 ** -8, 2.0 ** 0]))
    b2, e2 = G.bound(ref, mag, 264, "float16", True)
    assert np.allclose(e2, 266 * 2.0 ** -23 * mag + 2.0 ** -24 * np.abs(ref)) and np.allclose(b2, e2 + np.array([2.0 ** -11, 2.0 ** -3]))
