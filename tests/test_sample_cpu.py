"""CPU: the host side of fa_sample - the fp64 yardstick against an emulation of the device's fp32 / integer-mass arithmetic on
decisive inputs, the builder's margins, the C ABI's argument checks on host pointers, the ctypes mirror, the workspace query (which
needs no device), the torch.library ops' schemas and fake implementations and the Python wrapper's argument errors.  Nothing here
needs a GPU."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import sample_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


# the yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("V", [8, 60, 264, 4096, 32776])
def test_builder_finds_its_cuts_and_the_reference_equals_the_emulation(V, dtype):
    """on seeded randn rows (spread 2 - 4, T 1 / 0.7 / 0.5, k 0 / 1 / 5 / 50 / 1000, every filter alone and all together) the
    builder always finds its cuts - no case is skipped -, every margin is above 1.5 DELTA, and the fp64 reference agrees with the
    fp32 / integer-mass emulation in id, n_kept and the kept set"""
    n = 0
    for spread, T in ((2.0, 1.0), (3.0, 0.7), (4.0, 0.5)):
        for k in (0, 1, 5, 50, 1000):
            row = R.randn_row(V, dtype, seed=V + k, spread=spread)
            for mp, tp in ((False, False), (True, False), (False, True), (True, True)):
                if k == 1 and mp:
                    continue                                  # (one token: no two masses to cut between - top_k needs no margin)
                b = R.build(row, T, k, want_min_p=mp, want_top_p=tp, seed=n)
                assert all(m > 1.5 * R.DELTA for m in b["margins"].values()), b["margins"]
                assert set(b["margins"]) == {"u"} | ({"min_p"} if mp else set()) | ({"top_p"} if tp else set())
                a = R.row_ref(row, T, k, b["top_p"], b["min_p"], b["u"])
                e = R.row_ref(row, T, k, b["top_p"], b["min_p"], b["u"], emulate=True)
                assert a["id"] == e["id"] == b["id"] and a["n_kept"] == e["n_kept"] == b["n_kept"]
                assert (a["kept"] == e["kept"]).all() and a["kept"].sum() == a["n_kept"] and a["kept"][a["id"]]
                assert abs(a["lse"] - e["lse"]) <= R.lse_bound(row, T, a["lse"])
                n += 1
    assert n == 3 * (4 * 4 + 2)


def test_mass_bound_is_what_the_header_says():
    x = np.array([64.0, -64.0, 0.0])
    assert R.mass_rel_bound(x, 64.0).max() < R.MASS_BOUND == 2.0 ** -15 and R.DELTA == 4 * R.MASS_BOUND
    # the emulated masses stay inside the bound on the builder's range
    row = R.randn_row(4096, torch.float32, seed=1, spread=4.0)
    v = R.values(row)
    e, _, _ = R.masses(v, 0.5)
    ee, _, _ = R.masses(v, 0.5, emulate=True)
    x = v / 0.5
    big = e > 2.0 ** -100
    assert (np.abs(ee[big] / e[big] - 1.0) <= R.mass_rel_bound(x, x.max())[big]).all()
    with pytest.raises(AssertionError, match="range"):
        R.build(row * 10, 0.5)


def test_reference_rules_on_exact_cases():
    """the cases that need no margin: all-equal logits, u at the ends, empty / NaN / +inf rows, k = 1, k >= V, top_p <= 0,
    min_p > 1, a cold row"""
    row = torch.zeros(8)
    for u, want in ((0.0, 0), (0.49, 3), (1 - 2.0 ** -24, 7), (1.0, 7), (float("nan"), 0), (-0.5, 0)):
        assert R.row_ref(row, 1.0, u=u)["id"] == want
    r = R.row_ref(row, 1.0, k=3, u=0.5)
    assert r["n_kept"] == 3 and r["kept"].tolist() == [True] * 3 + [False] * 5 and r["id"] == 1   # ties: the lowest indices
    assert R.row_ref(row, 1.0, k=8, u=0.99)["n_kept"] == 8 and R.row_ref(row, 1.0, k=100, u=0.99)["id"] == 7
    for kw in (dict(top_p=0.0), dict(top_p=-1.0), dict(k=1)):
        r = R.row_ref(torch.tensor([0.0, 2.0, 1.0, 2.0]), 1.0, u=0.99, **kw)
        assert (r["id"], r["n_kept"]) == (1, 1), kw
    r = R.row_ref(torch.tensor([0.0, 2.0, 1.0, 2.0]), 1.0, u=0.99, min_p=0.999)             # both maxima have e = 1
    assert (r["id"], r["n_kept"]) == (3, 2)
    r = R.row_ref(torch.tensor([0.0, 2.0, 1.0, 2.0]), 1.0, u=0.99, min_p=7.0)               # min(min_p, 1): the maxima stay
    assert (r["id"], r["n_kept"]) == (3, 2)
    r = R.row_ref(torch.tensor([0.0, 2.0, 1.0, 2.0]), 1.0, u=0.99, min_p=float("nan"), top_p=float("nan"))
    assert r["n_kept"] == 4
    empty = R.row_ref(torch.full((5,), float("-inf")), 1.0)
    assert (empty["id"], empty["n_kept"], empty["lse"]) == (-1, 0, -math.inf) and not empty["kept"].any()
    nan = R.row_ref(torch.tensor([float("nan"), -1.0, float("nan"), -1.0]), 0.0)
    assert (nan["id"], nan["n_kept"]) == (1, 1)
    inf = R.row_ref(torch.tensor([0.0, float("inf"), 5.0, float("inf")]), 1.0, u=0.9)
    assert (inf["id"], inf["n_kept"]) == (1, 1) and math.isnan(inf["lse"]) and not inf["sampled"]
    for T in (0.0, -1.0, float("nan")):
        assert R.row_ref(torch.tensor([1.0, 3.0, 3.0]), T, u=0.9)["id"] == 1
    assert R.iters(1) == R.iters(8192) == 1 and R.iters(8193) == 2 and R.iters(32767) == 4 and R.iters(262144) == 2 and R.wave_run(262144) == 1024


# the C ABI -------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_struct_size(lib):
    for name in ("fa_sample", "fa_sample_workspace_bytes", "fa_sample_params_size"):
        assert hasattr(lib.lib, name) and name in lib.EXPORTS
    assert lib.lib.fa_sample_params_size() == ctypes.sizeof(lib.FaSampleParams)
    assert lib.FA_ABI_VERSION == 4 and lib.lib.fa_abi_version() == 4
    rows = {e: (s, q) for e, s, q in lib.ROW_OPS}
    assert rows["fa_sample"] == (lib.FaSampleParams, "fa_sample_workspace_bytes")
    import build
    assert "fa_sample.hip" in build.SOURCES


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
    return [f.split("[")[0] for f in fields]


def test_ctypes_mirror_matches_the_header(lib):
    fields = _header_fields("fa_sample_params")
    assert [f[0] for f in lib.FaSampleParams._fields_] == fields
    assert fields[0] == "struct_size" and fields[-1] == "reserved"
    assert ctypes.sizeof(lib.FaSampleParams) % 8 == 0 and ctypes.sizeof(dict(lib.FaSampleParams._fields_)["reserved"]) == 32
    for pair in ("temperature", "top_k", "top_p", "min_p"):
        assert pair in fields and pair + "_value" in fields


# host buffers behind a valid block: [8, 64] logits and filtered with room for fp32, [8] vectors, a workspace
_T = 8 * 64 * 4
_V4 = 8 * 4
_OFF = {}
_o = 0
for _n, _sz in (("logits", _T), ("filtered", _T), ("u", _V4), ("temperature", _V4), ("top_k", _V4), ("top_p", _V4), ("min_p", _V4),
                ("ids", _V4), ("n_kept", _V4), ("lse", _V4), ("workspace", 256)):
    _OFF[_n] = _o
    _o += _sz
_TOTAL = _o + 64
_ARRAYS = ("u", "temperature", "top_k", "top_p", "min_p", "ids", "n_kept", "lse")


def _block(lib, buf, form="bf16"):
    """a valid fa_sample block over host memory: 8 rows of 64 columns, every array given.  form: 'bf16', 'fp32', 'view' (row
    strides 96 / 80, 5 rows), 'scalars' (no parameter arrays), 'filter' (filtered alone: no ids, no u)"""
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaSampleParams()
    s.struct_size = ctypes.sizeof(lib.FaSampleParams)
    for name in ("logits", "filtered") + _ARRAYS:
        setattr(s, name, base + _OFF[name])
    s.rows, s.vocab, s.logits_row_stride, s.filtered_row_stride = 8, 64, 64, 64
    s.dtype = lib.FA_FP32 if form == "fp32" else lib.FA_BF16
    s.temperature_value, s.top_k_value, s.top_p_value, s.min_p_value = 1.0, 0, 1.0, 0.0
    if form == "view":
        s.rows, s.logits_row_stride, s.filtered_row_stride = 5, 96, 80
    if form == "scalars":
        s.temperature = s.top_k = s.top_p = s.min_p = None
    if form == "filter":
        s.ids = s.u = s.n_kept = s.lse = None
    return s, base


_at = lambda name, add=0: (lambda b: b + _OFF[name] + add)      # noqa: E731
_FORMS = ("bf16", "fp32", "view", "scalars", "filter")


def test_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_sample fires before any device work, and the workspace query answers 0 for a block
    the call rejects"""
    buf = (ctypes.c_char * _TOTAL)()

    def bad(match, form="bf16", code="(-1)", **kw):
        s, base = _block(lib, buf, form)
        for k, v in kw.items():
            setattr(s, k, v(base) if callable(v) else v)
        with pytest.raises(RuntimeError, match=match) as e:
            lib.call_sample(s, 0)
        assert code in str(e.value) and "sample" in str(e.value)
        assert lib.sample_workspace_bytes(s) == 0
    for form in _FORMS:
        bad("struct_size", form, struct_size=ctypes.sizeof(lib.FaSampleParams) - 8)
        bad("logits must not be NULL", form, logits=None)
        bad("reserved", form, reserved=(ctypes.c_int64 * 4)(0, 0, 1, 0))
        bad("fp16, bf16 or fp32", form, dtype=lib.FA_FP8_E4M3)
        bad("fp16, bf16 or fp32", form, dtype=9)
        bad("vocab must be at least 1", form, vocab=0)
        bad("vocab must be at least 1", form, vocab=-3)
        bad("rows must be non-negative", form, rows=-1)
        bad("row strides", form, logits_row_stride=-64)
        bad("row strides", form, logits_row_stride=63)                   # rows overlap themselves
        bad("row strides", form, filtered_row_stride=40)
        bad("aligned", form, logits=_at("logits", 1))
        bad("aligned", form, filtered=_at("filtered", 1))
        bad("workspace must be 16-byte aligned", form, workspace=_at("workspace", 8), workspace_bytes=64)
        bad("filtered overlaps logits", form, filtered=_at("logits", 0))   # in place is not supported
        bad("filtered overlaps logits", form, filtered=_at("logits", 32))
    for form in ("bf16", "fp32", "view", "scalars"):
        bad("ids needs u", form, u=None)
        for name in _ARRAYS:
            if form == "scalars" and name in ("temperature", "top_k", "top_p", "min_p"):
                continue
            bad("aligned", form, **{name: _at(name, 2)})
        bad("ids overlaps logits", form, ids=_at("logits", 64))
        bad("ids overlaps u", form, ids=_at("u", 0))
        bad("filtered overlaps u", form, u=_at("filtered", 128))
        bad("ids overlaps n_kept", form, n_kept=_at("ids", 4))
        bad("n_kept overlaps lse", form, lse=_at("n_kept", 0))
    for name in ("temperature", "top_k", "top_p", "min_p"):
        bad("ids overlaps " + name, **{name: _at("ids", 8)})
    bad("aligned", "fp32", logits=_at("logits", 2))
    bad("at least one of ids and filtered", "filter", filtered=None)
    bad("ids needs u", "scalars", u=None, temperature_value=1e-30)        # any temperature above 0 samples
    # FA_ERR_UNSUPPORTED
    bad(r"2\^20", code="(-2)", vocab=2 ** 20 + 1, logits_row_stride=2 ** 20 + 1, filtered_row_stride=2 ** 20 + 1, rows=1,
        logits=_at("workspace", 1024))
    bad(r"2\^31", code="(-2)", rows=2 ** 31, vocab=1, logits_row_stride=1, filtered_row_stride=1)


def test_valid_blocks_pass_the_checks(lib):
    """rows == 0 is FA_OK without a launch; non-finite and out-of-range HOST scalars follow the per-row rules and are not rejected;
    u may be missing where the host temperature is not above 0 or ids is not asked for; a valid block reaches the launch (which
    fails here: there is no device)"""
    buf = (ctypes.c_char * _TOTAL)()
    for form in _FORMS:
        s, _ = _block(lib, buf, form)
        s.rows = 0
        lib.call_sample(s, 0)
    for kw in (dict(temperature_value=float("nan")), dict(temperature_value=-1.0), dict(temperature_value=float("inf")),
               dict(top_k_value=-5), dict(top_k_value=2 ** 31 - 1), dict(top_p_value=float("nan")), dict(top_p_value=-2.0),
               dict(top_p_value=float("inf")), dict(min_p_value=float("nan")), dict(min_p_value=7.0), dict(min_p_value=-1.0)):
        s, _ = _block(lib, buf, "scalars")
        s.rows = 0
        for k, v in kw.items():
            setattr(s, k, v)
        lib.call_sample(s, 0)
    for t in (0.0, -1.0, float("nan")):
        s, _ = _block(lib, buf, "scalars")
        s.rows, s.u, s.temperature_value = 0, None, t
        lib.call_sample(s, 0)
    s, _ = _block(lib, buf, "bf16")
    s.rows, s.workspace, s.workspace_bytes = 0, None, 0
    lib.call_sample(s, 0)
    if not torch.cuda.is_available():
        s, _ = _block(lib, buf, "bf16")
        with pytest.raises(RuntimeError, match=r"fa_sample failed \(-3\)|launch"):
            lib.call_sample(s, 0)


def test_workspace_query_is_a_function_of_its_stated_inputs(lib):
    """one workgroup per row (V < 32768) asks for nothing; the split plan asks for rows x a per-row size that depends on the number
    of chunks alone (tests/sample_ref.py restates it) - whatever the dtype, the row strides, the pointers, the parameter values or
    which outputs are given; NULL and a short block answer 0"""
    buf = (ctypes.c_char * _TOTAL)()
    for code in (lib.FA_FP16, lib.FA_BF16, lib.FA_FP32):
        for rows, V in ((1, 1), (3, 60), (67, 8193), (5, 32767), (5, 32768), (7, 49152), (7, 49153), (1, 262144), (1024, 151936),
                        (2 ** 31 // 64 - 1, 2 ** 20)):
            s, _ = _block(lib, buf)
            s.rows, s.vocab, s.dtype, s.logits_row_stride, s.filtered_row_stride = rows, V, code, V, V
            want = lib.sample_workspace_bytes(s)
            assert want == R.workspace_bytes(rows, V) and (want > 0) == (V >= R.SPLIT_MIN), (rows, V)
            s.logits_row_stride, s.top_k_value, s.workspace, s.lse = V + 24, 50, None, None
            assert lib.sample_workspace_bytes(s) == want
    assert R.workspace_bytes(1, 262144) == 6144 and R.chunks(262144) == 16 and R.chunks(32767) == 1 and R.chunks(49153) == 4
    assert lib.lib.fa_sample_workspace_bytes(None) == 0
    s, _ = _block(lib, buf)
    s.struct_size = 8
    assert lib.sample_workspace_bytes(s) == 0


def test_split_plan_workspace_errors(lib):
    """a vocabulary of two chunks and more needs the workspace (the checks run on host pointers: nothing is launched)"""
    buf = (ctypes.c_char * (_TOTAL + 3 * 40000 * 2))()
    V = 40000

    def bad(match, code="(-1)", **kw):
        s, base = _block(lib, buf)
        big = base + _TOTAL                                   # (two long rows and filtered behind everything else)
        s.rows, s.vocab, s.logits_row_stride, s.filtered_row_stride = 1, V, V, V
        s.logits, s.filtered = big, big + 2 * V + 64
        need = R.workspace_bytes(1, V)
        assert need > 256
        s.workspace, s.workspace_bytes = base + _OFF["workspace"], need
        for k, v in kw.items():
            setattr(s, k, v(base) if callable(v) else v)
        with pytest.raises(RuntimeError, match=match) as e:
            lib.call_sample(s, 0)
        assert code in str(e.value)
    bad("the workspace holds", workspace=None)
    bad("the workspace holds", workspace_bytes=R.workspace_bytes(1, V) - 1)
    bad("workspace must be 16-byte aligned", workspace=_at("workspace", 8))
    bad("overlaps", workspace=_at("ids", 0))
    bad(r"2\^31", code="(-2)", rows=2 ** 31 // 3 + 1)


# Python ----------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors_on_cpu_tensors():
    from flash_attn_mi355.sample import greedy, sample, sample_forward, top_k_top_p_filter
    x = torch.zeros(4, 6, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="fp16, bf16 or fp32"):
        sample(x.double())
    with pytest.raises(RuntimeError, match=r"\[\.\.\., V\] with V >= 1"):
        sample(x[..., :0])
    with pytest.raises(RuntimeError, match="temperature must be a number or a tensor of one value per row"):
        sample(x, temperature=torch.ones(5))
    with pytest.raises(RuntimeError, match="top_k must be an integer tensor"):
        sample(x, top_k=torch.ones(24))
    with pytest.raises(RuntimeError, match="top_p must be a floating-point tensor"):
        top_k_top_p_filter(x, top_p=torch.ones(24, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="min_p must be a number"):
        sample(x, min_p="a")
    with pytest.raises(RuntimeError, match="u must be a float32 tensor of one value per row"):
        sample_forward(x, torch.zeros(3))
    with pytest.raises(RuntimeError, match="u is needed"):
        sample_forward(x, None)
    # everything else in order: the CPU tensor itself is the error
    with pytest.raises(RuntimeError, match="GPU"):
        sample(x, temperature=0.7, top_k=50, top_p=0.9, min_p=0.05)
    with pytest.raises(RuntimeError, match="GPU"):
        sample(x, temperature=torch.ones(4, 6), top_k=torch.ones(24, dtype=torch.int64), u=torch.zeros(4, 6), return_lse=True)
    with pytest.raises(RuntimeError, match="GPU"):
        sample_forward(x, None, temperature=0.0)
    with pytest.raises(RuntimeError, match="GPU"):
        top_k_top_p_filter(x, top_k=5)
    with pytest.raises(RuntimeError, match="GPU"):
        greedy(x)


def test_wrapper_signatures():
    import flash_attn_mi355.sample as S
    sig = lambda f: [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]      # noqa: E731
    KW, E = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty
    filt = [("temperature", 1.0, KW), ("top_k", 0, KW), ("top_p", 1.0, KW), ("min_p", 0.0, KW)]
    assert sig(S.sample) == [("logits", E, inspect.Parameter.POSITIONAL_OR_KEYWORD)] + filt + [
        ("u", None, KW), ("generator", None, KW), ("return_lse", False, KW), ("return_n_kept", False, KW)]
    assert sig(S.top_k_top_p_filter) == [("logits", E, inspect.Parameter.POSITIONAL_OR_KEYWORD)] + filt
    assert sig(S.greedy) == [("logits", E, inspect.Parameter.POSITIONAL_OR_KEYWORD)]


def test_torch_op_schemas_and_fake_implementations():
    """sample / sample_filter are functional, each parameter an optional tensor plus a scalar; the fake implementations give the
    shapes, dtypes and (contiguous) strides"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    import flash_attn_mi355.torch_ops as T
    ns = torch.ops.flash_attn_mi355
    smp, flt = ns.sample.default._schema, ns.sample_filter.default._schema
    assert not [a.name for a in smp.arguments if a.alias_info is not None]
    assert not [a.name for a in flt.arguments if a.alias_info is not None]
    pairs = ["temperature", "temperature_value", "top_k", "top_k_value", "top_p", "top_p_value", "min_p", "min_p_value"]
    assert [a.name for a in smp.arguments] == ["logits", "u"] + pairs and [a.name for a in flt.arguments] == ["logits"] + pairs
    assert [str(a.type) for a in flt.arguments[1:]] == ["Optional[Tensor]", "float", "Optional[Tensor]", "int", "Optional[Tensor]",
                                                        "float", "Optional[Tensor]", "float"]
    assert len(smp.returns) == 3 and len(flt.returns) == 1
    with FakeTensorMode():
        for dt in (torch.float16, torch.bfloat16, torch.float32):
            wide = torch.empty(5, 7, 1024, dtype=dt, device="cuda")
            x = wide[..., :1001]                             # a strided view: the outputs are fresh contiguous tensors
            u = torch.empty(5, 7, dtype=torch.float32, device="cuda")
            k = torch.empty(35, dtype=torch.int32, device="cuda")
            ids, n_kept, lse = ns.sample(x, u, None, 0.7, k, 0, None, 0.9, u, 0.0)
            for o, odt in ((ids, torch.int32), (n_kept, torch.int32), (lse, torch.float32)):
                assert o.shape == (5, 7) and o.dtype == odt and o.is_contiguous()
            f = ns.sample_filter(x, None, 1.0, None, 50, None, 1.0, None, 0.0)
            assert f.shape == x.shape and f.dtype == dt and f.is_contiguous()
    for name in ("sample", "sample_filter"):
        assert name not in T.__all__                        # reached through torch.ops only


def test_public_name_lists_are_unchanged():
    import flash_attn
    import flash_attn_mi355
    for name in ("sample", "sample_forward", "top_k_top_p_filter", "greedy", "sample_filter"):
        assert name not in flash_attn.__all__ and name not in flash_attn_mi355.__all__
