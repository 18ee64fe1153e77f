"""CPU: the host side of fa_quant_fp8 / fa_add_norm_quant / fa_act_mul_quant - the torch fp32 yardstick of the GPU tests
(quant_ref.py) against exact arithmetic, the properties the rule promises, the variants the GPU checks must tell apart, the C ABI's
argument checks on host pointers, the ctypes mirrors, the torch.library ops' schemas and fake implementations, and the public
name lists.  Nothing here needs a GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import kv_store_ref
import quant_ref as R

DTYPES = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


# the yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["row", "group"])
def test_reference_scale_is_the_correctly_rounded_quotient_or_the_floor(mode, dtype):
    """scale = fl(a' / 448) or 2^-64: 448 s is exact in float64 (24 + 9 bits), so s is the correctly rounded quotient iff neither
    float32 neighbour of s lies closer to a' / 448; a' = min(amax, scale_ub)"""
    y = R.inputs(67, 384, dtype, seed=1)
    y[5] = 0
    for ub in (None, 3.0):
        _, s = R.quant_ref(y, mode, scale_ub=ub)
        yy = y.double().abs()
        a = (yy.reshape(67, 3, 128) if mode == "group" else yy).amax(-1)
        a = a if ub is None else a.clamp(max=ub)
        assert s.dtype == torch.float32 and tuple(s.shape) == ((67, 3) if mode == "group" else (67,))
        floored = a / 448 <= R.FLOOR
        assert bool(floored.any()) and bool((s[floored] == R.FLOOR).all())
        s, a = s[~floored], a[~floored]
        err = lambda t: (t.double() * 448 - a).abs()             # noqa: E731
        up, down = torch.nextafter(s, torch.full_like(s, float("inf"))), torch.nextafter(s, torch.zeros_like(s))
        assert bool((err(s) <= err(up)).all()) and bool((err(s) <= err(down)).all())
        if ub is not None:
            assert bool((s <= torch.tensor(ub / 448, dtype=torch.float32)).all()) and bool((a == ub).any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_codes_are_the_nearest_e4m3_ties_to_even_saturating(dtype):
    """code = the e4m3 value nearest to the fp32 product y * inv (searched over the decoded table, not cast), a tie to the even
    code, +-448 beyond; the product is the fp32 one: the reference's only freedom is the cast"""
    y = R.inputs(67, 264, dtype, seed=2)
    for mode, kw in (("row", {}), ("row", {"scale_ub": 2.0}), ("static", {"scale": 0.37})):
        codes, s = R.quant_ref(y, mode, **kw)
        s = torch.tensor(kw["scale"], dtype=torch.float32).expand(67) if s is None else s
        prod = y.float() * (torch.tensor(1.0) / s).unsqueeze(-1)
        assert R.same_bits(codes.view(torch.uint8), R.nearest_e4m3(prod.double()))
        if "scale_ub" in kw:
            assert bool((prod.abs() > 448).any())                 # saturation is exercised
    # the ties themselves: midpoints of neighbouring codes go to the even one
    tab = R.decode_table()[:127]
    mid = (tab[:-1] + tab[1:]) / 2
    got = R.nearest_e4m3(torch.cat([mid, -mid]))
    assert bool((got % 2 == 0).all())
    cast = torch.cat([mid, -mid]).float().to(R.FP8).view(torch.uint8)
    assert torch.equal(cast, got)
    assert R.nearest_e4m3(torch.tensor([1e9, -1e9, 464.0, 0.0, -0.0, 2.0 ** -11], dtype=torch.float64)).tolist() == [0x7E, 0xFE, 0x7E, 0, 0x80, 0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_static_mode_is_kv_store_quantise(dtype):
    y = R.inputs(33, 136, dtype, seed=3)
    for d in (1.0, 0.0625, 0.05, 0.013, 3.7):
        assert R.same_bits(R.quant_ref(y, "static", scale=d)[0], kv_store_ref.quantise(y, d))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["row", "group"])
def test_every_uncapped_row_or_group_reaches_448_and_the_error_bound_holds(mode, dtype):
    """where the scale is neither floored nor capped, a * inv rounds to 448: at least one code of magnitude 448.  And
    |code * scale - y| <= 2^-4 |y| + scale 2^-9: e4m3 has 3 mantissa bits, so a normal code is within half an ulp = 2^-4 relative
    of the product; below the smallest normal 2^-6 the codes are 2^-9 apart, half a step is 2^-10; the two fp32 roundings (inv, the
    product) add 2^-23 relative each, which the second 2^-10 of the stated 2^-9 covers many times over; no product exceeds 448
    without a scale_ub, so nothing saturates"""
    y = R.inputs(67, 384, dtype, seed=4)
    y[7] = 0
    codes, s = R.quant_ref(y, mode)
    G = 3 if mode == "group" else 1
    mag = codes.view(torch.uint8).reshape(67, G, -1) & 0x7F
    live = s.reshape(67, G) > R.FLOOR
    assert bool((~live).any()) and bool(((mag == 0x7E).any(-1) == live).all())
    deq = codes.double().reshape(67, G, -1) * s.double().reshape(67, G, 1)
    y64 = y.double().reshape(67, G, -1)
    assert bool(((deq - y64).abs() <= 2.0 ** -4 * y64.abs() + s.double().reshape(67, G, 1) * 2.0 ** -9).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_gpu_checks_are_not_vacuous(dtype):
    """on the inputs the GPU tests use the reference differs from: y / scale instead of y * inv; the fp32 value quantised before
    its rounding to 16 bits; amax without fabs; 240 in place of 448; groups of 64 columns"""
    y = R.inputs(67, 4096, dtype, seed=0)
    differs = lambda a, b: not R.same_bits(a, b)                 # noqa: E731
    for mode in ("row", "group"):
        codes, s = R.quant_ref(y, mode)
        assert differs(codes, R.quant_ref(y, mode, divide=True)[0]), mode
        c2, s2 = R.quant_ref(y, mode, no_abs=True)
        assert differs(codes, c2) and differs(s, s2), mode
        c3, s3 = R.quant_ref(y, mode, fp8_max=240.0)
        assert differs(codes, c3) and differs(s, s3), mode
    assert differs(R.quant_ref(y, "static", scale=0.3)[0], R.quant_ref(y, "static", scale=0.3, divide=True)[0])
    c64, s64 = R.quant_ref(y, "group", group=64)
    c128, s128 = R.quant_ref(y, "group")
    assert differs(c64, c128) and s64.shape[-1] == 2 * s128.shape[-1]
    # before the 16-bit rounding: an fp32 value and its rounded self give other codes and another scale somewhere
    y32 = y.float() * 1.0009765625 + 1e-4
    for mode in ("row", "group"):
        a, sa = R.quant_ref(y32, mode)
        b, sb = R.quant_ref(y32.to(dtype), mode)
        assert differs(a, b) and differs(sa, sb), mode


def test_reference_special_values():
    """what flash_attn_mi355/quant.py documents, on the reference"""
    y = torch.tensor([[0.0, -0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                      [1.0, float("nan"), -2.0, 0.5, 0.0, 0.0, 0.0, 0.0],
                      [1.0, float("inf"), -2.0, float("-inf"), 0.0, -0.0, 0.0, 0.0],
                      [float("nan")] * 8], dtype=torch.bfloat16)
    codes, s = R.quant_ref(y, "row")
    c = codes.view(torch.uint8)
    assert float(s[0]) == R.FLOOR and c[0].tolist() == [0, 0x80, 0, 0, 0, 0, 0, 0]
    clean = y[1].clone()
    clean[1] = 0
    cc, cs = R.quant_ref(clean[None], "row")
    assert float(s[1]) == float(cs[0]) == float(torch.tensor(2.0) / 448) and c[1, 1] == 0xFE and c[1, 2] == 0xFE and c[1, 0] == 0x76
    assert [int(v) for i, v in enumerate(c[1]) if i != 1] == [int(v) for i, v in enumerate(cc.view(torch.uint8)[0]) if i != 1]
    assert float(s[2]) == float("inf") and c[2].tolist() == [0, 0xFE, 0x80, 0xFE, 0, 0x80, 0, 0]
    assert float(s[3]) == R.FLOOR and c[3].tolist() == [0xFE] * 8
    cu, su = R.quant_ref(y, "row", scale_ub=4.0)
    assert float(su[2]) == float(torch.tensor(4.0) / 448) and cu.view(torch.uint8)[2, :4].tolist() == [0x6E, 0x7E, 0x76 | 0x80, 0xFE]
    st = R.quant_ref(y, "static", scale=1.0)[0].view(torch.uint8)
    assert st[2, 1] == 0x7E and st[2, 3] == 0xFE and st[1, 1] == 0xFE
    assert not bool(((torch.cat([c, cu.view(torch.uint8), st]) & 0x7F) == 0x7F).any())        # never the e4m3 NaN


# the C ABI -------------------------------------------------------------------------------------------------------------------
_NEW = (("fa_quant_fp8", "FaQuantFp8Params"), ("fa_add_norm_quant", "FaAddNormQuantParams"), ("fa_act_mul_quant", "FaActMulQuantParams"))


def test_library_exports_and_struct_sizes(lib):
    rows = {e: (s, q) for e, s, q in lib.ROW_OPS}
    for entry, mirror in _NEW:
        for name in (entry, entry + "_params_size"):
            assert hasattr(lib.lib, name) and name in lib.EXPORTS
        assert getattr(lib.lib, entry + "_params_size")() == ctypes.sizeof(getattr(lib, mirror))
        assert rows[entry] == (getattr(lib, mirror), None) and callable(getattr(lib, "call_" + entry[3:]))
    assert lib.FA_ABI_VERSION == 4 and lib.lib.fa_abi_version() == 4
    # no existing block changed its size
    assert ctypes.sizeof(lib.FaAddNormParams) == 144 and ctypes.sizeof(lib.FaActMulParams) == 112 and ctypes.sizeof(lib.FaActMulBwdParams) == 144


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "fa_mi355.h")).read(), flags=re.S)


def _header_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        if stmt.strip():
            names = stmt.strip().split(",")
            fields.append(names[0].split()[-1].lstrip("*"))
            fields += [n.strip().lstrip("*") for n in names[1:]]
    return [f.split("[")[0] for f in fields]


def test_ctypes_mirrors_match_the_header(lib):
    for entry, mirror in _NEW:
        m = getattr(lib, mirror)
        fields = _header_fields(entry + "_params")
        assert [f[0] for f in m._fields_] == fields, entry
        assert fields[0] == "struct_size" and fields[-1] == "reserved"
        assert ctypes.sizeof(m) % 8 == 0 and ctypes.sizeof(dict(m._fields_)["reserved"]) == 32
    assert dict(lib.FaAddNormQuantParams._fields_)["norm"] is lib.FaAddNormParams
    body = re.search(r"typedef enum fa_quant_mode \{(.*?)\} fa_quant_mode;", _header(), flags=re.S).group(1)
    enum = {k: int(v) for k, v in re.findall(r"(FA_QUANT_\w+)\s*=\s*(\d+)", body)}
    assert enum == {"FA_QUANT_ROW": lib.FA_QUANT_ROW, "FA_QUANT_GROUP": lib.FA_QUANT_GROUP, "FA_QUANT_STATIC": lib.FA_QUANT_STATIC}
    from flash_attn_mi355 import quant
    assert quant.MODES == {"row": 0, "group": 1, "static": 2}


# host buffers behind valid blocks: [8, 256] tensors
_ROWS, _N = 8, 256
_T = _ROWS * _N * 4
_OFF = {n: i * _T for i, n in enumerate(("x", "up", "residual", "residual_out", "codes", "scales", "weight", "bias"))}
_TOTAL = len(_OFF) * _T + 64


def _rule(s, lib, mode):
    s.mode = {"row": lib.FA_QUANT_ROW, "group": lib.FA_QUANT_GROUP, "static": lib.FA_QUANT_STATIC}[mode]
    if mode == "static":
        s.scale, s.scales = 0.25, None


def _quant_block(lib, buf, mode):
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaQuantFp8Params()
    s.struct_size = ctypes.sizeof(lib.FaQuantFp8Params)
    s.x, s.codes, s.scales = base + _OFF["x"], base + _OFF["codes"], base + _OFF["scales"]
    s.x_row_stride = s.codes_row_stride = _N
    s.rows, s.n, s.dtype = _ROWS, _N, lib.FA_BF16
    _rule(s, lib, mode)
    return s, base


def _act_block(lib, buf, mode):
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaActMulQuantParams()
    s.struct_size = ctypes.sizeof(lib.FaActMulQuantParams)
    s.gate, s.up, s.codes, s.scales = base + _OFF["x"], base + _OFF["up"], base + _OFF["codes"], base + _OFF["scales"]
    s.gate_row_stride = s.up_row_stride = s.codes_row_stride = _N
    s.rows, s.n, s.dtype, s.activation = _ROWS, _N, lib.FA_FP16, lib.FA_ACT_GELU
    _rule(s, lib, mode)
    return s, base


def _norm_block(lib, buf, mode):
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaAddNormQuantParams()
    s.struct_size = ctypes.sizeof(lib.FaAddNormQuantParams)
    n = s.norm
    n.struct_size = ctypes.sizeof(lib.FaAddNormParams)
    n.x, n.residual, n.residual_out = base + _OFF["x"], base + _OFF["residual"], base + _OFF["residual_out"]
    n.weight, n.bias = base + _OFF["weight"], base + _OFF["bias"]
    n.x_row_stride = n.residual_row_stride = n.residual_out_row_stride = _N
    n.rows, n.n, n.dtype = _ROWS, _N, lib.FA_BF16
    n.residual_dtype = n.residual_out_dtype = n.weight_dtype = lib.FA_BF16
    n.is_rms_norm, n.eps = 1, 1e-6
    s.codes, s.scales, s.codes_row_stride = base + _OFF["codes"], base + _OFF["scales"], _N
    _rule(s, lib, mode)
    return s, base


_at = lambda name, add=0: (lambda b: b + _OFF[name] + add)      # noqa: E731


def _set(s, k, v):
    obj = s
    *path, leaf = k.split("__")
    for p in path:
        obj = getattr(obj, p)
    setattr(obj, leaf, v)


def _bad(call, block, lib, buf, qmode, op, match, code="(-1)", **kw):
    s, base = block(lib, buf, qmode)
    for k, v in kw.items():
        _set(s, k, v(base) if callable(v) else v)
    with pytest.raises(RuntimeError, match=match) as e:
        call(s, 0)
    assert code in str(e.value) and op in str(e.value), str(e.value)


def _reaches_the_device(call, s, rows_field="rows"):
    """a block that passes every check gets as far as the launch - FA_ERR_LAUNCH without a device, never an argument error.
    (Host pointers: where there is a device the kernel must not run on them, so only rows == 0 is called.)"""
    if torch.cuda.is_available():
        _set(s, rows_field, 0)
        call(s, 0)
        return
    try:
        call(s, 0)
    except RuntimeError as e:
        assert "(-3)" in str(e) or "(-4)" in str(e), str(e)


def _common_rule_errors(bad, mode):
    bad("unknown mode", mode=3)
    bad("unknown mode", mode=-1)
    bad("codes must not be NULL", codes=None)
    bad("reserved", reserved=(ctypes.c_int64 * 4)(0, 1, 0, 0))
    bad("has_scale_ub must be 0 or 1", has_scale_ub=2)
    if mode == "static":
        bad("finite and > 0", scale=0.0)
        bad("finite and > 0", scale=-1.0)
        bad("finite and > 0", scale=float("inf"))
        bad("finite and > 0", scale=float("nan"))
        bad("scale_ub goes with the dynamic modes", has_scale_ub=1, scale_ub=1.0)
        bad("scale_ub goes with the dynamic modes", scale_ub=1.0)
        bad("scales must be NULL", scales=_at("scales"))
    else:
        bad("scale is given in the static mode only", scale=0.5)
        bad("scales must not be NULL", scales=None)
        bad("scales must be 4-byte aligned", scales=_at("scales", 2))
        bad("scale_ub must be finite and > 0", has_scale_ub=1, scale_ub=0.0)
        bad("scale_ub must be finite and > 0", has_scale_ub=1, scale_ub=float("inf"))
        bad("scale_ub must be finite and > 0", has_scale_ub=1, scale_ub=float("nan"))
        bad("scale_ub must be 0 where has_scale_ub is 0", scale_ub=1.0)


@pytest.mark.parametrize("mode", ["row", "group", "static"])
def test_quant_fp8_argument_errors_without_gpu(lib, mode):
    buf = (ctypes.c_char * _TOTAL)()
    bad = lambda match, code="(-1)", **kw: _bad(lib.call_quant_fp8, _quant_block, lib, buf, mode, "quant_fp8", match, code, **kw)   # noqa: E731
    bad("struct_size", struct_size=8)
    bad("x must not be NULL", x=None)
    bad("fp16 or bf16", dtype=lib.FA_FP32)
    bad("fp16 or bf16", dtype=lib.FA_FP8_E4M3)
    for n in (0, 4, 260, 65544, -8):
        bad(r"multiple of 8 in \[8, 65536\]", n=n)
    _common_rule_errors(bad, mode)
    if mode == "group":
        bad("multiple of 128", n=136, x_row_stride=136, codes_row_stride=136)
    bad("rows must be non-negative", rows=-1)
    bad("row strides", x_row_stride=_N - 8)
    bad("row strides", codes_row_stride=-_N)
    bad("aligned to its element", x=_at("x", 1))
    bad(r"2\^31", code="(-2)", rows=2 ** 31)
    bad("codes overlaps x", codes=_at("x", 16))
    if mode != "static":
        bad("scales overlaps x", scales=_at("x", 64))
        bad("codes overlaps scales", scales=_at("codes", 4))
    s, _ = _quant_block(lib, buf, mode)
    _reaches_the_device(lib.call_quant_fp8, s)
    s, _ = _quant_block(lib, buf, mode)
    s.x_row_stride, s.codes_row_stride, s.rows = 2 * _N, _N + 1, 4          # a padded input, codes with any stride
    if mode != "static":
        s.has_scale_ub, s.scale_ub = 1, 2.5
    _reaches_the_device(lib.call_quant_fp8, s)


@pytest.mark.parametrize("mode", ["row", "group", "static"])
def test_act_mul_quant_argument_errors_without_gpu(lib, mode):
    buf = (ctypes.c_char * _TOTAL)()
    bad = lambda match, **kw: _bad(lib.call_act_mul_quant, _act_block, lib, buf, mode, "act_mul_quant", match, **kw)   # noqa: E731
    bad("struct_size", struct_size=ctypes.sizeof(lib.FaActMulQuantParams) - 8)
    bad("gate must not be NULL", gate=None)
    bad("reserved", reserved0=1)
    bad("fp16 or bf16", dtype=lib.FA_FP32)
    bad("unknown activation", activation=5)
    for n in (0, 12, 65544):
        bad(r"multiple of 8 in \[8, 65536\]", n=n)
    _common_rule_errors(bad, mode)
    if mode == "group":
        bad("multiple of 128", n=200)
    bad("rows must be non-negative", rows=-1)
    bad("row strides", up_row_stride=_N - 1)
    bad("aligned to their element", up=_at("up", 1))
    bad("codes overlaps gate", codes=_at("x", 8))
    bad("codes overlaps up", codes=_at("up"))
    if mode != "static":
        bad("scales overlaps up", scales=_at("up", 128))
    for ungated in (False, True):
        s, _ = _act_block(lib, buf, mode)
        if ungated:
            s.up, s.up_row_stride = None, 0
        _reaches_the_device(lib.call_act_mul_quant, s)
    s, base = _act_block(lib, buf, mode)                                       # the packed halves of one [8, 512]
    s.gate, s.up, s.gate_row_stride, s.up_row_stride = base + _OFF["x"], base + _OFF["x"] + 2 * _N, 2 * _N, 2 * _N
    s.rows = 4
    _reaches_the_device(lib.call_act_mul_quant, s)


@pytest.mark.parametrize("mode", ["row", "group", "static"])
def test_add_norm_quant_argument_errors_without_gpu(lib, mode):
    buf = (ctypes.c_char * _TOTAL)()
    bad = lambda match, **kw: _bad(lib.call_add_norm_quant, _norm_block, lib, buf, mode, "add_norm_quant", match, **kw)   # noqa: E731
    bad("struct_size", struct_size=16)
    bad("norm.struct_size", norm__struct_size=8)
    bad("norm.out must be NULL", norm__out=_at("up"))
    bad("norm.out must be NULL", norm__out_row_stride=_N)
    bad("x must not be NULL", norm__x=None)
    bad("weight must not be NULL", norm__weight=None)
    bad("fp16 or bf16", norm__dtype=lib.FA_FP32)
    for n in (0, 12, 16392):
        bad(r"multiple of 8 in \[8, 16384\]", norm__n=n)
    bad("reserved", norm__reserved=(ctypes.c_int64 * 2)(1, 0))
    bad("eps", norm__eps=float("nan"))
    _common_rule_errors(bad, mode)
    if mode == "group":
        bad("multiple of 128", norm__n=136)
    bad("codes must be 8-byte aligned", codes=_at("codes", 4))
    bad("codes must be 8-byte aligned", codes_row_stride=_N + 4)
    bad("codes must be 8-byte aligned", codes_row_stride=_N - 8)
    bad("codes overlaps x", codes=_at("x", 8))
    bad("codes overlaps residual", codes=_at("residual"))
    bad("codes overlaps weight", codes=_at("weight"))
    bad("residual_out overlaps codes", norm__residual_out=_at("codes"))
    bad("residual_out overlaps x", norm__residual_out=_at("x"))
    if mode != "static":
        bad("scales overlaps bias", scales=_at("bias"))
        bad("residual_out overlaps scales", norm__residual_out=_at("scales"))
    s, _ = _norm_block(lib, buf, mode)
    _reaches_the_device(lib.call_add_norm_quant, s, "norm__rows")
    s, _ = _norm_block(lib, buf, mode)                                        # residual_out is residual itself: legal
    s.norm.residual_out = s.norm.residual
    _reaches_the_device(lib.call_add_norm_quant, s, "norm__rows")
    s, _ = _norm_block(lib, buf, mode)                                        # no residual, no residual_out, LayerNorm, fp32 weights
    s.norm.residual = s.norm.residual_out = None
    s.norm.is_rms_norm, s.norm.weight_dtype = 0, lib.FA_FP32
    _reaches_the_device(lib.call_add_norm_quant, s, "norm__rows")


def test_wrapper_argument_errors_without_gpu():
    """the Python wrappers name what is wrong before anything is allocated; a CPU tensor itself is an error"""
    from flash_attn_mi355.quant import act_and_mul_quant, act_mul_quant, add_norm_quant, quant_fp8
    x = torch.zeros(4, 256, dtype=torch.bfloat16)
    w = torch.ones(256, dtype=torch.bfloat16)
    calls = {"quant_fp8": lambda **kw: quant_fp8(x, **kw), "add_norm_quant": lambda **kw: add_norm_quant(x, x, w, **kw),
             "act_mul_quant": lambda **kw: act_mul_quant(x, x, **kw), "act_and_mul_quant": lambda **kw: act_and_mul_quant(x, **kw)}
    for name, call in calls.items():
        op = "act_mul_quant" if name == "act_and_mul_quant" else name
        with pytest.raises(RuntimeError, match=op + ": mode must be one of"):
            call(mode="tensor")
        with pytest.raises(RuntimeError, match=op + ": mode='static' needs scale"):
            call(mode="static")
        with pytest.raises(RuntimeError, match=op + ": scale is given with mode='static' only"):
            call(mode="row", scale=1.0)
        with pytest.raises(RuntimeError, match=op + ": scale_ub goes with the dynamic modes"):
            call(mode="static", scale=1.0, scale_ub=1.0)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(RuntimeError, match=op + ": scale must be finite and > 0"):
                call(mode="static", scale=bad)
            with pytest.raises(RuntimeError, match=op + ": scale_ub must be finite and > 0"):
                call(mode="group", scale_ub=bad)
        for kw in ({}, {"mode": "group"}, {"mode": "static", "scale": 0.5}, {"scale_ub": 3.0}):
            with pytest.raises(RuntimeError, match="GPU"):      # everything else in order: the CPU tensor itself is the error
                call(**kw)
    with pytest.raises(RuntimeError, match="quant_fp8: x must be fp16 or bf16"):
        quant_fp8(x.float())
    with pytest.raises(RuntimeError, match=r"quant_fp8: N must be a multiple of 8 in \[8, 65536\]"):
        quant_fp8(x[:, :12])
    with pytest.raises(RuntimeError, match=r"quant_fp8: N must be a multiple of 8"):
        quant_fp8(torch.zeros(1, 65544, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="quant_fp8: mode='group' needs N to be a multiple of 128"):
        quant_fp8(x[:, :136], mode="group")
    with pytest.raises(RuntimeError, match=r"multiple of 8 in \[8, 16384\]"):
        add_norm_quant(torch.zeros(1, 16392, dtype=torch.float16), None, w)
    with pytest.raises(RuntimeError, match="act_mul_quant: up must have gate's dtype and shape"):
        act_mul_quant(x, x[:2])
    with pytest.raises(RuntimeError, match="activation must be one of"):
        act_mul_quant(x, x, activation="tanh")
    with pytest.raises(RuntimeError, match=r"\[\.\.\., 2N\]"):
        act_and_mul_quant(x[:, :255])
    with pytest.raises(RuntimeError, match="quant_fp8: out must be the pair"):
        quant_fp8(x, out=x)
    with pytest.raises(RuntimeError, match=r"quant_fp8: out\[0\] must be float8_e4m3fn"):
        quant_fp8(x, out=(x, None))
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="quant_fp8: x requires grad"):
        quant_fp8(xg)
    with pytest.raises(RuntimeError, match="add_norm_quant: weight requires grad"):
        add_norm_quant(x, None, w.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="act_mul_quant: up requires grad"):
        act_mul_quant(x, xg)
    with pytest.raises(RuntimeError, match="act_and_mul_quant: x requires grad"):
        act_and_mul_quant(xg)


def test_signatures():
    import flash_attn_mi355.quant as Q
    import flash_attn_mi355.act_mul as A
    import flash_attn_mi355.add_norm as N
    kinds = lambda f: {p.name: p.kind for p in inspect.signature(f).parameters.values()}            # noqa: E731
    for f in (Q.quant_fp8, Q.add_norm_quant, Q.act_mul_quant, Q.act_and_mul_quant):
        k = kinds(f)
        assert all(k[n] == inspect.Parameter.KEYWORD_ONLY for n in ("mode", "scale", "scale_ub")), f
        d = {p.name: p.default for p in inspect.signature(f).parameters.values()}
        assert d["mode"] == "row" and d["scale"] is None and d["scale_ub"] is None
    assert list(kinds(Q.quant_fp8))[:1] == ["x"] and list(kinds(Q.add_norm_quant))[:4] == ["x", "residual", "weight", "bias"]
    assert list(kinds(Q.act_mul_quant))[:2] == ["gate", "up"] and kinds(Q.act_mul_quant)["activation"] == inspect.Parameter.KEYWORD_ONLY
    # the 16-bit ops keep their signatures
    assert list(kinds(A.act_mul)) == ["gate", "up", "activation", "inplace_backward"]
    assert list(kinds(N.add_norm)) == ["x", "weight", "bias", "residual", "eps", "weight_offset", "is_rms_norm", "prenorm",
                                       "residual_in_fp32", "inplace"]
    for mod in (Q, A, N):
        assert "fp8" in mod.__doc__


def test_torch_op_schemas_and_fake_implementations():
    """the four ops are functional; the fakes give shapes, dtypes, devices and contiguous strides for strided inputs; the static
    mode's scales and a missing residual_out are empty tensors of shape (0,)"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    import flash_attn_mi355.torch_ops as T
    ns = torch.ops.flash_attn_mi355
    names = ("quant_fp8", "add_norm_quant", "act_mul_quant", "act_and_mul_quant")
    sch = {n: getattr(ns, n).default._schema for n in names}
    for n in names:
        assert not [a.name for a in sch[n].arguments if a.alias_info is not None], n
        assert n not in T.__all__                                # reached through torch.ops only
    assert [a.name for a in sch["quant_fp8"].arguments] == ["x", "mode", "scale", "scale_ub"]
    assert [a.name for a in sch["add_norm_quant"].arguments] == ["x", "residual", "weight", "bias", "eps", "weight_offset", "is_rms_norm",
                                                                 "prenorm", "residual_in_fp32", "mode", "scale", "scale_ub"]
    assert [a.name for a in sch["act_mul_quant"].arguments] == ["gate", "up", "activation", "mode", "scale", "scale_ub"]
    assert [a.name for a in sch["act_and_mul_quant"].arguments] == ["x", "activation", "mode", "scale", "scale_ub"]
    assert [len(sch[n].returns) for n in names] == [2, 3, 2, 2]
    f8, f32 = torch.float8_e4m3fn, torch.float32
    with FakeTensorMode():
        for dt in DTYPES:
            x = torch.empty(5, 7, 2048, dtype=dt, device="cuda")[..., :768]          # a strided view
            w = torch.empty(768, dtype=dt, device="cuda")
            for mode, kw, sshape in (("row", (None, None), (5, 7)), ("group", (None, 2.0), (5, 7, 6)), ("static", (0.5, None), (0,))):
                def check(c, s, last=768):
                    assert tuple(c.shape) == (5, 7, last) and c.dtype == f8 and c.is_contiguous() and c.device == x.device
                    want = sshape if mode != "group" else (5, 7, last // 128)
                    assert tuple(s.shape) == want and s.dtype == f32 and s.is_contiguous() and s.device == x.device
                check(*ns.quant_fp8(x, mode, *kw))
                check(*ns.act_mul_quant(x, x, "silu", mode, *kw))
                check(*ns.act_mul_quant(x, None, "relu2", mode, *kw))
                check(*ns.act_and_mul_quant(x, "gelu", mode, *kw), last=384)
                c, s, ro = ns.add_norm_quant(x, None, w, None, 1e-6, 0.0, True, False, False, mode, *kw)
                check(c, s)
                assert tuple(ro.shape) == (0,)
                c, s, ro = ns.add_norm_quant(x, x, w, w, 1e-6, 1.0, False, False, True, mode, *kw)
                check(c, s)
                assert ro.shape == x.shape and ro.dtype == f32 and ro.is_contiguous()
                c, s, ro = ns.add_norm_quant(x, None, w, None, 1e-6, 0.0, True, True, False, mode, *kw)
                assert ro.shape == x.shape and ro.dtype == dt


def test_public_name_lists_are_unchanged():
    import flash_attn
    import flash_attn_mi355
    import flash_attn_mi355.torch_ops as T
    assert flash_attn.__all__ == ["flash_attn_func", "flash_attn_gpu", "flash_attn_varlen_func", "flash_attn_varlen_gpu",
                                  "flash_attn_with_kvcache", "flash_attn_with_kvcache_gpu", "flash_attn_qkvpacked_func",
                                  "flash_attn_kvpacked_func", "flash_attn_varlen_qkvpacked_func",
                                  "flash_attn_varlen_kvpacked_func", "__version__"]
    for name in ("quant", "quant_fp8", "add_norm_quant", "act_mul_quant", "act_and_mul_quant"):
        assert name not in flash_attn.__all__ and name not in flash_attn_mi355.__all__ and name not in T.__all__
    assert T.__all__[:12] == ["fwd", "bwd", "varlen_fwd", "varlen_bwd", "fwd_kvcache", "fwd_kvcache_tree", "fwd_out",
                              "varlen_fwd_out", "bwd_out", "merge_states", "rotary", "rotary_"] and T.__all__[12:] == ["kv_store"]
