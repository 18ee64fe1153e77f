"""CPU: the host side of fa_act_mul / fa_act_mul_bwd - the fp64 yardstick of the GPU tests against torch's own activations and
their autograd, its special values, the bounds on the GPU tests' inputs, the launch plan against the library's query, the C ABI's
argument checks on host pointers, the ctypes mirrors, the torch.library ops' schemas and fake implementations, and the
upstream-named wrappers' signatures.  Nothing here needs a GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import act_mul_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


_TORCH = {"silu": F.silu, "gelu": lambda x: F.gelu(x, approximate="none"), "gelu_tanh": lambda x: F.gelu(x, approximate="tanh"),
          "relu": torch.relu, "relu2": lambda x: torch.relu(x) ** 2}


# the yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("activation", R.ACTIVATIONS)
def test_reference_equals_torch_and_its_autograd(activation, gated):
    """act_mul_ref == torch's activation times up in float64 and torch autograd of that composition, to 1e-12 (relative to the
    largest value)"""
    g, u, d = R.inputs(23, 301, torch.float32, seed=3)
    g[(g.abs() > 20) | (g == 0)] = 0.5                       # (torch's own float64 gelu and relu'(0) are not what is compared here)
    u = u if gated else None
    g64 = g.double().requires_grad_(True)
    u64 = None if u is None else u.double().requires_grad_(True)
    y = _TORCH[activation](g64) * (1 if u64 is None else u64)
    out, D = R.forward_ref(g, u, activation)
    rel = lambda a, c: float((a - c).abs().max() / c.abs().max().clamp(min=1e-300))       # noqa: E731
    assert rel(out, y.detach()) <= 1e-12
    grads = torch.autograd.grad(y, (g64,) if u64 is None else (g64, u64), d.double())
    dg, dp, Dg, Dp = R.backward_ref(d, g, u, activation)
    assert rel(dg, grads[0]) <= 1e-12
    assert (dp is None) == (not gated) and (dp is None or rel(dp, grads[1]) <= 1e-12)
    assert (D >= 0).all() and (Dg >= 0).all()


def test_reference_special_values():
    """the values flash_attn_mi355/act_mul.py documents, on the reference: act(-100) and act'(-100) are finite and below 2^-126
    - where the kernel's e overflows and gives -0 -, never NaN; +-0 gives 0 and 0.5 (the ReLUs: 0 and 0); act(100) = 100 and
    act' = 1"""
    g = torch.tensor([-100.0, 100.0, 0.0, -0.0, -30.0, 30.0])
    for act in R.ACTIVATIONS:
        a, d, Da, Dd = R.act_ref(g, act)
        assert torch.isfinite(a).all() and torch.isfinite(d).all() and torch.isfinite(Da).all() and torch.isfinite(Dd).all()
        assert abs(float(a[0])) < R.FLUSH and abs(float(d[0])) < R.FLUSH and float(a[2]) == 0 and float(a[3]) == 0
        if act in ("relu", "relu2"):
            assert float(d[2]) == 0 and float(d[3]) == 0 and float(a[1]) == (100.0 if act == "relu" else 1e4)
        else:
            assert float(d[2]) == 0.5 and float(d[3]) == 0.5 and float(a[1]) == 100.0 and float(d[1]) == 1.0
            assert abs(float(a[4])) < 1e-11 and float(a[5]) == pytest.approx(30.0, rel=1e-11)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("N", [264, 1001])
def test_bounds_are_not_vacuous(N, dtype):
    """on the inputs the GPU tests use: the reference rounded once lies inside the bounds; the two-rounding form of HF / vLLM
    (bf16), gate and up swapped, the erf and the tanh GELU exchanged, silu' without its g (1 - s) term and dup from act' instead
    of act each lie outside them somewhere by more than 2x"""
    g, u, d = R.inputs(12, N, dtype, seed=N)
    W = lambda got, ref, D, wrong=True: R.worst(got.to(dtype), ref, R.bound(ref, D, dtype), wrong, dtype)   # noqa: E731
    for act in R.ACTIVATIONS:
        for up in (u, None):
            out, D = R.forward_ref(g, up, act)
            dg, dp, Dg, Dp = R.backward_ref(d, g, up, act)
            assert W(out, out, D, False) <= 1.0 and W(dg, dg, Dg, False) <= 1.0 and (dp is None or W(dp, dp, Dp, False) <= 1.0)
        out, D = R.forward_ref(g, u, act)
        dg, dp, Dg, Dp = R.backward_ref(d, g, u, act)
        assert W(R.forward_ref(u, g, act)[0], out, D) > 2.0, act                         # gate and up swapped
        assert W(R.backward_ref(d, g, u, act, leave_out="dup_act")[1], dp, Dp) > 2.0, act
        if act.startswith("gelu"):
            other = "gelu" if act == "gelu_tanh" else "gelu_tanh"
            assert W(R.forward_ref(g, u, other)[0], out, D) > 2.0 and W(R.backward_ref(d, g, u, other)[0], dg, Dg) > 2.0
            assert W(R.forward_ref(g, None, other)[0], *R.forward_ref(g, None, act)) > 2.0
        if act == "silu":
            assert W(R.backward_ref(d, g, u, act, leave_out="silu_term")[0], dg, Dg) > 2.0
            if dtype == torch.bfloat16:
                a16 = R.act_ref(g, act)[0].to(dtype)
                assert W(a16.double() * u.double(), out, D) > 2.0                         # round16(round16(silu) * up)
                assert float(((a16 * u).double() != out.to(dtype).double()).float().mean()) > 0.1


def test_plan_restated(lib):
    """act_mul_ref.plan() restates csrc/fa_act_mul.hip's act_plan, which the library answers without a device: runs of equal
    length within a row, whole waves of pieces, a grid capped at GRID_CAP"""
    for rows in (1, 3, 67, 128, 8192, 65536, 2 ** 20):
        for N in (1, 7, 8, 9, 264, 1001, R.STEP, R.STEP + 8, 8192, 8193, 11008, 14336, 18944, 28672, R.second_trip_n(67), 2 ** 31 - 1):
            p = R.plan(rows, N)
            if p["items"] > 2 ** 31 - 1:
                with pytest.raises(RuntimeError, match=r"\(-2\).*2\^31"):
                    lib.act_mul_plan(rows, N)
                continue
            assert lib.act_mul_plan(rows, N) == (p["run_columns"], p["items"], p["grid"]), (rows, N)
            assert p["run_columns"] % 512 == 0 and p["run_columns"] <= 8192 and p["nchunks"] * p["run_columns"] >= N
            assert (p["nchunks"] - 1) * p["run_columns"] < N
    # the MLP widths: the runs of a row differ by less than a wave's 512 columns - no workgroup a quarter empty
    for N, runs in ((11008, 2), (14336, 2), (18944, 3), (28672, 4)):
        p = R.plan(8192, N)
        assert p["nchunks"] == runs and p["run_columns"] - (N - (runs - 1) * p["run_columns"]) < 512 * runs
    assert R.plan(67, R.second_trip_n(67))["items"] > R.GRID_CAP == R.plan(67, R.second_trip_n(67))["grid"]
    with pytest.raises(RuntimeError, match=r"\(-1\).*n must be at least 1"):
        lib.act_mul_plan(4, 0)
    with pytest.raises(RuntimeError, match=r"\(-1\).*rows"):
        lib.act_mul_plan(-1, 8)


# the C ABI -------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_struct_sizes(lib):
    for name in ("fa_act_mul", "fa_act_mul_params_size", "fa_act_mul_plan", "fa_act_mul_bwd", "fa_act_mul_bwd_params_size"):
        assert hasattr(lib.lib, name) and name in lib.EXPORTS
    assert lib.lib.fa_act_mul_params_size() == ctypes.sizeof(lib.FaActMulParams)
    assert lib.lib.fa_act_mul_bwd_params_size() == ctypes.sizeof(lib.FaActMulBwdParams)
    assert lib.FA_ABI_VERSION == 4 and lib.lib.fa_abi_version() == 4
    rows = {e: (s, q) for e, s, q in lib.ROW_OPS}
    assert rows["fa_act_mul"] == (lib.FaActMulParams, None) and rows["fa_act_mul_bwd"] == (lib.FaActMulBwdParams, None)
    assert callable(lib.call_act_mul) and callable(lib.call_act_mul_bwd)


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
    for cname, mirror in (("fa_act_mul_params", lib.FaActMulParams), ("fa_act_mul_bwd_params", lib.FaActMulBwdParams)):
        fields = _header_fields(cname)
        assert [f[0] for f in mirror._fields_] == fields
        assert fields[0] == "struct_size" and fields[-1] == "reserved"
        assert ctypes.sizeof(mirror) % 8 == 0 and ctypes.sizeof(dict(mirror._fields_)["reserved"]) == 32
    body = re.search(r"typedef enum fa_act \{(.*?)\} fa_act;", _header(), flags=re.S).group(1)
    enum = {k: int(v) for k, v in re.findall(r"(FA_ACT_\w+)\s*=\s*(\d+)", body)}
    assert enum == {"FA_ACT_SILU": lib.FA_ACT_SILU, "FA_ACT_GELU": lib.FA_ACT_GELU, "FA_ACT_GELU_TANH": lib.FA_ACT_GELU_TANH,
                    "FA_ACT_RELU": lib.FA_ACT_RELU, "FA_ACT_RELU2": lib.FA_ACT_RELU2}
    from flash_attn_mi355 import act_mul
    assert set(act_mul.ACTIVATIONS) == set(R.ACTIVATIONS) and sorted(act_mul.ACTIVATIONS.values()) == [0, 1, 2, 3, 4]


# host buffers behind valid blocks: five [8, 64] tensors and one packed [8, 128] pair
_T = 8 * 64 * 2
_OFF = {n: i * _T for i, n in enumerate(("gate", "up", "out", "dout", "dgate", "dup", "packed", "packed_hi", "dpacked", "dpacked_hi"))}
_TOTAL = len(_OFF) * _T + 64


def _fwd_block(lib, buf, form="gated"):
    """a valid fa_act_mul block over host memory: 8 rows of 64 columns.  form: 'gated', 'ungated', 'view' (5 rows, strides 96),
    'packed' (the halves of one [8, 128]), 'on_gate' / 'on_up' (out is exactly gate / up)"""
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaActMulParams()
    s.struct_size = ctypes.sizeof(lib.FaActMulParams)
    s.gate, s.up, s.out = base + _OFF["gate"], base + _OFF["up"], base + _OFF["out"]
    s.rows, s.n, s.dtype, s.activation = 8, 64, lib.FA_BF16, lib.FA_ACT_SILU
    s.gate_row_stride = s.up_row_stride = s.out_row_stride = 64
    if form == "ungated":
        s.up, s.up_row_stride = None, 0
    elif form == "view":
        s.rows, s.gate_row_stride, s.up_row_stride = 5, 96, 96
    elif form == "packed":
        s.gate, s.up = base + _OFF["packed"], base + _OFF["packed"] + 128
        s.gate_row_stride = s.up_row_stride = 128
    elif form == "on_gate":
        s.out = s.gate
    elif form == "on_up":
        s.out = s.up
    return s, base


def _bwd_block(lib, buf, form="gated"):
    """a valid fa_act_mul_bwd block.  form: 'gated', 'ungated', 'inplace' (dgate = gate, dup = up), 'packed' (gate / up and dgate
    / dup the halves of one packed tensor each), 'packed_inplace' (the gradient over the packed input itself)"""
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaActMulBwdParams()
    s.struct_size = ctypes.sizeof(lib.FaActMulBwdParams)
    for name in ("dout", "gate", "up", "dgate", "dup"):
        setattr(s, name, base + _OFF[name])
        setattr(s, name + "_row_stride", 64)
    s.rows, s.n, s.dtype, s.activation = 8, 64, lib.FA_FP16, lib.FA_ACT_GELU
    if form == "ungated":
        s.up = s.dup = None
    elif form == "inplace":
        s.dgate, s.dup = s.gate, s.up
    elif form in ("packed", "packed_inplace"):
        s.gate, s.up = base + _OFF["packed"], base + _OFF["packed"] + 128
        s.dgate, s.dup = (s.gate, s.up) if form == "packed_inplace" else (base + _OFF["dpacked"], base + _OFF["dpacked"] + 128)
        s.gate_row_stride = s.up_row_stride = s.dgate_row_stride = s.dup_row_stride = 128
    return s, base


_at = lambda name, add=0: (lambda b: b + _OFF[name] + add)      # noqa: E731


def _bad(lib, call, block, op, buf, match, form, code="(-1)", **kw):
    s, base = block(lib, buf, form)
    for k, v in kw.items():
        setattr(s, k, v(base) if callable(v) else v)
    with pytest.raises(RuntimeError, match=match) as e:
        call(s, 0)
    assert code in str(e.value) and op in str(e.value)


def _reaches_the_device(call, s):
    """a block that passes every check: the call gets as far as the launch - FA_ERR_LAUNCH (-3) without a device, never an
    argument error.  (Host pointers: where there is a device the kernel must not run on them, so only rows == 0 is called.)"""
    if torch.cuda.is_available():
        s.rows = 0
        call(s, 0)
        return
    try:
        call(s, 0)
    except RuntimeError as e:
        assert "(-3)" in str(e) or "(-4)" in str(e), str(e)


def test_forward_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_act_mul fires before any device work; the packed halves and the exact aliases
    pass the checks"""
    buf = (ctypes.c_char * _TOTAL)()
    bad = lambda match, form="gated", **kw: _bad(lib, lib.call_act_mul, _fwd_block, "act_mul", buf, match, form, **kw)   # noqa: E731
    forms = ("gated", "ungated", "view", "packed", "on_gate", "on_up")
    for form in forms:
        bad("struct_size", form, struct_size=8)
        bad("struct_size", form, struct_size=ctypes.sizeof(lib.FaActMulParams) - 8)
        bad("must not be NULL", form, gate=None)
        bad("must not be NULL", form, out=None)
        bad("reserved", form, reserved=(ctypes.c_int64 * 4)(0, 0, 1, 0))
        bad("reserved", form, reserved0=1)
        bad("fp16 or bf16", form, dtype=lib.FA_FP32)
        bad("fp16 or bf16", form, dtype=lib.FA_FP8_E4M3)
        bad("unknown activation", form, activation=5)
        bad("unknown activation", form, activation=-1)
        bad("n must be at least 1", form, n=0)
        bad("n must be at least 1", form, n=-64)
        bad("rows must be non-negative", form, rows=-1)
        bad("row strides", form, gate_row_stride=-64)
        bad("row strides", form, out_row_stride=63)
        bad("aligned", form, gate=_at("gate", 1))
        bad("aligned", form, out=_at("out", 1))
    for form in ("gated", "view", "packed"):
        bad("row strides", form, up_row_stride=32)
        bad("aligned", form, up=_at("up", 3))
    bad("out overlaps gate", out=_at("gate", 16))                      # shifted by 8 elements: not the exact alias
    bad("out overlaps up", out=_at("up", 2 * 64 * 2))                  # two rows further
    bad("out shares gate's base", "on_gate", out_row_stride=128)
    bad("out shares up's base", "on_up", out_row_stride=96, rows=1)
    bad("out overlaps gate", "packed", out=_at("packed", 64), out_row_stride=128)        # straddles both halves
    bad("out overlaps up", "on_gate", up=_at("gate", 32))              # out == gate is fine, but up lies inside it
    s, _ = _fwd_block(lib, buf)
    s.rows, s.n = 2 ** 31 - 1, 8192 + 8
    s.gate_row_stride = s.up_row_stride = s.out_row_stride = s.n
    with pytest.raises(RuntimeError, match=r"\(-2\).*2\^31"):           # FA_ERR_UNSUPPORTED
        lib.call_act_mul(s, 0)
    for form in forms:
        s, _ = _fwd_block(lib, buf, form)
        s.rows = 0                                                      # rows == 0: FA_OK without a launch
        lib.call_act_mul(s, 0)
        _reaches_the_device(lib.call_act_mul, _fwd_block(lib, buf, form)[0])
    s, base = _fwd_block(lib, buf, "packed")                            # out over the gate half of the packed tensor
    s.out, s.out_row_stride = s.gate, 128
    _reaches_the_device(lib.call_act_mul, s)


def test_backward_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_act_mul_bwd fires before any device work; the packed-halves and exact-alias
    blocks pass the checks"""
    buf = (ctypes.c_char * _TOTAL)()
    bad = lambda match, form="gated", **kw: _bad(lib, lib.call_act_mul_bwd, _bwd_block, "act_mul_bwd", buf, match, form, **kw)   # noqa: E731
    forms = ("gated", "ungated", "inplace", "packed", "packed_inplace")
    for form in forms:
        bad("struct_size", form, struct_size=ctypes.sizeof(lib.FaActMulBwdParams) - 8)
        for name in ("dout", "gate", "dgate"):
            bad("must not be NULL", form, **{name: None})
        bad("reserved", form, reserved=(ctypes.c_int64 * 4)(1, 0, 0, 0))
        bad("reserved", form, reserved0=-1)
        bad("fp16 or bf16", form, dtype=lib.FA_FP32)
        bad("unknown activation", form, activation=7)
        bad("n must be at least 1", form, n=0)
        bad("rows must be non-negative", form, rows=-2)
        bad("row strides", form, dout_row_stride=60)
        bad("row strides", form, dgate_row_stride=-64)
        bad("aligned", form, dout=_at("dout", 1))
        bad("aligned", form, dgate=_at("dgate", 1))
    bad("up and dup go together", "gated", dup=None)
    bad("up and dup go together", "gated", up=None)
    bad("up and dup go together", "ungated", dup=_at("dup"))
    bad("up and dup go together", "ungated", up=_at("up"))
    bad("dgate shares gate's base", "inplace", dgate_row_stride=128)
    bad("dup shares up's base", "inplace", dup_row_stride=128)
    bad("dgate overlaps gate", dgate=_at("gate", 16))
    bad("dgate overlaps up", dgate=_at("up", 0))                        # dgate over up: not its own input
    bad("dup overlaps gate", dup=_at("gate", 0))
    bad("dgate overlaps dout", dgate=_at("dout", 0))
    bad("dup overlaps dout", dup=_at("dout", 0))
    bad("dgate overlaps dup", dup=_at("dgate", 32))
    bad("dgate overlaps up|dgate overlaps gate", "packed", dgate=_at("packed", 64))      # straddles both halves
    bad("dgate overlaps dup", "packed", dup=_at("dpacked", 64))
    s, _ = _bwd_block(lib, buf)
    s.rows, s.n = 2 ** 31 - 1, 8192 + 8
    for name in ("dout", "gate", "up", "dgate", "dup"):
        setattr(s, name + "_row_stride", s.n)
    with pytest.raises(RuntimeError, match=r"\(-2\).*2\^31"):
        lib.call_act_mul_bwd(s, 0)
    for form in forms:
        s, _ = _bwd_block(lib, buf, form)
        s.rows = 0
        lib.call_act_mul_bwd(s, 0)
        _reaches_the_device(lib.call_act_mul_bwd, _bwd_block(lib, buf, form)[0])


# Python ----------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors_on_cpu_tensors():
    from flash_attn_mi355.act_mul import act_and_mul, act_mul, act_mul_backward, act_mul_forward
    g = torch.zeros(4, 6, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="activation must be one of"):
        act_mul_forward(g, g, activation="swish")
    with pytest.raises(RuntimeError, match="activation must be one of"):
        act_and_mul(g, activation="glu")
    with pytest.raises(RuntimeError, match="gate must be fp16 or bf16"):
        act_mul_forward(g.float(), g.float())
    with pytest.raises(RuntimeError, match=r"\[\.\.\., N\] with N >= 1"):
        act_mul_forward(g[..., :0])
    with pytest.raises(RuntimeError, match="up must have gate's dtype"):
        act_mul_forward(g, g.half())
    with pytest.raises(RuntimeError, match="up must have gate's shape"):
        act_mul_forward(g, g[:2])
    with pytest.raises(RuntimeError, match="out must have gate's shape"):
        act_mul_forward(g, g, out=g[..., :32])
    with pytest.raises(RuntimeError, match="dout must have gate's shape"):
        act_mul_backward(g[:1], g, g)
    with pytest.raises(RuntimeError, match="exclude each other"):
        act_mul_backward(g, g, g, inplace=True, out=(g, g))
    with pytest.raises(RuntimeError, match="out must be the pair"):
        act_mul_backward(g, g, g, out=g)
    with pytest.raises(RuntimeError, match="dup exactly where up is given"):
        act_mul_backward(g, g, g, out=(g, None))
    with pytest.raises(RuntimeError, match="dup exactly where up is given"):
        act_mul_backward(g, g, None, out=(g, g))
    with pytest.raises(RuntimeError, match=r"\[\.\.\., 2N\]"):
        act_and_mul(g[..., :63])
    # everything else in order: the CPU tensor itself is the error - there is no torch fallback
    for call in (lambda: act_mul_forward(g, g, activation="gelu"), lambda: act_mul_forward(g, out=g),
                 lambda: act_mul_backward(g, g, g, activation="gelu_tanh", inplace=True),
                 lambda: act_mul_backward(g, g, out=(g.clone(), None)), lambda: act_mul(g, g, inplace_backward=True),
                 lambda: act_mul(g, activation="relu2"), lambda: act_and_mul(g, activation="relu")):
        with pytest.raises(RuntimeError, match="GPU"):
            call()


def test_torch_op_schemas_and_fake_implementations():
    """act_mul / act_and_mul / act_mul_bwd / act_and_mul_bwd are functional, act_mul_bwd_ writes gate and up; the fake
    implementations give the shapes, dtypes and contiguous strides for a strided input; the ungated act_mul_bwd returns an empty
    dup"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    import flash_attn_mi355.torch_ops as T
    ns = torch.ops.flash_attn_mi355
    sch = {n: getattr(ns, n).default._schema for n in ("act_mul", "act_and_mul", "act_mul_bwd", "act_and_mul_bwd", "act_mul_bwd_")}
    written = lambda s: [a.name for a in s.arguments if a.alias_info is not None and a.alias_info.is_write]   # noqa: E731
    for n in ("act_mul", "act_and_mul", "act_mul_bwd", "act_and_mul_bwd"):
        assert not [a.name for a in sch[n].arguments if a.alias_info is not None], n
    assert written(sch["act_mul_bwd_"]) == ["gate", "up"]
    assert [a.name for a in sch["act_mul"].arguments] == ["gate", "up", "activation", "inplace_backward"]
    assert [a.name for a in sch["act_and_mul"].arguments] == ["x", "activation", "inplace_backward"]
    assert [a.name for a in sch["act_mul_bwd"].arguments] == ["dout", "gate", "up", "activation"]
    assert [a.name for a in sch["act_mul_bwd_"].arguments] == ["dout", "gate", "up", "activation"]
    assert [a.name for a in sch["act_and_mul_bwd"].arguments] == ["dout", "x", "activation"]
    assert [len(sch[n].returns) for n in ("act_mul", "act_and_mul", "act_mul_bwd", "act_and_mul_bwd", "act_mul_bwd_")] == [1, 1, 2, 1, 0]
    with FakeTensorMode():
        for dt in (torch.float16, torch.bfloat16):
            x = torch.empty(5, 7, 2048, dtype=dt, device="cuda")[..., :2002]         # a strided view
            gate, up = x[..., :1001], x[..., 1001:]
            for u in (up, None):
                out = ns.act_mul(gate, u, "silu", False)
                assert out.shape == gate.shape and out.dtype == dt and out.is_contiguous()
                dg, dp = ns.act_mul_bwd(out, gate, u, "silu")
                assert dg.shape == gate.shape and dg.dtype == dt and dg.is_contiguous()
                assert (dp.shape == gate.shape and dp.is_contiguous()) if u is not None else tuple(dp.shape) == (0,)
                assert ns.act_mul_bwd_(out, gate, u, "gelu") is None
            out = ns.act_and_mul(x, "gelu_tanh", False)
            assert tuple(out.shape) == (5, 7, 1001) and out.dtype == dt and out.is_contiguous()
            dx = ns.act_and_mul_bwd(out, x, "gelu_tanh")
            assert dx.shape == x.shape and dx.dtype == dt and dx.is_contiguous()
    for name in sch:
        assert name not in T.__all__                        # reached through torch.ops only


def test_public_name_lists_are_unchanged():
    import flash_attn
    import flash_attn_mi355
    for name in ("act_mul", "act_and_mul", "act_mul_forward", "act_mul_backward", "swiglu", "activations", "gelu_fwd"):
        assert name not in flash_attn.__all__ and name not in flash_attn_mi355.__all__


# the upstream-named wrappers ---------------------------------------------------------------------------------------------------
def _sig(f):
    return [(p.name, p.default if p.default is not inspect.Parameter.empty else "<required>")
            for p in inspect.signature(f).parameters.values()]


_REQ = "<required>"


def test_upstream_named_entries_have_the_specified_signatures():
    import flash_attn.ops.activations as A
    import flash_attn_mi355.act_mul as M
    req = lambda *names: [(n, _REQ) for n in names]           # noqa: E731
    assert _sig(A.swiglu) == req("x", "y") and _sig(A.swiglu_fwd) == req("x", "y") and _sig(A.swiglu_bwd) == req("x", "y", "g")
    assert _sig(A.gelu_fwd) == req("x") and _sig(A.gelu_bwd) == req("g", "x") and _sig(A.fast_gelu_impl) == req("x")
    assert _sig(A.sqrelu_fwd) == req("x") and _sig(A.sqrelu_bwd) == req("g", "x") and _sig(A.relu_bwd) == req("g", "x")
    for name in ("bias_gelu", "bias_gelu_back", "bias_gelu_impl"):
        assert not hasattr(A, name)                          # a bias gradient is a column sum: out of scope
    assert _sig(M.act_mul_forward) == [("gate", _REQ), ("up", None), ("activation", "silu"), ("out", None)]
    assert _sig(M.act_mul_backward) == [("dout", _REQ), ("gate", _REQ), ("up", None), ("activation", "silu"), ("inplace", False),
                                        ("out", None)]
    assert _sig(M.act_mul) == [("gate", _REQ), ("up", None), ("activation", "silu"), ("inplace_backward", False)]
    assert _sig(M.act_and_mul) == [("x", _REQ), ("activation", "silu"), ("inplace_backward", False)]
    for f, kw in ((M.act_mul_forward, ("activation", "out")), (M.act_mul_backward, ("activation", "inplace", "out")),
                  (M.act_mul, ("activation", "inplace_backward")), (M.act_and_mul, ("activation", "inplace_backward"))):
        kinds = {p.name: p.kind for p in inspect.signature(f).parameters.values()}
        assert all(kinds[n] == inspect.Parameter.KEYWORD_ONLY for n in kw)
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    for call in (lambda: A.swiglu(x, x), lambda: A.swiglu_fwd(x, x), lambda: A.swiglu_bwd(x, x, x), lambda: A.gelu_fwd(x),
                 lambda: A.gelu_bwd(x, x), lambda: A.fast_gelu_impl(x), lambda: A.sqrelu_fwd(x), lambda: A.sqrelu_bwd(x, x),
                 lambda: A.relu_bwd(x, x)):
        with pytest.raises(RuntimeError, match="GPU"):       # everything served: the CPU tensor itself is the error
            call()
