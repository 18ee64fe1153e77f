"""CPU: the host side of fa_add_norm / fa_add_norm_bwd - the fp64 yardstick of the GPU tests against torch autograd, the C ABI's
argument checks on host pointers, the ctypes mirrors, the workspace query (which needs no device), the torch.library ops' schemas
and fake implementations, the upstream-named wrappers' signatures and the arguments they do not serve.  Nothing here needs a GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import add_norm_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


# the yardstick ---------------------------------------------------------------------------------------------------------------
def _inputs(rows, n, dtype, seed=0, ln=False):
    """rows of magnitude 1e-3, 1 and 1e2 side by side; LayerNorm: a row mean of four standard deviations; weights around 1 with
    both signs; a non-zero bias"""
    g = torch.Generator().manual_seed(100 + seed)
    scale = torch.tensor([1e-3, 1.0, 1e2])[torch.arange(rows) % 3][:, None]
    mean = 4.0 * scale if ln else 0.0
    x = (torch.randn(rows, n, generator=g) * scale + mean).to(dtype)
    res = (torch.randn(rows, n, generator=g) * scale + mean).to(dtype)
    dy = torch.randn(rows, n, generator=g).to(dtype)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    w = (sign * (1 + 0.2 * torch.randn(n, generator=g))).to(dtype)
    b = (0.5 * torch.randn(n, generator=g)).to(dtype)
    return x, res, dy, w, b


@pytest.mark.parametrize("is_rms", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("prenorm", [True, False])
def test_reference_backward_equals_autograd_of_the_float64_composition(is_rms, bias, prenorm):
    """add_norm_ref.backward_ref (the analytic formulas of the op) == torch autograd of forward64 to 1e-12 relative; norm_ref ==
    forward64; the magnitudes bound what they are meant to bound"""
    rows, n, eps, off = 13, 72, 1e-6, 1.0
    x, res, dy, w, b = _inputs(rows, n, torch.bfloat16, ln=not is_rms)
    b = b if bias else None
    z = R.add_ref(x, res, torch.bfloat16)
    dro = torch.randn(rows, n, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16) if prenorm else None
    z64 = z.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = None if b is None else b.double().requires_grad_(True)
    y = R.forward64(z64, w64, b64, R._f32(eps), R._f32(off), is_rms)
    loss_in = [z64, w64] + ([] if b is None else [b64])
    outs, gouts = [y], [dy.double()]
    if prenorm:
        outs.append(z64 * 1.0)
        gouts.append(dro.double())
    grads = torch.autograd.grad(outs, loss_in, gouts)
    ref = R.backward_ref(dy, z, w, dro, eps, off, is_rms)
    rel = lambda a, c: float((a - c).abs().max() / c.abs().max())       # noqa: E731
    assert rel(ref["dz"], grads[0]) <= 1e-12
    assert rel(ref["dw"], grads[1]) <= 1e-12
    if bias:
        assert rel(ref["db"], grads[2]) <= 1e-12
    yr, M = R.norm_ref(z, w, b, eps, off, is_rms)
    assert rel(yr, y.detach()) <= 1e-12
    assert (M >= yr.abs() * (1 - 1e-12)).all() and (ref["A"] >= ref["dz"].abs() * (1 - 1e-12)).all()
    assert (ref["Sw"] >= ref["dw"].abs() * (1 - 1e-12)).all() and (ref["Sb"] >= ref["db"].abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n", [8, 264, 16384])
def test_forward_bound_is_not_vacuous(n, dtype):
    """on the inputs the GPU tests use, the reference with eps, the bias, weight_offset or the mean subtraction left out lies
    outside the forward bound - and the reference rounded once lies inside it"""
    rows, eps, off = 6, 1e-6, 1.0
    for is_rms in (True, False):
        x, res, _, w, b = _inputs(rows, n, dtype, seed=n, ln=not is_rms)
        z = R.add_ref(x, res, dtype)
        y, M = R.norm_ref(z, w, b, eps, off, is_rms)
        bound = R.fwd_bound(y, M, n, dtype)
        assert R.worst(y.to(dtype), y, bound) <= 1.0
        assert float((bound / (0.5 * R.ulp(y, dtype))).median()) < 1.25   # the fp32 part is a fraction of the rounding to 16 bits
        for term in ("eps", "bias", "offset") + (() if is_rms else ("mean",)):
            wrong, _ = R.norm_ref(z, w, b, eps, off, is_rms, leave_out=term)
            assert R.worst(wrong.to(dtype), y, bound) > 2.0, (term, is_rms)


def test_depth_and_plan_restated(lib):
    """add_norm_ref.depth() / plan() restate csrc/fa_rowsum.h and csrc/fa_add_norm_bwd.hip: the workspace the library reports"""
    assert [R.row_shape(n) for n in (8, 72, 256, 264, 1000, 4096, 5120, 16384)] == [
        (1, 1, 1), (16, 1, 1), (32, 1, 1), (64, 1, 1), (128, 1, 2), (256, 2, 4), (256, 4, 4), (256, 8, 4)]
    assert R.depth(16384) == 24 and R.depth(8) == 8
    buf = (ctypes.c_char * _TOTAL)()
    for rows, n, db in ((1, 8, False), (67, 72, True), (1031, 256, True), (1031, 264, False), (65536, 4096, True), (3, 16384, True),
                        (2 ** 31 - 1, 16384, True), (100000, 64, False)):
        s, _ = _bwd_block(lib, buf)
        s.rows, s.n = rows, n
        s.dy_row_stride = s.z_row_stride = s.dx_row_stride = s.dres_out_row_stride = s.dres_row_stride = n
        if not db:
            s.dbias = None
        assert lib.add_norm_bwd_workspace_bytes(s) == R.plan(rows, n, db)["workspace_bytes"], (rows, n, db)


# the C ABI -------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_struct_sizes(lib):
    for name in ("fa_add_norm", "fa_add_norm_params_size", "fa_add_norm_bwd", "fa_add_norm_bwd_workspace_bytes",
                 "fa_add_norm_bwd_params_size"):
        assert hasattr(lib.lib, name) and name in lib.EXPORTS
    assert lib.lib.fa_add_norm_params_size() == ctypes.sizeof(lib.FaAddNormParams)
    assert lib.lib.fa_add_norm_bwd_params_size() == ctypes.sizeof(lib.FaAddNormBwdParams)
    assert lib.FA_ABI_VERSION == 4 and lib.lib.fa_abi_version() == 4


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


def test_ctypes_mirrors_match_the_header(lib):
    for cname, mirror in (("fa_add_norm_params", lib.FaAddNormParams), ("fa_add_norm_bwd_params", lib.FaAddNormBwdParams)):
        fields = _header_fields(cname)
        assert [f[0] for f in mirror._fields_] == fields
        assert fields[0] == "struct_size" and fields[-1] == "reserved"
        assert ctypes.sizeof(mirror) % 8 == 0


# host buffers behind valid blocks: [8, 64] tensors with room for fp32, [64] parameters with room for fp32, a workspace
_T = 8 * 64 * 4
_W = 64 * 4
_WS = 1 << 12
_OFF = {}
_o = 0
for _n, _sz in (("x", _T), ("residual", _T), ("out", _T), ("residual_out", _T), ("dy", _T), ("z", _T), ("dres_out", _T), ("dx", _T),
                ("dres", _T), ("weight", _W), ("bias", _W), ("dweight", _W), ("dbias", _W), ("workspace", _WS)):
    _OFF[_n] = _o
    _o += _sz
_TOTAL = _o + 64


def _fwd_block(lib, buf, form="out"):
    """a valid fa_add_norm block over host memory.  form: 'out' (residual, out of place), 'inplace' (out = x, residual_out =
    residual), 'plain' (no residual, no residual_out, no bias), 'fp32' (fp32 residual, residual_out and weights)"""
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaAddNormParams()
    s.struct_size = ctypes.sizeof(lib.FaAddNormParams)
    s.x, s.out, s.weight = base + _OFF["x"], base + _OFF["out"], base + _OFF["weight"]
    s.x_row_stride = s.out_row_stride = 64
    s.rows, s.n = 8, 64
    s.dtype = s.weight_dtype = s.residual_dtype = s.residual_out_dtype = lib.FA_FP16
    s.is_rms_norm, s.eps = 1, 1e-6
    if form != "plain":
        s.residual, s.residual_out, s.bias = base + _OFF["residual"], base + _OFF["residual_out"], base + _OFF["bias"]
        s.residual_row_stride = s.residual_out_row_stride = 64
    if form == "inplace":
        s.out, s.residual_out = s.x, s.residual
    if form == "fp32":
        s.residual_dtype = s.residual_out_dtype = s.weight_dtype = lib.FA_FP32
    return s, base


def _bwd_block(lib, buf, form="out"):
    """a valid fa_add_norm_bwd block.  form: 'out' (dx, dres, dweight, dbias, dres_out), 'inplace' (dx = dy), 'nodw' (no weight
    or bias gradient, no workspace), 'fp32' (fp32 z, dres_out, dres and weights)"""
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaAddNormBwdParams()
    s.struct_size = ctypes.sizeof(lib.FaAddNormBwdParams)
    for name in ("dy", "z", "dres_out", "dx", "dres", "weight"):
        setattr(s, name, base + _OFF[name])
    s.dy_row_stride = s.z_row_stride = s.dres_out_row_stride = s.dx_row_stride = s.dres_row_stride = 64
    s.rows, s.n = 8, 64
    s.dtype = s.weight_dtype = s.z_dtype = s.dres_dtype = lib.FA_FP16
    s.is_rms_norm, s.eps = 0, 1e-6
    if form == "inplace":
        s.dx = s.dy
    if form == "fp32":
        s.z_dtype = s.dres_dtype = s.weight_dtype = lib.FA_FP32
    if form != "nodw":
        s.dweight, s.dbias = base + _OFF["dweight"], base + _OFF["dbias"]
        s.workspace, s.workspace_bytes = base + _OFF["workspace"], _WS
    return s, base


_at = lambda name, add=0: (lambda b: b + _OFF[name] + add)      # noqa: E731


def _bad(lib, call, block, op, buf, match, form, **kw):
    s, base = block(lib, buf, form)
    for k, v in kw.items():
        setattr(s, k, v(base) if callable(v) else v)
    with pytest.raises(RuntimeError, match=match) as e:
        call(s, 0)
    assert "(-1)" in str(e.value) and op in str(e.value)   # FA_ERR_INVALID_ARGUMENT
    return s


def test_forward_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_add_norm fires before any device work"""
    buf = (ctypes.c_char * _TOTAL)()
    bad = lambda match, form="out", **kw: _bad(lib, lib.call_add_norm, _fwd_block, "add_norm", buf, match, form, **kw)  # noqa: E731
    for form in ("out", "inplace", "plain", "fp32"):
        bad("struct_size", form, struct_size=8)
        bad("x and out must not be NULL", form, x=None)
        bad("x and out must not be NULL", form, out=None)
        bad("weight must not be NULL", form, weight=None)
        bad("reserved", form, reserved=(ctypes.c_int64 * 2)(0, 1))
        bad("fp16 or bf16", form, dtype=lib.FA_FP32)
        bad("weight_dtype", form, weight_dtype=lib.FA_BF16)
        bad("weight_dtype", form, weight_dtype=lib.FA_FP8_E4M3)
        for n in (0, 4, 60, 16392, -8):
            bad(r"multiple of 8 in \[8, 16384\]", form, n=n)
        bad("rows must be non-negative", form, rows=-1)
        bad("row strides", form, x_row_stride=-64)
        bad("row strides", form, out_row_stride=68)
        bad("row strides", form, x_row_stride=56)                       # rows overlap
        bad("16-byte aligned", form, x=_at("x", 8), out=_at("out", 0))
        bad("16-byte aligned", form, weight=_at("weight", 2))
        bad("eps", form, eps=-1e-6)
        bad("eps", form, eps=float("nan"))
        bad("eps", form, eps=float("inf"))
        bad("weight_offset", form, weight_offset=float("inf"))
        bad("weight_offset", form, weight_offset=float("nan"))
    for form in ("out", "inplace", "fp32"):
        bad("a residual needs residual_out", form, residual_out=None)
        bad("residual_dtype", form, residual_dtype=lib.FA_BF16)
        bad("residual_out_dtype", form, residual_out_dtype=lib.FA_FP8_E4M3)
        bad("row strides", form, residual_row_stride=4)
        bad("16-byte aligned", form, bias=_at("bias", 8))
    bad("an fp32 residual needs an fp32 residual_out", "out", residual_dtype=lib.FA_FP32)
    bad("out shares x's base", "inplace", out_row_stride=128)
    bad("residual_out shares residual's base", "inplace", residual_out_row_stride=128)
    bad("residual_out shares residual's base", "inplace", residual_out_dtype=lib.FA_FP32)
    for form in ("out", "fp32"):
        bad("out overlaps x", form, out=_at("x", 16))
        bad("out overlaps residual", form, out=_at("residual", 0))
        bad("out overlaps weight", form, out=_at("weight", 0))
        bad("out overlaps bias", form, out=_at("bias", 0))
        bad("residual_out overlaps x", form, residual_out=_at("x", 0))
        bad("overlaps residual", form, residual_out=_at("residual", 64))       # (fp32: it reaches into out as well)
        bad("out overlaps residual_out", form, residual_out=_at("out", 0))
    bad("overlaps", "inplace", residual_out=_at("x", 0), residual=_at("x", 0))                   # out = x = residual = residual_out
    s, _ = _fwd_block(lib, buf)
    s.rows = 2 ** 31
    with pytest.raises(RuntimeError, match=r"\(-2\).*2\^31"):           # FA_ERR_UNSUPPORTED
        lib.call_add_norm(s, 0)
    # rows == 0: FA_OK without a launch (there is no device here); column ranges of one wider buffer are not an overlap
    for form in ("out", "inplace", "plain", "fp32"):
        s, base = _fwd_block(lib, buf, form)
        s.rows = 0
        lib.call_add_norm(s, 0)
    s, base = _fwd_block(lib, buf, "plain")
    s.rows, s.out, s.x_row_stride, s.out_row_stride = 0, base + _OFF["x"] + 64 * 2, 128, 128
    lib.call_add_norm(s, 0)


def test_backward_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_add_norm_bwd fires before any device work; the workspace query answers 0 for a
    block the call rejects (for a reason other than the workspace or where the tensors lie)"""
    buf = (ctypes.c_char * _TOTAL)()

    def bad(match, form="out", **kw):
        s = _bad(lib, lib.call_add_norm_bwd, _bwd_block, "add_norm_bwd", buf, match, form, **kw)
        if "workspace" not in match and "overlaps" not in match:
            assert lib.add_norm_bwd_workspace_bytes(s) == 0

    for form in ("out", "inplace", "nodw", "fp32"):
        bad("struct_size", form, struct_size=ctypes.sizeof(lib.FaAddNormBwdParams) - 8)
        bad("dy and z must not be NULL", form, dy=None, dx=_at("dx"))
        bad("dy and z must not be NULL", form, z=None)
        bad("weight must not be NULL", form, weight=None)
        bad("reserved", form, reserved=(ctypes.c_int64 * 2)(1, 0))
        bad("fp16 or bf16", form, dtype=9)
        bad("weight_dtype", form, weight_dtype=lib.FA_BF16)
        bad("z_dtype", form, z_dtype=lib.FA_BF16)
        bad("dres_dtype", form, dres_dtype=lib.FA_FP8_E4M3)
        for n in (0, 12, 16392):
            bad(r"multiple of 8 in \[8, 16384\]", form, n=n)
        bad("rows must be non-negative", form, rows=-3)
        for name in ("dy_row_stride", "z_row_stride", "dres_out_row_stride", "dres_row_stride"):
            bad("row strides", form, **{name: -64})
            bad("row strides", form, **{name: 60})
        bad("16-byte aligned", form, z=_at("z", 8))
        bad("16-byte aligned", form, dres=_at("dres", 4))
        bad("eps", form, eps=-1.0)
        bad("eps", form, eps=float("nan"))
        bad("weight_offset", form, weight_offset=float("-inf"))
    bad("dx shares dy's base", "inplace", dx_row_stride=128)
    for form in ("out", "inplace", "fp32"):
        bad("16-byte aligned", form, dweight=_at("dweight", 8))
        bad("the workspace holds", form, workspace=None)
        bad("the workspace holds", form, workspace_bytes=2 * 64 * 4 - 1)          # 8 rows of n 64: one partial row [2][64]
        bad("workspace must be 16-byte aligned", form, workspace=_at("workspace", 8))
        bad("dweight overlaps dbias", form, dbias=_at("dweight", 0))
        bad("dweight overlaps weight", form, dweight=_at("weight", 0))
        bad("dbias overlaps z", form, dbias=_at("z", 64))
        bad("dweight overlaps workspace", form, workspace=_at("dweight", 0))
        bad("workspace overlaps dy|dx overlaps workspace", form, workspace=_at("dy", 0))     # (in place: dx is dy)
        bad("dres overlaps dy|dx overlaps dres", form, dres=_at("dy", 0))                     # (in place: dx is dy)
        bad("dres overlaps dres_out", form, dres=_at("dres_out", 0))
    for form in ("out", "nodw", "fp32"):
        bad("dx overlaps dy", form, dx=_at("dy", 16))
        bad("dx overlaps z", form, dx=_at("z", 0))
        bad("dx overlaps dres_out", form, dx=_at("dres_out", 0))
        bad("dx overlaps weight", form, dx=_at("weight", 0))
        bad("dx overlaps dres", form, dres=_at("dx", 0))
    s, _ = _bwd_block(lib, buf, "nodw")
    s.rows = 2 ** 31
    with pytest.raises(RuntimeError, match=r"\(-2\).*2\^31"):
        lib.call_add_norm_bwd(s, 0)
    # FA_OK without device work: no output asked for; no rows and no weight gradient
    s, _ = _bwd_block(lib, buf, "nodw")
    s.dx = s.dres = None
    lib.call_add_norm_bwd(s, 0)
    s, _ = _bwd_block(lib, buf, "nodw")
    s.rows = 0
    lib.call_add_norm_bwd(s, 0)


def test_workspace_query(lib):
    """0 without dweight / dbias; a function of (rows, n, dbias given) alone; at most 32 MiB at the limits; needs no device"""
    buf = (ctypes.c_char * _TOTAL)()
    ws = lib.add_norm_bwd_workspace_bytes
    s, _ = _bwd_block(lib, buf, "nodw")
    assert ws(s) == 0
    s, _ = _bwd_block(lib, buf)
    assert ws(s) == 2 * 64 * 4                              # 8 rows, n 64: one pass of one workgroup, [2][64] fp32
    s.dbias = None
    assert ws(s) == 64 * 4
    s, _ = _bwd_block(lib, buf)
    for rows in (1, 2, 33, 1031, 8192, 65536, 10 ** 6, 2 ** 31 - 1):
        s.rows = rows
        assert ws(s) == R.plan(rows, 64, True)["workspace_bytes"] <= 256 * 2 * 64 * 4
    assert ws(s) == 256 * 2 * 64 * 4
    s.rows, s.n = 5000, 4096
    for name in ("dy_row_stride", "z_row_stride", "dres_out_row_stride", "dx_row_stride", "dres_row_stride"):
        setattr(s, name, 4096)
    want = ws(s)
    assert want == R.plan(5000, 4096, True)["workspace_bytes"] > 0
    s.dy_row_stride = s.dx_row_stride = 8192                # strides, which outputs, the dtypes, eps: no influence
    s.dx = s.dres = s.dres_out = s.dweight = None
    s.z_dtype = s.weight_dtype = lib.FA_FP32
    s.is_rms_norm, s.eps, s.weight_offset = 1, 1e-5, 1.0
    s.workspace = None
    assert ws(s) == want
    s.rows, s.n = 2 ** 31 - 1, 16384
    for name in ("dy_row_stride", "z_row_stride"):
        setattr(s, name, 16384)
    base = (ctypes.addressof(buf) + 15) & ~15
    s.dweight, s.dbias = base + _OFF["dweight"], None
    assert ws(s) == 256 * 16384 * 4
    s.dweight, s.dbias = None, base + _OFF["dbias"]          # dbias alone: the partial rows still hold both
    assert ws(s) == 256 * 2 * 16384 * 4 == 32 << 20
    s.n = 16392
    assert ws(s) == 0                                       # a block the call would reject
    assert lib.lib.fa_add_norm_bwd_workspace_bytes(None) == 0


# Python ----------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors_on_cpu_tensors():
    from flash_attn_mi355.add_norm import add_norm_backward, add_norm_forward, fused_add_rms_norm_
    x = torch.zeros(4, 6, 64, dtype=torch.float16)
    w = torch.ones(64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="fp16 or bf16"):
        add_norm_forward(x.float(), w)
    with pytest.raises(RuntimeError, match=r"multiple of 8 in \[8, 16384\]"):
        add_norm_forward(x[..., :60], w[:60])
    with pytest.raises(RuntimeError, match=r"multiple of 8 in \[8, 16384\]"):
        add_norm_forward(torch.zeros(1, 16392, dtype=torch.float16), torch.ones(16392, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="weight must not be None"):
        add_norm_forward(x, None)
    with pytest.raises(RuntimeError, match="weight must have x's dtype"):
        add_norm_forward(x, w.bfloat16())
    with pytest.raises(RuntimeError, match=r"weight must have shape \(N,\)"):
        add_norm_forward(x, w[:32])
    with pytest.raises(RuntimeError, match="bias must have weight's dtype"):
        add_norm_forward(x, w, w.float())
    with pytest.raises(RuntimeError, match="residual must have x's dtype"):
        add_norm_forward(x, w, None, x.bfloat16())
    with pytest.raises(RuntimeError, match="residual must have x's shape"):
        add_norm_forward(x, w, None, x[:2])
    with pytest.raises(RuntimeError, match="eps must be finite"):
        add_norm_forward(x, w, eps=-1.0)
    with pytest.raises(RuntimeError, match="weight_offset must be finite"):
        add_norm_forward(x, w, weight_offset=float("nan"))
    with pytest.raises(RuntimeError, match="z must have dy's shape"):
        add_norm_backward(x, x[:2], w)
    with pytest.raises(RuntimeError, match="dres_out must have z's dtype"):
        add_norm_backward(x, x.float(), w, x)
    with pytest.raises(RuntimeError, match="dres_dtype"):
        add_norm_backward(x, x, w, dres_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="needs a residual"):
        fused_add_rms_norm_(x, None, w)
    # everything else in order: the CPU tensor itself is the error
    with pytest.raises(RuntimeError, match="GPU"):
        add_norm_forward(x, w.float(), w.float(), x.float(), is_rms_norm=False, prenorm=True, weight_offset=1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        add_norm_backward(x, x.float(), w, x.float(), dres_dtype=torch.float32, need_dres=True, need_db=True)


_DT = (torch.float16, torch.bfloat16)


def test_torch_op_schemas_and_fake_implementations():
    """add_norm / add_norm_bwd are functional, add_norm_ mutates x and residual; the fake implementations give the shapes, dtypes
    and (contiguous) strides for every prenorm / residual_in_fp32 / dtype combination"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    import flash_attn_mi355.torch_ops as T
    ns = torch.ops.flash_attn_mi355
    fwd, inp, bwd = ns.add_norm.default._schema, ns.add_norm_.default._schema, ns.add_norm_bwd.default._schema
    assert not [a.name for a in fwd.arguments if a.alias_info is not None]
    assert not [a.name for a in bwd.arguments if a.alias_info is not None]
    assert [a.name for a in inp.arguments if a.alias_info is not None and a.alias_info.is_write] == ["x", "residual"]
    assert [a.name for a in fwd.arguments] == ["x", "weight", "bias", "residual", "eps", "weight_offset", "is_rms_norm", "prenorm",
                                               "residual_in_fp32"]
    assert [a.name for a in inp.arguments] == ["x", "residual", "weight", "bias", "eps", "weight_offset", "is_rms_norm"]
    assert [a.name for a in bwd.arguments] == ["dy", "z", "dres_out", "weight", "eps", "weight_offset", "is_rms_norm", "dres_fp32",
                                               "need_dx", "need_dres", "need_dweight", "need_dbias"]
    assert len(fwd.returns) == 2 and len(inp.returns) == 0 and len(bwd.returns) == 4
    with FakeTensorMode():
        for dt in _DT:
            wide = torch.empty(5, 7, 2 * 264, dtype=dt, device="cuda")
            x = wide[..., :264]                              # a strided view: the outputs are fresh contiguous tensors
            for wdt in (dt, torch.float32):
                w = torch.empty(264, dtype=wdt, device="cuda")
                for rdt in (None, dt, torch.float32):
                    res = None if rdt is None else torch.empty(5, 7, 264, dtype=rdt, device="cuda")
                    for prenorm in (False, True):
                        for in32 in (False, True):
                            out, ro = ns.add_norm(x, w, w, res, 1e-6, 0.0, True, prenorm, in32)
                            assert out.shape == x.shape and out.dtype == dt and out.is_contiguous()
                            if res is None and not prenorm:
                                assert ro.shape == (0,)
                            else:
                                want = torch.float32 if (rdt == torch.float32 or in32) else dt
                                assert ro.shape == x.shape and ro.dtype == want and ro.is_contiguous()
                assert ns.add_norm_(wide[..., :264], None, w, None, 1e-6, 1.0, False) is None
                z = torch.empty(5, 7, 264, dtype=torch.float32, device="cuda")
                dx, dres, dw, db = ns.add_norm_bwd(x, z, z, w, 1e-6, 0.0, False, True, True, True, True, True)
                assert dx.shape == dres.shape == x.shape and dx.dtype == dt and dres.dtype == torch.float32
                assert dx.is_contiguous() and dres.is_contiguous()
                assert dw.shape == db.shape == (264,) and dw.dtype == db.dtype == wdt
                dx, dres, dw, db = ns.add_norm_bwd(x, x, None, w, 1e-6, 0.0, True, False, True, False, False, False)
                assert dx.shape == x.shape and dres.shape == dw.shape == db.shape == (0,)
                dx, dres, dw, db = ns.add_norm_bwd(x, x, None, w, 1e-6, 0.0, True, False, False, True, True, False)
                assert dx.shape == db.shape == (0,) and dres.shape == x.shape and dres.dtype == dt and dw.shape == (264,)
    for name in ("add_norm", "add_norm_", "add_norm_bwd"):
        assert name not in T.__all__                        # reached through torch.ops only


def test_public_name_lists_are_unchanged():
    import flash_attn
    import flash_attn_mi355
    for name in ("add_norm", "add_norm_backward", "fused_add_rms_norm_", "rms_norm", "layer_norm", "RMSNorm", "ops"):
        assert name not in flash_attn.__all__ and name not in flash_attn_mi355.__all__


# the upstream-named wrappers ---------------------------------------------------------------------------------------------------
def _sig(f):
    return [(p.name, p.default if p.default is not inspect.Parameter.empty else "<required>")
            for p in inspect.signature(f).parameters.values() if p.name != "self"]


_REQ = "<required>"
_DROPOUT_ADD = [("x0", _REQ), ("residual", _REQ), ("weight", _REQ), ("bias", _REQ), ("dropout_p", _REQ), ("epsilon", _REQ),
                ("rowscale", None), ("layerscale", None), ("prenorm", False), ("residual_in_fp32", False),
                ("return_dropout_mask", False)]
_MODULE = [("hidden_size", _REQ), ("prenorm", False), ("p", 0.0), ("eps", 1e-5), ("residual_in_fp32", False), ("device", None),
           ("dtype", None)]
_LN_FN = [("x", _REQ), ("weight", _REQ), ("bias", _REQ), ("residual", None), ("x1", None), ("weight1", None), ("bias1", None),
          ("eps", 1e-6), ("dropout_p", 0.0), ("rowscale", None), ("prenorm", False), ("residual_in_fp32", False),
          ("zero_centered_weight", False), ("is_rms_norm", False), ("return_dropout_mask", False), ("out_dtype", None), ("out", None),
          ("residual_out", None)]


def test_upstream_named_entries_have_the_specified_signatures():
    import flash_attn.ops.layer_norm as L
    import flash_attn.ops.rms_norm as M
    import flash_attn.ops.triton.layer_norm as TL
    assert _sig(M.rms_norm) == [("x", _REQ), ("weight", _REQ), ("epsilon", _REQ)]
    assert _sig(M.dropout_add_rms_norm) == _DROPOUT_ADD
    assert _sig(M.RMSNorm.__init__) == [("hidden_size", _REQ), ("eps", 1e-5), ("device", None), ("dtype", None)]
    assert _sig(M.DropoutAddRMSNorm.__init__) == _MODULE
    assert _sig(L.layer_norm) == [("x", _REQ), ("weight", _REQ), ("bias", _REQ), ("epsilon", _REQ)]
    assert _sig(L.dropout_add_layer_norm) == _DROPOUT_ADD
    assert _sig(L.DropoutAddLayerNorm.__init__) == _MODULE
    assert _sig(TL.layer_norm_fn) == _LN_FN
    assert _sig(TL.rms_norm_fn) == [p for p in _LN_FN if p[0] != "is_rms_norm"]
    assert _sig(TL.RMSNorm.__init__) == [("hidden_size", _REQ), ("eps", 1e-5), ("dropout_p", 0.0), ("zero_centered_weight", False),
                                         ("device", None), ("dtype", None)]
    assert _sig(TL.RMSNorm.forward) == [("x", _REQ), ("residual", None), ("prenorm", False), ("residual_in_fp32", False)]
    assert _sig(M.RMSNorm.forward) == [("x", _REQ)]
    assert _sig(M.DropoutAddRMSNorm.forward) == _sig(L.DropoutAddLayerNorm.forward) == [("x0", _REQ), ("residual", None)]
    m = TL.RMSNorm(64, zero_centered_weight=True, dtype=torch.bfloat16)
    assert m.weight.dtype == torch.bfloat16 and float(m.weight.detach().abs().max()) == 0.0 and m.bias is None
    l = L.DropoutAddLayerNorm(64, dtype=torch.float32)
    assert float(l.weight.detach().min()) == 1.0 and float(l.bias.detach().abs().max()) == 0.0 and tuple(l.weight.shape) == (64,)
    assert M.RMSNorm(64).bias is None and M.DropoutAddRMSNorm(64).bias is None


def test_unsupported_arguments_raise_with_their_name():
    import flash_attn.ops.layer_norm as L
    import flash_attn.ops.rms_norm as M
    import flash_attn.ops.triton.layer_norm as TL
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.ones(64, dtype=torch.bfloat16)
    one = torch.ones(4)
    for f in (M.dropout_add_rms_norm, L.dropout_add_layer_norm):
        for name, kw in (("dropout_p", {}), ("rowscale", {"rowscale": one}), ("layerscale", {"layerscale": w}),
                         ("return_dropout_mask", {"return_dropout_mask": True})):
            with pytest.raises(RuntimeError, match=f"`{name}`"):
                f(x, None, w, w, 0.1 if name == "dropout_p" else 0.0, 1e-5, **kw)
    for f in (TL.layer_norm_fn, TL.rms_norm_fn):
        for name, kw in (("dropout_p", {"dropout_p": 0.5}), ("rowscale", {"rowscale": one}), ("x1", {"x1": x}),
                         ("weight1", {"weight1": w}), ("bias1", {"bias1": w}), ("return_dropout_mask", {"return_dropout_mask": True}),
                         ("out_dtype", {"out_dtype": torch.float32})):
            with pytest.raises(RuntimeError, match=f"`{name}`"):
                f(x, w, None, **kw)
    m = M.DropoutAddRMSNorm(64, p=0.1, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="`dropout_p`"):
        m(x)                                                 # training mode: dropout would apply
    m.eval()
    with pytest.raises(RuntimeError, match="GPU"):           # eval: dropout_p is 0, the CPU tensor itself is the error
        m(x)
    t = TL.RMSNorm(64, dropout_p=0.1, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="`dropout_p`"):
        t(x)
    with pytest.raises(RuntimeError, match="GPU"):
        t.eval()(x, residual=x, prenorm=True)
