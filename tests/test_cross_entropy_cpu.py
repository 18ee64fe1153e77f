"""CPU: the host side of fa_cross_entropy / fa_cross_entropy_bwd - the fp64 yardstick of the GPU tests against torch's own
cross-entropy and its autograd, the bounds on the GPU tests' inputs, the C ABI's argument checks on host pointers, the ctypes
mirrors, the workspace query (which needs no device), the torch.library ops' schemas and fake implementations, the upstream-named
wrappers' signatures and the arguments they do not serve.  Nothing here needs a GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import cross_entropy_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


# the yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ls,scale,zs,masked", [(0.0, 1.0, 0.0, False), (0.1, 0.5, 1e-4, False), (0.0, 0.5, 1e-4, False),
                                                (0.1, 1.0, 0.0, False), (0.0, 1.0, 0.0, True), (0.0, 0.5, 1e-4, True)])
def test_reference_equals_torch_cross_entropy_and_its_autograd(ls, scale, zs, masked):
    """cross_entropy_ref == F.cross_entropy(logit_scale x, y, ignore_index, label_smoothing) + lse_square_scale lse^2 and torch
    autograd of that composition, to 1e-12; ignored rows give 0 and a zero gradient row.  -inf entries are compared at
    label_smoothing == 0: with smoothing torch charges a masked entry log(0) = -inf, the op leaves masked entries out of
    sum_j l_j by definition."""
    rows, V = 23, 301
    x, y, dloss = R.inputs(rows, V, torch.float32, seed=3, chunk=64)
    if not masked:
        x = torch.where(torch.isinf(x), torch.zeros_like(x), x)
    assert bool(torch.isinf(x).any()) == masked and int((y == R.IGNORE).sum()) >= rows // 3
    ref = R.forward_ref(x, y, ls, scale, zs)
    x64 = x.double().requires_grad_(True)
    l = R._f32(scale) * x64
    lse = torch.logsumexp(l, -1)
    z = torch.where(y == R.IGNORE, torch.zeros_like(lse), R._f32(zs) * lse * lse)
    loss = F.cross_entropy(l, y, ignore_index=R.IGNORE, label_smoothing=R._f32(ls), reduction="none") + z
    rel = lambda a, c: float((a - c).abs().max() / c.abs().max().clamp(min=1e-300))       # noqa: E731
    assert rel(ref["lse"], lse.detach()) <= 1e-12
    assert rel(ref["loss"], loss.detach()) <= 1e-12 and float((ref["z"] - z.detach()).abs().max()) <= 1e-12
    assert (ref["loss"][y == R.IGNORE] == 0).all() and (ref["z"][y == R.IGNORE] == 0).all()
    (grad,) = torch.autograd.grad(loss, x64, dloss.double())
    dx, mags = R.backward_ref(dloss, x, y, ref["lse"], ls, scale, zs)
    assert rel(dx, grad) <= 1e-12
    assert (dx[y == R.IGNORE] == 0).all()
    assert (mags["A"] >= dx.abs() * (1 - 1e-12)).all() and (ref["M"] >= ref["loss"].abs() * (1 - 1e-12)).all()


def test_reference_special_values():
    """a row of -inf, a row with +inf and a row with a NaN give lse = loss = NaN; a label outside [0, V) gives NaN loss and a
    NaN gradient row and leaves its neighbours alone"""
    x = torch.randn(5, 40)
    x[0] = float("-inf")
    x[1, 7] = float("inf")
    x[2, 39] = float("nan")
    y = torch.tensor([3, 3, 3, 40, 5])
    ref = R.forward_ref(x, y, 0.1, 1.0, 1e-4)
    assert torch.isnan(ref["lse"][:3]).all() and torch.isnan(ref["loss"][:4]).all() and torch.isnan(ref["z"][3])
    assert torch.isfinite(ref["lse"][3:]).all() and torch.isfinite(ref["loss"][4])
    dx, _ = R.backward_ref(torch.ones(5), x, y, ref["lse"], 0.1, 1.0, 1e-4)
    assert torch.isnan(dx[:4]).all() and torch.isfinite(dx[4]).all()
    y[3] = -1
    assert torch.isnan(R.forward_ref(x, y)["loss"][3])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [264, 1001, None])
def test_bounds_are_not_vacuous(V, dtype):
    """on the inputs the GPU tests use: the reference with logit_scale, the smoothing term, the z-loss term or the (1 + 2 z lse)
    factor left out, or with every label shifted by one column, lies outside the bounds by more than 2x - and the reference
    rounded once lies inside them"""
    rows, ls, scale, zs = 12, 0.1, 0.5, 1e-4
    V = R.CHUNK[dtype] + 13 if V is None else V             # (None: a second chunk)
    x, y, dloss = R.inputs(rows, V, dtype, seed=V)
    steps = R.plan(rows, V, dtype)["steps"]
    ref = R.forward_ref(x, y, ls, scale, zs)
    bl, bo, bz = R.lse_bound(ref, steps), R.loss_bound(ref, steps, ls, zs, V), R.z_bound(ref, steps, zs)
    lse32 = ref["lse"].float()
    dx, mags = R.backward_ref(dloss, x, y, lse32, ls, scale, zs)
    bd = R.dx_bound(dx, mags, dtype)
    assert R.worst(lse32, ref["lse"], bl) <= 1.0 and R.worst(ref["loss"].float(), ref["loss"], bo) <= 1.0
    assert R.worst(ref["z"].float(), ref["z"], bz) <= 1.0 and R.worst(dx.to(dtype), dx, bd) <= 1.0
    live = y != R.IGNORE
    for term, kw in (("scale", {"leave_out": "scale"}), ("smoothing", {"leave_out": "smoothing"}), ("zloss", {"leave_out": "zloss"}),
                     ("zfactor", {"leave_out": "zfactor"}), ("label", {"label_shift": 1})):
        yy = y.clone()
        if term == "label":
            yy[yy == V - 1] = V - 2                           # (stay inside the vocabulary: a bad label is NaN, not a wrong value)
            base = R.forward_ref(x, yy, ls, scale, zs)
            bdx, bm = R.backward_ref(dloss, x, yy, lse32, ls, scale, zs)
            b_o, b_d = R.loss_bound(base, steps, ls, zs, V), R.dx_bound(bdx, bm, dtype)
        else:
            base, bdx, b_o, b_d = ref, dx, bo, bd
        wrong = R.forward_ref(x, yy, ls, scale, zs, **kw)
        wdx, _ = R.backward_ref(dloss, x, yy, lse32, ls, scale, zs, **kw)
        if term in ("scale", "smoothing", "zloss", "label"):
            assert R.worst(wrong["loss"].float(), base["loss"], b_o, rows=live, wrong=True) > 2.0, term
        if term in ("scale", "smoothing", "zfactor", "label"):
            assert R.worst(wdx.to(dtype), bdx, b_d, rows=live, wrong=True) > 2.0, term


def test_plan_restated(lib):
    """cross_entropy_ref.plan() restates csrc/fa_cross_entropy.hip: the workspace the library reports, a function of (rows, V,
    dtype) alone, rows x nchunks x 16 bytes, 0 where a row is one chunk - also past rows x V = 2^32"""
    buf = (ctypes.c_char * _TOTAL)()
    codes = {torch.float16: lib.FA_FP16, torch.bfloat16: lib.FA_BF16, torch.float32: lib.FA_FP32}
    for dtype, code in codes.items():
        C = R.CHUNK[dtype]
        for rows, V in ((1, 1), (3, 7), (1031, C), (67, C + 1), (67, 2 * C + 13), (8192, 128256), (65536, 128256), (128, 262144),
                        (1, 2 ** 31 - 1), (2 ** 20, 50257)):
            s, _ = _fwd_block(lib, buf)
            s.rows, s.vocab, s.dtype, s.logits_row_stride = rows, V, code, V
            p = R.plan(rows, V, dtype)
            assert p["nchunks"] == -(-V // C) and p["workspace_bytes"] <= rows * p["nchunks"] * 16
            assert lib.cross_entropy_workspace_bytes(s) == p["workspace_bytes"], (rows, V, dtype)
            if V <= C:
                assert p["workspace_bytes"] == 0
            s.logits_row_stride, s.label_smoothing, s.workspace = V + 24, 0.1, None          # no influence
            assert lib.cross_entropy_workspace_bytes(s) == p["workspace_bytes"]
    assert 65536 * 128256 > 2 ** 32 and R.plan(65536, 128256, torch.bfloat16)["workspace_bytes"] == 65536 * -(-128256 // R.CHUNK[torch.bfloat16]) * 16 > 0
    s, _ = _fwd_block(lib, buf)
    s.vocab = 0
    assert lib.cross_entropy_workspace_bytes(s) == 0          # a block the call would reject
    assert lib.lib.fa_cross_entropy_workspace_bytes(None) == 0


# the C ABI -------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_struct_sizes(lib):
    for name in ("fa_cross_entropy", "fa_cross_entropy_workspace_bytes", "fa_cross_entropy_params_size", "fa_cross_entropy_bwd",
                 "fa_cross_entropy_bwd_params_size"):
        assert hasattr(lib.lib, name) and name in lib.EXPORTS
    assert lib.lib.fa_cross_entropy_params_size() == ctypes.sizeof(lib.FaCrossEntropyParams)
    assert lib.lib.fa_cross_entropy_bwd_params_size() == ctypes.sizeof(lib.FaCrossEntropyBwdParams)
    assert lib.FA_ABI_VERSION == 4 and lib.lib.fa_abi_version() == 4
    rows = {e: (s, q) for e, s, q in lib.ROW_OPS}
    assert rows["fa_cross_entropy"] == (lib.FaCrossEntropyParams, "fa_cross_entropy_workspace_bytes")
    assert rows["fa_cross_entropy_bwd"] == (lib.FaCrossEntropyBwdParams, None)


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
    for cname, mirror in (("fa_cross_entropy_params", lib.FaCrossEntropyParams),
                          ("fa_cross_entropy_bwd_params", lib.FaCrossEntropyBwdParams)):
        fields = _header_fields(cname)
        assert [f[0] for f in mirror._fields_] == fields
        assert fields[0] == "struct_size" and fields[-1] == "reserved"
        assert ctypes.sizeof(mirror) % 8 == 0
        assert ctypes.sizeof(dict(mirror._fields_)["reserved"]) == 32   # room for class_start, total_classes, a precomputed lse


# host buffers behind valid blocks: [8, 64] logits with room for fp32, [8] vectors, a workspace
_T = 8 * 64 * 4
_V8 = 8 * 8
_WS = 1 << 12
_OFF = {}
_o = 0
for _n, _sz in (("logits", _T), ("dlogits", _T), ("labels", _V8), ("losses", _V8), ("z_losses", _V8), ("lse", _V8), ("dlosses", _V8),
                ("workspace", _WS)):
    _OFF[_n] = _o
    _o += _sz
_TOTAL = _o + 64


def _fwd_block(lib, buf, form="bf16"):
    """a valid fa_cross_entropy block over host memory: 8 rows of 64 columns.  form: 'bf16', 'fp32', 'view' (row stride 96)"""
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaCrossEntropyParams()
    s.struct_size = ctypes.sizeof(lib.FaCrossEntropyParams)
    for name in ("logits", "labels", "losses", "z_losses", "lse"):
        setattr(s, name, base + _OFF[name])
    s.rows, s.vocab, s.logits_row_stride = 8, 64, 64
    s.dtype = lib.FA_FP32 if form == "fp32" else lib.FA_BF16
    s.logit_scale, s.ignore_index = 1.0, -100
    if form == "view":
        s.rows, s.logits_row_stride = 5, 96
    return s, base


def _bwd_block(lib, buf, form="bf16"):
    """a valid fa_cross_entropy_bwd block.  form: 'bf16', 'fp32', 'inplace' (dlogits = logits), 'bcast' (dlosses stride 0)"""
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaCrossEntropyBwdParams()
    s.struct_size = ctypes.sizeof(lib.FaCrossEntropyBwdParams)
    for name in ("dlosses", "logits", "labels", "lse", "dlogits"):
        setattr(s, name, base + _OFF[name])
    s.rows, s.vocab, s.logits_row_stride, s.dlogits_row_stride, s.dlosses_stride = 8, 64, 64, 64, 1
    s.dtype = lib.FA_FP32 if form == "fp32" else lib.FA_BF16
    s.logit_scale, s.ignore_index = 1.0, -100
    if form == "inplace":
        s.dlogits = s.logits
    if form == "bcast":
        s.dlosses_stride = 0
    return s, base


_at = lambda name, add=0: (lambda b: b + _OFF[name] + add)      # noqa: E731


def _bad(lib, call, block, op, buf, match, form, code="(-1)", **kw):
    s, base = block(lib, buf, form)
    for k, v in kw.items():
        setattr(s, k, v(base) if callable(v) else v)
    with pytest.raises(RuntimeError, match=match) as e:
        call(s, 0)
    assert code in str(e.value) and op in str(e.value)
    return s


def test_forward_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_cross_entropy fires before any device work, and the workspace query answers 0
    for a block the call rejects (for a reason other than the workspace or where the tensors lie)"""
    buf = (ctypes.c_char * _TOTAL)()

    def bad(match, form="bf16", **kw):
        s = _bad(lib, lib.call_cross_entropy, _fwd_block, "cross_entropy", buf, match, form, **kw)
        if "workspace" not in match and "overlaps" not in match:
            assert lib.cross_entropy_workspace_bytes(s) == 0
    for form in ("bf16", "fp32", "view"):
        bad("struct_size", form, struct_size=8)
        for name in ("logits", "labels", "losses", "z_losses", "lse"):
            bad("must not be NULL", form, **{name: None})
        bad("reserved", form, reserved=(ctypes.c_int64 * 4)(0, 0, 0, 1))
        bad("reserved", form, reserved0=1)
        bad("fp16, bf16 or fp32", form, dtype=lib.FA_FP8_E4M3)
        bad("fp16, bf16 or fp32", form, dtype=7)
        bad("vocab must be at least 1", form, vocab=0)
        bad("vocab must be at least 1", form, vocab=-5)
        bad("rows must be non-negative", form, rows=-1)
        bad("row stride", form, logits_row_stride=-64)
        bad("row stride", form, logits_row_stride=63)                    # rows overlap
        bad("aligned", form, logits=_at("logits", 1))
        bad("aligned", form, labels=_at("labels", 4))
        bad("aligned", form, lse=_at("lse", 2))
        for v in (-0.1, 1.0, 1.5, float("nan")):
            bad("label_smoothing", form, label_smoothing=v)
        for v in (float("inf"), float("-inf"), float("nan")):
            bad("logit_scale", form, logit_scale=v)
        for v in (-1e-4, float("inf"), float("nan")):
            bad("lse_square_scale", form, lse_square_scale=v)
        bad("losses overlaps logits", form, losses=_at("logits", 64))
        bad("lse overlaps labels", form, lse=_at("labels", 8))
        bad("losses overlaps z_losses", form, z_losses=_at("losses", 4))
        bad("z_losses overlaps lse", form, lse=_at("z_losses", 0))
    bad("aligned", "fp32", logits=_at("logits", 2))
    # a vocabulary of more than one chunk needs the workspace (the checks run on host pointers: nothing is launched)
    V = R.CHUNK[torch.bfloat16] + 1
    big = dict(vocab=V, logits_row_stride=V, rows=1, logits=_at("workspace", 2048))   # (the long row lies past everything else)
    bad("the workspace holds", workspace=None, **big)
    bad("the workspace holds", workspace=_at("workspace"), workspace_bytes=31, **big)
    bad("workspace must be 16-byte aligned", workspace=_at("workspace", 8), workspace_bytes=64, **big)
    bad("workspace overlaps labels|lse overlaps workspace", workspace=_at("lse"), workspace_bytes=64, **big)
    s, _ = _fwd_block(lib, buf)
    s.rows, s.vocab, s.logits_row_stride = 2 ** 31 - 1, V, V
    with pytest.raises(RuntimeError, match=r"\(-2\).*2\^31"):           # FA_ERR_UNSUPPORTED
        lib.call_cross_entropy(s, 0)
    # rows == 0: FA_OK without a launch (there is no device here); a padded row stride is not an overlap
    for form in ("bf16", "fp32", "view"):
        s, _ = _fwd_block(lib, buf, form)
        s.rows = 0
        lib.call_cross_entropy(s, 0)


def test_backward_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_cross_entropy_bwd fires before any device work"""
    buf = (ctypes.c_char * _TOTAL)()
    bad = lambda match, form="bf16", **kw: _bad(lib, lib.call_cross_entropy_bwd, _bwd_block, "cross_entropy_bwd", buf, match,  # noqa: E731
                                                form, **kw)
    for form in ("bf16", "fp32", "inplace", "bcast"):
        bad("struct_size", form, struct_size=ctypes.sizeof(lib.FaCrossEntropyBwdParams) - 8)
        for name in ("dlosses", "logits", "labels", "lse", "dlogits"):
            bad("must not be NULL", form, **{name: None})
        bad("reserved", form, reserved=(ctypes.c_int64 * 4)(1, 0, 0, 0))
        bad("reserved", form, reserved0=-1)
        bad("fp16, bf16 or fp32", form, dtype=lib.FA_FP8_E4M3)
        bad("vocab must be at least 1", form, vocab=0)
        bad("rows must be non-negative", form, rows=-2)
        bad("row strides", form, logits_row_stride=60)
        bad("row strides", form, dlogits_row_stride=-64)
        bad("dlosses_stride", form, dlosses_stride=-1)
        bad("aligned", form, dlosses=_at("dlosses", 2))
        bad("aligned", form, labels=_at("labels", 4))
        bad("label_smoothing", form, label_smoothing=1.0)
        bad("logit_scale", form, logit_scale=float("nan"))
        bad("lse_square_scale", form, lse_square_scale=-1.0)
    bad("aligned", "bf16", dlogits=_at("dlogits", 1))
    bad("dlogits shares logits' base", "inplace", dlogits_row_stride=128)
    for form in ("bf16", "fp32", "bcast"):
        bad("dlogits overlaps logits", form, dlogits=_at("logits", 16))
        bad("dlogits overlaps dlosses", form, dlosses=_at("dlogits", 64))
        bad("dlogits overlaps labels", form, labels=_at("dlogits", 0))
        bad("dlogits overlaps lse", form, lse=_at("dlogits", 128))
    s, _ = _bwd_block(lib, buf)
    s.rows, s.vocab = 2 ** 31 - 1, R.BWD_CHUNK + 1
    s.logits_row_stride = s.dlogits_row_stride = s.vocab
    with pytest.raises(RuntimeError, match=r"\(-2\).*2\^31"):
        lib.call_cross_entropy_bwd(s, 0)
    for form in ("bf16", "fp32", "inplace", "bcast"):        # rows == 0: FA_OK without a launch
        s, _ = _bwd_block(lib, buf, form)
        s.rows = 0
        lib.call_cross_entropy_bwd(s, 0)


# Python ----------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors_on_cpu_tensors():
    from flash_attn_mi355.cross_entropy import cross_entropy, cross_entropy_backward, cross_entropy_forward
    x = torch.zeros(4, 6, 64, dtype=torch.bfloat16)
    y = torch.zeros(4, 6, dtype=torch.int64)
    one = torch.ones(4, 6)
    with pytest.raises(RuntimeError, match="fp16, bf16 or fp32"):
        cross_entropy_forward(x.double(), y)
    with pytest.raises(RuntimeError, match=r"\[\.\.\., V\] with V >= 1"):
        cross_entropy_forward(x[..., :0], y)
    with pytest.raises(RuntimeError, match="labels must have logits' leading shape"):
        cross_entropy_forward(x, y[:2])
    with pytest.raises(RuntimeError, match=r"labels must be an int64 \(or int32\)"):
        cross_entropy_forward(x, y.float())
    for kw, match in (({"label_smoothing": 1.0}, "label_smoothing"), ({"label_smoothing": -0.5}, "label_smoothing"),
                      ({"logit_scale": float("inf")}, "logit_scale"), ({"lse_square_scale": -1.0}, "lse_square_scale"),
                      ({"lse_square_scale": float("nan")}, "lse_square_scale"), ({"ignore_index": 2 ** 63}, "ignore_index")):
        with pytest.raises(RuntimeError, match="cross_entropy: " + match):
            cross_entropy_forward(x, y, **kw)
        with pytest.raises(RuntimeError, match="cross_entropy: " + match):
            cross_entropy_backward(one, x, y, one, **kw)
    with pytest.raises(RuntimeError, match="dlosses and lse must have labels' shape"):
        cross_entropy_backward(one[:2], x, y, one)
    with pytest.raises(RuntimeError, match="dlosses and lse must be float32"):
        cross_entropy_backward(one.double(), x, y, one)
    # everything else in order: the CPU tensor itself is the error
    with pytest.raises(RuntimeError, match="GPU"):
        cross_entropy_forward(x, y.int(), label_smoothing=0.1, logit_scale=0.5, lse_square_scale=1e-4, ignore_index=-1)
    with pytest.raises(RuntimeError, match="GPU"):
        cross_entropy_backward(one[:1, :1].expand(4, 6), x, y, one, inplace=True)
    with pytest.raises(RuntimeError, match="GPU"):
        cross_entropy(x, y, inplace_backward=True)


def test_torch_op_schemas_and_fake_implementations():
    """cross_entropy / cross_entropy_bwd are functional, cross_entropy_bwd_ mutates the logits; the fake implementations give the
    shapes, dtypes and (contiguous) strides"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    import flash_attn_mi355.torch_ops as T
    ns = torch.ops.flash_attn_mi355
    fwd, bwd, inp = ns.cross_entropy.default._schema, ns.cross_entropy_bwd.default._schema, ns.cross_entropy_bwd_.default._schema
    assert not [a.name for a in fwd.arguments if a.alias_info is not None]
    assert not [a.name for a in bwd.arguments if a.alias_info is not None]
    assert [a.name for a in inp.arguments if a.alias_info is not None and a.alias_info.is_write] == ["logits"]
    assert [a.name for a in fwd.arguments] == ["logits", "labels", "label_smoothing", "logit_scale", "lse_square_scale", "ignore_index",
                                               "inplace_backward"]
    tail = ["dlosses", "logits", "labels", "lse", "label_smoothing", "logit_scale", "lse_square_scale", "ignore_index"]
    assert [a.name for a in bwd.arguments] == tail and [a.name for a in inp.arguments] == tail
    assert len(fwd.returns) == 3 and len(bwd.returns) == 1 and len(inp.returns) == 0
    with FakeTensorMode():
        for dt in (torch.float16, torch.bfloat16, torch.float32):
            wide = torch.empty(5, 7, 1024, dtype=dt, device="cuda")
            x = wide[..., :1001]                             # a strided view: the outputs are fresh contiguous tensors
            y = torch.empty(5, 7, dtype=torch.int64, device="cuda")
            outs = ns.cross_entropy(x, y, 0.1, 1.0, 1e-4, -100, False)
            for o in outs:
                assert o.shape == y.shape and o.dtype == torch.float32 and o.is_contiguous()
            dx = ns.cross_entropy_bwd(outs[0], x, y, outs[2], 0.1, 1.0, 1e-4, -100)
            assert dx.shape == x.shape and dx.dtype == dt and dx.is_contiguous()
            assert ns.cross_entropy_bwd_(outs[0], x, y, outs[2], 0.1, 1.0, 1e-4, -100) is None
    for name in ("cross_entropy", "cross_entropy_bwd", "cross_entropy_bwd_"):
        assert name not in T.__all__                        # reached through torch.ops only


def test_public_name_lists_are_unchanged():
    import flash_attn
    import flash_attn_mi355
    for name in ("cross_entropy", "cross_entropy_forward", "cross_entropy_backward", "cross_entropy_loss", "CrossEntropyLoss", "losses"):
        assert name not in flash_attn.__all__ and name not in flash_attn_mi355.__all__


# the upstream-named wrappers ---------------------------------------------------------------------------------------------------
def _sig(f):
    return [(p.name, p.default if p.default is not inspect.Parameter.empty else "<required>")
            for p in inspect.signature(f).parameters.values() if p.name != "self"]


_REQ = "<required>"


def test_upstream_named_entries_have_the_specified_signatures():
    import flash_attn.losses.cross_entropy as L
    import flash_attn.ops.triton.cross_entropy as TC
    import flash_attn_mi355.cross_entropy as C
    assert _sig(TC.cross_entropy_loss) == [("logits", _REQ), ("labels", _REQ), ("precomputed_lse", None), ("label_smoothing", 0.0),
                                           ("logit_scale", 1.0), ("lse_square_scale", 0.0), ("ignore_index", -100),
                                           ("inplace_backward", False), ("process_group", None)]
    assert _sig(L.CrossEntropyLoss.__init__) == [("ignore_index", -100), ("reduction", "mean"), ("label_smoothing", 0.0),
                                                 ("logit_scale", 1.0), ("lse_square_scale", 0.0), ("inplace_backward", False),
                                                 ("process_group", None), ("return_z_loss", False)]
    assert _sig(L.CrossEntropyLoss.forward) == [("input", _REQ), ("target", _REQ), ("precomputed_lse", None)]
    scal = [("label_smoothing", 0.0), ("logit_scale", 1.0), ("lse_square_scale", 0.0), ("ignore_index", -100)]
    assert _sig(C.cross_entropy_forward) == [("logits", _REQ), ("labels", _REQ)] + scal
    assert _sig(C.cross_entropy_backward) == [("dlosses", _REQ), ("logits", _REQ), ("labels", _REQ), ("lse", _REQ)] + scal + [
        ("inplace", False)]
    assert _sig(C.cross_entropy) == [("logits", _REQ), ("labels", _REQ)] + scal + [("inplace_backward", False)]
    kinds = {p.name: p.kind for p in inspect.signature(C.cross_entropy).parameters.values()}
    assert all(kinds[n] == inspect.Parameter.KEYWORD_ONLY for n, _ in scal + [("inplace_backward", False)])
    with pytest.raises(NotImplementedError):
        L.CrossEntropyLoss(reduction="max")
    assert isinstance(L.CrossEntropyLoss(reduction="sum", return_z_loss=True), torch.nn.Module)


def test_unsupported_arguments_raise_with_their_name():
    import flash_attn.losses.cross_entropy as L
    import flash_attn.ops.triton.cross_entropy as TC
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    y = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="`process_group`"):
        TC.cross_entropy_loss(x, y, process_group=object())
    with pytest.raises(RuntimeError, match="`precomputed_lse`"):
        TC.cross_entropy_loss(x, y, precomputed_lse=torch.zeros(4))
    with pytest.raises(RuntimeError, match="`process_group`"):
        L.CrossEntropyLoss(process_group=object())(x, y)
    with pytest.raises(RuntimeError, match="`precomputed_lse`"):
        L.CrossEntropyLoss()(x, y, precomputed_lse=torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU"):           # everything served: the CPU tensor itself is the error
        L.CrossEntropyLoss(reduction="none", label_smoothing=0.1, return_z_loss=True, inplace_backward=True)(x, y)
