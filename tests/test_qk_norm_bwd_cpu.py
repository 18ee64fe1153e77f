"""CPU: the host side of fa_qk_norm_rope_bwd - the fp64 yardstick of the GPU tests against torch autograd, the C ABI's argument
checks on host pointers, the ctypes mirror, the workspace query (which needs no device), the Python-level argument errors of
qk_norm.qk_norm_rope_backward / qk_norm_rope, the torch.library ops' schemas and fake implementations.  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import qk_norm_bwd_ref as B


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


# the yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ["neox-full", "interleaved-full", "neox-32", "interleaved-32", "none"])
@pytest.mark.parametrize("weight", [True, False])
def test_reference_backward_equals_autograd_of_the_float64_composition(rot, weight):
    """qk_norm_bwd_ref.backward_ref (the analytic formulas of the op) == torch autograd of forward64 (RMSNorm, rotation at the
    positions, no rounding) to 1e-12 relative, both pair rules, a partial rotary_dim, rows outside the table"""
    T, H, D, S = 13, 3, 64, 20
    g = torch.Generator().manual_seed(3)
    x = torch.randn(T, H, D, generator=g).to(torch.bfloat16)
    dz = torch.randn(T, H, D, generator=g).to(torch.bfloat16)
    w = (1 + 0.2 * torch.randn(D, generator=g)).to(torch.bfloat16) if weight else None
    pos = torch.tensor([3, 4, 5, 19, 0, 7, 7, 2, 11, -1, S, S + 5, 1])
    cos = sin = None
    if rot != "none":
        rd = D if rot.endswith("full") else 32
        ang = torch.arange(S, dtype=torch.float32)[:, None] / (10000 ** (torch.arange(0, rd, 2, dtype=torch.float32) / rd))[None, :]
        cos, sin = torch.cos(ang).to(torch.bfloat16), torch.sin(ang).to(torch.bfloat16)
    il, eps, off = rot.startswith("interleaved"), 1e-6, 0.5
    x64 = x.double().requires_grad_(True)
    w64 = None if w is None else w.double().requires_grad_(True)
    z = B.forward64(x64, w64, pos, None if cos is None else cos.double(), None if sin is None else sin.double(), il, eps, off)
    grads = torch.autograd.grad(z, [x64] + ([] if w is None else [w64]), dz.double())
    ref = B.backward_ref(dz, x, w, pos, cos, sin, il, eps, off)
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()       # noqa: E731
    assert rel(ref["dx"], grads[0].numpy()) <= 1e-12
    if weight:
        assert rel(ref["dw"], grads[1].numpy()) <= 1e-12
        assert (ref["A"] >= np.abs(ref["dx"]) * (1 - 1e-12)).all()            # A bounds what enters the cancellation
        assert (ref["S"] >= np.abs(ref["dw"]) * (1 - 1e-12)).all()
        t = B.backward_ref_torch(dz, x, w, pos, cos, sin, il, eps, off)         # the large-shape form of the same formulas
        for name in ("dx", "dw", "A", "S"):
            assert rel(t[name].numpy(), ref[name]) <= 1e-12, name
        fake = torch.from_numpy(ref["dx"]).to(torch.bfloat16)                  # (the reference rounded once: inside the bound)
        r_np = B.worst(fake, ref["dx"], B.dx_bound(ref["dx"], ref["A"], D, torch.bfloat16))
        assert abs(B.dx_worst_torch(fake, t["dx"], t["A"], torch.bfloat16) - r_np) <= 1e-6 and 0.5 < r_np <= 1.0
    if rot != "none":
        plain = B.backward_ref(dz, x, w, pos, None, None, il, eps, off)
        assert np.abs(plain["dx"][:9] - ref["dx"][:9]).max() > 1e-3              # the rotation matters ...
        assert np.array_equal(plain["dx"][9:12], ref["dx"][9:12])               # ... and rows outside the table are not rotated


def test_plan_restated_in_the_reference_matches_the_library(lib):
    """qk_norm_bwd_ref.plan() (from which the dw bound's L is taken) reports the workspace the library reports"""
    buf = (ctypes.c_char * _TOTAL)()
    for T, Hq, Hk, D in ((77, 4, 2, 128), (1, 1, 1, 8), (5000, 4, 2, 80), (200000, 32, 8, 128), (3, 0, 1, 256), (40000, 4, 2, 256)):
        s, _ = _block(lib, buf)
        s.total_rows, s.nheads_q, s.nheads_k, s.head_dim, s.rotary_dim = T, Hq, Hk, D, 16 if D >= 16 else 0
        if D < 16:
            s.seqlen_ro = 0
        assert lib.qk_norm_rope_bwd_workspace_bytes(s) == B.plan(T, Hq, Hk, D)["workspace_bytes"], (T, Hq, Hk, D)


# the C ABI -------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_struct_size(lib):
    for name in ("fa_qk_norm_rope_bwd", "fa_qk_norm_rope_bwd_workspace_bytes", "fa_qk_norm_rope_bwd_params_size"):
        assert hasattr(lib.lib, name) and name in lib.EXPORTS
    assert lib.lib.fa_qk_norm_rope_bwd_params_size() == ctypes.sizeof(lib.FaQkNormRopeBwdParams)


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
    fields = _header_fields("fa_qk_norm_rope_bwd_params")
    assert [f[0] for f in lib.FaQkNormRopeBwdParams._fields_] == fields
    assert fields[0] == "struct_size" and fields[-1] == "reserved1"
    assert ctypes.sizeof(lib.FaQkNormRopeBwdParams) % 8 == 0


# layout of the host buffer behind a valid block: dq_out / q / dq [8, 4, 64], dk_out / k / dk [8, 2, 64] fp16; positions [8] int64;
# cos / sin [64, 32]; the weights and their gradients [64] (room for fp32); a workspace
_Q = 8 * 4 * 64 * 2
_K = 8 * 2 * 64 * 2
_TAB = 64 * 32 * 2
_W = 64 * 4
_WS = 1 << 14
_OFF = {}
_o = 0
for _n, _sz in (("dq_out", _Q), ("dk_out", _K), ("q", _Q), ("k", _K), ("dq", _Q), ("dk", _K), ("positions", 64), ("rotary_cos", _TAB),
                ("rotary_sin", _TAB), ("q_weight", _W), ("k_weight", _W), ("dq_weight", _W), ("dk_weight", _W), ("workspace", _WS)):
    _OFF[_n] = _o
    _o += _sz
_TOTAL = _o + 64


def _block(lib, buf, form="out"):
    """a valid block over host memory.  form: 'out' (out of place), 'inplace' (dq = dq_out, dk = dk_out), 'norope' (seqlen_ro 0,
    no tables), 'nodw' (no weight gradients, no workspace)"""
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaQkNormRopeBwdParams()
    s.struct_size = ctypes.sizeof(lib.FaQkNormRopeBwdParams)
    for name in ("dq_out", "dk_out", "q", "k", "dq", "dk", "q_weight", "k_weight"):
        setattr(s, name, base + _OFF[name])
    if form == "inplace":
        s.dq, s.dk = s.dq_out, s.dk_out
    s.dqo_row_stride = s.q_row_stride = s.dq_row_stride = 4 * 64
    s.dko_row_stride = s.k_row_stride = s.dk_row_stride = 2 * 64
    s.dqo_head_stride = s.q_head_stride = s.dq_head_stride = s.dko_head_stride = s.k_head_stride = s.dk_head_stride = 64
    if form != "norope":
        s.positions = base + _OFF["positions"]
        s.rotary_cos, s.rotary_sin = base + _OFF["rotary_cos"], base + _OFF["rotary_sin"]
        s.rotary_dim, s.seqlen_ro = 64, 64
    s.total_rows, s.nheads_q, s.nheads_k, s.head_dim = 8, 4, 2, 64
    s.dtype = s.weight_dtype = lib.FA_FP16
    s.eps = 1e-6
    if form != "nodw":
        s.dq_weight, s.dk_weight = base + _OFF["dq_weight"], base + _OFF["dk_weight"]
        s.workspace, s.workspace_bytes = base + _OFF["workspace"], _WS
    return s, base


FORMS = ("out", "inplace", "norope", "nodw")


def test_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_qk_norm_rope_bwd fires before any device work"""
    buf = (ctypes.c_char * _TOTAL)()
    at = lambda name, add=0: (lambda b: b + _OFF[name] + add)      # noqa: E731

    def bad(match, form="out", **kw):
        s, base = _block(lib, buf, form)
        for k, v in kw.items():
            setattr(s, k, v(base) if callable(v) else v)
        with pytest.raises(RuntimeError, match=match) as e:
            lib.call_qk_norm_rope_bwd(s, 0)
        assert "(-1)" in str(e.value)                      # FA_ERR_INVALID_ARGUMENT
        assert "qk_norm_rope_bwd" in str(e.value)
        if "workspace" not in match and "overlaps" not in match:       # (the query looks at neither the workspace nor addresses)
            assert lib.qk_norm_rope_bwd_workspace_bytes(s) == 0

    for form in FORMS:
        bad("struct_size", form, struct_size=8)
        bad("struct_size", form, struct_size=ctypes.sizeof(lib.FaQkNormRopeBwdParams) - 8)
        bad("k and dk_out must not be NULL", form, k=None)
        bad("k and dk_out must not be NULL", form, dk_out=None, dk=None)
        bad("q needs dq_out", form, dq_out=None, dq=None)
        bad("dq needs q", form, q=None)
        bad("reserved", form, reserved=1)
        bad("fp16 or bf16", form, dtype=7, weight_dtype=lib.FA_FP32)
        bad("multiple of 8", form, head_dim=60, rotary_dim=32)
        bad("<= 256", form, head_dim=264)
        for name in ("total_rows", "nheads_q", "nheads_k", "head_dim", "seqlen_ro"):
            bad("non-negative", form, **{name: -1})
        for name in ("dqo_row_stride", "dqo_head_stride", "dko_row_stride", "dko_head_stride", "q_row_stride", "q_head_stride",
                     "k_row_stride", "k_head_stride", "dq_row_stride", "dq_head_stride", "dk_row_stride", "dk_head_stride"):
            bad("strides must be non-negative", form, **{name: -64})
        bad("multiples of 16 bytes", form, k=at("k", 8))
        bad("multiples of 16 bytes", form, dk_out=at("dk_out", 8), dk=at("dk", 0))
        for name in ("q_row_stride", "k_head_stride", "dqo_head_stride", "dko_row_stride"):
            bad("multiples of 16 bytes", form, **{name: 2 * 64 + 4})
        bad("weight_dtype", form, weight_dtype=lib.FA_BF16)
        bad("weight_dtype", form, weight_dtype=lib.FA_FP8_E4M3)
        bad("weight_dtype", form, weight_dtype=9)
        bad("16-byte aligned", form, q_weight=at("q_weight", 8))
        bad("16-byte aligned", form, k_weight=at("k_weight", 2))
        bad("eps", form, eps=-1e-6)
        bad("eps", form, eps=float("inf"))
        bad("eps", form, eps=float("nan"))
        bad("weight_offset", form, weight_offset=float("inf"))
        bad("weight_offset", form, weight_offset=float("nan"))
    for form in ("out", "inplace", "nodw"):
        for name in ("positions", "rotary_cos", "rotary_sin"):
            bad("NULL only where seqlen_ro == 0", form, **{name: None})
        bad("divisible by 16", form, rotary_dim=0)
        bad("divisible by 16", form, rotary_dim=24)
        bad("<= head_dim", form, rotary_dim=80)
        bad("8-byte", form, positions=at("positions", 4))
        bad("16-byte aligned", form, rotary_cos=at("rotary_cos", 8))
    for form in ("out", "inplace", "norope"):
        bad("dq_weight needs q_weight", form, q_weight=None)
        bad("dk_weight needs k_weight", form, k_weight=None)
        bad("16-byte aligned", form, dq_weight=at("dq_weight", 8))
        bad("the workspace holds", form, workspace=None)
        bad("the workspace holds", form, workspace_bytes=2 * 64 * 4 - 1)            # (8 rows: one partial row)
        bad("workspace must be 16-byte aligned", form, workspace=at("workspace", 8))
        bad("dq_weight overlaps dk_weight", form, dk_weight=at("dq_weight", 0))
        bad("dq_weight overlaps q_weight", form, dq_weight=at("q_weight", 0))
        bad("dk_weight overlaps k", form, dk_weight=at("k", 64))
        bad("dq_weight overlaps workspace", form, workspace=at("dq_weight", 0))
        bad("workspace", form, workspace=at("q", 0))                         # the workspace over an input
    bad("dq shares dq_out's base", "inplace", dq_row_stride=8 * 64)
    bad("dk shares dk_out's base", "inplace", dk_head_stride=128)
    for form in ("out", "norope", "nodw"):
        bad("dq overlaps dq_out without being in place", form, dq=at("dq_out", 16))
        bad("dk overlaps dk_out without being in place", form, dk=at("dk_out", 128))
        bad("dq overlaps q", form, dq=at("q", 0))
        bad("dk overlaps k", form, dk=at("k", 0))
        bad("dq overlaps dk", form, dk=at("dq", 256))
        bad("dq overlaps q_weight", form, dq=at("q_weight", 0))
        bad("dk overlaps q_weight", form, dk=at("q_weight", 256 - 16), weight_dtype=lib.FA_FP32)
        bad("dk overlaps k_weight", form, dk=at("k_weight", 0))
    bad("dk overlaps rotary_cos", "out", dk=at("rotary_cos", 32))
    bad("dq overlaps dk_weight", "out", dq=at("dk_weight", 0))
    bad("dk overlaps workspace", "out", dk=at("workspace", 0))
    with pytest.raises(RuntimeError, match="must not be NULL"):
        lib.lib.fa_qk_norm_rope_bwd.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        try:
            if lib.lib.fa_qk_norm_rope_bwd(None, None) != 0:
                raise RuntimeError(lib.lib.fa_last_error().decode())
        finally:
            lib.lib.fa_qk_norm_rope_bwd.argtypes = [ctypes.POINTER(lib.FaQkNormRopeBwdParams), ctypes.c_void_p]


def test_heads_of_one_packed_buffer_are_not_an_overlap(lib):
    """dq and dk as the head slices of ONE packed [T, Hq + Hk, D] gradient interleave row by row without sharing an element: legal
    out of place (into a second packed buffer) - the address ranges overlap, the elements do not.  total_rows 0: nothing runs"""
    buf = (ctypes.c_char * _TOTAL)()
    s, base = _block(lib, buf, "nodw")
    s.dq, s.dk = base + _OFF["dq"], base + _OFF["dq"] + 4 * 64 * 2
    s.dq_row_stride = s.dk_row_stride = 6 * 64
    assert lib.qk_norm_rope_bwd_workspace_bytes(s) == 0
    s.total_rows = 4                                       # (4 rows of 6 heads fit where 8 rows of 4 heads were)
    s2, _ = _block(lib, buf, "nodw")
    s2.dq, s2.dk = base + _OFF["dq"], base + _OFF["dq"] + 3 * 64 * 2          # one head too early: dk starts inside dq's row
    s2.dq_row_stride = s2.dk_row_stride = 6 * 64
    s2.total_rows = 4
    with pytest.raises(RuntimeError, match="dq overlaps dk"):
        lib.call_qk_norm_rope_bwd(s2, 0)


def test_empty_problems_are_ok_without_launch(lib):
    buf = (ctypes.c_char * _TOTAL)()
    for form in ("nodw",):
        for kw in ({"total_rows": 0}, {"nheads_q": 0, "nheads_k": 0}, {"total_rows": 0, "nheads_k": 0},
                   {"total_rows": 0, "q_weight": None, "k_weight": None, "weight_dtype": 9},
                   {"total_rows": 0, "weight_dtype": lib.FA_FP32, "weight_offset": 1.0, "eps": 0.0}):
            s, base = _block(lib, buf, form)
            for k, v in kw.items():
                setattr(s, k, v)
            lib.call_qk_norm_rope_bwd(s, 0)                # FA_OK: nothing is launched (there is no device here)
    # a NULL q counts as no q heads; all four outputs NULL: nothing to do; without a table rotary_dim is not read
    s, base = _block(lib, buf, "nodw")
    s.q = s.dq_out = s.dq = None
    s.nheads_k = 0
    lib.call_qk_norm_rope_bwd(s, 0)
    s, base = _block(lib, buf, "nodw")
    s.seqlen_ro, s.total_rows, s.rotary_dim, s.positions = 0, 0, 24, base + _OFF["positions"] + 4
    lib.call_qk_norm_rope_bwd(s, 0)


def test_workspace_query(lib):
    """0 without weight gradients; non-decreasing in total_rows; saturates at the grid cap; independent of strides and of which
    outputs are asked for next to a dw; needs no device"""
    buf = (ctypes.c_char * _TOTAL)()
    ws = lib.qk_norm_rope_bwd_workspace_bytes
    s, _ = _block(lib, buf, "nodw")
    assert ws(s) == 0
    s, _ = _block(lib, buf)
    s.q_weight = s.k_weight = s.dq_weight = s.dk_weight = None
    assert ws(s) == 0
    s, _ = _block(lib, buf)
    assert ws(s) > 0 and ws(s) % (2 * 64 * 4) == 0        # whole partial rows [2][head_dim] fp32
    prev, sizes = 0, []
    for T in (1, 2, 8, 77, 1000, 5000, 20000, 100000, 1000000, 2 ** 31 - 1):
        s.total_rows = T
        n = ws(s)
        assert n >= prev, (T, n, prev)
        prev = n
        sizes.append(n)
    assert sizes[0] == 2 * 64 * 4 and sizes[-1] == sizes[-2] == B.GRID_CAP * 2 * 64 * 4       # one partial row; the cap
    assert sizes[-1] <= 2 << 20
    s.total_rows = 5000
    n = ws(s)
    s.q_row_stride = s.dq_row_stride = s.dqo_row_stride = 10 * 64
    s.k_head_stride = 128
    s.k_row_stride = 4 * 128
    assert ws(s) == n
    s.dq = s.dk = None
    s.dk_weight = None
    assert ws(s) > 0                                        # only dq_weight is asked for
    s.head_dim, s.rotary_dim = 256, 64
    s.total_rows = 2 ** 31 - 1
    assert ws(s) == B.GRID_CAP * 2 * 256 * 4 <= 2 << 20


# Python ----------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors_on_cpu_tensors():
    from flash_attn_mi355.qk_norm import qk_norm_rope_backward as f
    q = torch.zeros(8, 4, 64, dtype=torch.float16)
    k = torch.zeros(8, 2, 64, dtype=torch.float16)
    pos = torch.arange(8)
    cos = torch.zeros(32, 32, dtype=torch.float16)
    w = torch.ones(64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="fp16 or bf16"):
        f(q.float(), k.float(), q.float(), k.float(), pos, cos, cos)
    with pytest.raises(RuntimeError, match=r"k must be \(total_rows"):
        f(q, k[None], q, k[None], pos, cos, cos)
    with pytest.raises(RuntimeError, match="dk_out must have k's dtype and shape"):
        f(q, k[:7], q, k, pos, cos, cos)
    with pytest.raises(RuntimeError, match="dk_out must have k's dtype and shape"):
        f(q, None, q, k, pos, cos, cos)
    with pytest.raises(RuntimeError, match="q must have k's dtype"):
        f(q, k, q.bfloat16(), k, pos, cos, cos)
    with pytest.raises(RuntimeError, match=r"q must be \(total_rows"):
        f(q, k, q[:7], k, pos, cos, cos)
    with pytest.raises(RuntimeError, match="dq_out must have q's dtype and shape"):
        f(q[:, :2], k, q, k, pos, cos, cos)
    with pytest.raises(RuntimeError, match="dq_out without q"):
        f(q, k, None, k, pos, cos, cos)
    k60 = torch.zeros(8, 2, 60, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        f(None, k60, None, k60, pos, cos[:, :16], cos[:, :16])
    with pytest.raises(RuntimeError, match="go together"):
        f(q, k, q, k, None, cos, cos)
    with pytest.raises(RuntimeError, match="k's dtype"):
        f(q, k, q, k, pos, cos.float(), cos.float())
    with pytest.raises(RuntimeError, match="same shape"):
        f(q, k, q, k, pos, cos, cos[:16])
    with pytest.raises(RuntimeError, match="multiple of 16"):
        f(q, k, q, k, pos, cos[:, :12], cos[:, :12])
    with pytest.raises(RuntimeError, match="<= headdim"):
        big = torch.zeros(32, 40, dtype=torch.float16)
        f(q, k, q, k, pos, big, big)
    with pytest.raises(RuntimeError, match="positions must be"):
        f(q, k, q, k, pos[:5], cos, cos)
    with pytest.raises(RuntimeError, match="q_weight must have k's dtype"):
        f(q, k, q, k, pos, cos, cos, q_weight=w.bfloat16())
    with pytest.raises(RuntimeError, match=r"k_weight must have shape \(headdim,\)"):
        f(q, k, q, k, pos, cos, cos, w, w[:32])
    with pytest.raises(RuntimeError, match="same dtype"):
        f(q, k, q, k, pos, cos, cos, w, w.float())
    with pytest.raises(RuntimeError, match="q_weight without q"):
        f(None, k, None, k, pos, cos, cos, w, w)
    with pytest.raises(RuntimeError, match="eps must be finite"):
        f(q, k, q, k, pos, cos, cos, w, w, eps=-1.0)
    with pytest.raises(RuntimeError, match="weight_offset must be finite"):
        f(q, k, q, k, pos, cos, cos, w, w, weight_offset=float("inf"))
    # everything else in order: the CPU tensor itself is the error
    with pytest.raises(RuntimeError, match="GPU"):
        f(q, k, q, k, pos, cos, cos, w, w)
    with pytest.raises(RuntimeError, match="GPU"):
        f(None, k, None, k, pos.int(), cos, cos, None, w.float(), weight_offset=1.0, interleaved=True, inplace=True, need_dw=False)
    with pytest.raises(RuntimeError, match="GPU"):
        f(q, k, q, k, None, None, None, w.float(), w.float(), need_dq=False, need_dk=False)


def test_torch_op_schemas_and_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import flash_attn_mi355.torch_ops as T
    fwd = torch.ops.flash_attn_mi355.qk_norm_rope.default._schema
    bwd = torch.ops.flash_attn_mi355.qk_norm_rope_bwd.default._schema
    for schema in (fwd, bwd):
        assert not [a.name for a in schema.arguments if a.alias_info is not None]      # functional: nothing is mutated
    assert [a.name for a in fwd.arguments] == ["q", "k", "positions", "rotary_cos", "rotary_sin", "q_weight", "k_weight", "eps",
                                               "weight_offset", "interleaved"]
    assert len(fwd.returns) == 2
    assert [a.name for a in bwd.arguments] == ["dq_out", "dk_out", "q", "k", "positions", "rotary_cos", "rotary_sin", "q_weight",
                                               "k_weight", "eps", "weight_offset", "interleaved", "need_dq", "need_dk",
                                               "need_dq_weight", "need_dk_weight"]
    assert len(bwd.returns) == 4
    with FakeTensorMode():
        qkv = torch.empty(200, 8, 64, dtype=torch.bfloat16, device="cuda")
        q, k = qkv[:, :4], qkv[:, 4:6]
        ids = torch.empty(200, dtype=torch.int64, device="cuda")
        cos = torch.empty(64, 32, dtype=torch.bfloat16, device="cuda")
        w = torch.empty(64, dtype=torch.float32, device="cuda")
        f, b = torch.ops.flash_attn_mi355.qk_norm_rope, torch.ops.flash_attn_mi355.qk_norm_rope_bwd
        qo, ko = f(q, k, ids, cos, cos, w, w, 1e-6, 0.0, False)
        assert qo.shape == q.shape and ko.shape == k.shape and qo.dtype == ko.dtype == torch.bfloat16 and qo.is_contiguous()
        qo, ko = f(None, k, None, None, None, None, w, 1e-5, 1.0, True)
        assert qo.shape == (0,) and ko.shape == k.shape
        dq, dk, dqw, dkw = b(q, k, q, k, ids, cos, cos, w, w, 1e-6, 0.0, False, True, True, True, True)
        assert dq.shape == q.shape and dk.shape == k.shape and dq.dtype == torch.bfloat16
        assert dqw.shape == dkw.shape == (64,) and dqw.dtype == dkw.dtype == torch.float32
        dq, dk, dqw, dkw = b(None, k, None, k, ids, cos, cos, None, w, 1e-6, 0.0, False, True, False, True, True)
        assert dq.shape == dk.shape == dqw.shape == (0,) and dkw.shape == (64,)
        dq, dk, dqw, dkw = b(q, k, q, k, None, None, None, w, None, 1e-6, 0.0, False, False, True, False, False)
        assert dq.shape == dqw.shape == dkw.shape == (0,) and dk.shape == k.shape
    assert "qk_norm_rope" not in T.__all__ and "qk_norm_rope_bwd" not in T.__all__      # reached through torch.ops only


def test_public_name_lists_are_unchanged_and_abi_version(lib):
    import flash_attn
    import flash_attn_mi355
    for name in ("qk_norm_rope", "qk_norm_rope_backward", "qk_norm_rope_bwd"):
        assert name not in flash_attn.__all__ and name not in flash_attn_mi355.__all__
    assert lib.FA_ABI_VERSION == 4 and lib.lib.fa_abi_version() == 4
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert re.search(r"#define FA_ABI_VERSION 4\b", open(os.path.join(root, "include", "fa_mi355.h")).read())
