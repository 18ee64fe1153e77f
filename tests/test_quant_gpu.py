"""GPU: fa_quant_fp8 against the torch fp32 restatement of the rule (quant_ref.py, held to exact arithmetic in test_quant_cpu.py),
and the fused forms against the unfused ones - add_norm_quant == quant_fp8(add_norm), act_mul_quant == quant_fp8(act_mul).
Everything is bit for bit: codes, scales, residual_out.  Then the layouts, a row alone, the library's own fp8 consumer, the special
values, the guard bands, a captured graph, rows 2^30 elements apart and opcheck."""
import pytest
import torch

import act_mul_ref
import guard
import quant_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
FP8 = torch.float8_e4m3fn
ROWS = (1, 3, 67)
MODES = ("row", "group", "static")
ACTIVATIONS = ("silu", "gelu", "gelu_tanh", "relu", "relu2")
STATIC = {"scale": 0.37}


def _mods():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import act_mul, add_norm, quant
    return quant, add_norm, act_mul


def _same(got, want, name):
    if want is None or got is None:
        assert got is None and want is None, name
        return
    R.assert_same(got, want.to(got.device), name)


def _kw(mode, scale_ub=None):
    return dict(mode=mode, **(STATIC if mode == "static" else {}), **({} if scale_ub is None else {"scale_ub": scale_ub}))


_INPUTS = {}


def _x(rows, N, dtype, seed=0):
    """quant_ref.inputs on the GPU, made once per key and never written"""
    key = (rows, N, dtype, seed)
    if key not in _INPUTS:
        _INPUTS[key] = R.inputs(rows, N, dtype, seed=seed, device="cuda")
    return _INPUTS[key]


def _ref(x, mode, scale_ub=None):
    """the reference on the CPU (torch's own float8 cast), from the GPU tensor's values"""
    return R.quant_ref(x.cpu(), **_kw(mode, scale_ub))


# fa_quant_fp8 against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_quant_fp8_equals_the_reference(mode, dtype):
    """every N at which the kernel takes another path: one piece; the small form with a ragged last group of lanes; its last N
    and the first wide one; 4096 / 4104 (one and two pieces a lane), 16384 (8 pieces, 256 lanes), 65536 (8 pieces, 1024 lanes);
    group mode at 128, 384 (lanes past the row in the small form) and 14336"""
    Q, _, _ = _mods()
    for N in (128, 384, 14336) if mode == "group" else (8, 136, 256, 264, 512, 520, 4096, 4104, 16384, 65536):
        for rows in ROWS:
            x = _x(rows, N, dtype)
            snap = x.clone()
            codes, scales = Q.quant_fp8(x, **_kw(mode))
            rc, rs = _ref(x, mode)
            _same(codes, rc, f"codes N {N} rows {rows}")
            _same(scales, rs, f"scales N {N} rows {rows}")
            _same(x, snap, "x is unchanged")
            assert codes.is_contiguous() and tuple(codes.shape) == (rows, N) and codes.dtype == FP8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_quant_fp8_layouts_and_edge_rows(mode, dtype):
    """a padded row stride; rows misaligned by 2 bytes with codes on odd addresses (the element paths); scale_ub below and above
    the amax; an all-zero row (floored scale, +0 codes); the amax in the last column and in the first; [B, S, N]"""
    Q, _, _ = _mods()
    for N, rows in ((384, 67), (4224, 3)):
        x = _x(rows, N, dtype, seed=3).clone()
        x[0] = 0
        x[1 % rows, :] = x[1 % rows, :].clamp(-1, 1)
        x[1 % rows, N - 1] = -1000.0
        x[2 % rows, :] = x[2 % rows, :].clamp(-1, 1)
        x[2 % rows, 0] = 777.0
        for ub in (None, 2.0, 1e6) if mode != "static" else (None,):
            want = _ref(x, mode, ub)
            got = Q.quant_fp8(x, **_kw(mode, ub))
            _same(got[0], want[0], f"codes N {N} ub {ub}")
            _same(got[1], want[1], f"scales N {N} ub {ub}")
            if mode != "static":
                s = got[1].reshape(rows, -1)
                assert float(s[0].max()) == R.FLOOR and not bool(got[0][0].view(torch.uint8).any())
                if ub == 2.0:
                    assert bool((s == torch.tensor(2.0 / 448, dtype=torch.float32)).any()) and bool((s < 2.0 / 448).any())
        want = Q.quant_fp8(x, **_kw(mode))
        # a [:, :N] view of wider rows
        wide = torch.full((rows, N + 24), float("nan"), dtype=dtype, device="cuda")
        wide[:, :N] = x
        got = Q.quant_fp8(wide[:, :N], **_kw(mode))
        _same(got[0], want[0], "padded stride codes")
        _same(got[1], want[1], "padded stride scales")
        # every row starts 2 bytes off a 16-byte boundary (and off a 4-byte one); codes rows on odd addresses
        flat = torch.full((rows * (N + 8) + 8,), float("nan"), dtype=dtype, device="cuda")
        xm = flat[1:1 + rows * (N + 8)].view(rows, N + 8)[:, :N]
        xm.copy_(x)
        assert all(xm[r].data_ptr() % 16 == 2 for r in range(rows))
        cflat = torch.zeros(rows * (N + 1) + 8, dtype=torch.uint8, device="cuda").view(FP8)
        cm = cflat[1:1 + rows * (N + 1)].view(rows, N + 1)[:, :N]
        sc = None if mode == "static" else torch.empty_like(want[1])
        got = Q.quant_fp8(xm, **_kw(mode), out=(cm, sc))
        assert got[0] is cm and got[1] is sc
        _same(cm.contiguous(), want[0], "misaligned codes")
        _same(sc, want[1], "misaligned scales")
        # [B, S, N]
        if rows == 67:
            continue
        x3 = x.view(1, rows, N)
        got = Q.quant_fp8(x3, **_kw(mode))
        _same(got[0], want[0].view(1, rows, N), "3-D codes")
        if mode != "static":
            assert tuple(got[1].shape) == ((1, rows) if mode == "row" else (1, rows, N // 128))


# fused == unfused -----------------------------------------------------------------------------------------------------------
_NORM_CASES = [
    # (is_rms_norm, residual, bias, fp32 weights, options)
    (True, None, False, False, {}),
    (True, "io", False, False, {}),
    (True, "fp32", False, True, {"weight_offset": 1.0}),
    (False, "io", True, False, {"residual_in_fp32": True}),
    (False, None, True, True, {"prenorm": True, "eps": 1e-5}),
    (False, "io", False, False, {"inplace": True}),
    (True, "fp32", True, False, {"inplace": True}),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_add_norm_quant_equals_quant_of_add_norm(mode, dtype):
    """codes, scales and residual_out at both of add_norm's forms and every `pieces` case of the wide kernel (264: one, 4096:
    two, 8192: four, 16384: eight), RMSNorm and LayerNorm, with and without residual, bias, fp32 residual, fp32 weights, and with
    residual_out being residual itself"""
    Q, A, _ = _mods()
    for N in (256, 2048, 4096, 8192, 16384) if mode == "group" else (8, 64, 256, 264, 2048, 4096, 8192, 16384):
        w16 = (_x(1, N, dtype, seed=11)[0].float().clamp(-2, 2) * 0.5 + 1).to(dtype)
        b16 = _x(1, N, dtype, seed=12)[0].float().clamp(-1, 1).to(dtype)
        for rows in ROWS:
            x, r = _x(rows, N, dtype, seed=5), _x(rows, N, dtype, seed=6)
            for rms, res, bias, w32, opt in _NORM_CASES:
                w = w16.float() if w32 else w16
                b = None if not bias else (b16.float() if w32 else b16)
                res_a = None if res is None else (r.float() if res == "fp32" else r.clone())
                res_b = None if res_a is None else res_a.clone()
                opt = dict(opt)
                inplace = opt.pop("inplace", False)
                out, ro = A.add_norm_forward(x, w, b, res_a, is_rms_norm=rms, **opt)
                want = Q.quant_fp8(out, **_kw(mode))
                got = Q.add_norm_quant(x, res_b, w, b, is_rms_norm=rms, inplace_residual=inplace, **opt, **_kw(mode))
                name = f"N {N} rows {rows} rms {rms} residual {res} bias {bias} w32 {w32} {opt} inplace {inplace}"
                _same(got[0], want[0], "codes " + name)
                _same(got[1], want[1], "scales " + name)
                _same(got[2], ro, "residual_out " + name)
                if inplace and res is not None:
                    assert got[2] is res_b
                elif res_b is not None:
                    _same(res_b, res_a, "residual is unchanged " + name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("activation", ACTIVATIONS)
def test_act_mul_quant_equals_quant_of_act_mul(activation, dtype):
    """gated, ungated and packed; row, group and static; 8 and 520 (one wave, a ragged second one), 5632 / 11008 / 14336 (4 and 8
    pieces a lane on 256 lanes), 28672 / 53248 (4 and 8 pieces on 1024 lanes) - the last three widths at rows = 3 only"""
    Q, _, M = _mods()
    for N in (8, 520, 5632, 11008, 14336, 28672, 53248):
        for rows in ROWS if N < 14336 else (3,):
            g, u, _ = act_mul_ref.inputs(rows, N, dtype, seed=1, device="cuda")
            packed = torch.cat([g, u], dim=-1)
            for mode in MODES:
                if mode == "group" and N % 128:
                    continue
                for form in ("gated", "ungated", "packed"):
                    if form == "packed":
                        want = Q.quant_fp8(M.act_mul_forward(packed[:, :N], packed[:, N:], activation=activation), **_kw(mode))
                        got = Q.act_and_mul_quant(packed, activation=activation, **_kw(mode))
                    else:
                        up = u if form == "gated" else None
                        want = Q.quant_fp8(M.act_mul_forward(g, up, activation=activation), **_kw(mode))
                        got = Q.act_mul_quant(g, up, activation=activation, **_kw(mode))
                    _same(got[0], want[0], f"codes N {N} rows {rows} {mode} {form}")
                    _same(got[1], want[1], f"scales N {N} rows {rows} {mode} {form}")
            del g, u, packed


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_forms_on_misaligned_rows(dtype):
    """act_mul_quant on rows that start 2 bytes off a 16-byte boundary (element by element) has the aligned bits"""
    Q, _, _ = _mods()
    rows, N = 3, 4104
    g, u, _ = act_mul_ref.inputs(rows, N, dtype, seed=2, device="cuda")
    for mode in ("row", "static"):
        want = Q.act_mul_quant(g, u, **_kw(mode))
        flat = torch.zeros(2 * rows * (N + 8) + 16, dtype=dtype, device="cuda")
        gm = flat[1:1 + rows * (N + 8)].view(rows, N + 8)[:, :N]
        um = flat[rows * (N + 8) + 9:rows * (N + 8) + 9 + rows * (N + 8)].view(rows, N + 8)[:, :N]
        gm.copy_(g)
        um.copy_(u)
        assert gm.data_ptr() % 16 == 2 and um.data_ptr() % 16 == 2
        got = Q.act_mul_quant(gm, um, **_kw(mode))
        _same(got[0], want[0], "codes")
        _same(got[1], want[1], "scales")


# a row depends on itself alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ("row", "group"))
def test_a_row_does_not_depend_on_the_batch_and_calls_repeat(mode, dtype):
    Q, A, M = _mods()
    for N in (256, 4096):
        x, r = _x(67, N, dtype, seed=7), _x(67, N, dtype, seed=8)
        w = (_x(1, N, dtype, seed=11)[0].float().clamp(-2, 2) * 0.5 + 1).to(dtype)
        calls = {
            "quant_fp8": lambda t, t2: Q.quant_fp8(t, **_kw(mode)),
            "add_norm_quant": lambda t, t2: Q.add_norm_quant(t, t2, w, **_kw(mode))[:2],
            "add_layer_norm_quant": lambda t, t2: Q.add_norm_quant(t, t2, w, is_rms_norm=False, **_kw(mode))[:2],
            "act_mul_quant": lambda t, t2: Q.act_mul_quant(t, t2, **_kw(mode)),
        }
        for name, call in calls.items():
            full, again = call(x, r), call(x, r)
            _same(again[0], full[0], name + " repeats: codes")
            _same(again[1], full[1], name + " repeats: scales")
            for i in (0, 41, 66):
                one = call(x[i:i + 1], r[i:i + 1])
                _same(one[0], full[0][i:i + 1], f"{name} row {i} alone: codes")
                _same(one[1], full[1][i:i + 1], f"{name} row {i} alone: scales")


# the library's own consumer -------------------------------------------------------------------------------------------------
def test_static_codes_feed_the_fp8_attention_forward():
    """flash_attn_func on quant_fp8(q | k | v, mode='static', scale=d) returns the bits it returns on the torch-built codes: the
    codes are equal, so this is an integration check"""
    import flash_attn
    Q, _, _ = _mods()
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(2, 200, h, 128, generator=g).mul(s).to(torch.bfloat16).cuda() for h, s in ((4, 1.5), (2, 2.0), (2, 0.7)))
    ds = (0.05, 0.0625, 0.013)
    eager = [(t.float() * (torch.tensor(1.0) / torch.tensor(d))).clamp(-448, 448).to(FP8) for t, d in zip((q, k, v), ds)]
    ours = [Q.quant_fp8(t, mode="static", scale=d)[0] for t, d in zip((q, k, v), ds)]
    for a, b, name in zip(ours, eager, "qkv"):
        _same(a, b, name + " codes")
        assert a.shape == b.shape and a.is_contiguous()
    kw = dict(causal=True, softmax_scale=128 ** -0.5 * ds[0] * ds[1])    # (descales fold into the scale; out * ds[2] is the caller's)
    want = flash_attn.flash_attn_func(*eager, **kw)
    got = flash_attn.flash_attn_func(*ours, **kw)
    assert want.dtype == torch.bfloat16 and bool(torch.isfinite(want.float()).all())
    _same(got, want, "attention out")


# special values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_special_values(mode, dtype):
    """NaN and +-inf in one row: no fault, the other rows' bits are unchanged, and the row is what flash_attn_mi355/quant.py
    says - the reference's bits (test_quant_cpu.py pins those to the documented values); the same through the fused forms"""
    Q, A, M = _mods()
    N = 4096
    x = _x(3, N, dtype, seed=9)
    clean = Q.quant_fp8(x, **_kw(mode))
    for ub in (None, 3.0) if mode != "static" else (None,):
        for vals in ((float("nan"),), (float("inf"), float("-inf")), (float("nan"), float("inf"))):
            y = x.clone()
            for j, v in enumerate(vals):
                y[1, 5 + 1000 * j] = v
            got = Q.quant_fp8(y, **_kw(mode, ub))
            want = _ref(y, mode, ub)
            _same(got[0], want[0], f"codes {vals} ub {ub}")
            _same(got[1], want[1], f"scales {vals} ub {ub}")
            assert not bool(((got[0].view(torch.uint8) & 0x7F) == 0x7F).any())
            if ub is None:
                _same(got[0][[0, 2]], clean[0][[0, 2]], "the other rows' codes")
                if mode != "static":
                    _same(got[1][[0, 2]], clean[1][[0, 2]], "the other rows' scales")
            if mode == "row" and ub is None:
                want_scale = clean[1][1] if len(vals) == 1 else torch.tensor(float("inf"))       # (a NaN alone is skipped)
                assert float(got[1][1]) == float(want_scale)
            # the fused forms see the same y: an ungated relu passes positive values, +inf and NaN through
            fused = Q.act_mul_quant(y, None, activation="relu", **_kw(mode, ub))
            unf = Q.quant_fp8(M.act_mul_forward(y, None, activation="relu"), **_kw(mode, ub))
            _same(fused[0], unf[0], "relu codes")
            _same(fused[1], unf[1], "relu scales")
            w = torch.ones(N, dtype=dtype, device="cuda")
            fused = Q.add_norm_quant(y, None, w, **_kw(mode, ub))
            unf = Q.quant_fp8(A.add_norm_forward(y, w)[0], **_kw(mode, ub))
            _same(fused[0], unf[0], "norm codes")
            _same(fused[1], unf[1], "norm scales")
    torch.cuda.synchronize()


# guard bands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_outputs_stay_inside_their_tensors(mode):
    """codes (gapped rows), scales and residual_out between NaN bands: nothing outside their elements is written, every element
    inside is, and the inputs' surroundings are not read into the results (they are NaN)"""
    Q, A, M = _mods()
    dtype = torch.bfloat16
    for rows, N in ((3, 264), (67, 4224), (3, 16384)):
        if mode == "group" and N % 128:
            continue
        x, r = _x(rows, N, dtype, seed=13), _x(rows, N, dtype, seed=14)
        w = torch.ones(N, dtype=dtype, device="cuda")
        xb, xv, xs = guard.guarded(x, row_dim=0)
        sshape = None if mode == "static" else ((rows,) if mode == "row" else (rows, N // 128))

        def outs():
            cb, cv, cs = guard.guarded(shape=(rows, N), dtype=FP8, gaps=True, device="cuda", row_dim=0)
            if sshape is None:
                return (cb, cv, cs), None
            sb, sv = guard.slab(sshape + (1,) * (2 - len(sshape)), torch.float32, gaps=False, device="cuda", check_prep=False, row_dim=0)
            return (cb, cv, cs), (sb, sv, guard.snapshot(sb))

        def check(c, s, name):
            torch.cuda.synchronize()
            guard.assert_untouched(*c, name + " codes")
            assert not bool((c[1].view(torch.uint8) == 0x7F).any()), name + ": a code was not written"
            if s is not None:
                guard.assert_untouched(*s, name + " scales")
                assert not bool(torch.isnan(s[1]).any()), name + ": a scale was not written"

        c, s = outs()
        want = Q.quant_fp8(x, **_kw(mode))
        Q.quant_fp8(xv, **_kw(mode), out=(c[1], None if s is None else s[1].view(sshape)))
        check(c, s, "quant_fp8")
        _same(c[1].contiguous(), want[0], "quant_fp8 codes")
        guard.assert_untouched(xb, xv, xs, "x")
        c, s = outs()
        Q.act_mul_quant(xv, None, activation="gelu", **_kw(mode), out=(c[1], None if s is None else s[1].view(sshape)))
        check(c, s, "act_mul_quant")
        c, s = outs()
        rb, rv, rs = guard.guarded(r, row_dim=0)
        _, _, ro = Q.add_norm_quant(xv, rv, w, inplace_residual=True, **_kw(mode), out=(c[1], None if s is None else s[1].view(sshape)))
        check(c, s, "add_norm_quant")
        assert ro is rv
        torch.cuda.synchronize()
        guard.assert_untouched(rb, rv, rs, "residual_out")
        _same(rv.contiguous(), A.add_norm_forward(x, w, None, r)[1], "residual_out")


# a captured graph -----------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    """one graph, one stream, no parallel branches: each op replayed on new contents gives the eager bits"""
    Q, A, M = _mods()
    dtype, rows, N = torch.bfloat16, 67, 4096
    x, r = _x(rows, N, dtype, seed=15).clone(), _x(rows, N, dtype, seed=16)
    w = torch.ones(N, dtype=dtype, device="cuda")

    def fn():
        a = Q.quant_fp8(x, mode="row")
        b = Q.add_norm_quant(x, r, w, mode="group")
        c = Q.act_mul_quant(x, r, mode="row", scale_ub=5.0)
        d = Q.quant_fp8(x, mode="static", scale=0.5)[:1]
        return a + b + c + d
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = fn()
    x.copy_(_x(rows, N, dtype, seed=17))                    # new contents, same buffers
    g.replay()
    torch.cuda.synchronize()
    eager = fn()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(outs, eager)):
        _same(a, b, f"output {i}")


# rows 2^30 elements apart -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["quant_fp8", "add_norm_quant", "act_mul_quant"])
def test_rows_a_gibi_element_apart(op):
    """a 3-row view whose row stride is 2^30 elements, input and codes (the last row starts 4 GiB into the input and 2 GiB into the
    codes): the allocations are not filled, only the rows are checked - against the same rows held contiguously"""
    Q, A, M = _mods()
    dtype, N, RS = torch.bfloat16, 4104 if op != "add_norm_quant" else 4096, 2 ** 30
    x = _x(3, N, dtype, seed=18)
    big = torch.empty(2 * RS + N, dtype=dtype, device="cuda")
    xv = big.as_strided((3, N), (RS, 1))
    xv.copy_(x)
    cbig = torch.empty(2 * RS + N, dtype=torch.uint8, device="cuda").view(FP8)
    cv = cbig.as_strided((3, N), (RS, 1))
    sc = torch.empty(3, dtype=torch.float32, device="cuda")
    if op == "quant_fp8":
        want = Q.quant_fp8(x, mode="row")
        Q.quant_fp8(xv, mode="row", out=(cv, sc))
    elif op == "act_mul_quant":
        want = Q.act_mul_quant(x, None, activation="silu", mode="row")
        Q.act_mul_quant(xv, None, activation="silu", mode="row", out=(cv, sc))
    else:
        w = torch.ones(N, dtype=dtype, device="cuda")
        want = Q.add_norm_quant(x, None, w, mode="row")
        Q.add_norm_quant(xv, None, w, mode="row", out=(cv, sc))
    _same(cv.contiguous(), want[0], "codes")
    _same(sc, want[1], "scales")
    del big, cbig


# opcheck --------------------------------------------------------------------------------------------------------------------
def test_opcheck_on_the_four_ops():
    """test_schema and test_faketensor; a tensor that requires grad raises by name"""
    import flash_attn_mi355.torch_ops  # noqa: F401
    ns = torch.ops.flash_attn_mi355
    dtype = torch.bfloat16
    x, r = _x(3, 256, dtype, seed=19), _x(3, 256, dtype, seed=20)
    w = torch.ones(256, dtype=dtype, device="cuda")
    cases = []
    for mode, scale, ub in (("row", None, None), ("group", None, 2.0), ("static", 0.5, None)):
        cases += [(ns.quant_fp8.default, (x, mode, scale, ub)),
                  (ns.add_norm_quant.default, (x, r, w, None, 1e-6, 0.0, True, False, False, mode, scale, ub)),
                  (ns.add_norm_quant.default, (x, None, w, w, 1e-6, 0.0, False, True, True, mode, scale, ub)),
                  (ns.act_mul_quant.default, (x, r, "silu", mode, scale, ub)),
                  (ns.act_mul_quant.default, (x, None, "gelu", mode, scale, ub)),
                  (ns.act_and_mul_quant.default, (x, "gelu_tanh", mode, scale, ub))]
    for op, args in cases:
        torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))
    Q, _, _ = _mods()
    c, s = ns.quant_fp8(x, "static", 0.5, None)
    assert tuple(s.shape) == (0,) and s.dtype == torch.float32
    _same(c, Q.quant_fp8(x, mode="static", scale=0.5)[0], "static codes through torch.ops")
    c, s, ro = ns.add_norm_quant(x, None, w, None, 1e-6, 0.0, True, False, False, "row", None, None)
    assert tuple(ro.shape) == (0,)
    want = Q.add_norm_quant(x, None, w)
    _same(c, want[0], "codes through torch.ops")
    _same(s, want[1], "scales through torch.ops")
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="quant_fp8: x requires grad"):
        ns.quant_fp8(xg, "row", None, None)
    with pytest.raises(RuntimeError, match="add_norm_quant: .*weight requires grad"):
        ns.add_norm_quant(x, None, w.clone().requires_grad_(True), None, 1e-6, 0.0, True, False, False, "row", None, None)
    with pytest.raises(RuntimeError, match="act_mul_quant: up requires grad"):
        ns.act_mul_quant(x, xg, "silu", "row", None, None)
    with pytest.raises(RuntimeError, match="act_and_mul_quant: x requires grad"):
        ns.act_and_mul_quant(xg, "silu", "row", None, None)
    with torch.no_grad():
        ns.quant_fp8(xg, "row", None, None)
