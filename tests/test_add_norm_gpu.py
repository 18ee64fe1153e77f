"""GPU: fa_add_norm / fa_add_norm_bwd (flash_attn_mi355.add_norm) - residual add + RMSNorm / LayerNorm over the hidden size and its
backward.  out, dx, dres, dweight and dbias are held against the fp64 restatement (add_norm_ref) within bounds derived by counting
roundings (written out in add_norm_ref's docstring):
    forward    |out - y|   <= 0.5 ulp16(y)  + k_fwd(N) u M,   k_fwd = 2 (depth(N) + 8)  <= 64,   u = 2^-24
    backward   |dx - dz|   <= 0.5 ulp(dz)   + k_bwd(N) u A,   k_bwd = 6 depth(N) + 44   <= 188
    dw / db    |got - ref| <= 0.5 ulp_w(ref) + gamma(L + depth(N) + 8) S,  L the longest addition chain of the launch plan
with depth(N) <= 24 the longest chain of roundings of one fixed-order row sum, M / A / S the magnitudes that enter the respective
cancellation (for LayerNorm they carry R = mean|z| rstd, the size of what enters z - mean).  The reference is fed the kernel's own
residual_out; the residual add itself, in-place forms, prenorm, batch invariance, repeatability, the N <= 256 equality with the
QK-norm kernels, autograd, a captured graph and the guard bands are bit for bit.
Inputs (test_add_norm_cpu._inputs): rows of magnitude 1e-3, 1 and 1e2 side by side (eps = 1e-6 matters in the first), for
LayerNorm a row mean of four standard deviations, weights around 1 with both signs, a non-zero bias.
Shapes: N 8 (one lane a row), 72 (lanes of the group past the row), 256 (the largest group), 264 (the first workgroup-per-row
size, one wave partly empty), 1000 (two waves, the last partly empty), 4096 (two pieces a lane), 5120 (three of four pieces),
16384 (the largest register tile); rows 1, 3, 67 and 1031 (more rows than the 256 partial rows)."""
import ctypes

import pytest
import torch

import add_norm_ref as R
import guard
import test_add_norm_cpu as C
from util import DT

pytestmark = pytest.mark.gpu

EPS = 1e-6
SHAPES = [(8, 1031), (72, 67), (256, 1031), (264, 3), (264, 1031), (1000, 67), (4096, 1), (4096, 1031), (5120, 3), (16384, 1),
          (16384, 67)]
# (is_rms_norm, bias, fp32 weights, residual: None / "io" / "fp32", residual_in_fp32, weight_offset)
CONFIGS = [(True, False, False, "io", False, 0.0), (True, False, True, "fp32", False, 1.0), (True, True, False, None, False, 1.0),
           (False, True, False, "io", True, 0.0), (False, True, True, "fp32", False, 1.0), (False, False, True, None, True, 0.0)]


def _A():
    from flash_attn_mi355 import add_norm
    return add_norm


def _inputs(rows, n, dt, ln, fp32w=False, res="io", seed=0):
    x, r, dy, w, b = (t.cuda() for t in C._inputs(rows, n, DT[dt], seed=seed, ln=ln))
    if fp32w:
        w, b = w.float(), b.float()
    r = None if res is None else (r.float() if res == "fp32" else r)
    return x, r, dy, w, b


def _eq(got, want, name):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert torch.equal(guard.bits(got), guard.bits(want)), f"{name}: the bits differ"


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("n,rows", SHAPES)
def test_forward_against_the_fp64_reference_within_the_derived_bound(n, rows, dt):
    """out against add_norm_ref.norm_ref of the kernel's own residual_out within fwd_bound, and residual_out against the one
    fp32 add and one rounding, bit for bit; RMSNorm and LayerNorm, with and without bias, both weight dtypes, both residual
    dtypes, residual_in_fp32, both values of weight_offset"""
    A = _A()
    for is_rms, bias, fp32w, res, in32, off in CONFIGS:
        x, r, _, w, b = _inputs(rows, n, dt, not is_rms, fp32w, res, seed=n)
        b = b if bias else None
        snap = [t.clone() for t in (x, w) + (() if r is None else (r,))]
        out, ro = A.add_norm_forward(x, w, b, r, eps=EPS, weight_offset=off, is_rms_norm=is_rms, prenorm=True, residual_in_fp32=in32)
        torch.cuda.synchronize()
        for t, t0 in zip((x, w) + (() if r is None else (r,)), snap):
            _eq(t, t0, "an input (read only)")
        ro_dtype = torch.float32 if (res == "fp32" or in32) else DT[dt]
        _eq(ro, R.add_ref(x, r, ro_dtype), "residual_out")
        y, M = R.norm_ref(ro, w, b, EPS, off, is_rms)
        ratio = R.worst(out, y, R.fwd_bound(y, M, n, DT[dt]))
        print(f"N {n} rows {rows} {dt} rms {is_rms} bias {bias} w32 {fp32w} res {res}: out worst error / bound {ratio:.3f}")
        assert out.dtype == DT[dt] and ratio <= 1.0, f"out worst error / bound {ratio:.3f} ({is_rms}, {bias}, {fp32w}, {res}, {off})"


# 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("n,rows", [(72, 67), (256, 1031), (1000, 67), (5120, 3), (16384, 3)])
def test_forms_of_the_forward_are_bit_identical(n, rows, dt):
    """add_norm(x, residual) == add_norm(residual_out); inplace == out of place; fused_add_rms_norm_ == add_norm; prenorm returns
    the same out; a strided view == its contiguous copy"""
    A = _A()
    for is_rms, bias, fp32w, res, in32, off in CONFIGS:
        if res is None:
            continue
        x, r, _, w, b = _inputs(rows, n, dt, not is_rms, fp32w, res, seed=n + 1)
        b = b if bias else None
        kw = dict(eps=EPS, weight_offset=off, is_rms_norm=is_rms)
        out, ro = A.add_norm(x, w, b, r, prenorm=True, residual_in_fp32=in32, **kw)
        _eq(A.add_norm(x, w, b, r, residual_in_fp32=in32, **kw), out, "out without prenorm")
        if ro.dtype == x.dtype:
            _eq(A.add_norm(ro, w, b, **kw), out, "the norm of residual_out")
        else:                                                  # (fp32 residual_out: the same op on the same stored values)
            zero = torch.zeros_like(x)
            out2, ro2 = A.add_norm(zero, w, b, ro, prenorm=True, **kw)
            _eq(ro2, ro, "residual_out + 0"); _eq(out2, out, "the norm of residual_out + 0")
        xi, ri = x.clone(), r.clone()
        got = A.add_norm(xi, w, b, ri, prenorm=True, residual_in_fp32=in32, inplace=True, **kw)
        assert got[0] is xi and (got[1] is ri) == (r.dtype == ro.dtype)
        _eq(xi, out, "out in place"); _eq(got[1], ro, "residual_out in place")
        wide_x, wide_r = torch.zeros(rows, 2 * n + 8, dtype=x.dtype, device="cuda"), torch.zeros(rows, 2 * n + 8, dtype=r.dtype, device="cuda")
        wide_x[:, 8:8 + n], wide_r[:, n:2 * n] = x, r
        out3, ro3 = A.add_norm(wide_x[:, 8:8 + n], w, b, wide_r[:, n:2 * n], prenorm=True, residual_in_fp32=in32, **kw)
        _eq(out3, out, "out of strided views"); _eq(ro3, ro, "residual_out of strided views")
        if is_rms and not bias and off == 0.0:
            xi, ri = x.clone(), r.clone()
            gx, gr = A.fused_add_rms_norm_(xi, ri, w, EPS)
            assert gx is xi and gr is ri
            _eq(xi, out, "fused_add_rms_norm_ x"); _eq(ri, R.add_ref(x, r, r.dtype), "fused_add_rms_norm_ residual")


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("n", [8, 72, 128, 256])
def test_small_rows_have_the_bits_of_the_qk_norm_kernels(n, dt):
    """N <= 256, RMSNorm without bias: out == qk_norm.qk_rms_norm on x.view(-1, Hk, N), and dx == qk_norm.qk_norm_rope_backward
    without rotation (and without dres_out), for both weight dtypes and both values of weight_offset"""
    from flash_attn_mi355 import qk_norm
    A = _A()
    rows, hk = 66, 3
    for fp32w, off in ((False, 0.0), (True, 1.0)):
        x, _, dy, w, _ = _inputs(rows, n, dt, False, fp32w, None, seed=n + 2)
        out = A.add_norm(x, w, eps=EPS, weight_offset=off)
        _, want = qk_norm.qk_rms_norm(None, x.view(-1, hk, n), None, w, EPS, weight_offset=off)
        _eq(out.view(-1, hk, n), want, "out vs qk_rms_norm")
        dx, _, dw, _ = A.add_norm_backward(dy, x, w, eps=EPS, weight_offset=off)
        _, dk, _, dkw = qk_norm.qk_norm_rope_backward(None, dy.view(-1, hk, n), None, x.view(-1, hk, n), None, None, None, None, w, EPS, off)
        _eq(dx.view(-1, hk, n), dk, "dx vs qk_norm_rope_backward")
        assert dw.dtype == dkw.dtype


@pytest.mark.parametrize("is_rms", [True, False])
@pytest.mark.parametrize("n", [72, 264, 4096, 16384])
def test_a_row_does_not_depend_on_the_batch(n, is_rms):
    """a row alone, first, last and in the middle of a batch of 1031 rows has the same out, residual_out and dx bits; two runs of
    the backward give identical dweight / dbias bits"""
    A = _A()
    dt, rows = "bf16", 1031
    x, r, dy, w, b = _inputs(rows, n, dt, not is_rms, True, "io", seed=n + 3)
    kw = dict(eps=EPS, weight_offset=1.0, is_rms_norm=is_rms)
    out, ro = A.add_norm(x, w, b, r, prenorm=True, **kw)
    dro = torch.flip(dy, (0,))
    dx, _, dw, db = A.add_norm_backward(dy, ro, w, dro, need_db=True, **kw)
    for i in (0, 517, rows - 1):
        o1, r1 = A.add_norm(x[i:i + 1], w, b, r[i:i + 1], prenorm=True, **kw)
        _eq(o1, out[i:i + 1], f"out of row {i} alone"); _eq(r1, ro[i:i + 1], f"residual_out of row {i} alone")
        d1 = A.add_norm_backward(dy[i:i + 1], ro[i:i + 1], w, dro[i:i + 1], need_dw=False, **kw)[0]
        _eq(d1, dx[i:i + 1], f"dx of row {i} alone")
    sub = slice(500, 567)                                      # the row first and last in another batch
    o2 = A.add_norm(x[sub], w, b, r[sub], **kw)
    _eq(o2, out[sub], "out of rows 500 .. 566 as their own batch")
    d2 = A.add_norm_backward(dy[sub], ro[sub], w, dro[sub], need_db=True, **kw)
    _eq(d2[0], dx[sub], "dx of rows 500 .. 566 as their own batch (with a weight gradient)")
    again = A.add_norm_backward(dy, ro, w, dro, need_db=True, **kw)
    _eq(again[0], dx, "dx, second run"); _eq(again[2], dw, "dweight, second run"); _eq(again[3], db, "dbias, second run")


# 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("n,rows", SHAPES)
def test_backward_against_the_fp64_reference_within_the_derived_bounds(n, rows, dt):
    """dx, dres, dweight, dbias against add_norm_ref.backward_ref within dz_bound / dw_bound; z of the io dtype and of fp32, a
    dres_out added in (prenorm), dres of both dtypes; dx == dres where their dtypes agree"""
    A = _A()
    for is_rms, bias, fp32w, res, in32, off in CONFIGS:
        x, r, dy, w, _ = _inputs(rows, n, dt, not is_rms, fp32w, res, seed=n + 4)
        z = R.add_ref(x, r, torch.float32 if (res == "fp32" or in32) else DT[dt])
        dro = None if res is None else (0.5 * torch.flip(dy, (0,)).float()).to(z.dtype)
        dres_dtype = torch.float32 if res == "fp32" else DT[dt]
        snap = [t.clone() for t in (dy, z, w)]
        dx, dres, dw, db = A.add_norm_backward(dy, z, w, dro, eps=EPS, weight_offset=off, is_rms_norm=is_rms, dres_dtype=dres_dtype,
                                               need_dres=True, need_db=bias)
        torch.cuda.synchronize()
        for t, t0 in zip((dy, z, w), snap):
            _eq(t, t0, "an input (read only)")
        ref = R.backward_ref(dy, z, w, dro, EPS, off, is_rms)
        L = R.plan(rows, n, bias)["L"]
        rx = R.worst(dx, ref["dz"], R.dz_bound(ref["dz"], ref["A"], n, DT[dt]))
        rr = R.worst(dres, ref["dz"], R.dz_bound(ref["dz"], ref["A"], n, dres_dtype))
        rw = R.worst(dw, ref["dw"], R.dw_bound(ref["dw"], ref["Sw"], L, n, w.dtype))
        rb = R.worst(db, ref["db"], R.dw_bound(ref["db"], ref["Sb"], L, n, w.dtype)) if bias else 0.0
        print(f"N {n} rows {rows} {dt} rms {is_rms} w32 {fp32w} res {res}: worst error / bound dx {rx:.3f} dres {rr:.3f} "
              f"dw {rw:.3f} db {rb:.3f} (L = {L})")
        assert dx.dtype == DT[dt] and dres.dtype == dres_dtype and dw.dtype == w.dtype and (db is None) == (not bias)
        assert max(rx, rr, rw, rb) <= 1.0, (rx, rr, rw, rb)
        if dres_dtype == DT[dt]:
            _eq(dres, dx, "dres vs dx (the same dtype)")
        if dro is not None and rows >= 3:                      # dres_out is added in (a row of magnitude 1e2: dz is small next to it)
            plain = R.backward_ref(dy, z, w, None, EPS, off, is_rms)["dz"]
            assert R.worst(dx, plain, R.dz_bound(plain, ref["A"], n, DT[dt])) > 2.0


def test_skipped_outputs_and_in_place_backward():
    """each need_* switch off: that output is None and the others keep their bits (dweight alone: the same partial rows); in
    place dx is dy itself with the out-of-place bits"""
    A = _A()
    n, rows, dt = 1000, 67, "bf16"
    x, r, dy, w, _ = _inputs(rows, n, dt, True, True, "fp32", seed=9)
    z = R.add_ref(x, r, torch.float32)
    kw = dict(eps=EPS, weight_offset=0.0, is_rms_norm=False, dres_dtype=torch.float32)
    full = A.add_norm_backward(dy, z, w, None, need_dres=True, need_db=True, **kw)
    for skip in range(4):
        need = [i != skip for i in range(4)]
        got = A.add_norm_backward(dy, z, w, None, need_dx=need[0], need_dres=need[1], need_dw=need[2], need_db=need[3], **kw)
        for i, name in enumerate(("dx", "dres", "dweight", "dbias")):
            if i == skip:
                assert got[i] is None
            else:                                              # (without dbias the partial rows are [1][N]: the same sums)
                _eq(got[i], full[i], f"{name} without output {skip}")
    assert A.add_norm_backward(dy, z, w, None, need_dx=False, need_dw=False, **kw) == (None, None, None, None)
    dyi = dy.clone()
    got = A.add_norm_backward(dyi, z, w, None, inplace=True, need_dres=True, need_db=True, **kw)
    assert got[0] is dyi
    for i, name in enumerate(("dx", "dres", "dweight", "dbias")):
        _eq(got[i], full[i], f"{name} in place")


# 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rms-prenorm-fp32res", "ln-bias", "rms-plain", "ln-prenorm-in32", "rms-prenorm-nores-in32"])
def test_autograd_equals_the_backward_bit_for_bit(case):
    """torch.autograd through torch.ops.flash_attn_mi355.add_norm (add_norm.add_norm) == add_norm_backward on the same tensors"""
    A = _A()
    n, rows, dt = 264, 67, "bf16"
    is_rms = case.startswith("rms")
    res = "fp32" if "fp32res" in case else (None if case == "rms-plain" or "nores" in case else "io")
    in32, prenorm, bias = "in32" in case, "prenorm" in case, case.startswith("ln")
    x, r, dy, w, b = _inputs(rows, n, dt, not is_rms, True, res, seed=11)
    b = b if bias else None
    leaves = [t.clone().requires_grad_(True) for t in (x, w) + ((b,) if bias else ()) + ((r,) if r is not None else ())]
    xl, wl = leaves[0], leaves[1]
    bl = leaves[2] if bias else None
    rl = leaves[-1] if r is not None else None
    kw = dict(eps=EPS, weight_offset=1.0, is_rms_norm=is_rms)
    got = A.add_norm(xl, wl, bl, rl, prenorm=prenorm, residual_in_fp32=in32, **kw)
    out, ro = got if prenorm else (got, None)
    out0, ro0 = A.add_norm_forward(x, w, b, r, prenorm=True, residual_in_fp32=in32, **kw)
    _eq(out.detach(), out0, "out")
    dro = None
    if prenorm:
        _eq(ro.detach(), ro0, "residual_out")
        dro = (0.25 * torch.flip(dy, (1,)).float()).to(ro.dtype)
    grads = torch.autograd.grad([out] + ([ro] if prenorm else []), leaves, [dy] + ([dro] if prenorm else []))
    z = ro0 if (r is not None or prenorm) else x           # (without a residual: the prenorm copy of x, in its dtype)
    need_r = r is not None
    same = need_r and r.dtype == x.dtype
    want = A.add_norm_backward(dy, z, w, dro, dres_dtype=None if r is None else r.dtype, need_dres=need_r and not same, need_db=bias, **kw)
    torch.cuda.synchronize()
    _eq(grads[0], want[0], "dx through autograd"); _eq(grads[1], want[2], "dweight through autograd")
    if bias:
        _eq(grads[2], want[3], "dbias through autograd")
    if need_r:
        _eq(grads[-1], want[0] if same else want[1], "dresidual through autograd")


def test_autograd_through_the_upstream_named_modules():
    """flash_attn.ops.triton.layer_norm.RMSNorm (zero-centred weight, residual, prenorm), flash_attn.ops.rms_norm.RMSNorm and
    flash_attn.ops.layer_norm.DropoutAddLayerNorm in eval mode: forward and gradients equal add_norm / add_norm_backward bit for
    bit; layer_norm_fn writes into caller-owned out / residual_out"""
    from flash_attn.ops.layer_norm import DropoutAddLayerNorm
    from flash_attn.ops.rms_norm import RMSNorm as OpsRMSNorm
    from flash_attn.ops.triton.layer_norm import RMSNorm, layer_norm_fn
    A = _A()
    n, rows, dt = 1000, 67, "bf16"
    x, r, dy, w, b = _inputs(rows, n, dt, True, False, "io", seed=12)
    m = RMSNorm(n, eps=EPS, zero_centered_weight=True, device="cuda", dtype=DT[dt])
    with torch.no_grad():
        m.weight.copy_(w)
    xl, rl = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    out, ro = m(xl, residual=rl, prenorm=True)
    out0, ro0 = A.add_norm_forward(x, w, None, r, eps=EPS, weight_offset=1.0, prenorm=True)
    _eq(out.detach(), out0, "RMSNorm out"); _eq(ro.detach(), ro0, "RMSNorm residual_out")
    dro = torch.flip(dy, (0,))
    gx, gr, gw = torch.autograd.grad([out, ro], [xl, rl, m.weight], [dy, dro])
    want = A.add_norm_backward(dy, ro0, w, dro, eps=EPS, weight_offset=1.0)
    _eq(gx, want[0], "RMSNorm dx"); _eq(gr, want[0], "RMSNorm dresidual"); _eq(gw, want[2], "RMSNorm dweight")
    o = OpsRMSNorm(n, eps=EPS, device="cuda", dtype=DT[dt])
    _eq(o(x).detach(), A.add_norm_forward(x, torch.ones_like(w), eps=EPS)[0], "ops.rms_norm.RMSNorm")
    ln = DropoutAddLayerNorm(n, prenorm=True, p=0.1, eps=EPS, residual_in_fp32=True, device="cuda", dtype=torch.float32).eval()
    with torch.no_grad():
        ln.weight.copy_(w.float()); ln.bias.copy_(b.float())
    y, res = ln(x, r)
    y0, res0 = A.add_norm_forward(x, w.float(), b.float(), r, eps=EPS, is_rms_norm=False, prenorm=True, residual_in_fp32=True)
    _eq(y.detach(), y0, "DropoutAddLayerNorm out"); _eq(res.detach(), res0, "DropoutAddLayerNorm residual_out")
    assert res.dtype == torch.float32
    buf_o, buf_r = torch.empty_like(x), torch.empty(rows, n, dtype=torch.float32, device="cuda")
    got = layer_norm_fn(x, w.float(), b.float(), residual=r, eps=EPS, prenorm=True, residual_in_fp32=True, out=buf_o, residual_out=buf_r)
    assert got[0] is buf_o and got[1] is buf_r
    _eq(buf_o, y0, "layer_norm_fn out="); _eq(buf_r, res0, "layer_norm_fn residual_out=")


def test_forward_and_backward_replay_in_a_graph():
    """forward (residual, prenorm) + backward with dweight / dbias (both launches, the workspace allocated during capture)
    captured in one graph; replayed after the inputs were overwritten in place: every output equals the eager result bit for bit"""
    A = _A()
    n, rows, dt = 4096, 67, "bf16"
    kw = dict(eps=EPS, weight_offset=0.0, is_rms_norm=False)
    sets = [_inputs(rows, n, dt, True, True, "io", seed=20 + i) for i in range(3)]

    def run(x, r, dy, w, b):
        out, ro = A.add_norm_forward(x, w, b, r, prenorm=True, **kw)
        dx, _, dw, db = A.add_norm_backward(dy, ro, w, None, need_db=True, **kw)
        return out, ro, dx, dw, db

    ref = [tuple(t.clone() for t in run(*s)) for s in sets]
    st = [t.clone() for t in sets[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(*st)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(*st)
    for i in (1, 2, 0):
        for dst, src in zip(st, sets[i]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for got, want, name in zip(outs, ref[i], ("out", "residual_out", "dx", "dweight", "dbias")):
            _eq(got, want, f"replay {i}: {name}")
    assert not torch.equal(guard.bits(ref[0][0]), guard.bits(ref[1][0]))


# 5 -------------------------------------------------------------------------------------------------------------------------
def _fwd_into(x, r, out, ro, w, b, is_rms, off):
    """fa_add_norm with caller-owned outputs: the C ABI through the ctypes mirror, filled the way add_norm_forward fills it"""
    from flash_attn_mi355 import _lib
    from flash_attn_mi355 import flash_attn_interface as fi
    io = fi._DTYPES[x.dtype]
    code = lambda t: _lib.FA_FP32 if t.dtype == torch.float32 else io      # noqa: E731
    s = _lib.FaAddNormParams()
    s.struct_size = ctypes.sizeof(_lib.FaAddNormParams)
    for name, t in (("x", x), ("residual", r), ("out", out), ("residual_out", ro)):
        setattr(s, name, t.data_ptr())
        setattr(s, name + "_row_stride", t.stride(0))
    s.weight, s.bias = w.data_ptr(), b.data_ptr()
    s.rows, s.n, s.dtype = x.shape[0], x.shape[1], io
    s.residual_dtype, s.residual_out_dtype, s.weight_dtype = code(r), code(ro), code(w)
    s.is_rms_norm, s.eps, s.weight_offset = int(is_rms), EPS, off
    _lib.call_add_norm(s, fi._stream(x.device))


def _bwd_into(dy, z, dro, dx, dres, w, dw, db, is_rms, off, workspace):
    from flash_attn_mi355 import _lib
    from flash_attn_mi355 import flash_attn_interface as fi
    io = fi._DTYPES[dy.dtype]
    code = lambda t: _lib.FA_FP32 if t.dtype == torch.float32 else io      # noqa: E731
    s = _lib.FaAddNormBwdParams()
    s.struct_size = ctypes.sizeof(_lib.FaAddNormBwdParams)
    for name, t in (("dy", dy), ("z", z), ("dres_out", dro), ("dx", dx), ("dres", dres)):
        setattr(s, name, t.data_ptr())
        setattr(s, name + "_row_stride", t.stride(0))
    s.weight, s.dweight, s.dbias = w.data_ptr(), dw.data_ptr(), db.data_ptr()
    s.rows, s.n, s.dtype = dy.shape[0], dy.shape[1], io
    s.z_dtype, s.dres_dtype, s.weight_dtype = code(z), code(dres), code(w)
    s.is_rms_norm, s.eps, s.weight_offset = int(is_rms), EPS, off
    nbytes = _lib.add_norm_bwd_workspace_bytes(s)
    ws = workspace(nbytes, dy.device)
    if nbytes:
        s.workspace, s.workspace_bytes = ws.data_ptr(), nbytes
    _lib.call_add_norm_bwd(s, fi._stream(dy.device))
    return nbytes


def _guarded_1d(t):
    """(buf, view): the [N] tensor exactly sized between two bands of 4096 elements that hold -1 / all-ones bits"""
    buf = torch.full((4096 + t.numel() + 4096,), -1, dtype=guard._INT_OF[t.dtype], device="cuda").view(t.dtype)
    view = buf[4096:4096 + t.numel()]
    view.copy_(t)
    return buf, view


def _bands_hold(buf, n, name):
    b = guard.bits(buf)
    assert bool((b[:4096] == -1).all()) and bool((b[4096 + n:] == -1).all()), f"{name}: written outside its {n} elements"


@pytest.mark.parametrize("n,rows,is_rms,fp32", [(72, 67, True, False), (1000, 67, False, True), (16384, 3, False, False)])
def test_guard_bands(n, rows, is_rms, fp32):
    """x, residual, out, residual_out, dy, z, dres_out, dx and dres are views with gaps between their rows inside NaN-filled
    slabs, the weight, the bias and their gradients sit exactly sized inside guarded buffers, and the workspace has exactly the
    queried size between sentinel bands (its interior pre-filled with 0xFF: a partial row read before it is written would show):
    nothing outside a tensor's logical elements or the reported workspace is written, the NaN of the gaps reaches no output, the
    inputs are bit-unchanged"""
    A = _A()
    dt, off = "bf16", 1.0
    x_d, r_d, dy_d, w_d, b_d = _inputs(rows, n, dt, not is_rms, fp32, "fp32" if fp32 else "io", seed=30)
    want_o, want_ro = A.add_norm_forward(x_d, w_d, b_d, r_d, eps=EPS, weight_offset=off, is_rms_norm=is_rms, prenorm=True)
    dro_d = torch.flip(dy_d, (0,)).to(want_ro.dtype)
    want = A.add_norm_backward(dy_d, want_ro, w_d, dro_d, eps=EPS, weight_offset=off, is_rms_norm=is_rms, dres_dtype=r_d.dtype,
                               need_dres=True, need_db=True)
    ins = [guard.guarded(t) for t in (x_d, r_d)]
    ob, o, osnap = guard.guarded(shape=(rows, n), dtype=DT[dt], device="cuda")
    rob, ro, rosnap = guard.guarded(shape=(rows, n), dtype=want_ro.dtype, device="cuda")
    (wb, w), (bb, b) = _guarded_1d(w_d), _guarded_1d(b_d)
    assert o.stride(0) > n and ins[0][1].stride(0) > n       # gaps between the rows
    _fwd_into(ins[0][1], ins[1][1], o, ro, w, b, is_rms, off)
    torch.cuda.synchronize()
    _eq(o, want_o, "out"); _eq(ro, want_ro, "residual_out")
    for (buf, view, snap), name in zip(ins, ("x", "residual")):
        assert torch.equal(guard.bits(buf), snap), f"{name} was written"
    guard.assert_untouched(ob, o, osnap, "out"); guard.assert_untouched(rob, ro, rosnap, "residual_out")

    bins = [guard.guarded(t) for t in (dy_d, want_ro, dro_d)]
    dxb, dx, dxs = guard.guarded(shape=(rows, n), dtype=DT[dt], device="cuda")
    drb, dres, drs = guard.guarded(shape=(rows, n), dtype=r_d.dtype, device="cuda")
    (dwb, dw), (dbb, db) = _guarded_1d(torch.zeros_like(w_d)), _guarded_1d(torch.zeros_like(w_d))
    workspace, check_ws = guard.guarded_workspace("ones")
    nbytes = _bwd_into(bins[0][1], bins[1][1], bins[2][1], dx, dres, w, dw, db, is_rms, off, workspace)
    torch.cuda.synchronize()
    assert nbytes == R.plan(rows, n, True)["workspace_bytes"] and check_ws()["sizes"] == [nbytes]
    _eq(dx, want[0], "dx"); _eq(dres, want[1], "dres"); _eq(dw.clone(), want[2], "dweight"); _eq(db.clone(), want[3], "dbias")
    for (buf, view, snap), name in zip(bins, ("dy", "z", "dres_out")):
        assert torch.equal(guard.bits(buf), snap), f"{name} was written"
    guard.assert_untouched(dxb, dx, dxs, "dx"); guard.assert_untouched(drb, dres, drs, "dres")
    for buf, name in ((wb, "weight"), (bb, "bias"), (dwb, "dweight"), (dbb, "dbias")):
        _bands_hold(buf, n, name)
    _eq(w.clone(), w_d, "weight (read only)"); _eq(b.clone(), b_d, "bias (read only)")
    # in place through the Python layer: the gapped x and residual are taken as they are and rewritten where they are
    xb, xv, xs = guard.guarded(x_d)
    rb, rv, rs = guard.guarded(r_d)
    workspace2, check2 = guard.guarded_workspace("random")
    from flash_attn_mi355 import flash_attn_interface as fi
    got = A.add_norm(xv, w_d, b_d, rv, eps=EPS, weight_offset=off, is_rms_norm=is_rms, prenorm=True, inplace=True)
    torch.cuda.synchronize()
    assert got[0] is xv and got[1] is rv
    _eq(xv, want_o, "out in place"); _eq(rv, want_ro, "residual_out in place")
    guard.assert_untouched(xb, xv, xs, "x in place"); guard.assert_untouched(rb, rv, rs, "residual in place")
    saved = fi._workspace
    fi._workspace = workspace2
    try:
        again = A.add_norm_backward(bins[0][1], bins[1][1], w_d, bins[2][1], eps=EPS, weight_offset=off, is_rms_norm=is_rms,
                                    dres_dtype=r_d.dtype, need_dres=True, need_db=True)
    finally:
        fi._workspace = saved
    assert check2()["sizes"] == [nbytes]
    for g, wnt, name in zip(again, want, ("dx", "dres", "dweight", "dbias")):
        _eq(g, wnt, f"{name} (random workspace)")
