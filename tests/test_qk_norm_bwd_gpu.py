"""GPU: fa_qk_norm_rope_bwd (flash_attn_mi355.qk_norm.qk_norm_rope_backward / qk_norm_rope) - the backward of the per-head RMSNorm +
RoPE at per-token positions.  dx and dw are held against the fp64 restatement (qk_norm_bwd_ref) within bounds derived by counting
roundings; without weights the op is held bit for bit against the rotary backward (apply_rotary with conjugate=True); everything
else - batch invariance, in place, skipped outputs, guard bands, autograd, a captured graph - is bit for bit against the op itself.
Base shape: T = 77 rows, Hq 4, Hk 2, the positions of test_qk_norm_gpu.py (a ragged batch, a block of tree depths, three
out-of-table values), weights 1 + 0.2 randn."""
import ctypes

import numpy as np
import pytest
import torch

import guard
import qk_norm_bwd_ref as B
import test_qk_norm_gpu as F
from util import DT, rand16

pytestmark = pytest.mark.gpu

T, HQ, HK, SEQLEN_RO, EPS = F.T, F.HQ, F.HK, F.SEQLEN_RO, F.EPS
_bits, _eq, _tables, _weights, _positions = F._bits, F._eq, F._tables, F._weights, F._positions


def _bwd(*a, **kw):
    from flash_attn_mi355.qk_norm import qk_norm_rope_backward
    return qk_norm_rope_backward(*a, **kw)


def _rot(rot, D, dt):
    """(cos, sin, interleaved) of one of test_qk_norm_gpu.py's four rotary forms, or no rotation"""
    return (None, None, False) if rot == "none" else _tables(rot, D, dt)


def _data(D, dt, hq=HQ, hk=HK, rows=T, seed=0):
    """dq_out, dk_out, q, k"""
    return (rand16((rows, hq, D), dt, 41 + seed), rand16((rows, hk, D), dt, 42 + seed), rand16((rows, hq, D), dt, 1 + seed),
            rand16((rows, hk, D), dt, 2 + seed))


def _eqw(got, want, name):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert torch.equal(guard.bits(got), guard.bits(want)), f"{name}: the bits differ"


def _hold(name, got_dx, got_dw, dz, x, w, pos, cos, sin, il, off, dt, L):
    """one tensor's dx (and dw) against the fp64 reference within the derived bounds; returns the worst ratios"""
    D = x.shape[-1]
    ref = B.backward_ref(dz, x, w, None if cos is None else pos, cos, sin, il, EPS, off)
    if w is None:
        r = B.worst(got_dx, ref["dx"], B.dx_bound_plain(ref["dx"], DT[dt]))
        print(f"{name}: dx worst error / bound {r:.3f}")
        assert r <= 1.0, f"{name}: dx worst error / bound {r:.3f}"
        assert got_dw is None
        return
    assert np.abs(ref["dx"] - B.backward_ref(dz, x, None, None if cos is None else pos, cos, sin, il, EPS, off)["dx"]).max() > 1e-2
    r = B.worst(got_dx, ref["dx"], B.dx_bound(ref["dx"], ref["A"], D, DT[dt]))
    rw = B.worst(got_dw, ref["dw"], B.dw_bound(ref["dw"], ref["S"], L, D, got_dw.dtype))
    print(f"{name}: dx worst error / bound {r:.3f}, dw {rw:.3f} (L = {L})")
    assert r <= 1.0, f"{name}: dx worst error / bound {r:.3f}"
    assert rw <= 1.0, f"{name}: dw worst error / bound {rw:.3f}"


# a -------------------------------------------------------------------------------------------------------------------------
_SHAPES = [(8, "none")] + [(D, rot) for D in (64, 80, 128, 256) for rot in F.ROTS + ["none"]]


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D,rot", _SHAPES)
def test_against_the_fp64_reference_within_the_derived_bounds(D, rot, dt):
    """dq, dk, dq_weight, dk_weight against qk_norm_bwd_ref within dx_bound / dw_bound, for weights of the io type and of fp32 and
    weight_offset 0 and 1.  D 8: one lane a head; 80: lanes of the group past the head; 256: 32 lanes a head"""
    cos, sin, il = _rot(rot, D, dt)
    pos = _positions().cuda()
    dzq, dzk, q, k = _data(D, dt)
    L = B.plan(T, HQ, HK, D)["L"]
    for fp32, off in ((False, 0.0), (True, 1.0), (False, 1.0), (True, 0.0)):
        qw, kw = _weights(D, dt, fp32)
        snap = [t.clone() for t in (dzq, dzk, q, k)]
        dq, dk, dqw, dkw = _bwd(dzq, dzk, q, k, None if cos is None else pos, cos, sin, qw, kw, EPS, off, il)
        torch.cuda.synchronize()
        for t, t0 in zip((dzq, dzk, q, k), snap):
            _eq(t, t0, "an input (read only)")
        assert dqw.dtype == qw.dtype and dkw.dtype == kw.dtype and dqw.shape == dkw.shape == (D,)
        _hold(f"q w{'32' if fp32 else '16'} off{off}", dq, dqw, dzq, q, qw, pos, cos, sin, il, off, dt, L)
        _hold(f"k w{'32' if fp32 else '16'} off{off}", dk, dkw, dzk, k, kw, pos, cos, sin, il, off, dt, L)


@pytest.mark.parametrize("rot", ["neox-full", "interleaved-32", "none"])
def test_optional_forms_against_the_fp64_reference(rot):
    """q_weight=None (q only rotated back), k_weight=None, q=None, and dq_out / dk_out / q / k as strided views of one packed
    [T, Hq + 2 Hk, D] gradient and one packed input, taken without a copy: the bounds of test (a); the strided call gives the bits
    of the contiguous one"""
    from flash_attn_mi355 import flash_attn_interface as fi
    D, dt = 128, "bf16"
    cos, sin, il = _rot(rot, D, dt)
    pos = _positions().cuda()
    p = None if cos is None else pos
    dzq, dzk, q, k = _data(D, dt)
    qw, kw = _weights(D, dt)
    L = B.plan(T, HQ, HK, D)["L"]
    full = _bwd(dzq, dzk, q, k, p, cos, sin, qw, kw, EPS, 0.0, il)
    dq, dk, dqw, dkw = _bwd(dzq, dzk, q, k, p, cos, sin, None, kw, EPS, 0.0, il)
    torch.cuda.synchronize()
    assert dqw is None
    _hold("q (no weight)", dq, None, dzq, q, None, pos, cos, sin, il, 0.0, dt, L)
    _eq(dk, full[1], "dk (q_weight=None)"); _eqw(dkw, full[3], "dk_weight (q_weight=None)")
    dq, dk, dqw, dkw = _bwd(dzq, dzk, q, k, p, cos, sin, qw, None, EPS, 0.0, il)
    torch.cuda.synchronize()
    assert dkw is None
    _hold("k (no weight)", dk, None, dzk, k, None, pos, cos, sin, il, 0.0, dt, L)
    _eq(dq, full[0], "dq (k_weight=None)"); _eqw(dqw, full[2], "dq_weight (k_weight=None)")
    dq, dk, dqw, dkw = _bwd(None, dzk, None, k, p, cos, sin, None, kw, EPS, 0.0, il)
    torch.cuda.synchronize()
    assert dq is None and dqw is None
    _eq(dk, full[1], "dk (q=None)")
    _hold("k (q=None)", dk, dkw, dzk, k, kw, pos, cos, sin, il, 0.0, dt, B.plan(T, 0, HK, D)["L"])
    gqkv, qkv = rand16((T, HQ + 2 * HK, D), dt, 7), rand16((T, HQ + 2 * HK, D), dt, 8)
    gq, gk, xq, xk = gqkv[:, :HQ], gqkv[:, HQ:HQ + HK], qkv[:, :HQ], qkv[:, HQ:HQ + HK]
    assert all(fi._prep(t, D) is t for t in (gq, gk, xq, xk))    # the wrapper takes the views as they are
    want = _bwd(gq.contiguous(), gk.contiguous(), xq.contiguous(), xk.contiguous(), p, cos, sin, qw, kw, EPS, 0.0, il)
    got = _bwd(gq, gk, xq, xk, p, cos, sin, qw, kw, EPS, 0.0, il)
    torch.cuda.synchronize()
    _eq(got[0], want[0], "dq (strided views)"); _eq(got[1], want[1], "dk (strided views)")
    _eqw(got[2], want[2], "dq_weight (strided views)"); _eqw(got[3], want[3], "dk_weight (strided views)")
    _hold("q (strided views)", got[0], got[2], gq, xq, qw, pos, cos, sin, il, 0.0, dt, L)


# b -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("rot", F.ROTS)
def test_without_weights_the_bits_of_the_rotary_backward(rot, dt):
    """no weights: dq, dk == flash_attn.layers.rotary.apply_rotary(..., conjugate=True) - the function of that module that takes
    `conjugate`; apply_rotary_emb's own backward calls it - on a packed batch whose positions are offset + i per sequence, bit for
    bit; the rows whose position is outside the table equal dz"""
    from flash_attn.layers.rotary import apply_rotary
    D = 128
    cos, sin, il = _tables(rot, D, dt)
    lens, offs = [20, 1, 25, 31], [3, 40, 7, 40]            # the last sequence runs out of the table (56 rows) after 16 rows
    assert sum(lens) == T
    pos = torch.tensor([o + i for n, o in zip(lens, offs) for i in range(n)], dtype=torch.int64).cuda()
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32).cuda()
    so = torch.tensor(offs, dtype=torch.int32).cuda()
    dzq, dzk, q, k = _data(D, dt)
    dq, dk, dqw, dkw = _bwd(dzq, dzk, q, k, pos, cos, sin, interleaved=il)
    want_q = apply_rotary(dzq, cos, sin, seqlen_offsets=so, cu_seqlens=cu, max_seqlen=max(lens), interleaved=il, conjugate=True)
    want_k = apply_rotary(dzk, cos, sin, seqlen_offsets=so, cu_seqlens=cu, max_seqlen=max(lens), interleaved=il, conjugate=True)
    torch.cuda.synchronize()
    assert dqw is None and dkw is None
    _eq(dq, want_q, "dq"); _eq(dk, want_k, "dk")
    out = (pos >= SEQLEN_RO)
    assert int(out.sum()) == 15
    _eq(dq[out], dzq[out], "dq, rows outside the table"); _eq(dk[out], dzk[out], "dk, rows outside the table")
    assert not torch.equal(_bits(dq[~out]), _bits(dzq[~out]))


# c -------------------------------------------------------------------------------------------------------------------------
def test_batch_invariance_and_repeatability():
    """dq / dk of rows 10 .. 40 computed alone == those rows of the full call, and one head alone == that head, bit for bit (a
    head's sums never see another row or head); two identical calls give identical bits in all four outputs"""
    D, dt = 80, "bf16"
    cos, sin, il = _tables("neox-32", D, dt)
    pos = _positions().cuda()
    dzq, dzk, q, k = _data(D, dt)
    qw, kw = _weights(D, dt)
    a = _bwd(dzq, dzk, q, k, pos, cos, sin, qw, kw, EPS, 0.0, il)
    b = _bwd(dzq, dzk, q, k, pos, cos, sin, qw, kw, EPS, 0.0, il)
    sub = slice(10, 40)
    s = _bwd(dzq[sub], dzk[sub], q[sub], k[sub], pos[sub], cos, sin, qw, kw, EPS, 0.0, il)
    one = _bwd(dzq[:, 2:3], dzk, q[:, 2:3], k, pos, cos, sin, qw, kw, EPS, 0.0, il, need_dw=False)
    torch.cuda.synchronize()
    _eq(a[0], b[0], "dq, second call"); _eq(a[1], b[1], "dk, second call")
    _eqw(a[2], b[2], "dq_weight, second call"); _eqw(a[3], b[3], "dk_weight, second call")
    _eq(s[0], a[0][sub], "dq, rows 10 .. 40 alone"); _eq(s[1], a[1][sub], "dk, rows 10 .. 40 alone")
    _eq(one[0], a[0][:, 2:3], "dq, one head alone")
    assert not torch.equal(guard.bits(s[2]), guard.bits(a[2]))                       # (dw does depend on the rows)


# d -------------------------------------------------------------------------------------------------------------------------
def test_dw_over_many_workgroups_and_grid_stride_trips():
    """T = about twice the rows at which the workspace stops growing, plus 13: a ragged tail, more than one grid-stride trip, the
    grid cap's worth of partial rows.  D 128, NeoX, bf16, fp32 weights (a dropped partial row is not hidden by a 16-bit ulp); dw
    and dx against the fp64 formulas (torch float64 on the device: the numpy arrays would be gigabytes) within dw_bound with that
    plan's L and dx_bound"""
    import flash_attn_mi355._lib as lib
    D, dt = 128, "bf16"
    s = lib.FaQkNormRopeBwdParams()
    s.struct_size = ctypes.sizeof(s)
    s.nheads_q, s.nheads_k, s.head_dim, s.dtype, s.weight_dtype = HQ, HK, D, lib.FA_BF16, lib.FA_FP32
    for name in ("dk_out", "k", "q", "dq_out", "q_weight", "k_weight", "dq_weight", "dk_weight"):
        setattr(s, name, 4096)                             # (the query reads no memory: any aligned non-NULL address)
    sat, prev = None, -1
    for rows in range(1024, 1 << 20, 1024):
        s.total_rows = rows
        n = lib.qk_norm_rope_bwd_workspace_bytes(s)
        assert n >= prev
        if n == prev:
            sat = rows - 1024
            break
        prev = n
    assert sat is not None and prev == B.GRID_CAP * 2 * D * 4
    rows = 2 * sat + 13
    plan = B.plan(rows, HQ, HK, D)
    assert plan["grid"] == B.GRID_CAP and plan["steps"] >= 2 and rows % plan["group_rows"] != 0
    cos, sin, il = _tables("neox-full", D, dt)
    g = torch.Generator(device="cuda").manual_seed(5)
    pos = torch.randint(-2, SEQLEN_RO + 2, (rows,), generator=g, device="cuda")
    mk = lambda h: torch.randn((rows, h, D), generator=g, device="cuda", dtype=torch.float32).to(DT[dt])   # noqa: E731
    dzq, dzk, q, k = mk(HQ), mk(HK), mk(HQ), mk(HK)
    qw, kw = _weights(D, dt, fp32=True)
    dq, dk, dqw, dkw = _bwd(dzq, dzk, q, k, pos, cos, sin, qw, kw, EPS, 0.0, il)
    again = _bwd(dzq, dzk, q, k, pos, cos, sin, qw, kw, EPS, 0.0, il, need_dq=False, need_dk=False)
    torch.cuda.synchronize()
    _eqw(again[2], dqw, "dq_weight, second call"); _eqw(again[3], dkw, "dk_weight, second call")
    for dx, got, dz, x, w, name in ((dq, dqw, dzq, q, qw, "q"), (dk, dkw, dzk, k, kw, "k")):
        ref = B.backward_ref_torch(dz, x, w, pos, cos, sin, il, EPS, 0.0)
        dw_ref, S = ref["dw"].cpu().numpy(), ref["S"].cpu().numpy()
        r = B.worst(got, dw_ref, B.dw_bound(dw_ref, S, plan["L"], D, torch.float32))
        rx = B.dx_worst_torch(dx, ref["dx"], ref["A"], DT[dt])
        print(f"{name}: dw worst error / bound {r:.3e} (L = {plan['L']}), dx {rx:.3f}")
        assert r <= 1.0, f"{name}: dw worst error / bound {r:.3f}"
        assert rx <= 1.0, f"{name}: dx worst error / bound {rx:.3f}"


# e -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ["neox-full", "neox-32", "interleaved-full"])
def test_in_place_gives_the_out_of_place_bits(rot):
    """inplace=True on the head slices of one packed gradient: dq is dq_out, dk is dk_out, rewritten where they lie, equal to the
    out-of-place result bit for bit (a lane loads everything it owns before its first store; the NeoX partner piece comes from the
    partner lane's registers); the v heads of the packed gradient are unchanged"""
    D, dt = 128, "fp16"
    cos, sin, il = _tables(rot, D, dt)
    pos = _positions().cuda()
    gqkv, qkv = rand16((T, HQ + 2 * HK, D), dt, 7), rand16((T, HQ + 2 * HK, D), dt, 8)
    g0 = gqkv.clone()
    gq, gk, xq, xk = gqkv[:, :HQ], gqkv[:, HQ:HQ + HK], qkv[:, :HQ], qkv[:, HQ:HQ + HK]
    for qw, kw in (_weights(D, dt), (None, None)):
        gqkv.copy_(g0)
        want = _bwd(gq, gk, xq, xk, pos, cos, sin, qw, kw, EPS, 0.0, il)
        torch.cuda.synchronize()
        assert torch.equal(_bits(gqkv), _bits(g0))                  # out of place: the gradient is read only
        got = _bwd(gq, gk, xq, xk, pos, cos, sin, qw, kw, EPS, 0.0, il, inplace=True)
        torch.cuda.synchronize()
        assert got[0] is gq and got[1] is gk
        _eq(gqkv[:, :HQ], want[0], "dq in place"); _eq(gqkv[:, HQ:HQ + HK], want[1], "dk in place")
        _eq(gqkv[:, HQ + HK:], g0[:, HQ + HK:], "the v heads (unchanged)")
        assert not torch.equal(_bits(gqkv[:, :HQ + HK]), _bits(g0[:, :HQ + HK]))
        if qw is not None:
            _eqw(got[2], want[2], "dq_weight in place"); _eqw(got[3], want[3], "dk_weight in place")


# f -------------------------------------------------------------------------------------------------------------------------
def test_skipped_outputs_leave_the_others_unchanged():
    """each of need_dq / need_dk / need_dw=False gives None in its place and the bits of the full call elsewhere; without a weight
    gradient the workspace is 0 bytes"""
    import flash_attn_mi355._lib as lib
    D, dt = 64, "bf16"
    cos, sin, il = _tables("interleaved-full", D, dt)
    pos = _positions().cuda()
    dzq, dzk, q, k = _data(D, dt)
    qw, kw = _weights(D, dt, fp32=True)
    args = (dzq, dzk, q, k, pos, cos, sin, qw, kw, EPS, 1.0, il)
    full = _bwd(*args)
    sizes = []
    query = lib.qk_norm_rope_bwd_workspace_bytes
    lib.qk_norm_rope_bwd_workspace_bytes = lambda s: sizes.append(query(s)) or sizes[-1]
    try:
        for kwd, keep in ((dict(need_dq=False), (1, 2, 3)), (dict(need_dk=False), (0, 2, 3)), (dict(need_dw=False), (0, 1)),
                          (dict(need_dq=False, need_dk=False), (2, 3)), (dict(need_dq=False, need_dw=False), (1,))):
            got = _bwd(*args, **kwd)
            torch.cuda.synchronize()
            for i in range(4):
                if i in keep:
                    (_eq if i < 2 else _eqw)(got[i], full[i], f"output {i} with {kwd}")
                else:
                    assert got[i] is None, (i, kwd)
    finally:
        lib.qk_norm_rope_bwd_workspace_bytes = query
    assert sizes == [2 * D * 4 * B.plan(T, HQ, HK, D)["grid"]] * 2 + [0] + [2 * D * 4 * B.plan(T, HQ, HK, D)["grid"]] + [0]


# g -------------------------------------------------------------------------------------------------------------------------
def _call_into(dzq, dzk, q, k, dq, dk, pos, cos, sin, il, qw, kw, dqw, dkw, workspace, rows=None):
    """fa_qk_norm_rope_bwd with caller-owned outputs and workspace (the Python function allocates its own): the C ABI through the
    ctypes mirror, filled the way qk_norm_rope_backward fills it"""
    from flash_attn_mi355 import _lib
    from flash_attn_mi355 import flash_attn_interface as fi
    s = _lib.FaQkNormRopeBwdParams()
    s.struct_size = ctypes.sizeof(_lib.FaQkNormRopeBwdParams)
    for name, t in (("dq_out", dzq), ("dk_out", dzk), ("q", q), ("k", k), ("dq", dq), ("dk", dk), ("positions", pos),
                    ("rotary_cos", cos), ("rotary_sin", sin), ("q_weight", qw), ("k_weight", kw), ("dq_weight", dqw), ("dk_weight", dkw)):
        setattr(s, name, t.data_ptr())
    for name, t in (("dqo", dzq), ("dko", dzk), ("q", q), ("k", k), ("dq", dq), ("dk", dk)):
        setattr(s, name + "_row_stride", t.stride(0))
        setattr(s, name + "_head_stride", t.stride(1))
    s.rotary_dim, s.seqlen_ro, s.rotary_interleaved = 2 * cos.shape[1], cos.shape[0], int(il)
    s.total_rows, s.nheads_q, s.nheads_k, s.head_dim = q.shape[0] if rows is None else rows, q.shape[1], k.shape[1], q.shape[2]
    s.dtype = fi._DTYPES[q.dtype]
    s.weight_dtype = _lib.FA_FP32 if qw.dtype == torch.float32 else s.dtype
    s.eps = EPS
    n = _lib.qk_norm_rope_bwd_workspace_bytes(s)
    ws = workspace(n, q.device)
    if n:
        s.workspace, s.workspace_bytes = ws.data_ptr(), n
    _lib.call_qk_norm_rope_bwd(s, fi._stream(q.device))
    return n


@pytest.mark.parametrize("case", ["neox-fp32w", "interleaved-32-16bitw"])
def test_guard_bands(case):
    """dq_out, dk_out, q, k, dq and dk are views with gaps inside NaN-filled slabs, both weights, both weight gradients and the
    positions sit exactly sized inside guarded buffers, and the workspace has exactly the queried size between sentinel bands (its
    interior pre-filled with 0xFF: a partial row that is read before it is written would show): nothing outside a tensor's logical
    elements is written, a read past an input would carry NaN into the results, the inputs are bit-unchanged"""
    dt, D = "bf16", 128
    fp32 = "fp32w" in case
    cos, sin, il = _tables("neox-full" if case.startswith("neox") else "interleaved-32", D, dt)
    pos = _positions().cuda()
    dzq_d, dzk_d, q_d, k_d = _data(D, dt)
    w_q, w_k = _weights(D, dt, fp32)
    want = _bwd(dzq_d, dzk_d, q_d, k_d, pos, cos, sin, w_q, w_k, EPS, 0.0, il)
    ins = [guard.guarded(t) for t in (dzq_d, dzk_d, q_d, k_d)]
    dqb, dq, dqs = guard.guarded(shape=(T, HQ, D), dtype=DT[dt], device="cuda")
    dkb, dk, dks = guard.guarded(shape=(T, HK, D), dtype=DT[dt], device="cuda")
    (pb, pv), (qwb, qw), (kwb, kw) = F._guarded_1d(pos), F._guarded_1d(w_q), F._guarded_1d(w_k)
    (dqwb, dqw), (dkwb, dkw) = F._guarded_1d(torch.zeros_like(w_q)), F._guarded_1d(torch.zeros_like(w_k))
    side0 = [b.clone() for b in (pb, qwb, kwb)]
    workspace, check_ws = guard.guarded_workspace("ones")
    n = _call_into(ins[0][1], ins[1][1], ins[2][1], ins[3][1], dq, dk, pv, cos, sin, il, qw, kw, dqw, dkw, workspace)
    torch.cuda.synchronize()
    assert n == B.plan(T, HQ, HK, D)["workspace_bytes"] and check_ws()["sizes"] == [n]
    _eq(dq, want[0], "dq"); _eq(dk, want[1], "dk")
    _eqw(dqw.clone(), want[2], "dq_weight"); _eqw(dkw.clone(), want[3], "dk_weight")
    for (buf, view, snap), name in zip(ins, ("dq_out", "dk_out", "q", "k")):
        assert torch.equal(guard.bits(buf), snap), f"{name} was written"
    guard.assert_untouched(dqb, dq, dqs, "dq"); guard.assert_untouched(dkb, dk, dks, "dk")
    for b, b0 in zip((pb, qwb, kwb), side0):
        assert torch.equal(b, b0)
    for b, name in ((dqwb, "dq_weight"), (dkwb, "dk_weight")):
        assert bool((b[:4096] == -1).all()) and bool((b[4096 + D:] == -1).all()), f"{name}: written outside its {D} elements"


def test_empty_problems_write_zeros_into_a_wanted_dw():
    """total_rows == 0 through the C ABI: FA_OK, no workspace, dq / dk untouched, dq_weight / dk_weight set to zeros on the
    stream; the Python function with zero rows returns empty dq / dk and zero weight gradients"""
    dt, D = "bf16", 64
    cos, sin, il = _tables("neox-full", D, dt)
    pos = _positions().cuda()
    dzq, dzk, q, k = _data(D, dt)
    qw, kw = _weights(D, dt, fp32=True)
    dq, dk = guard.fill_nan(torch.empty_like(q)), guard.fill_nan(torch.empty_like(k))
    dqw, dkw = guard.fill_nan(torch.empty_like(qw)), guard.fill_nan(torch.empty_like(kw))
    nan_q, nan_k = dq.clone(), dk.clone()
    n = _call_into(dzq, dzk, q, k, dq, dk, pos, cos, sin, il, qw, kw, dqw, dkw, lambda n, dev: None, rows=0)
    torch.cuda.synchronize()
    assert n == 0
    assert not dqw.any() and not dkw.any()
    _eq(dq, nan_q, "dq (no rows: untouched)"); _eq(dk, nan_k, "dk (no rows: untouched)")
    got = _bwd(dzq[:0], dzk[:0], q[:0], k[:0], pos[:0], cos, sin, qw, kw, EPS, 0.0, il)
    torch.cuda.synchronize()
    assert got[0].shape == (0, HQ, D) and got[1].shape == (0, HK, D)
    assert got[2].dtype == torch.float32 and not got[2].any() and not got[3].any()


# h -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ["neox-full", "interleaved-32"])
def test_autograd_through_qk_norm_rope(rot):
    """qk_norm_rope's forward == qk_norm_rope_and_store_kv(inplace=False) and torch.autograd.grad through it == a direct
    qk_norm_rope_backward, bit for bit; needs_input_grad maps to skipped outputs; q=None works; one step qk_norm_rope ->
    flash_attn_func -> sum().backward() leaves finite gradients on q, k and both weights"""
    import flash_attn as fa
    from flash_attn_mi355.qk_norm import qk_norm_rope, qk_norm_rope_and_store_kv
    D, dt = 128, "bf16"
    cos, sin, il = _tables(rot, D, dt)
    pos = _positions().cuda()
    dzq, dzk, q, k = _data(D, dt)
    qw, kw = _weights(D, dt, fp32=True)
    q.requires_grad_(True); k.requires_grad_(True); qw.requires_grad_(True); kw.requires_grad_(True)
    q_out, k_out = qk_norm_rope(q, k, pos, cos, sin, qw, kw, EPS, 0.0, il)
    fq, fk = qk_norm_rope_and_store_kv(q.detach(), k.detach(), None, pos, cos, sin, q_weight=qw.detach(), k_weight=kw.detach(),
                                       eps=EPS, interleaved=il, inplace=False)
    _eq(q_out.detach(), fq, "q_out"); _eq(k_out.detach(), fk, "k_out")
    grads = torch.autograd.grad([q_out, k_out], [q, k, qw, kw], [dzq, dzk], retain_graph=True)
    want = _bwd(dzq, dzk, q.detach(), k.detach(), pos, cos, sin, qw.detach(), kw.detach(), EPS, 0.0, il)
    torch.cuda.synchronize()
    _eq(grads[0], want[0], "dq through autograd"); _eq(grads[1], want[1], "dk through autograd")
    _eqw(grads[2], want[2], "dq_weight through autograd"); _eqw(grads[3], want[3], "dk_weight through autograd")
    gk, gkw = torch.autograd.grad([q_out, k_out], [k, kw], [dzq, dzk])       # q and q_weight need no gradient
    _eq(gk, want[1], "dk alone"); _eqw(gkw, want[3], "dk_weight alone")
    k2 = k.detach().clone().requires_grad_(True)
    none, k_only = qk_norm_rope(None, k2, pos, cos, sin, None, kw, EPS, 0.0, il)
    assert none is None
    _eq(k_only.detach(), fk, "k_out (q=None)")
    gk2, = torch.autograd.grad(k_only, k2, dzk)
    _eq(gk2, want[1], "dk (q=None)")
    # one training step
    v = rand16((T, HK, D), dt, 3).requires_grad_(True)
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, qw, kw)]
    qo, ko = qk_norm_rope(leaves[0], leaves[1], pos, cos, sin, leaves[2], leaves[3], EPS, 0.0, il)
    out = fa.flash_attn_func(qo.unsqueeze(0), ko.unsqueeze(0), v.unsqueeze(0), causal=True)
    out.float().sum().backward()
    torch.cuda.synchronize()
    for t, name in zip(leaves + [v], ("q", "k", "q_weight", "k_weight", "v")):
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype, name
        assert bool(torch.isfinite(t.grad.float()).all()) and float(t.grad.float().abs().max()) > 0, name


# i -------------------------------------------------------------------------------------------------------------------------
def test_backward_replays_in_a_graph():
    """the backward with weight gradients (both launches, the workspace allocated during capture) captured in a graph on one
    stream; replayed after the gradients, the inputs and the positions were overwritten in place: all four outputs equal the
    eager results bit for bit"""
    D, dt = 128, "bf16"
    cos, sin, il = _tables("neox-32", D, dt)
    qw, kw = _weights(D, dt)
    sets = []
    for i in range(3):
        pos = torch.roll(_positions(), i * 5).cuda()
        sets.append(_data(D, dt, seed=10 * i) + (pos,))
    ref = [_bwd(*s[:4], s[4], cos, sin, qw, kw, EPS, 0.0, il) for s in sets]
    torch.cuda.synchronize()
    st = [t.clone() for t in sets[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _bwd(*st[:4], st[4], cos, sin, qw, kw, EPS, 0.0, il)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _bwd(*st[:4], st[4], cos, sin, qw, kw, EPS, 0.0, il)
    for i in (1, 2, 0):
        for dst, src in zip(st, sets[i]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        _eq(out[0], ref[i][0], f"replay {i}: dq"); _eq(out[1], ref[i][1], f"replay {i}: dk")
        _eqw(out[2], ref[i][2], f"replay {i}: dq_weight"); _eqw(out[3], ref[i][3], f"replay {i}: dk_weight")
    assert not torch.equal(_bits(ref[0][0]), _bits(ref[1][0]))
