"""GPU: fa_moe_gemm_wgrad (csrc/fa_moe_gemm_wgrad.hip) and the differentiable expert layer moe_linear against the fp64 reference
and the witness data of moe_gemm_wgrad_ref.py.

Shapes and what they reach:
  segments   moe_gemm_wgrad_ref.PATTERN (0, 1, 15, 16, 17, 63, 64, 65, 129 rows: empty, one row, one under / at / over the MFMA
             step of 16 and the staging step of 64, two steps and a row) behind 5 unowned rows, so every segment starts at an
             unaligned row, and in front of a tail behind expert_offsets[E]; one segment of 2880 rows (45 staging steps: odd)
  N, K       (8, 8), (16, 40), (40, 264) (a third k tile of 8), (264, 264), 2880 once in each position
  E          2, 7 / 9, 512 (mostly empty; N 40, K 48)
  forms      "nk" / "kn", fp16 / bf16, dw of the io dtype and fp32 (with accumulate), plain and gathered x (moe_ref.sort_ref with
             align 1 and 16: padding slots inside the segments), with and without dbias (16-bit and fp32)
dw is always an expert-strided view between guard bands pre-filled with a NaN pattern: an empty expert's +0 and a stray write
both show.  Witness data are compared bit for bit, random data within moe_gemm_wgrad_ref.bound / dbias_bound - the first rests on
an assumption about the MFMA's additions that could not be sourced: every random test prints the share of the bound it measured
(profiles/moe_gemm_wgrad.txt records them)."""
import numpy as np
import pytest
import torch

import guard
import moe_gemm_ref as G
import moe_gemm_wgrad_ref as W
import moe_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DEV = "cuda"
HEAD = 5


def _M():
    from flash_attn_mi355 import moe
    import flash_attn_mi355.torch_ops  # noqa: F401
    return moe


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _same(got, want, name):
    assert got.shape == want.shape and got.dtype == want.dtype, name
    a, b = got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)
    assert torch.equal(a, b), f"{name}: {int((a != b).sum())} bytes differ"


def _dev(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype).to(DEV)


def _exact(got, want64, name):
    """bit for bit against float64 values that are exact in got's dtype (+0 where the reference has 0)"""
    _same(got, torch.from_numpy(np.asarray(want64)).to(got.dtype).to(got.device), name)


def _slab(shape, dtype):
    """(buf, flat view [E, N K], dw view of `shape`): experts contiguous, a gap between experts, NaN-filled guard bands around"""
    E = shape[0]
    buf, flat = guard.slab((E, shape[1] * shape[2]), dtype, gaps=True, device=DEV, check_prep=False)
    assert flat.stride(0) > shape[1] * shape[2] and flat.stride(0) % 8 == 0
    return buf, flat, buf.as_strided(shape, (flat.stride(0), shape[2], 1), flat.storage_offset())


def _shape(E, N, K, layout):
    return (E, N, K) if layout == "nk" else (E, K, N)


def _pattern_offsets(lengths=None, head=HEAD, align=1):
    return (W.offsets_of(W.PATTERN if lengths is None else lengths, align) + head).astype(np.int32)


def _witness_case(M, off, N, K, layout, dtype, out_dtype, seed, *, tail=3, dbias_dtype=None, with_dbias=True):
    E = len(off) - 1
    rows = int(max(off.max(), 0)) + tail
    dy, x = W.witness(rows, N, K, seed)
    assert W.witness_is_exact(dy, x, off, _name(out_dtype))
    buf, flat, view = _slab(_shape(E, N, K, layout), out_dtype)
    snap = guard.snapshot(buf)
    res = M.moe_gemm_wgrad(_dev(dy, dtype), _dev(x, dtype), torch.from_numpy(off).to(DEV), w_layout=layout, out=view,
                           need_dbias=with_dbias, dbias_dtype=dbias_dtype)
    torch.cuda.synchronize()
    dw, db = res if with_dbias else (res, None)
    assert dw is view
    guard.assert_untouched(buf, flat, snap, "dw")
    want, want_b = W.expected(dy, x, off, _name(out_dtype), layout=layout, dbias_name=_name(dbias_dtype or dtype))
    tag = f"witness E {E} N {N} K {K} {layout} {_name(dtype)} -> {_name(out_dtype)}"
    _exact(view, want, tag)
    if with_dbias:
        assert db.dtype == (dbias_dtype or dtype) and db.shape == (E, N)
        _exact(db, want_b, tag + " dbias")
    return view


NK_PAIRS = [(8, 8), (16, 40), (40, 264), (264, 264)]


@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("N,K", NK_PAIRS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_witness_every_segment_length(N, K, layout, dtype):
    """PATTERN at unaligned starts with a tail; dw in the io dtype and in fp32; dbias in the io dtype, fp32 or absent"""
    M = _M()
    i = NK_PAIRS.index((N, K))
    off = _pattern_offsets()
    _witness_case(M, off, N, K, layout, dtype, dtype, 100 + i, dbias_dtype=torch.float32 if i % 2 else None)
    _witness_case(M, off, N, K, layout, dtype, torch.float32, 110 + i, with_dbias=i % 2 == 0)


@pytest.mark.parametrize("layout", ["nk", "kn"])
def test_witness_2880_in_each_position(layout):
    """a segment of 2880 rows (45 staging steps; fp16 sums pass 2048: the one rounding), N = 2880 and K = 2880 over the pattern"""
    M = _M()
    off = np.array([3, 3, 2883, 2890], dtype=np.int32)
    _witness_case(M, off, 40, 48, layout, torch.float16, torch.float16, 201)
    _witness_case(M, off, 40, 48, layout, torch.bfloat16, torch.float32, 202, dbias_dtype=torch.float32)
    _witness_case(M, _pattern_offsets([17, 0, 65]), 2880, 40, layout, torch.bfloat16, torch.bfloat16, 203)
    _witness_case(M, _pattern_offsets([17, 0, 65]), 40, 2880, layout, torch.float16, torch.float16, 204)


@pytest.mark.parametrize("layout", ["nk", "kn"])
def test_witness_2_and_512_experts(layout):
    M = _M()
    _witness_case(M, _pattern_offsets([3, 40]), 40, 48, layout, torch.bfloat16, torch.bfloat16, 301)
    few = [0] * 512
    for e, n in ((0, 3), (5, 1), (63, 40), (64, 2), (300, 33), (511, 70)):
        few[e] = n
    view = _witness_case(M, _pattern_offsets(few), 40, 48, layout, torch.float16, torch.float16, 302, dbias_dtype=torch.float32)
    assert (view[1].view(torch.int16) == 0).all() and (view[510].view(torch.int16) == 0).all()     # +0, not -0, not NaN


def _sorted(T, topk, E, align, seed):
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(E)[:topk] for _ in range(T)]).astype(np.int32)
    if T > 2:
        ids[1, 0] = -1
        ids[T - 1, topk - 1] = E                              # (dropped slots: an expert-parallel expert_map)
    return R.sort_ref(ids, E, align=align)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("T,topk,E,align", [(67, 6, 7, 16), (67, 2, 7, 1), (300, 2, 8, 16)])
def test_gather_equals_permute_then_plain(T, topk, E, align, layout, dtype):
    """witness data through the sort's tables (padding slots, dropped ids): gather form == permute + plain form == exact, and
    two runs give the same bits"""
    M = _M()
    N, K = 136, 264
    ss, pos, off = _sorted(T, topk, E, align, 400 + T)
    assert align == 1 or (ss[:off[-1]] < 0).any()
    dy, x = W.witness(len(ss), N, K, 410 + T)
    x = x[:T]
    dyt, xt = _dev(dy, dtype), _dev(x, dtype)
    sst, offt = torch.from_numpy(ss).to(DEV), torch.from_numpy(off).to(DEV)
    out_dtype = torch.float32 if align == 1 else dtype
    fused, fb = M.moe_gemm_wgrad(dyt, xt, offt, w_layout=layout, sorted_slot=sst, top_k=topk, dw_dtype=out_dtype, need_dbias=True)
    again, ab = M.moe_gemm_wgrad(dyt, xt, offt, w_layout=layout, sorted_slot=sst, top_k=topk, dw_dtype=out_dtype, need_dbias=True)
    xp = M.moe_permute_forward(xt, sst, topk)
    plain, pb = M.moe_gemm_wgrad(dyt, xp, offt, w_layout=layout, dw_dtype=out_dtype, need_dbias=True)
    _same(fused, plain, "gather against permute + plain")
    _same(fused, again, "two runs")
    _same(fb, pb, "dbias")
    _same(fb, ab, "dbias, two runs")
    want, want_b = W.expected(dy, W.gather_ref(x, ss, topk), off, _name(out_dtype), layout=layout, dbias_name=_name(dtype))
    _exact(fused, want, "gather against the reference")
    _exact(fb, want_b, "dbias against the reference")


@pytest.mark.parametrize("layout", ["nk", "kn"])
def test_accumulate_twice_is_twice_the_gradient(layout):
    """fp32 dw += on integer data: exact; an empty expert's slab keeps its bits (a -0 and a NaN pattern included)"""
    M = _M()
    dtype, N, K = torch.bfloat16, 40, 264
    off = _pattern_offsets()
    E = len(off) - 1
    dy, x = W.witness(int(off[-1]) + 3, N, K, 500)
    buf, flat, view = _slab(_shape(E, N, K, layout), torch.float32)
    old = np.random.default_rng(3).integers(-50, 50, size=view.shape).astype(np.float64)
    view.copy_(torch.from_numpy(old).float())
    view[0].fill_(-0.0)
    guard.fill_nan(view[0, :2])                                  # expert 0 is empty: nothing of it may be read or written
    before0 = view[0].clone()
    snap = guard.snapshot(buf)
    dyt, xt, offt = _dev(dy, dtype), _dev(x, dtype), torch.from_numpy(off).to(DEV)
    for _ in range(2):
        M.moe_gemm_wgrad(dyt, xt, offt, w_layout=layout, out=view, accumulate=True)
    torch.cuda.synchronize()
    guard.assert_untouched(buf, flat, snap, "dw (accumulate)")
    once, _ = W.wgrad_ref(dy, x, off, layout=layout)
    assert W.witness_is_exact(dy, x, off, "float32", old=np.abs(old) + np.abs(once))
    _exact(view[1:], (old + 2 * once)[1:], "accumulate twice")
    _same(view[0], before0, "the empty expert's slab under accumulate")
    with pytest.raises(RuntimeError, match="accumulate"):
        M.moe_gemm_wgrad(dyt, xt, offt, w_layout=layout, accumulate=True, out=torch.zeros(_shape(E, N, K, layout), dtype=dtype, device=DEV))


@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("gather", [False, True])
def test_an_expert_sees_its_own_rows_alone(layout, gather):
    """random data.  (a) every row outside one expert's segment - the other segments, the unowned head, the tail behind
    offsets[E] - rewritten to NaN / inf: that expert's dW and dbias keep their bits.  (b) the segment moved to another place of a
    larger buffer among other experts: the same bits."""
    M = _M()
    dtype, N, K = torch.bfloat16, 136, 264
    off = _pattern_offsets()
    E = len(off) - 1
    rows = int(off[-1]) + 7
    g = torch.Generator().manual_seed(61)
    dy = torch.randn(rows, N, generator=g).to(dtype).to(DEV)
    xp = torch.randn(rows, K, generator=g).to(dtype).to(DEV)
    offt = torch.from_numpy(off).to(DEV)
    if gather:                                                   # a permutation as sorted_slot (top_k 1): x is xp un-permuted
        perm = torch.randperm(rows, generator=g).to(torch.int32).to(DEV)
        x = torch.empty_like(xp)
        x[perm.long()] = xp
        kw = dict(sorted_slot=perm, top_k=1)
    else:
        x, kw = xp, {}
    base, base_b = M.moe_gemm_wgrad(dy, x, offt, w_layout=layout, need_dbias=True, **kw)
    for e in (3, 8):                                             # 16 rows; 129 rows
        lo, hi = int(off[e]), int(off[e + 1])
        dy2, xp2 = dy.clone(), xp.clone()
        for t, bad in ((dy2, float("nan")), (xp2, float("inf"))):
            t[:lo] = bad
            t[hi:] = bad
        if gather:
            x2 = torch.empty_like(xp2)
            x2[perm.long()] = xp2
        else:
            x2 = xp2
        got, got_b = M.moe_gemm_wgrad(dy2, x2, offt, w_layout=layout, need_dbias=True, **kw)
        _same(got[e], base[e], f"expert {e} among NaN rows")
        _same(got_b[e], base_b[e], f"expert {e} dbias among NaN rows")
        assert torch.isnan(got[e - 1].float()).all() or hi - lo == 0
    if not gather:
        e, lo, hi = 8, int(off[8]), int(off[9])
        big_dy = torch.randn(700, N, generator=g).to(dtype).to(DEV)
        big_x = torch.randn(700, K, generator=g).to(dtype).to(DEV)
        at = 333
        big_dy[at:at + hi - lo] = dy[lo:hi]
        big_x[at:at + hi - lo] = xp[lo:hi]
        off2 = torch.tensor([0, 100, at, at + hi - lo, 650], dtype=torch.int32, device=DEV)
        moved, moved_b = M.moe_gemm_wgrad(big_dy, big_x, off2, w_layout=layout, need_dbias=True)
        _same(moved[2], base[e], "a segment moved to another place, another E")
        _same(moved_b[2], base_b[e], "its dbias")


def test_malformed_offsets_and_no_rows():
    """negative, decreasing and out-of-range offsets: wrong segments, but every write stays inside dw and nothing faults (the
    offsets are clamped and only compared); rows == 0 writes +0"""
    M = _M()
    dtype, N, K, E = torch.bfloat16, 40, 48, 7
    dy, x = W.witness(64, N, K, 900)
    bad = np.array([0, 40, 20, -5, 2 ** 31 - 1, 30, 64, 10 ** 6], dtype=np.int32)
    for layout in ("nk", "kn"):
        buf, flat, view = _slab(_shape(E, N, K, layout), dtype)
        snap = guard.snapshot(buf)
        _, db = M.moe_gemm_wgrad(_dev(dy, dtype), _dev(x, dtype), torch.from_numpy(bad).to(DEV), w_layout=layout, out=view, need_dbias=True)
        torch.cuda.synchronize()
        guard.assert_untouched(buf, flat, snap, "dw under malformed offsets")
        want, want_b = W.expected(dy, x, bad, _name(dtype), layout=layout)     # (the reference clamps as the kernel does)
        _exact(view, want, "malformed offsets")
        _exact(db, want_b, "malformed offsets, dbias")
    buf, flat, view = _slab((E, N, K), dtype)
    snap = guard.snapshot(buf)
    dw, db = M.moe_gemm_wgrad(_dev(dy[:0], dtype), _dev(x[:0], dtype), torch.zeros(E + 1, dtype=torch.int32, device=DEV), out=view,
                              need_dbias=True)
    torch.cuda.synchronize()
    guard.assert_untouched(buf, flat, snap, "dw without rows")
    assert (view.view(torch.int16) == 0).all() and (db.view(torch.int16) == 0).all()


def test_replays_in_a_graph_after_the_tables_and_dy_were_rewritten():
    M = _M()
    ns = torch.ops.flash_attn_mi355
    dtype, T, topk, E, N, K, align = torch.bfloat16, 67, 2, 8, 136, 264, 16
    tables = [_sorted(T, topk, E, align, 700 + i) for i in range(3)]
    assert not (tables[0][2] == tables[1][2]).all()
    rows = len(tables[0][0])
    dys = [_dev(W.witness(rows, N, K, 710 + i)[0], dtype) for i in range(3)]
    xt = _dev(W.witness(T, N, K, 720)[1], dtype)
    dev_tables = [(torch.from_numpy(t[0]).to(DEV), torch.from_numpy(t[2]).to(DEV)) for t in tables]
    ref = [[r.clone() for r in ns.moe_gemm_wgrad(dys[i], xt, dev_tables[i][1], "nk", dev_tables[i][0], topk, True, True, False, True)]
           for i in range(3)]
    ss, off, dy = dev_tables[0][0].clone(), dev_tables[0][1].clone(), dys[0].clone()
    ns.moe_gemm_wgrad(dy, xt, off, "nk", ss, topk, True, True, False, True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dw, db = ns.moe_gemm_wgrad(dy, xt, off, "nk", ss, topk, True, True, False, True)
    for i in (1, 2, 0):
        ss.copy_(dev_tables[i][0])
        off.copy_(dev_tables[i][1])
        dy.copy_(dys[i])
        graph.replay()
        torch.cuda.synchronize()
        _same(dw, ref[i][0], f"replay {i}")
        _same(db, ref[i][1], f"replay {i} dbias")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("layout", ["nk", "kn"])
def test_random_data_within_the_bounds(layout, dtype):
    """N(0, 1) inputs: |dw - ref| <= 0.5 ulp_out + (L + 2) 2^-23 sum |dy a|, |dbias - ref| <= 0.5 ulp_out + L 2^-24 sum |dy|.  The
    first's fp32 term rests on an assumption about the MFMA's additions that could not be sourced; "used" is its share alone."""
    M = _M()
    nm = _name(dtype)
    for lengths, N, K, out_dtype in ((W.PATTERN, 264, 136, dtype), ([2880, 0, 5], 136, 40, dtype), (W.PATTERN, 136, 264, torch.float32)):
        off = _pattern_offsets(lengths)
        rows = int(off[-1]) + 3
        g = torch.Generator().manual_seed(500 + K + rows)
        dy = torch.randn(rows, N, generator=g).to(dtype)
        x = torch.randn(rows, K, generator=g).to(dtype)
        dw, db = M.moe_gemm_wgrad(dy.to(DEV), x.to(DEV), torch.from_numpy(off).to(DEV), w_layout=layout, dw_dtype=out_dtype,
                                  need_dbias=True, dbias_dtype=out_dtype)
        ref, refb, mag, magb = W.wgrad_ref(R.widen(dy), R.widen(x), off, layout=layout, with_mag=True)
        L = W.seg_lengths(off, rows)
        on = _name(out_dtype)
        bnd, e32 = W.bound(ref, mag, L, on)
        err = np.abs(R.widen(dw) - ref)
        share = float((err / np.where(bnd > 0, bnd, 1)).max())
        used = np.maximum(err - R.half_ulp(np.abs(ref) + e32, on), 0) / np.where(e32 > 0, e32, 1)
        bb, _ = W.dbias_bound(refb, magb, L, on)
        errb = np.abs(R.widen(db) - refb)
        share_b = float((errb / np.where(bb > 0, bb, 1)).max())
        print(f"share moe_gemm_wgrad {layout} {nm} -> {on} L<={int(L.max())} N {N} K {K}: dw {share:.3f} used {float(used.max()):.3f}  "
              f"dbias {share_b:.3f}")
        assert (err <= bnd).all(), f"dw: {share:.3f} of the bound"
        assert (errb <= bb).all(), f"dbias: {share_b:.3f} of the bound"


# moe_linear -------------------------------------------------------------------------------------------------------------------
def _linear_case(M, layout, dtype, gather, N, K, seed, with_bias=True, bias_dtype=None):
    """witness tensors of an expert layer: (x, w, bias, tables, kwargs, the rows the GEMM sees f64, numpy originals)"""
    T, topk, E, align = 37, 2, 7, 16
    ss, pos, off = _sorted(T, topk, E, align, seed)
    rows = len(ss)
    a, w, bias = G.witness(T if gather else rows, K, N, E, layout, seed + 1, with_bias)
    g = W.witness(rows, N, 8, seed + 2)[0]                       # the incoming gradient: integers
    xt, wt = _dev(a, dtype), _dev(w, dtype)
    bt = None if bias is None else _dev(bias, bias_dtype or dtype)
    offt = torch.from_numpy(off).to(DEV)
    kw = dict(sorted_slot=torch.from_numpy(ss).to(DEV), top_k=topk, pos=torch.from_numpy(pos).to(DEV)) if gather else {}
    return xt, wt, bt, offt, kw, (a, w, bias, g, ss, off, topk)


def _dense_f64(a, w, bias, g, ss, off, topk, layout, gather):
    """y and the gradients of sum(y * g) by fp64 autograd of the dense definition"""
    x64 = torch.from_numpy(a).requires_grad_()
    w64 = torch.from_numpy(w).requires_grad_()
    b64 = None if bias is None else torch.from_numpy(bias).requires_grad_()
    if gather:
        idx = torch.from_numpy(np.where(ss >= 0, ss // topk, 0)).long()
        rows = x64[idx] * torch.from_numpy((ss >= 0).astype(np.float64))[:, None]
    else:
        rows = x64
    y = torch.zeros(len(ss), w.shape[1] if layout == "nk" else w.shape[2], dtype=torch.float64)
    parts = []
    for e in range(len(off) - 1):
        We = w64[e].t() if layout == "nk" else w64[e]
        p = rows[off[e]:off[e + 1]] @ We
        parts.append(p if b64 is None else p + b64[e])
    y = torch.cat(parts + [y[off[-1]:]])
    grads = torch.autograd.grad(y, [x64, w64] + ([] if b64 is None else [b64]), grad_outputs=torch.from_numpy(g))
    return y.detach(), grads


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("gather", [False, True], ids=["plain", "gather"])
def test_moe_linear_forward_bits_and_exact_gradients(layout, dtype, gather):
    """witness data: the forward has moe_gemm's bits; torch.autograd.grad equals the fp64 autograd of the dense definition bit for
    bit (integer gradients; in the gather form dx adds two 16-bit rows, so N is small enough for that sum to stay exact: 9 N top_k
    <= 256 in bf16, <= 2048 in fp16); and equals the three explicit calls"""
    M = _M()
    N, K = ((8, 264) if dtype == torch.bfloat16 else (40, 264)) if gather else (136, 264)
    xt, wt, bt, offt, kw, np_case = _linear_case(M, layout, dtype, gather, N, K, 800, bias_dtype=torch.float32 if gather else None)
    a, w, bias, g, ss, off, topk = np_case
    fkw = {k: v for k, v in kw.items() if k != "pos"}
    plain = M.moe_gemm(xt, wt, offt, w_layout=layout, bias=bt, **fkw)
    xr, wr, br = xt.clone().requires_grad_(), wt.clone().requires_grad_(), bt.clone().requires_grad_()
    y = M.moe_linear(xr, wr, offt, w_layout=layout, bias=br, **kw)
    _same(y.detach(), plain, "moe_linear forward against moe_gemm")
    gt = _dev(g, dtype)
    dx, dw, db = torch.autograd.grad(y, (xr, wr, br), grad_outputs=gt)
    y64, (dx64, dw64, db64) = _dense_f64(a, w, bias, g, ss, off, topk, layout, gather)
    end = int(off[-1])
    _exact(y.detach()[:end], G.round16(y64.numpy(), _name(dtype))[:end], "forward against fp64")
    _exact(dx, G.round16(dx64.numpy(), _name(dtype)), "dx against fp64 autograd")
    _exact(dw, G.round16(dw64.numpy(), _name(dtype)), "dw against fp64 autograd")
    assert db.dtype == bt.dtype
    _exact(db, W.round_out(db64.numpy(), _name(bt.dtype)), "dbias against fp64 autograd")
    if gather:
        assert np.abs(dx64.numpy()).max() <= (256 if dtype == torch.bfloat16 else 2048)
    # the three explicit calls
    other = "kn" if layout == "nk" else "nk"
    ex = M.moe_gemm(gt, wt, offt, w_layout=other)
    if gather:
        ex = M.moe_combine_forward(ex, None, kw["pos"])
    _same(dx, ex, "dx against moe_gemm (+ moe_combine)")
    ew, eb = M.moe_gemm_wgrad(gt, xt, offt, w_layout=layout, need_dbias=True, dbias_dtype=bt.dtype, **fkw)
    _same(dw, ew, "dw against moe_gemm_wgrad")
    _same(db, eb, "dbias against moe_gemm_wgrad")
    if gather:                                                   # without pos the backward inverts sorted_slot itself
        y2 = M.moe_linear(xr, wr, offt, w_layout=layout, bias=br, **fkw)
        _same(torch.autograd.grad(y2, xr, grad_outputs=gt)[0], dx, "dx without pos")


def test_moe_linear_computes_only_what_is_asked(monkeypatch):
    """needs_input_grad subsets: the gradients not asked for are None and their launches do not happen (the calls are counted)"""
    M = _M()
    dtype, layout = torch.bfloat16, "nk"
    xt, wt, bt, offt, kw, np_case = _linear_case(M, layout, dtype, True, 40, 264, 850)
    gt = _dev(np_case[3], dtype)
    calls = []
    real_w, real_g, real_c = M.moe_gemm_wgrad, M.moe_gemm, M.moe_combine_forward
    monkeypatch.setattr(M, "moe_gemm_wgrad", lambda *a, **k: (calls.append(("wgrad", k["need_dw"], k["need_dbias"])), real_w(*a, **k))[1])
    monkeypatch.setattr(M, "moe_gemm", lambda *a, **k: (calls.append(("gemm",)), real_g(*a, **k))[1])
    monkeypatch.setattr(M, "moe_combine_forward", lambda *a, **k: (calls.append(("combine",)), real_c(*a, **k))[1])
    full = None
    for need in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 1)):
        ins = [t.clone().requires_grad_(bool(n)) for t, n in zip((xt, wt, bt), need)]
        y = M.moe_linear(ins[0], ins[1], offt, w_layout=layout, bias=ins[2], **kw)
        del calls[:]
        grads = torch.autograd.grad(y, [t for t in ins if t.requires_grad], grad_outputs=gt)
        want_calls = ([("gemm",), ("combine",)] if need[0] else []) + ([("wgrad", bool(need[1]), bool(need[2]))] if need[1] or need[2] else [])
        assert calls == want_calls, (need, calls)
        got = iter(grads)
        got = [next(got) if n else None for n in need]
        if full is None:
            full = got
        for a, b, n in zip(got, full, need):
            if n:
                _same(a, b, f"subset {need}")
    y = M.moe_linear(xt.clone().requires_grad_(), wt, offt, w_layout=layout, bias=bt, **kw)
    y.sum().backward()                                           # w and bias do not require grad: their .grad stays None
    assert wt.grad is None and bt.grad is None


def test_opcheck():
    M = _M()
    ns = torch.ops.flash_attn_mi355
    dtype = torch.bfloat16
    xt, wt, bt, offt, kw, np_case = _linear_case(M, "nk", dtype, True, 24, 16, 950, bias_dtype=torch.float32)
    ss, topk, pos = kw["sorted_slot"], kw["top_k"], kw["pos"]
    gt = _dev(np_case[3], dtype)
    xp = M.moe_permute_forward(xt, ss, topk)
    torch.library.opcheck(ns.moe_gemm_wgrad, (gt, xt, offt, "nk", ss, topk, True, True, False, True))
    torch.library.opcheck(ns.moe_gemm_wgrad, (gt, xp, offt, "kn", None, None, True, False, True, False))
    torch.library.opcheck(ns.moe_gemm_wgrad, (gt, xp, offt, "nk", None, None, False, True, False, False))
    req = lambda t, r=True: t.clone().requires_grad_(r)          # noqa: E731
    torch.library.opcheck(ns.moe_linear, (req(xt), req(wt), offt, "nk", req(bt), ss, topk, pos))
    torch.library.opcheck(ns.moe_linear, (req(xt), req(wt, False), offt, "nk", None, ss, topk, None))
    torch.library.opcheck(ns.moe_linear, (req(xp, False), req(wt.transpose(1, 2).contiguous()), offt, "kn", req(bt), None, None, None))
    torch.library.opcheck(ns.moe_linear, (req(xp), req(wt), offt, "nk", None, None, None, None))


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / np.linalg.norm(ref))


def test_a_whole_block_through_autograd():
    """T 67, E 7, K 2, hidden 264, intermediate 136, random bf16: moe_route -> moe_sort -> moe_linear (gather, gate-up) ->
    act_and_mul -> moe_linear (down) -> moe_combine.  The gradients of x, both weights and the logits against float64 autograd
    of the dense definition; the tolerance comes from a torch-eager bf16 restatement of the block (the per-segment torch.mm
    loop, fp32 where the kernels compute in fp32, rounded to bf16 where they round) against the same reference: each tensor's
    relative Frobenius error is at most 2 x the eager one's - both round to 16 bits at the same places and differ only in
    accumulation order."""
    from flash_attn_mi355 import act_mul
    M = _M()
    T, E, K, H, I, align = 67, 7, 2, 264, 136, 16
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(62)
    logits0 = (torch.randn(T, E, generator=g) * 2).to(dt).to(DEV)
    x0 = torch.randn(T, H, generator=g).to(dt).to(DEV)
    W10 = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(dt).to(DEV)     # "nk": [E, 2 I, H], gate rows first
    W20 = (torch.randn(E, I, H, generator=g) / I ** 0.5).to(dt).to(DEV)         # "kn": [E, I, H]
    gout = torch.randn(T, H, generator=g).to(dt).to(DEV)
    leaves = lambda: [t.clone().requires_grad_() for t in (x0, W10, W20, logits0)]     # noqa: E731

    x, W1, W2, logits = leaves()
    w, ids = M.moe_route(logits, K)
    ss, pos, off = M.moe_sort(ids, E, align=align)
    h = M.moe_linear(x, W1, off, sorted_slot=ss, top_k=K, pos=pos)
    a = act_mul.act_and_mul(h)
    y = M.moe_linear(a, W2, off, w_layout="kn")
    out = M.moe_combine(y, w, pos)
    ours = torch.autograd.grad(out, (x, W1, W2, logits), grad_outputs=gout)

    offs, posl, ssl = off.cpu().tolist(), pos.long(), ss.long()
    live = (ssl >= 0)

    def block(x, W1, W2, logits, f):
        """the dense definition over the kernel's tables; f(t): the rounding a 16-bit stage applies (identity in fp64)"""
        wsel = torch.softmax(logits.float().gather(1, ids.long()) if f is not None else logits.gather(1, ids.long()), dim=1)
        xp = x[torch.where(live, ssl // K, 0)] * live[:, None].to(x.dtype)
        mm = lambda rows, Wt: torch.cat([rows[offs[e]:offs[e + 1]] @ Wt(e) for e in range(E)] + [rows[offs[E]:, :1] * 0 * Wt(0)[:1]])  # noqa: E731
        h = mm(xp, lambda e: W1[e].t())
        if f is not None:
            hf = h.float()
            a = f(torch.nn.functional.silu(hf[:, :I]) * hf[:, I:])
        else:
            a = torch.nn.functional.silu(h[:, :I]) * h[:, I:]
        y = mm(a, lambda e: W2[e])
        o = (wsel[:, :, None] * (y.float() if f is not None else y)[posl]).sum(1)
        return f(o) if f is not None else o

    lv = leaves()
    eager = torch.autograd.grad(block(*lv, lambda t: t.to(dt)), lv, grad_outputs=gout)
    lv64 = [t.detach().double().requires_grad_() for t in (x0, W10, W20, logits0)]
    ref = torch.autograd.grad(block(*lv64, None), lv64, grad_outputs=gout.double())
    for name, o, e, r in zip(("dx", "dW1", "dW2", "dlogits"), ours, eager, ref):
        eo, ee = _rel(R.widen(o), R.widen(r)), _rel(R.widen(e), R.widen(r))
        print(f"block grad {name}: relative Frobenius error ours {eo:.3e}  eager bf16 {ee:.3e}  ratio {eo / ee:.2f}")
        assert o.dtype == dt and o.shape == r.shape
        assert eo <= 2 * ee, f"{name}: {eo:.3e} against 2 x {ee:.3e}"
