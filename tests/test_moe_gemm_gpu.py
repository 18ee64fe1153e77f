"""GPU: fa_moe_gemm (csrc/fa_moe_gemm.hip) against the fp64 reference and the witness data of moe_gemm_ref.py.

Tile shapes the plan chooses (fa_moe_gemm_plan: block_m 32 where M_max <= 32 E, else 128) and the shapes below that reach them:
  block_m 128   moe_gemm_ref.PATTERN (226 rows over E = 7: segments of 0, 1, 31, 32, 33, 0, 129 rows - a tile that straddles its
                segment's end at every length, a segment of two tiles), the same with a +0 tail behind expert_offsets[E], the
                align-16 sort of 67 x 6 slots over E = 7, 16400 rows over E = 512
  block_m 32    200 rows all in the last of 7 experts (seven tiles of one segment), 86 rows over E = 512 (mostly empty), E = 2,
                the align-1 sort of 5 x 2 slots, a row alone
  both          K = 8 (half an MFMA step), 16, 24, 48 (an odd count of steps of 16, one staging step), 264 (a tail in the fifth
                staging step), 2880 (45 staging steps: odd); N = 8, 40, 264 (a third column tile of 8), 2880; "nk" / "kn",
                fp16 / bf16, with and without bias (fp32 and 16-bit), plain and fused-gather x
Witness data are compared bit for bit, random data within moe_gemm_ref.bound - whose assumption (each addition inside the MFMA
and along the chain errs by at most one fp32 ulp) could not be sourced: every random test prints the share of the bound it
measured, total ("share") and of the fp32 term alone ("used"), which profiles/moe_gemm.txt records."""
import numpy as np
import pytest
import torch

import guard
import moe_gemm_ref as G
import moe_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DEV = "cuda"


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


def _exact(got, want64, dtype, name):
    """bit for bit against float64 values that are exact in `dtype` (+0 where the reference has 0)"""
    want = torch.from_numpy(want64).to(dtype).to(got.device)
    _same(got, want, name)


def _plan(M, rows, N, K, E, layout, dtype):
    return M.moe_gemm_plan(rows, N, K, E, w_layout=layout, dtype=dtype)[0]


def _witness_case(M, lengths, K, N, layout, dtype, with_bias, seed, tail=0, align=1, block_m=None, bias_dtype=None):
    E = len(lengths)
    off = G.offsets_of(lengths, align)
    rows = int(off[E]) + tail
    x, w, bias = G.witness(rows, K, N, E, layout, seed, with_bias)
    if block_m is not None:
        assert _plan(M, rows, N, K, E, layout, dtype) == block_m
    out_buf, out_view = guard.slab((rows, N), dtype, gaps=True, device=DEV, check_prep=False)
    snap = guard.snapshot(out_buf)
    bt = None if bias is None else _dev(bias, bias_dtype or dtype)
    got = M.moe_gemm(_dev(x, dtype), _dev(w, dtype), torch.from_numpy(off).to(DEV), w_layout=layout, bias=bt, out=out_view)
    torch.cuda.synchronize()
    assert got is out_view
    guard.assert_untouched(out_buf, out_view, snap, "out")
    want = G.expected(x, w, off, _name(dtype), layout=layout, bias=bias)
    _exact(out_view, want, dtype, f"witness {lengths if E <= 8 else E} K {K} N {N} {layout} {_name(dtype)} bias {with_bias}")


KN_PAIRS = [(8, 8), (16, 40), (24, 264), (48, 2880), (264, 2880), (2880, 40), (2880, 264)]


@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("K,N", KN_PAIRS)
def test_witness_every_k_and_n(K, N, layout):
    """the wide plan over moe_gemm_ref.PATTERN, in a strided out between guard bands; dtype and bias alternate over the shapes"""
    i = KN_PAIRS.index((K, N))
    _witness_case(_M(), G.PATTERN, K, N, layout, DTYPES[i % 2], i % 3 != 0, 100 + i, block_m=128,
                  bias_dtype=torch.float32 if i % 2 else None)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_witness_segment_patterns(layout, dtype, with_bias):
    M = _M()
    K, N = 264, 264
    _witness_case(M, G.PATTERN, K, N, layout, dtype, with_bias, 201, tail=37, block_m=128)       # +0 rows behind offsets[E]
    _witness_case(M, [0] * 6 + [200], K, N, layout, dtype, with_bias, 202, block_m=32)           # all rows in the last expert
    _witness_case(M, [5, 0, 9, 16, 1, 0, 3], K, N, layout, dtype, with_bias, 203, align=16, tail=11, block_m=32)
    _witness_case(M, [3, 40], 48, 40, layout, dtype, with_bias, 204, block_m=32)                 # E = 2
    _witness_case(M, [129, 200], 48, 40, layout, dtype, with_bias, 205, block_m=128)


@pytest.mark.parametrize("layout", ["nk", "kn"])
def test_witness_512_experts(layout):
    M = _M()
    few = [0] * 512
    for e, n in ((0, 3), (5, 1), (63, 40), (64, 2), (300, 33), (511, 7)):
        few[e] = n
    _witness_case(M, few, 48, 40, layout, torch.bfloat16, True, 301, block_m=32)
    many = [32] * 512
    many[7], many[8], many[511] = 0, 64, 48
    _witness_case(M, many, 8, 8, layout, torch.float16, False, 302, tail=9, block_m=128)


def _sorted_case(M, T, K, E, align, seed, drop=True):
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(T)]).to(torch.int32)
    if drop and T > 2:
        ids[1, 0] = -1
        ids[T - 1, K - 1] = E                                # (dropped slots: an expert-parallel expert_map)
    return M.moe_sort(ids.to(DEV), E, align=align)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("T,topk,E,align", [(67, 6, 7, 16), (5, 2, 7, 1), (300, 2, 8, 1)])
def test_fused_gather_equals_permute_then_gemm(T, topk, E, align, layout, dtype):
    """witness data through moe_sort's own tables (padding slots, dropped ids): gather form == permute + plain form == exact"""
    M = _M()
    Kd, N = 264, 136
    sorted_slot, pos, offsets = _sorted_case(M, T, topk, E, align, 400 + T)
    x, w, bias = G.witness(T, Kd, N, E, layout, 410 + T, True)
    xt, wt, bt = _dev(x, dtype), _dev(w, dtype), _dev(bias, torch.float32)
    fused = M.moe_gemm(xt, wt, offsets, w_layout=layout, bias=bt, sorted_slot=sorted_slot, top_k=topk)
    xp = M.moe_permute_forward(xt, sorted_slot, topk)
    plain = M.moe_gemm(xp, wt, offsets, w_layout=layout, bias=bt)
    _same(fused, plain, "fused gather against permute + gemm")
    ss, off = sorted_slot.cpu().numpy(), offsets.cpu().numpy()
    assert (ss < 0).any()
    want = G.expected(G.gather_ref(x, ss, topk), w, off, _name(dtype), layout=layout, bias=bias)
    _exact(fused, want, dtype, "fused gather against the reference")
    assert (want[off[E]:] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_random_data_within_the_bound(layout, dtype, with_bias):
    """N(0, 1) inputs, both plans: |got - ref| <= 0.5 ulp16 + (K + 2) 2^-23 sum |a w| (+ 2^-24 |ref|).  The fp32 term rests on an
    assumption about the MFMA's additions that could not be sourced (module docstring); "used" is the share of it alone."""
    M = _M()
    nm = _name(dtype)
    for lengths, K, N in ((G.PATTERN, 2880, 264), ([3, 0, 8, 1, 0, 0, 5], 2880, 264), (G.PATTERN, 264, 2880)):
        E = len(lengths)
        off = G.offsets_of(lengths)
        rows = int(off[E])
        g = torch.Generator().manual_seed(500 + K + rows)
        x = torch.randn(rows, K, generator=g).to(dtype)
        w = (torch.randn((E, N, K) if layout == "nk" else (E, K, N), generator=g) / K ** 0.5).to(dtype)
        bias = torch.randn(E, N, generator=g) if with_bias else None
        got = M.moe_gemm(x.to(DEV), w.to(DEV), torch.from_numpy(off).to(DEV), w_layout=layout,
                         bias=None if bias is None else bias.to(DEV))
        ref, mag = G.gemm_ref(R.widen(x), R.widen(w), off, layout=layout, bias=None if bias is None else R.widen(bias), with_mag=True)
        bnd, e32 = G.bound(ref, mag, K, nm, with_bias)
        err = np.abs(R.widen(got) - ref)
        share = float((err / bnd).max())
        # how much of the fp32 term is needed once the final rounding's half ulp is taken off
        used = np.maximum(err - R.half_ulp16(np.abs(ref) + e32, nm), 0) / np.where(e32 > 0, e32, 1)
        print(f"share moe_gemm {layout} {nm} bias {with_bias} rows {rows} K {K} N {N}: {share:.3f}  used {float(used.max()):.3f}")
        assert share <= 1.0, f"{share:.3f} of the bound"


@pytest.mark.parametrize("layout", ["nk", "kn"])
def test_a_row_has_the_same_bits_alone_and_in_a_batch(layout):
    """random data: one source row alone (block_m 32), inside 226 rows (block_m 128) at two places of its segment, and twice"""
    M = _M()
    dtype, K, N, E = torch.bfloat16, 2880, 264, 7
    g = torch.Generator().manual_seed(77)
    w = (torch.randn((E, N, K) if layout == "nk" else (E, K, N), generator=g) / K ** 0.5).to(dtype).to(DEV)
    bias = torch.randn(E, N, generator=g).to(DEV)
    off = torch.from_numpy(G.offsets_of(G.PATTERN)).to(DEV)
    x = torch.randn(226, K, generator=g).to(dtype).to(DEV)
    e, r0, r1 = 6, 97 + 3, 97 + 128                          # expert 6 owns rows 97 .. 225: first tile, second tile
    x[r1] = x[r0]
    big = M.moe_gemm(x, w, off, w_layout=layout, bias=bias)
    _same(big, M.moe_gemm(x, w, off, w_layout=layout, bias=bias), "two runs")
    _same(big[r0], big[r1], "a row at two places of its segment")
    lone_off = torch.tensor([0] * (e + 1) + [1], dtype=torch.int32, device=DEV)
    assert _plan(M, 1, N, K, E, layout, dtype) == 32 and _plan(M, 226, N, K, E, layout, dtype) == 128
    lone = M.moe_gemm(x[r0:r0 + 1], w, lone_off, w_layout=layout, bias=bias)
    _same(lone[0], big[r0], "a row alone against the row in a batch")


def test_guard_bands_inputs_and_the_c_abi():
    """x, w, bias, the tables and out between guard bands: nothing outside out changes, every element of out is written, the
    inputs stay as they were - plain and gather form"""
    M = _M()
    dtype, T, topk, E, K, N = torch.bfloat16, 67, 2, 8, 264, 136
    sorted_slot, pos, offsets = _sorted_case(M, T, topk, E, 16, 600)
    x, w, bias = G.witness(T, K, N, E, "nk", 601, True)
    ins = [guard.guarded(t, gaps=True) for t in (_dev(x, dtype), _dev(bias, dtype))]
    xv, bv = ins[0][1], ins[1][1]
    wt = _dev(w, dtype)
    want = M.moe_gemm(xv.contiguous(), wt, offsets, bias=bv.contiguous(), sorted_slot=sorted_slot, top_k=topk)
    rows = sorted_slot.shape[0]
    buf, view = guard.slab((rows, N), dtype, gaps=False, device=DEV, check_prep=False)
    snap = guard.snapshot(buf)
    M.moe_gemm(xv, wt, offsets, bias=bv, sorted_slot=sorted_slot, top_k=topk, out=view)
    xpv = guard.guarded(M.moe_permute_forward(xv, sorted_slot, topk), gaps=True)
    buf2, view2 = guard.slab((rows, N), dtype, gaps=True, device=DEV, check_prep=False)
    snap2 = guard.snapshot(buf2)
    M.moe_gemm(xpv[1], wt, offsets, bias=bv, out=view2)
    torch.cuda.synchronize()
    for (b, v, s), name in zip(ins + [xpv], ("x", "bias", "xp")):
        assert torch.equal(guard.bits(b), s), f"{name} was written"
    guard.assert_untouched(buf, view, snap, "out (gather)")
    guard.assert_untouched(buf2, view2, snap2, "out (plain, strided)")
    _same(view, want, "gather into a slab")
    _same(view2, want, "plain into a strided slab")
    assert not torch.isnan(view.float()).any()


def test_replays_in_a_graph_after_the_tables_were_rewritten():
    """captured once; expert_offsets and sorted_slot are then rewritten in place to another segmentation and the replay equals
    the eager call: nothing of the launch depends on the tables"""
    M = _M()
    ns = torch.ops.flash_attn_mi355
    dtype, T, topk, E, K, N, align = torch.bfloat16, 67, 2, 8, 264, 136, 16
    tables = [_sorted_case(M, T, topk, E, align, 700 + i) for i in range(3)]
    assert not torch.equal(tables[0][2], tables[1][2])
    x, w, bias = G.witness(T, K, N, E, "nk", 710, True)
    xt, wt, bt = _dev(x, dtype), _dev(w, dtype), _dev(bias, torch.float32)
    ref = [ns.moe_gemm(xt, wt, t[2], "nk", bt, t[0], topk).clone() for t in tables]
    ss, off = tables[0][0].clone(), tables[0][2].clone()
    ns.moe_gemm(xt, wt, off, "nk", bt, ss, topk)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ns.moe_gemm(xt, wt, off, "nk", bt, ss, topk)
    for i in (1, 2, 0):
        ss.copy_(tables[i][0])
        off.copy_(tables[i][2])
        graph.replay()
        torch.cuda.synchronize()
        _same(out, ref[i], f"replay {i}")


def test_an_expert_stride_past_two_to_the_31():
    """w as a view whose experts lie 2^31 + 8 elements apart (E = 2, over an uninitialised allocation: only the two slabs are
    touched): every offset is 64-bit"""
    M = _M()
    dtype, K, N = torch.bfloat16, 48, 40
    stride = 2 ** 31 + 8
    for layout in ("nk", "kn"):
        x, w, bias = G.witness(40, K, N, 2, layout, 800, False)
        store = torch.empty(stride + N * K, dtype=dtype, device=DEV)
        wv = store.as_strided(w.shape, (stride, w.shape[2], 1))
        wv.copy_(_dev(w, dtype))
        off = G.offsets_of([7, 33])
        got = M.moe_gemm(_dev(x, dtype), wv, torch.from_numpy(off).to(DEV), w_layout=layout)
        _exact(got, G.expected(x, w, off, _name(dtype), layout=layout), dtype, f"expert stride 2^31 + 8 {layout}")
        del store, wv


def test_no_rows_and_malformed_offsets():
    M = _M()
    dtype, K, N, E = torch.bfloat16, 48, 40, 7
    x, w, _ = G.witness(64, K, N, E, "nk", 900, False)
    wt = _dev(w, dtype)
    out = M.moe_gemm(_dev(x[:0], dtype), wt, torch.zeros(E + 1, dtype=torch.int32, device=DEV))
    assert out.shape == (0, N)
    # decreasing and out-of-range offsets: wrong rows, but every write stays inside out (guard bands) and nothing faults
    buf, view = guard.slab((64, N), dtype, gaps=True, device=DEV, check_prep=False)
    snap = guard.snapshot(buf)
    bad = torch.tensor([0, 40, 20, -5, 2 ** 31 - 1, 30, 64, 10 ** 6], dtype=torch.int32, device=DEV)
    M.moe_gemm(_dev(x, dtype), wt, bad, out=view)
    torch.cuda.synchronize()
    guard.assert_untouched(buf, view, snap, "out under malformed offsets")


def test_opcheck():
    _M()
    ns = torch.ops.flash_attn_mi355
    dtype, T, topk, E, K, N = torch.bfloat16, 5, 2, 8, 16, 24
    sorted_slot, pos, offsets = _sorted_case(_M(), T, topk, E, 4, 950, drop=False)
    x, w, bias = G.witness(T, K, N, E, "nk", 951, True)
    xt, wt, bt = _dev(x, dtype), _dev(w, dtype), _dev(bias, torch.float32)
    xp = ns.moe_permute(xt, sorted_slot, topk, None, pos)
    torch.library.opcheck(ns.moe_gemm, (xt, wt, offsets, "nk", bt, sorted_slot, topk))
    torch.library.opcheck(ns.moe_gemm, (xp, wt, offsets, "nk", None, None, None))
    torch.library.opcheck(ns.moe_gemm, (xp, wt.transpose(1, 2).contiguous(), offsets, "kn", bt, None, None))


def test_a_tiny_moe_block_end_to_end():
    """T 67, E 8, K 2, hidden 264, intermediate 136, bf16: route -> sort -> moe_gemm (fused gather, gate-up "nk") -> act_and_mul
    -> moe_gemm (down, "kn") -> combine, against the dense fp64 definition sum_k w_k Down_e(silu(gate_e x) * up_e x).  The
    tolerance is the sum of the stage bounds, first order, each stage's input error carried through the next stage's
    derivative: h = gate-up GEMM (moe_gemm_ref.bound: eh), a = act(g) * u (act_mul_ref's fp32 term Da, |d a| <= (|act'(g)| |u|
    + |act(g)|) eh - bounded with |silu'| <= 1.1 -, and its rounding), y = down GEMM (its own bound on the exact a, + |W| ea),
    out = combine (route bound bw |y| + |w| ey + K u sum |w y| + its rounding)."""
    import act_mul_ref as A
    from flash_attn_mi355 import act_mul
    M = _M()
    T, E, K, H, I, align, scale = 67, 8, 2, 264, 136, 16, 1.5
    dt, nm = torch.bfloat16, "bfloat16"
    g = torch.Generator().manual_seed(61)
    logits = (torch.randn(T, E, generator=g) * 2).to(dt).to(DEV)
    x = torch.randn(T, H, generator=g).to(dt).to(DEV)
    W1 = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(dt).to(DEV)     # "nk": [E, 2 I, H], gate rows first
    W2 = (torch.randn(E, I, H, generator=g) / I ** 0.5).to(dt).to(DEV)         # "kn": [E, I, H]
    w, ids = M.moe_route_forward(logits, K, scale=scale)
    sorted_slot, pos, offsets = M.moe_sort(ids, E, align=align)
    h = M.moe_gemm(x, W1, offsets, sorted_slot=sorted_slot, top_k=K)
    a = act_mul.act_and_mul(h)
    y = M.moe_gemm(a, W2, offsets, w_layout="kn")
    out = M.moe_combine_forward(y, w, pos)

    lw, xw, W1w, W2w = R.widen(logits), R.widen(x), R.widen(W1), R.widen(W2)
    w_ref, ids_ref, _ = R.route_ref(lw, K, scale=scale)
    assert (ids.cpu().numpy() == ids_ref).all()
    bw = R.route_weight_bound(lw, w_ref, ids_ref, scoring="softmax", renormalize=True)
    hu = lambda v: R.half_ulp16(v, nm)                                          # noqa: E731
    u = R.U
    W1s, W2s = W1w[ids_ref], W2w[ids_ref]                                      # [T, K, 2I, H], [T, K, I, H]
    h_ref = np.einsum("th,tkjh->tkj", xw, W1s)
    h_mag = np.einsum("th,tkjh->tkj", np.abs(xw), np.abs(W1s))
    eh = (H + 2) * 2 * u * h_mag
    eh = eh + hu(np.abs(h_ref) + eh)
    gt, ut = torch.from_numpy(h_ref[..., :I]), torch.from_numpy(h_ref[..., I:])
    a_ref_t, Da = A.forward_ref(gt, ut, "silu")
    a_ref, Da = a_ref_t.numpy(), Da.numpy()
    act_g = (gt * torch.sigmoid(gt)).numpy()
    ea = 2 * Da + 1.1 * np.abs(ut.numpy()) * eh[..., :I] + np.abs(act_g) * eh[..., I:] + 1.1 * eh[..., :I] * eh[..., I:]
    ea = ea + hu(np.abs(a_ref) + ea)
    y_ref = np.einsum("tki,tkih->tkh", a_ref, W2s)
    y_mag = np.einsum("tki,tkih->tkh", np.abs(a_ref), np.abs(W2s))
    ey = (I + 2) * 2 * u * (y_mag + np.einsum("tki,tkih->tkh", ea, np.abs(W2s))) + np.einsum("tki,tkih->tkh", ea, np.abs(W2s))
    ey = ey + hu(np.abs(y_ref) + ey)
    out_ref = (w_ref[:, :, None] * y_ref).sum(1)
    e_out = (bw[:, :, None] * np.abs(y_ref) + np.abs(w_ref)[:, :, None] * ey).sum(1) + K * u * np.abs(w_ref[:, :, None] * y_ref).sum(1)
    e_out = (e_out + hu(np.abs(out_ref) + e_out)) * R.SLACK
    err = np.abs(R.widen(out) - out_ref)
    share = float((err / e_out).max())
    print(f"share moe_gemm end to end out: {share:.3f}")
    assert share <= 1.0
    # and the block's rows behind the last segment are +0 in both GEMM outputs
    end = int(offsets[E])
    assert (h[end:] == 0).all() and (y[end:] == 0).all()
