"""GPU: fa_sample against the fp64 reference of tests/sample_ref.py on DECISIVE inputs (every decision clear by DELTA = 2^-13 of
normalised mass, four times the counted bound on a mass: ids, n_kept and the filtered row are compared bit for bit and no row is
ever left out), on the exact cases that need no margin, on a stratified frequency count, and for repeatability, independence of
the batch, guard bands and graph capture.

The launch plan (csrc/fa_sample.hip; sample_ref.chunks / iters / wave_run).  A piece is 8 columns.  V < 32768: one workgroup of
1024 lanes per row, a sweep takes ITERS = ceil(ceil(V / 8) / 1024) steps and wave w owns the columns [w, w + 1) x ITERS x 512.
V >= 32768: the split plan - a row is cut into chunks of 16384 columns, one workgroup each, whose results meet in the workspace.
The boundaries and the vocabulary sizes just below, at and just above them:
    piece            7, 8, 9
    workgroup step   8191, 8192, 8193   (ITERS 1 -> 2: a wave's run grows from 512 to 1024 columns)
    split plan       32767, 32768, 32769   (one workgroup -> two chunks)
    chunk            49151, 49152, 49153   (three chunks -> four); V = 151936: 10 chunks; V = 262144: 16 chunks - the decisive
                     tokens are planted at index 0, V - 1 and on both sides of every chunk boundary
and 1, 60, 264 besides."""
import ctypes
import math

import numpy as np
import pytest
import torch

import guard
import sample_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SMALL_V = [1, 7, 8, 9, 60, 264, 8191, 8192, 8193, 32767, 32768, 32769, 49151, 49152, 49153]
NEG = float("-inf")


def _S():
    import __graft_entry__ as g
    g.build()
    import flash_attn_mi355.sample as S
    return S


def _batch(rows_cpu, pad=3):
    """[rows, V] on the GPU as a view with row stride V + pad: the rows start at every alignment"""
    rows, V = len(rows_cpu), rows_cpu[0].numel()
    wide = torch.zeros(rows, V + pad, dtype=rows_cpu[0].dtype, device="cuda")
    x = wide[:, :V]
    x.copy_(torch.stack(rows_cpu))
    return x


def _run(S, x, T, k, p, mp, u):
    """(ids, n_kept, lse, filtered) of one batch: the sampling call and the filter call"""
    ids, lse, n_kept = S.sample(x, temperature=T, top_k=k, top_p=p, min_p=mp, u=u, return_lse=True, return_n_kept=True)
    filtered = S.top_k_top_p_filter(x, temperature=T, top_k=k, top_p=p, min_p=mp)
    torch.cuda.synchronize()
    return ids.cpu(), n_kept.cpu(), lse.cpu(), filtered.cpu()


def _check_rows(out, rows_cpu, params, tag):
    """every row against the reference: ids, n_kept and filtered bit for bit, lse within the counted bound"""
    ids, n_kept, lse, filtered = out
    for r, (row, (T, k, p, mp, u)) in enumerate(zip(rows_cpu, params)):
        ref = R.row_ref(row, T, k, p, mp, u)
        where = f"{tag} row {r} (T {T}, k {k}, top_p {p}, min_p {mp}, u {u})"
        assert int(ids[r]) == ref["id"], f"{where}: id {int(ids[r])}, reference {ref['id']}"
        assert int(n_kept[r]) == ref["n_kept"], f"{where}: n_kept {int(n_kept[r])}, reference {ref['n_kept']}"
        want = R.filtered_ref(row, ref["kept"])
        assert torch.equal(guard.bits(filtered[r]), guard.bits(want)), f"{where}: filtered differs"
        got = float(lse[r])
        if ref["lse"] is None:
            assert not math.isfinite(got), f"{where}: lse {got} of a row whose x_j* overflows"
        elif math.isnan(ref["lse"]) or math.isinf(ref["lse"]):
            assert (math.isnan(got) and math.isnan(ref["lse"])) or got == ref["lse"], f"{where}: lse {got}, reference {ref['lse']}"
        else:
            bound = R.lse_bound(row, T if ref["sampled"] else 0.0, ref["lse"])
            print(f"{where}: |lse - reference| = {abs(got - ref['lse']):.3e}, bound {bound:.3e}")
            assert abs(got - ref["lse"]) <= bound, f"{where}: lse {got}, reference {ref['lse']}, bound {bound}"


def _configs(V):
    """(k, min_p on, top_p on): every filter alone, all together, and a top_k beyond the row"""
    if V == 1:
        return [(0, False, False), (0, False, True)]
    return [(0, False, False), (5, False, False), (0, True, False), (0, False, True), (5, True, True), (50, True, True)]


def _tensor(vals, dtype):
    return torch.tensor(vals, dtype=dtype, device="cuda")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", SMALL_V)
def test_decisive_rows_per_row_parameters(V, dtype):
    """one batch per V: a row for every filter setting (T 1 / 0.7 / 0.5 in turn) with its own decisive min_p, top_p and u, a greedy
    row (T = 0, u = NaN: not read) and a row with every filter off - the mixed batch is ONE call with [rows] parameter tensors"""
    S = _S()
    rows_cpu, params = [], []
    for n, (k, mp, tp) in enumerate(_configs(V)):
        T = (1.0, 0.7, 0.5)[n % 3]
        row = R.randn_row(V, dtype, seed=100 * V + n, spread=(2.0, 3.0, 4.0)[n % 3])
        b = R.build(row, T, k, want_min_p=mp, want_top_p=tp, seed=n)
        rows_cpu.append(row)
        params.append((T, k, b["top_p"], b["min_p"], b["u"]))
    rows_cpu.append(R.randn_row(V, dtype, seed=7 * V + 1))
    params.append((0.0, 3, 0.5, 0.1, float("nan")))              # greedy whatever the filters say
    rows_cpu.append(R.randn_row(V, dtype, seed=7 * V + 2))
    params.append((1.0, 0, 1.0, 0.0, R.build(rows_cpu[-1], 1.0)["u"]))
    x = _batch(rows_cpu)
    cols = list(zip(*params))
    out = _run(S, x, _tensor(cols[0], torch.float32), _tensor(cols[1], torch.int32), _tensor(cols[2], torch.float32),
               _tensor(cols[3], torch.float32), _tensor(cols[4], torch.float32))
    _check_rows(out, rows_cpu, params, f"V {V} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [9, 264, 8193])
def test_decisive_rows_scalar_parameters(V, dtype):
    """the same settings with NUMBERS for every parameter: a call per setting, two copies of the row at different alignments"""
    S = _S()
    for n, (k, mp, tp) in enumerate(_configs(V)):
        T = (1.0, 0.7, 0.5)[n % 3]
        row = R.randn_row(V, dtype, seed=100 * V + n, spread=(2.0, 3.0, 4.0)[n % 3])
        b = R.build(row, T, k, want_min_p=mp, want_top_p=tp, seed=n + 10)
        x = _batch([row, row])
        out = _run(S, x, T, k, b["top_p"], b["min_p"], _tensor([b["u"]] * 2, torch.float32))
        _check_rows(out, [row, row], [(T, k, b["top_p"], b["min_p"], b["u"])] * 2, f"V {V} {dtype} scalar setting {n}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [151936, 262144])
def test_decisive_rows_large_vocabulary(V, dtype):
    """one row of logits, up to 47 parameter sets (rows <= 67): tokens that carry mass are planted at index 0, V - 1 and on both
    sides of every chunk boundary.  One row per planted token draws it under top_k = 40; 8 rows put top_p's cut on a planted
    token and draw another; 5 rows run every filter together; one row is greedy, one has every filter off"""
    S = _S()
    plant = [0] + [c for w in range(1, R.chunks(V)) for c in (w * R.CHUNK - 1, w * R.CHUNK)] + [V - 1]
    n = len(plant)
    assert n == 2 * R.chunks(V) and len(set(plant)) == n and n <= 32
    row = R.randn_row(V, dtype, seed=V, spread=2.0, plant=plant)
    T = 1.0
    params = []
    for i in range(n):
        b = R.build(row, T, 40, draw_index=plant[i])
        params.append((T, 40, 1.0, 0.0, b["u"]))
    for i in range(8):
        b = R.build(row, T, 0, want_top_p=True, cut_index=plant[n - 1 - (i % 4)], draw_index=plant[(2 * i) % (n - 4)])
        params.append((T, 0, b["top_p"], 0.0, b["u"]))
    for i in range(5):
        k = (1000, 50, 40, 33, 5)[i]
        b = R.build(row, T, k, want_min_p=True, want_top_p=True, seed=i)
        params.append((T, k, b["top_p"], b["min_p"], b["u"]))
    params.append((0.0, 0, 1.0, 0.0, 0.5))
    params.append((T, 0, 1.0, 0.0, R.build(row, T, 0, draw_index=plant[n // 2])["u"]))
    rows_cpu = [row] * len(params)
    x = _batch(rows_cpu)
    cols = list(zip(*params))
    out = _run(S, x, _tensor(cols[0], torch.float32), _tensor(cols[1], torch.int32), _tensor(cols[2], torch.float32),
               _tensor(cols[3], torch.float32), _tensor(cols[4], torch.float32))
    _check_rows(out, rows_cpu, params, f"V {V} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_cases(dtype):
    """no margin needed.  All-equal logits: every q = 2^40, top_k's ties go to the lowest indices and id is the floor(u n)-th kept
    index, for u = 0, 1 - 2^-24, 1.0, NaN and a negative number; rows of -inf, with NaNs, with +inf; k = 1, k >= V, top_p <= 0,
    min_p > 1"""
    S = _S()
    V = 60
    rows_cpu, params, want = [], [], []
    flat = torch.full((V,), 1.5).to(dtype)
    for u in (0.0, 0.5, 0.37, 1 - 2.0 ** -24, 1.0, float("nan"), -3.0):
        for k in (0, 7, V, 100):
            n = k if 1 <= k < V else V
            uu = R.f32(u) if u > 0 else 0.0
            rows_cpu.append(flat)
            params.append((0.7, k, 1.0, 0.0, u))
            want.append((min(math.floor(uu * n), n - 1), n))
    rnd = R.randn_row(V, dtype, seed=5)
    top = int(R.order(R.values(rnd))[0])
    for kw in ((1, 1.0, 0.0), (0, 0.0, 0.0), (0, -1.0, 0.0), (0, 1.0, 1.5), (0, 1.0, float("inf"))):
        rows_cpu.append(rnd)
        params.append((1.0,) + kw + (0.9,))
        want.append((top, 1))
    rows_cpu.append(rnd); params.append((1e-38, 5, 0.9, 0.1, 0.9)); want.append((top, 1))      # 1 / T overflows x_j*: greedy
    minus = torch.full((V,), NEG).to(dtype)
    rows_cpu.append(minus); params.append((1.0, 5, 0.9, 0.1, 0.5)); want.append((-1, 0))
    rows_cpu.append(minus); params.append((0.0, 0, 1.0, 0.0, 0.5)); want.append((-1, 0))
    nans = rnd.clone(); nans[::2] = float("nan"); nans[top] = float("nan")
    rows_cpu.append(nans); params.append((0.0, 0, 1.0, 0.0, 0.5)); want.append((int(R.order(R.values(nans))[0]), 1))
    rows_cpu.append(nans); params.append((1.0, 200, 1.0, 0.0, 1.0)); want.append((None, V - len(range(0, V, 2)) - (top % 2)))
    allnan = torch.full((V,), float("nan")).to(dtype)
    rows_cpu.append(allnan); params.append((1.0, 0, 1.0, 0.0, 0.5)); want.append((-1, 0))
    inf = rnd.clone(); inf[41] = float("inf"); inf[50] = float("inf")
    rows_cpu.append(inf); params.append((1.0, 0, 0.9, 0.0, 0.99)); want.append((41, 1))
    one = rnd.clone(); one[:] = NEG; one[V - 1] = -2.0
    rows_cpu.append(one); params.append((0.5, 0, 0.3, 0.2, 0.99)); want.append((V - 1, 1))
    x = _batch(rows_cpu)
    cols = list(zip(*params))
    out = _run(S, x, _tensor(cols[0], torch.float32), _tensor(cols[1], torch.int32), _tensor(cols[2], torch.float32),
               _tensor(cols[3], torch.float32), _tensor(cols[4], torch.float32))
    for r, (wid, wn) in enumerate(want):
        if wid is not None:
            assert int(out[0][r]) == wid, (r, params[r], int(out[0][r]), wid)
        assert int(out[1][r]) == wn, (r, params[r], int(out[1][r]), wn)
    _check_rows(out, rows_cpu, params, f"exact {dtype}")
    # the all-equal top_k rows keep the LOWEST indices
    r = 1                                                        # u = 0, k = 7
    assert torch.isfinite(out[3][r][:7].float()).all() and (out[3][r][7:].float() == NEG).all()
    g = S.greedy(x)
    torch.cuda.synchronize()
    for r, row in enumerate(rows_cpu):
        assert int(g[r]) == R.row_ref(row, 0.0)["id"]


def test_stratified_frequency():
    """one V = 8 row 4096 times with u = (i + 0.5) / 4096: every token's count is within 2 of 4096 p_j - a boundary shifted by
    less than DELTA < 1 / 4096 moves at most one grid point per side"""
    S = _S()
    N = 4096
    row = R.randn_row(8, torch.float32, seed=11, spread=1.5)
    x = row.cuda().expand(N, 8)
    u = ((torch.arange(N, dtype=torch.float64) + 0.5) / N).float().cuda()
    ids = S.sample(x.contiguous(), temperature=0.8, u=u)
    torch.cuda.synchronize()
    e, _, _ = R.masses(R.values(row), 0.8)
    p = e / e.sum()
    counts = np.bincount(ids.cpu().numpy(), minlength=8)
    assert counts.sum() == N and ids.min() >= 0
    assert (np.abs(counts - N * p) <= 2.0).all(), (counts, N * p)
    assert (np.diff(ids.cpu().numpy()) >= 0).all()                # the inverse CDF is monotone in u


@pytest.mark.parametrize("V,dtype", [(8193, torch.bfloat16), (8193, torch.float32), (8193, torch.float16), (151936, torch.float16),
                                     (262144, torch.bfloat16)])
def test_repeatability_and_independence(V, dtype, monkeypatch):
    """the same call twice gives the same bits; a row alone gives the bits it has inside a batch at another index and alignment;
    the workspace arriving zeroed, 0xFF or random changes nothing (and no more than the queried bytes are asked for)"""
    S = _S()
    rows_cpu = [R.randn_row(V, dtype, seed=s, spread=3.0) for s in range(5)]
    g = torch.Generator().manual_seed(3)
    u = torch.rand(5, generator=g).cuda()
    kw = dict(temperature=_tensor([0.7, 1.0, 0.0, 0.5, 1.3], torch.float32), top_k=_tensor([50, 0, 0, 7, 1000], torch.int32),
              top_p=_tensor([0.9, 0.8, 0.5, 1.0, 0.95], torch.float32), min_p=_tensor([0.0, 0.01, 0.0, 0.05, 0.001], torch.float32))
    x = _batch(rows_cpu)
    first = _run(S, x, kw["temperature"], kw["top_k"], kw["top_p"], kw["min_p"], u)
    again = _run(S, x, kw["temperature"], kw["top_k"], kw["top_p"], kw["min_p"], u)
    same = lambda a, b: all(torch.equal(guard.bits(s) if s.is_floating_point() else s, guard.bits(t) if t.is_floating_point() else t)   # noqa: E731
                            for s, t in zip(a, b))
    assert same(first, again)
    for r in (0, 3, 4):
        alone = _run(S, rows_cpu[r].cuda().view(1, V), float(kw["temperature"][r]), int(kw["top_k"][r]), float(kw["top_p"][r]),
                     float(kw["min_p"][r]), u[r:r + 1])
        assert same(alone, [t[r:r + 1] for t in first]), r
    from flash_attn_mi355 import flash_attn_interface as fi
    for fill in ("zeros", "ones", "random"):
        workspace, check = guard.guarded_workspace(fill)
        monkeypatch.setattr(fi, "_workspace", workspace)
        out = _run(S, x, kw["temperature"], kw["top_k"], kw["top_p"], kw["min_p"], u)
        assert same(first, out), fill
        assert check()["sizes"] == [R.workspace_bytes(5, V)] * 2     # (the sampling call and the filter call; bands intact)
    assert (R.workspace_bytes(5, V) > 0) == (V >= R.SPLIT_MIN)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1001, 33001])
def test_guard_bands(V, dtype):
    """logits and filtered are views inside NaN-filled slabs (gaps between the rows), ids / n_kept / lse / u and the parameter
    arrays sit exactly sized between bands, the workspace (V = 33001: the split plan) has exactly the queried size between sentinel
    bands and arrives filled with 0xFF: nothing outside a tensor's elements is written, no NaN of a gap reaches an output, the
    inputs are unchanged, and the results are the unguarded call's"""
    S = _S()
    from flash_attn_mi355 import _lib
    from flash_attn_mi355 import flash_attn_interface as fi
    codes = {torch.float16: _lib.FA_FP16, torch.bfloat16: _lib.FA_BF16, torch.float32: _lib.FA_FP32}
    rows = 6
    rows_cpu = [R.randn_row(V, dtype, seed=s, spread=3.0) for s in range(rows)]
    g = torch.Generator().manual_seed(9)
    u = torch.rand(rows, generator=g).cuda()
    T = _tensor([0.7, 1.0, 0.0, 0.5, 1.3, 1.0], torch.float32)
    k = _tensor([50, 0, 0, 7, 1000, 3], torch.int32)
    p = _tensor([0.9, 0.8, 0.5, 1.0, 0.95, 0.2], torch.float32)
    mp = _tensor([0.0, 0.01, 0.0, 0.05, 0.001, 0.0], torch.float32)
    want = _run(S, torch.stack(rows_cpu).cuda(), T, k, p, mp, u)

    band = 4096

    def banded(t):
        it = guard._INT_OF.get(t.dtype, t.dtype)
        buf = torch.full((band + t.numel() + band,), -1, dtype=it, device="cuda").view(t.dtype)
        view = buf[band:band + t.numel()]
        view.copy_(t)
        return buf, view

    def holds(buf, n, name):
        b = buf.view(guard._INT_OF.get(buf.dtype, buf.dtype))
        assert bool((b[:band] == -1).all()) and bool((b[band + n:] == -1).all()), f"{name}: written outside its {n} elements"

    xb, x, xsnap = guard.guarded(torch.stack(rows_cpu).cuda(), gaps=True)
    fb, f, fsnap = guard.guarded(shape=(rows, V), dtype=dtype, device="cuda", gaps=True)
    ins = {n: banded(t) for n, t in (("u", u), ("temperature", T), ("top_k", k), ("top_p", p), ("min_p", mp))}
    outs = {"ids": banded(torch.zeros(rows, dtype=torch.int32)), "n_kept": banded(torch.zeros(rows, dtype=torch.int32)),
            "lse": banded(torch.zeros(rows, dtype=torch.float32))}
    s = _lib.FaSampleParams()
    s.struct_size = ctypes.sizeof(_lib.FaSampleParams)
    s.logits, s.logits_row_stride = x.data_ptr(), x.stride(0)
    s.filtered, s.filtered_row_stride = f.data_ptr(), f.stride(0)
    for n, (_, v) in list(ins.items()) + list(outs.items()):
        setattr(s, n, v.data_ptr())
    s.rows, s.vocab, s.dtype = rows, V, codes[dtype]
    nbytes = _lib.sample_workspace_bytes(s)
    assert nbytes == R.workspace_bytes(rows, V)
    workspace, check_ws = guard.guarded_workspace("ones")      # (0xFF: a bin or a partial read before it is written would show)
    wsp = workspace(nbytes, x.device)
    if wsp is not None:
        s.workspace, s.workspace_bytes = wsp.data_ptr(), nbytes
    _lib.call_sample(s, fi._stream(x.device))
    torch.cuda.synchronize()
    assert check_ws()["sizes"] == [nbytes]
    guard.assert_untouched(fb, f, fsnap, "filtered")
    assert torch.equal(guard.bits(xb), xsnap), "logits were written"
    for n, (buf, _) in list(ins.items()) + list(outs.items()):
        holds(buf, rows, n)
    assert torch.equal(outs["ids"][1].cpu(), want[0]) and torch.equal(outs["n_kept"][1].cpu(), want[1])
    assert torch.equal(guard.bits(outs["lse"][1].cpu()), guard.bits(want[2]))
    assert torch.equal(guard.bits(f.contiguous().cpu()), guard.bits(want[3]))


def test_opcheck_on_the_torch_ops():
    """torch.ops.flash_attn_mi355.sample / .sample_filter pass torch.library.opcheck with tensors and with numbers"""
    _S()
    import flash_attn_mi355.torch_ops  # noqa: F401  (registers the ops)
    x = torch.stack([R.randn_row(264, torch.bfloat16, seed=s) for s in range(3)]).cuda()
    u = _tensor([0.1, 0.5, 0.9], torch.float32)
    T, k = _tensor([0.7, 0.0, 1.0], torch.float32), _tensor([5, 0, 50], torch.int32)
    p, mp = _tensor([0.9, 1.0, 0.5], torch.float32), _tensor([0.0, 0.1, 0.01], torch.float32)
    ns = torch.ops.flash_attn_mi355
    torch.library.opcheck(ns.sample.default, (x, u, T, 1.0, k, 0, p, 1.0, mp, 0.0))
    torch.library.opcheck(ns.sample.default, (x, u, None, 0.8, None, 40, None, 0.9, None, 0.02))
    torch.library.opcheck(ns.sample_filter.default, (x, T, 1.0, k, 0, p, 1.0, mp, 0.0))
    torch.library.opcheck(ns.sample_filter.default, (x[:, :261], None, 0.8, None, 40, None, 0.9, None, 0.02))


@pytest.mark.parametrize("V", [8193, 40000])
def test_graph_capture(V):
    """a capture of one call (V = 40000: the split plan's launches and its workspace) replays with fresh u and matches the eager
    call"""
    S = _S()
    rows = 4
    x = torch.stack([R.randn_row(V, torch.bfloat16, seed=s, spread=3.0) for s in range(rows)]).cuda()
    kw = dict(temperature=0.8, top_k=50, top_p=0.9, min_p=0.01)
    u = torch.full((rows,), 0.25, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        S.sample_forward(x, u, **kw)                             # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ids, n_kept, lse = S.sample_forward(x, u, **kw)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(3):
        fresh = torch.rand(rows, device="cuda", generator=gen)
        u.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        eager = S.sample_forward(x, fresh, **kw)
        torch.cuda.synchronize()
        assert torch.equal(ids, eager[0]) and torch.equal(n_kept, eager[1]) and torch.equal(guard.bits(lse), guard.bits(eager[2]))
