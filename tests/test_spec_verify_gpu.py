"""GPU: fa_spec_accept / fa_spec_walk against the fp64 reference of tests/spec_verify_ref.py, BIT FOR BIT.  The accept / recovered
decisions run on the reference's constructed batches (spec_verify_ref.batch_case: tau >= 1/4, the recovered token and the draft
token planted at index 0, V - 1 and on both sides of every chunk boundary, u_accept and u_recover clear of the device's rounding by
the margins derived in that file - tests/test_spec_verify_cpu.py holds the fp64 decision against the fp32 emulation on the same
cases) and on exact cases that need no margin; the walk is integer work and is compared on random trees.  Then the whole step
(`verify`), batch invariance, repeatability, the commit on a paged cache, guard bands, workspace fills and a graph capture.

The launch plan (csrc/fa_spec_verify.hip): a row is cut into chunks of 16384 columns, a piece is 8 columns; the sizes just below,
at and just above the boundaries: piece 7, 8, 9; a lane's second piece 8191, 8192, 8193; one chunk -> two 16383, 16384, 16385;
two -> three 32767, 32768, 32769; four chunks 49153; ten chunks 151936."""
import ctypes
import math

import numpy as np
import pytest
import torch

import guard
import sample_ref as R
import spec_verify_ref as SR
import tree_ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
NEG = float("-inf")
NAN = float("nan")


def _D():
    import __graft_entry__ as g
    g.build()
    import flash_attn_mi355.spec_decode as D
    return D


def _padded(t, pad=3):
    """[B, T, V] on the GPU as a view whose rows are V + pad apart: they start at every alignment"""
    B, T, V = t.shape
    wide = torch.zeros(B, T, V + pad, dtype=t.dtype, device="cuda")
    x = wide[:, :, :V]
    x.copy_(t)
    return x


def _cuda(c):
    return {k: v.cuda() for k, v in c.items()}


def _i32(rows):
    return torch.tensor(rows, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("V", SR.ACCEPT_V)
def test_accept_and_recovered_on_planted_batches(V):
    """every child node of the reference's batches: accept and recovered bit for bit, node 0 and the padding node 0 / -1; the
    tensors contiguous (odd V: rows that are not 16-byte aligned) and as padded-stride views"""
    D = _D()
    for tdtype, qdtype in SR.dtype_pairs(V):
        c = SR.batch_case(V, tdtype, qdtype)
        g = _cuda(c)
        for view in (lambda t: t, _padded):
            accept, recovered = D.accept_forward(view(g["target"]), view(g["draft"]), g["draft_ids"], g["u_accept"], g["u_recover"],
                                                 parents=g["parents"], temperature=g["temperature"])
            torch.cuda.synchronize()
            where = f"V {V} {tdtype} / {qdtype}"
            assert torch.equal(accept.cpu(), c["accept"]), (where, accept.cpu(), c["accept"])
            assert torch.equal(recovered.cpu(), c["recovered"]), (where, recovered.cpu(), c["recovered"])


def _chain_pairs(D, cases, dtype, qdtype=torch.float32):
    """each case (target row, draft row, d, T, u_accept, u_recover) as a request of two nodes (the chain): the op's (accept,
    recovered) of node 1 per case and the reference's"""
    B, V = len(cases), cases[0][0].numel()
    target = torch.zeros(B, 2, V, dtype=dtype)
    draft = torch.full((B, 2, V), NAN, dtype=qdtype)
    for b, (trow, qrow, *_) in enumerate(cases):
        target[b, 0], target[b, 1], draft[b, 1] = trow.to(dtype), NAN, qrow.to(qdtype)
    cols = list(zip(*[c[2:] for c in cases]))
    pair = lambda vals, dt: torch.stack([torch.zeros(B, dtype=dt), torch.tensor(vals, dtype=dt)], 1).cuda()   # noqa: E731
    accept, recovered = D.accept_forward(target.cuda(), draft.cuda(), pair(cols[0], torch.int64), pair(cols[2], torch.float32),
                                         pair(cols[3], torch.float32), temperature=torch.tensor(cols[1]).cuda())
    torch.cuda.synchronize()
    assert accept[:, 0].abs().sum() == 0 and (recovered[:, 0] == -1).all()
    got = list(zip(accept[:, 1].tolist(), recovered[:, 1].tolist()))
    want = [SR.accept_ref(target[b, 0], draft[b, 1], *cases[b][2:]) for b in range(B)]
    return got, want


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_cases(dtype):
    """no margin needed: a one-hot q (the residual is p with d removed), q all ones (R == 0: the fallback draw over the target's
    own masses), u = 0 / 1 - 2^-24 / 1 / NaN, d = -1 and d = V, a filtered target row with -inf, an all -inf row, a +inf row, and
    greedy rows next to sampled ones through the per-request temperature tensor - one call"""
    D = _D()
    V, d, dk, top, rnd, filt, cases = _exact_cases(dtype)
    got, want = _chain_pairs(D, cases, dtype)
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    _exact_spelled_out(got, V, d, dk, top, rnd, filt)


def _exact_cases(dtype):
    V = 60
    rnd = R.randn_row(V, dtype, seed=5)
    top = int(R.order(R.values(rnd))[0])
    d = 17
    onehot = torch.zeros(V); onehot[d] = 1.0
    ones = torch.ones(V)
    filt = rnd.clone().float()
    keep = R.order(R.values(rnd))[:5]
    filt[:] = NEG
    filt[keep] = rnd.float()[keep]
    dk = int(sorted(keep)[2])
    hotk = torch.zeros(V); hotk[dk] = 1.0
    inf = rnd.clone(); inf[41] = float("inf"); inf[50] = float("inf")
    us = (0.0, 1 - 2.0 ** -24, 1.0, NAN)
    cases = []
    for u in us:
        cases.append((rnd, onehot, d, 1.0, u, u))                   # recovered: the first / last token other than d
        cases.append((rnd, ones, d, 0.7, u, u))                     # R == 0
        cases.append((filt, hotk, dk, 1.0, u, u))                   # the first / last kept token other than dk
        cases.append((filt, hotk, d, 1.0, u, u))                    # p_d = 0: a reject even at u = 0
    for bad in (-1, V, 2 ** 31 + 5, -2 ** 40):
        cases.append((rnd, onehot, bad, 1.0, 0.0, 0.0))
    cases.append((torch.full((V,), NEG), ones, 3, 1.0, 0.0, 0.5))   # empty
    cases.append((torch.full((V,), NAN), ones, 3, 0.0, 0.0, 0.5))   # empty and greedy: empty wins
    cases.append((inf, ones * NAN, 41, 1.0, NAN, NAN))              # +inf: greedy, the first one
    cases.append((inf, ones * NAN, 50, 1.0, NAN, NAN))
    for T in (0.0, -2.0, NAN):
        cases.append((rnd, ones * NAN, top, T, NAN, NAN))           # greedy rows read neither q nor u
        cases.append((rnd, ones * NAN, d, T, NAN, NAN))
    cases.append((rnd, ones * NAN, top, 1e-38, NAN, NAN))           # 1 / T overflows x_j*: greedy
    return V, d, dk, top, rnd, filt, cases


def _exact_spelled_out(got, V, d, dk, top, rnd, filt):
    """what the rules say about _exact_cases, case by case"""
    first = lambda row, skip: min(j for j in range(V) if j != skip and row[j] > NEG)    # noqa: E731
    last = lambda row, skip: max(j for j in range(V) if j != skip and row[j] > NEG)     # noqa: E731
    rf = rnd.float()
    assert got[0] == (1, first(rf, d)) and got[4] == (0, last(rf, d)) and got[8] == (0, last(rf, d)) and got[12] == (1, first(rf, d))
    assert got[1] == (1, 0) and got[5] == (0, V - 1) and got[9] == (0, V - 1) and got[13] == (1, 0)
    assert got[2] == (1, first(filt, dk)) and got[6] == (0, last(filt, dk))
    assert [g[0] for g in got[3:16:4]] == [0, 0, 0, 0]
    assert [g[0] for g in got[16:20]] == [0, 0, 0, 0]
    assert got[20] == got[21] == (0, -1) and got[22] == (1, 41) and got[23] == (0, 41)
    assert got[24:30] == [(1, top), (0, top)] * 3 and got[30] == (1, top)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [1000, 16385, 32768, 32777])
def test_recovered_is_fa_sample_where_the_residual_is_empty(V, dtype):
    """the two ops against each other, the reference takes no part: with a draft row of all 1.0f every r_j = min(max(p_j - 1, 0), 1)
    is 0, so R == 0 and `recovered` is the index-order inverse CDF over the target's own masses at u_recover - fa_sample's `ids`
    for the parent's row, the same temperature and u = u_recover, no filter: the same int32, bit for bit.  A chain of T = 3 (nodes
    1 and 2 read rows 0 and 1), B = 2; V: one chunk with a scalar tail, two chunks in spec where sample still runs one workgroup,
    sample's first split vocab, the split plan with a ragged last piece.  Temperature 0.7, a per-request tensor (a sampled and a
    greedy request) and 0.0; u_recover holds 0.0, 0.99999994 and seeded random numbers.  Every row holds its maximum twice: a
    greedy row must give the first one in both ops.  That R == 0 for these inputs is confirmed here on the CPU with
    spec_verify_ref's fp32 emulation: the residual masses that accept_ref(..., emulate=True) sums add up to 0, and accept_ref
    returns the draw over the target's own masses."""
    D = _D()
    import flash_attn_mi355.sample as S
    B, T = 2, 3
    target = torch.stack([torch.stack([R.randn_row(V, dtype, seed=V + 10 * b + t) for t in range(T)]) for b in range(B)])
    target[:, :, V - 1] = target[:, :, :V - 1].max(dim=-1).values
    gen = torch.Generator().manual_seed(V)
    u_recover = torch.rand(B, T, generator=gen)
    u_recover[0, 1], u_recover[1, 2] = 0.0, 0.99999994
    u_accept = torch.rand(B, T, generator=gen)
    draft_ids = torch.randint(0, V, (B, T), generator=gen, dtype=torch.int32)
    ones = torch.ones(B, T, V)
    first = [[int(np.flatnonzero(v == v.max())[0]) for v in (R.values(target[b, t]) for t in range(T - 1))] for b in range(B)]
    for temperature in (0.7, torch.tensor([1.3, 0.0]), 0.0):
        temps = temperature.tolist() if isinstance(temperature, torch.Tensor) else [temperature] * B
        for b, t in [(b, t) for b in range(B) for t in range(1, T) if temps[b] > 0]:     # the CPU side: R == 0 on every sampled node
            p, qm = SR.probs(R.values(target[b, t - 1]), temps[b], emulate=True)
            assert int(SR.residual(p, np.ones(V), emulate=True)[1].sum()) == 0
            rr = min(math.floor(float(u_recover[b, t]) * int(qm.sum())), int(qm.sum()) - 1)
            own = int(np.searchsorted(np.cumsum(qm), np.uint64(rr), side="right"))
            assert SR.accept_ref(target[b, t - 1], ones[b, t], 0, temps[b], 0.5, float(u_recover[b, t]), emulate=True)[1] == own
        on_gpu = temperature.cuda() if isinstance(temperature, torch.Tensor) else temperature
        _, recovered = D.accept_forward(target.cuda(), ones.cuda(), draft_ids.cuda(), u_accept.cuda(), u_recover.cuda(), temperature=on_gpu)
        rows = on_gpu.repeat_interleave(T - 1) if isinstance(temperature, torch.Tensor) else temperature
        ids, _, _ = S.sample_forward(target[:, :T - 1].contiguous().cuda(), u_recover[:, 1:].contiguous().cuda(), temperature=rows)
        torch.cuda.synchronize()
        assert recovered.dtype == ids.dtype == torch.int32
        assert torch.equal(recovered[:, 1:].cpu(), ids.cpu()), (V, dtype, temperature, recovered.cpu(), ids.cpu())
        assert (recovered[:, 0] == -1).all()
        for b in range(B):
            if not temps[b] > 0:
                assert recovered[b, 1:].tolist() == first[b] == ids[b].tolist(), (V, dtype, temperature, b)


def _random_walk_inputs(T, B, seed):
    rng = np.random.default_rng(seed)
    par = np.stack([tree_ref.random_parents(T, rng) for _ in range(B)]).astype(np.int32)
    draft = rng.integers(0, 3, (B, T)).astype(np.int32)
    target = rng.integers(-1, 3, (B, T)).astype(np.int32)
    target[target == -1] = np.where(rng.random((target == -1).sum()) < 0.3, -1, 1)
    accept = (rng.random((B, T)) < 0.7).astype(np.int32)
    recovered = rng.integers(-1, 100, (B, T)).astype(np.int32)
    return par, draft, target, accept, recovered


def _check_walk(out, par, draft, target, accept, recovered, tag):
    toks, num, path = (t.cpu().tolist() for t in out)
    for b in range(len(draft)):
        want = SR.walk_ref(None if par is None else (par[b] if np.ndim(par) == 2 else par), draft[b],
                           target[b], None if accept is None else accept[b], None if accept is None else recovered[b])
        assert (toks[b], num[b], path[b]) == want, (tag, b, (toks[b], num[b], path[b]), want)


@pytest.mark.parametrize("T", [1, 2, 5, 33, 64])
def test_walk_on_random_trees(T):
    """random trees of tree_ref.random_parents (a parent of -1 behind node 0 is a padding node), ids from a three-letter alphabet
    so that siblings repeat (the lowest index wins) and -1 targets occur; both modes; per-request, shared and absent parents"""
    D = _D()
    B = 9
    par, draft, target, accept, recovered = _random_walk_inputs(T, B, seed=T)
    g = [torch.from_numpy(a).cuda() for a in (par, draft, target, accept, recovered)]
    _check_walk(D.walk(g[1], g[2], parents=g[0]), par, draft, target, None, None, f"T {T} mode A")
    _check_walk(D.walk(g[1].long(), g[2], parents=g[0], accept=g[3], recovered=g[4]), par, draft, target, accept, recovered, f"T {T} mode B")
    _check_walk(D.walk(g[1], g[2], parents=g[0][3]), par[3], draft, target, None, None, f"T {T} shared tree")
    _check_walk(D.walk(g[1], g[2], accept=g[3], recovered=g[4]), None, draft, target, accept, recovered, f"T {T} chain")
    _check_walk(D.walk(g[1], g[2][:, 0].contiguous(), accept=g[3], recovered=g[4]), None, draft, target[:, 0], accept, recovered,
                f"T {T} chain, one bonus id")
    wild = par.copy()
    wild[:, 1:] = np.where(np.random.default_rng(T + 1).random((B, T - 1)) < 0.3, T + 5, wild[:, 1:])     # >= t: padding
    _check_walk(D.walk(g[1], g[2], parents=torch.from_numpy(wild).cuda()), wild, draft, target, None, None, f"T {T} wild parents")


def test_walk_named_cases():
    D = _D()
    draft = _i32([[9, 5, 6, 7, 8]] * 5)
    tgt = _i32([[5, 6, 7, 8, 42]] * 5)
    # mode A on the chain: everything matches - the bonus token is emitted, T tokens in all
    out = D.walk(draft, tgt)
    assert out[0][0].tolist() == [5, 6, 7, 8, 42] and out[1][0].item() == 5 and out[2][0].tolist() == [0, 1, 2, 3, 4]
    # mode B: a fully accepted chain, a reject at node 1, a reject in the middle
    acc = _i32([[0, 1, 1, 1, 1], [0, 0, 1, 1, 1], [0, 1, 1, 0, 1], [0, 1, 1, 1, 1], [0, 1, 1, 1, 1]])
    rec = _i32([[-1, 11, 12, 13, 14]] * 5)
    toks, num, path = D.walk(draft, tgt, accept=acc, recovered=rec)
    assert toks[0].tolist() == [5, 6, 7, 8, 42] and num[0].item() == 5 and path[0].tolist() == [0, 1, 2, 3, 4]
    assert toks[1].tolist() == [11, -1, -1, -1, -1] and num[1].item() == 1 and path[1].tolist() == [0, -1, -1, -1, -1]
    assert toks[2].tolist() == [5, 6, 13, -1, -1] and num[2].item() == 3 and path[2].tolist() == [0, 1, 2, -1, -1]
    # siblings: mode A takes the lowest-index child that matches; mode B looks at the first child only
    par = _i32([-1, 0, 0, 0, 2])
    d2 = _i32([[9, 4, 5, 5, 6]])
    t2 = _i32([[5, 0, 6, 0, 77]])
    toks, num, path = D.walk(d2, t2, parents=par)
    assert toks[0].tolist() == [5, 6, 77, -1, -1] and num[0].item() == 3 and path[0].tolist() == [0, 2, 4, -1, -1]
    toks, num, path = D.walk(d2, t2, parents=par, accept=_i32([[0, 0, 1, 1, 1]]), recovered=_i32([[-1, 31, 32, 33, 34]]))
    assert toks[0].tolist() == [31, -1, -1, -1, -1] and path[0].tolist() == [0, -1, -1, -1, -1]      # node 1 rejected: 2, 3 ignored
    toks, num, path = D.walk(d2, t2, parents=par, accept=_i32([[0, 1, 0, 0, 0]]), recovered=_i32([[-1, 31, 32, 33, 34]]))
    assert toks[0].tolist() == [4, 0, -1, -1, -1] and num[0].item() == 2 and path[0].tolist() == [0, 1, -1, -1, -1]   # node 1 has no child: its bonus
    # a target id of -1 is emitted and ends the walk
    toks, num, _ = D.walk(_i32([[9, -1, 3]]), _i32([[-1, 5, 5]]))
    assert toks[0].tolist() == [-1, -1, -1] and num[0].item() == 1


def test_verify_end_to_end():
    """mode A on a chain equals sample.sample on the same rows followed by the reference walk; mode B on the reference's batch
    (its tree, and request 0 alone as a chain) equals the reference walk over the planted decisions and the sampled target ids"""
    D = _D()
    import flash_attn_mi355.sample as S
    B, T, V = 3, 5, 264
    target = torch.stack([torch.stack([R.randn_row(V, torch.bfloat16, seed=10 * b + t, spread=3.0) for t in range(T)]) for b in range(B)]).cuda()
    temp = torch.tensor([0.8, 0.0, 1.2], device="cuda")
    u = torch.rand(B, T, generator=torch.Generator().manual_seed(1)).cuda()
    ids = S.sample(target, temperature=temp.repeat_interleave(T), u=u).cpu()
    draft = torch.zeros(B, T, dtype=torch.int64)
    draft[:, 1:] = ids[:, :-1]
    draft[1, 3] = (draft[1, 3] + 1) % V                              # request 1 stops at node 3, request 2 at node 1
    draft[2, 1] = (draft[2, 1] + 1) % V
    out = D.verify(target, draft.cuda(), temperature=temp, u_sample=u)
    torch.cuda.synchronize()
    _check_walk(out, None, draft.tolist(), ids.tolist(), None, None, "mode A")
    assert out[1].tolist() == [5, 3, 1]
    c = SR.batch_case(V, torch.bfloat16, torch.float32)
    g = _cuda(c)
    us = torch.rand(3, 5, generator=torch.Generator().manual_seed(2)).cuda()
    ids = S.sample(g["target"], temperature=g["temperature"].repeat_interleave(5), u=us).cpu()
    out = D.verify(g["target"], g["draft_ids"], draft_probs=g["draft"], parents=g["parents"], temperature=g["temperature"],
                   u_sample=us, u_accept=g["u_accept"], u_recover=g["u_recover"])
    _check_walk(out, c["parents"].numpy(), c["draft_ids"].tolist(), ids.tolist(), c["accept"].tolist(), c["recovered"].tolist(), "mode B")
    out = D.verify(g["target"][:1], g["draft_ids"][:1], draft_probs=g["draft"][:1], temperature=1.0, u_sample=us[:1],
                   u_accept=g["u_accept"][:1], u_recover=g["u_recover"][:1])
    _check_walk(out, None, c["draft_ids"][:1].tolist(), ids[:1, 4].tolist(), c["accept"][:1].tolist(), c["recovered"][:1].tolist(),
                "mode B chain")
    # drawn uniform numbers: the generator decides, and the same seed gives the same step
    gen = torch.Generator(device="cuda")
    a = D.verify(g["target"], g["draft_ids"], draft_probs=g["draft"], parents=g["parents"], generator=gen.manual_seed(7))
    b = D.verify(g["target"], g["draft_ids"], draft_probs=g["draft"], parents=g["parents"], generator=gen.manual_seed(7))
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and (a[1] >= 1).all() and (a[1] <= 5).all()


@pytest.mark.parametrize("V", [8193, 49153])
def test_invariance_repeatability_and_workspace_fills(V, monkeypatch):
    """the same call twice gives the same bits; a request alone gives the bits it has inside the batch; the workspace arriving
    zeroed, 0xFF or random changes nothing, and exactly the queried bytes are asked for"""
    D = _D()
    c = SR.batch_case(V, torch.bfloat16, torch.float32)
    g = _cuda(c)
    g["u_accept"] = torch.rand(3, 5, generator=torch.Generator().manual_seed(3)).cuda()      # (no margin needed: device against device)
    g["u_recover"] = torch.rand(3, 5, generator=torch.Generator().manual_seed(4)).cuda()
    run = lambda sl=slice(None), temp=None: D.accept_forward(                                  # noqa: E731
        g["target"][sl], g["draft"][sl], g["draft_ids"][sl], g["u_accept"][sl], g["u_recover"][sl], parents=g["parents"][sl],
        temperature=g["temperature"] if temp is None else temp)
    first = run()
    again = run()
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    for b in range(3):
        alone = run(slice(b, b + 1), float(c["temperature"][b]))
        assert torch.equal(alone[0], first[0][b:b + 1]) and torch.equal(alone[1], first[1][b:b + 1]), b
    from flash_attn_mi355 import flash_attn_interface as fi
    for fill in ("zeros", "ones", "random"):
        workspace, check = guard.guarded_workspace(fill)
        monkeypatch.setattr(fi, "_workspace", workspace)
        out = run()
        assert torch.equal(first[0], out[0]) and torch.equal(first[1], out[1]), fill
        assert check()["sizes"] == [SR.workspace_bytes(15, V)]


def test_commit_slots_and_move_kv_cache_on_a_paged_cache():
    """the accepted path of a walk, turned into slots by commit_slots and moved by move_kv_cache, leaves the cache the Python
    loop of the reference leaves"""
    D = _D()
    from flash_attn_mi355.kv_gather import move_kv_cache
    B, T, page, H, Dh = 3, 6, 16, 2, 64
    lens = torch.tensor([13, 0, 27], dtype=torch.int32)
    bt, nblk, _ = guard.paged_table([int(l) + T for l in lens], page, seed=3)
    gen = torch.Generator().manual_seed(0)
    kc = torch.randn(nblk, page, H, Dh, generator=gen).half()
    vc = torch.randn(nblk, page, H, Dh, generator=gen).half()
    par, draft, target, accept, recovered = _random_walk_inputs(T, B, seed=12)
    accept[:, 1:] = 1
    accept[1, 2:] = 0
    path = D.walk(torch.from_numpy(draft).cuda(), torch.from_numpy(target).cuda(), parents=torch.from_numpy(par).cuda(),
                  accept=torch.from_numpy(accept).cuda(), recovered=torch.from_numpy(recovered).cuda())[2]
    src, dst = D.commit_slots(path, lens.cuda(), block_table=bt.cuda(), page_block_size=page)
    want_src, want_dst = SR.commit_ref(path.cpu().tolist(), lens.tolist(), block_table=bt.tolist(), page_block_size=page)
    assert (src.tolist(), dst.tolist()) == (want_src, want_dst) and sum(s >= 0 for s in want_src) > B
    kg, vg = kc.cuda(), vc.cuda()
    move_kv_cache(kg, vg, src, dst)
    torch.cuda.synchronize()
    for cache, got in ((kc, kg), (vc, vg)):
        flat = cache.reshape(nblk * page, H, Dh)
        rows = [flat[s].clone() for s in want_src]                   # (every read before any write)
        want = flat.clone()
        for r, d in zip(rows, want_dst):
            if d >= 0:
                want[d] = r
        assert torch.equal(guard.bits(got.cpu().reshape(nblk * page, H, Dh)), guard.bits(want))


@pytest.mark.parametrize("tdtype,qdtype", [(torch.bfloat16, torch.float32), (torch.float32, torch.float16)])
def test_guard_bands(tdtype, qdtype):
    """target_logits and draft_probs are views inside NaN-filled slabs with gaps between the rows, every int32 / fp32 array sits
    exactly sized between bands, the workspace has exactly the queried size between sentinel bands and arrives filled with 0xFF:
    nothing outside a tensor's elements is written, no NaN of a gap reaches an output, the inputs are unchanged and the results are
    the unguarded call's - for both kernels"""
    D = _D()
    from flash_attn_mi355 import _lib
    from flash_attn_mi355 import flash_attn_interface as fi
    codes = {torch.float16: _lib.FA_FP16, torch.bfloat16: _lib.FA_BF16, torch.float32: _lib.FA_FP32}
    V = 16385
    c = SR.batch_case(V, tdtype, qdtype)
    g = _cuda(c)
    B, T = 3, 5
    want = D.accept_forward(g["target"], g["draft"], g["draft_ids"], g["u_accept"], g["u_recover"], parents=g["parents"],
                            temperature=g["temperature"])
    tids = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(5), dtype=torch.int32).cuda()
    want_walk = D.walk(g["draft_ids"], tids, parents=g["parents"], accept=want[0], recovered=want[1])
    band = 4096

    def banded(t):
        it = guard._INT_OF.get(t.dtype, t.dtype)
        buf = torch.full((band + t.numel() + band,), -1, dtype=it, device="cuda").view(t.dtype)
        view = buf[band:band + t.numel()]
        view.copy_(t.reshape(-1))
        return buf, view

    def holds(buf, n, name):
        b = buf.view(guard._INT_OF.get(buf.dtype, buf.dtype))
        assert bool((b[:band] == -1).all()) and bool((b[band + n:] == -1).all()), f"{name}: written outside its {n} elements"

    xb, x, xsnap = guard.guarded(g["target"].reshape(B * T, V), gaps=True)
    qb, q, qsnap = guard.guarded(g["draft"].reshape(B * T, V), gaps=True)
    ins = {n: banded(g[n]) for n in ("draft_ids", "parents", "u_accept", "u_recover", "temperature")}
    ins["target_ids"] = banded(tids)
    outs = {n: banded(torch.zeros(B * T, dtype=torch.int32)) for n in ("accept", "recovered", "out_tokens", "path_nodes")}
    outs["num_out"] = banded(torch.zeros(B, dtype=torch.int32))
    s = _lib.FaSpecAcceptParams()
    s.struct_size = ctypes.sizeof(_lib.FaSpecAcceptParams)
    s.target_logits, s.logits_row_stride = x.data_ptr(), x.stride(0)
    s.draft_probs, s.probs_row_stride = q.data_ptr(), q.stride(0)
    for n in ("draft_ids", "parents", "u_accept", "u_recover", "temperature"):
        setattr(s, n, ins[n][1].data_ptr())
    s.accept, s.recovered = outs["accept"][1].data_ptr(), outs["recovered"][1].data_ptr()
    s.parents_batch_stride, s.batch, s.nodes, s.vocab = T, B, T, V
    s.dtype, s.probs_dtype = codes[tdtype], codes[qdtype]
    nbytes = _lib.spec_accept_workspace_bytes(s)
    assert nbytes == SR.workspace_bytes(B * T, V) > 0
    workspace, check_ws = guard.guarded_workspace("ones")           # (0xFF: a partial read before it is written would show)
    wsp = workspace(nbytes, x.device)
    s.workspace, s.workspace_bytes = wsp.data_ptr(), nbytes
    _lib.call_spec_accept(s, fi._stream(x.device))
    w = _lib.FaSpecWalkParams()
    w.struct_size = ctypes.sizeof(_lib.FaSpecWalkParams)
    for n in ("parents", "draft_ids", "target_ids"):
        setattr(w, n, ins[n][1].data_ptr())
    for n in ("accept", "recovered", "out_tokens", "num_out", "path_nodes"):
        setattr(w, n, outs[n][1].data_ptr())
    w.parents_batch_stride = w.target_ids_batch_stride = T
    w.target_ids_node_stride, w.batch, w.nodes = 1, B, T
    _lib.call_spec_walk(w, fi._stream(x.device))
    torch.cuda.synchronize()
    assert check_ws()["sizes"] == [nbytes]
    assert torch.equal(guard.bits(xb), xsnap) and torch.equal(guard.bits(qb), qsnap), "an input was written"
    for n, (buf, view) in list(ins.items()) + list(outs.items()):
        holds(buf, view.numel(), n)
    assert torch.equal(outs["accept"][1].view(B, T), want[0]) and torch.equal(outs["recovered"][1].view(B, T), want[1])
    assert torch.equal(want[0].cpu(), c["accept"]) and torch.equal(want[1].cpu(), c["recovered"])
    assert torch.equal(outs["out_tokens"][1].view(B, T), want_walk[0]) and torch.equal(outs["num_out"][1], want_walk[1])
    assert torch.equal(outs["path_nodes"][1].view(B, T), want_walk[2])


def test_opcheck_on_the_torch_ops():
    """torch.ops.flash_attn_mi355.spec_accept / .spec_walk / .spec_verify pass torch.library.opcheck in both modes"""
    _D()
    import flash_attn_mi355.torch_ops  # noqa: F401  (registers the ops)
    g = _cuda(SR.batch_case(264, torch.bfloat16, torch.float32))
    us = torch.rand(3, 5, device="cuda")
    ns = torch.ops.flash_attn_mi355
    torch.library.opcheck(ns.spec_accept.default, (g["target"], g["draft"], g["draft_ids"], g["u_accept"], g["u_recover"],
                                                   g["parents"], g["temperature"], 1.0))
    torch.library.opcheck(ns.spec_accept.default, (g["target"], g["draft"], g["draft_ids"], g["u_accept"], g["u_recover"], None,
                                                   None, 0.8))
    acc, rec = ns.spec_accept(g["target"], g["draft"], g["draft_ids"], g["u_accept"], g["u_recover"], g["parents"], None, 1.0)
    torch.library.opcheck(ns.spec_walk.default, (g["draft_ids"], g["draft_ids"], g["parents"], acc, rec))
    torch.library.opcheck(ns.spec_walk.default, (g["draft_ids"], g["draft_ids"], None, None, None))
    torch.library.opcheck(ns.spec_verify.default, (g["target"], g["draft_ids"], g["draft"], g["parents"], g["temperature"], 1.0, us,
                                                   g["u_accept"], g["u_recover"]))
    torch.library.opcheck(ns.spec_verify.default, (g["target"], g["draft_ids"], None, None, None, 0.7, us, None, None))


@pytest.mark.parametrize("V", [264, 20001])
def test_graph_capture(V):
    """a capture of `verify` in mode B (V = 20001: two chunks) replays with fresh uniform numbers and matches the eager call"""
    D = _D()
    g = _cuda(SR.batch_case(V, torch.bfloat16, torch.float32) if V == 264 else _plain_case(V))
    us, ua, ur = (torch.full((3, 5), 0.25, device="cuda") for _ in range(3))
    kw = dict(draft_probs=g["draft"], parents=g["parents"], temperature=g["temperature"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        D.verify(g["target"], g["draft_ids"], u_sample=us, u_accept=ua, u_recover=ur, **kw)          # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = D.verify(g["target"], g["draft_ids"], u_sample=us, u_accept=ua, u_recover=ur, **kw)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(3):
        fresh = [torch.rand(3, 5, device="cuda", generator=gen) for _ in range(3)]
        for dst, src in zip((us, ua, ur), fresh):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        eager = D.verify(g["target"], g["draft_ids"], u_sample=fresh[0], u_accept=fresh[1], u_recover=fresh[2], **kw)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))


def _plain_case(V):
    """seeded rows without planted decisions (device against device): bf16 logits, fp32 softmax draft rows, tree_parents"""
    gen = torch.Generator().manual_seed(V)
    target = (torch.randn(3, 5, V, generator=gen) * 3).bfloat16()
    draft = torch.softmax(torch.randn(3, 5, V, generator=gen) * 3, -1)
    ids = torch.randint(0, V, (3, 5), generator=gen, dtype=torch.int32)
    return dict(target=target, draft=draft, draft_ids=ids, parents=torch.from_numpy(SR.tree_parents(5)),
                temperature=torch.tensor([1.0, 0.7, 0.0]))
