"""GPU: the dense, varlen and KV-cache entry points against what the reference's host C++ check functions returned
(`cpu_attention_forward`: O and LSE; `cpu_attention_backward`: dQ, dK, dV), stored in tests/golden/hostcpp_*.npz by
tests/golden/make_golden.py.  The fixtures' inputs are exact in fp16 and bf16, so both kernel dtypes see the very numbers
the C++ saw.  Only tests/golden/ is read.

Gates: the calibrated ones of tests/util.py as the dense tests pass them - mult 1.0 for O, 2.0 for gradients, LSE_ATOL for
the LSE - so FA_TOL_LOG records what is achieved.
"""
import functools
import glob
import os

import numpy as np
import pytest
import torch

from util import DT, LSE_ATOL, assert_close, assert_lse_close, f64, rand16

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "hostcpp_*.npz")))
DTYPES = ["fp16", "bf16"]


def _fa():
    import flash_attn
    return flash_attn


@functools.lru_cache(maxsize=None)
def _load(name):
    """One fixture, read once and never written: 2-D arrays q, do, o, dq [M, D], k, v, dk, dv [N, D], lse [M]."""
    g = np.load(os.path.join(GOLD, name))
    d = {n: g[n][0, 0] for n in ("q", "k", "v", "do", "o", "lse", "dq", "dk", "dv")}
    for a in d.values():
        a.setflags(write=False)
    d["scale"], d["causal"] = float(g["scale"]), bool(g["causal"])
    d["M"], d["N"], d["D"] = d["q"].shape[0], d["k"].shape[0], d["q"].shape[1]
    return d


def _dev(a, dt):
    """[rows, D] fixture array -> [rows, 1 head, D] on the GPU in the kernel dtype (an exact conversion)"""
    return torch.from_numpy(np.array(a)).to(DT[dt]).cuda()[:, None, :]


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")


def _named(*names):
    assert set(names) <= set(FIXTURES), names
    return list(names)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", FIXTURES)
def test_dense_fwd_bwd(name, dt):
    g = _load(name)
    q, k, v = (_dev(g[n], dt)[None].requires_grad_(True) for n in ("q", "k", "v"))     # [1, S, 1, D]
    out, lse, _ = _fa().flash_attn_func(q, k, v, softmax_scale=g["scale"], causal=g["causal"], return_attn_probs=True)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), _dev(g["do"], dt)[None])
    assert_close(f64(out)[0, :, 0], g["o"], dt, "out", mult=1.0)
    assert_lse_close(f64(lse)[0, 0], g["lse"], "lse", atol=LSE_ATOL)
    assert_close(f64(dq)[0, :, 0], g["dq"], dt, "dq", mult=2.0)
    assert_close(f64(dk)[0, :, 0], g["dk"], dt, "dk", mult=2.0)
    assert_close(f64(dv)[0, :, 0], g["dv"], dt, "dv", mult=2.0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", FIXTURES)
def test_varlen_fwd(name, dt):
    """Causal fixture: its prefixes of lengths (M, 1, 33, M - 1) as the sequences of one call - the rows of a prefix of a
    square causal problem are the rows of the whole problem.  Non-causal fixture: query subsets of lengths (M, 1, 17)
    against all N keys."""
    g = _load(name)
    M, N = g["M"], g["N"]
    if g["causal"]:
        rows = [np.arange(L) for L in (M, 1, 33, M - 1)]
        lens_k = [len(r) for r in rows]
        k = torch.cat([_dev(g["k"][:L], dt) for L in lens_k])
        v = torch.cat([_dev(g["v"][:L], dt) for L in lens_k])
    else:
        rows = [np.arange(M), np.array([M // 2]), np.arange(max(M - 17, 0), M)]      # (M = 1: three times the one row)
        lens_k = [N] * len(rows)
        k = torch.cat([_dev(g["k"], dt)] * len(rows))
        v = torch.cat([_dev(g["v"], dt)] * len(rows))
    idx = np.concatenate(rows)
    lens_q = [len(r) for r in rows]
    q = _dev(g["q"][idx], dt)
    out, lse, _ = _fa().flash_attn_varlen_func(q, k, v, _cu(lens_q), _cu(lens_k), max(lens_q), max(lens_k),
                                               softmax_scale=g["scale"], causal=g["causal"], return_attn_probs=True)
    assert out.shape == q.shape and lse.shape == (1, len(idx))
    assert_close(f64(out)[:, 0], g["o"][idx], dt, "out", mult=1.0)
    assert_lse_close(f64(lse)[0], g["lse"][idx], "lse", atol=LSE_ATOL)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", FIXTURES)
def test_varlen_bwd_between_decoys(name, dt):
    """The fixture between two decoy sequences of other lengths (random inputs and dO): its rows of O, LSE, dQ, dK and dV
    are the fixture's."""
    g = _load(name)
    M, N, D = g["M"], g["N"], g["D"]
    lens_q, lens_k = [37, M, 21], [37, N, 150]
    mk = lambda n, rows, seed: torch.cat([rand16((rows[0], 1, D), dt, seed), _dev(g[n], dt), rand16((rows[2], 1, D), dt, seed + 1)])
    q, k, v = mk("q", lens_q, 11).requires_grad_(True), mk("k", lens_k, 13).requires_grad_(True), mk("v", lens_k, 15).requires_grad_(True)
    do = mk("do", lens_q, 17)
    out, lse, _ = _fa().flash_attn_varlen_func(q, k, v, _cu(lens_q), _cu(lens_k), max(lens_q), max(lens_k),
                                               softmax_scale=g["scale"], causal=g["causal"], return_attn_probs=True)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), do)
    sq, sk = slice(37, 37 + M), slice(37, 37 + N)
    assert_close(f64(out)[sq, 0], g["o"], dt, "out", mult=1.0)
    assert_lse_close(f64(lse)[0, sq], g["lse"], "lse", atol=LSE_ATOL)
    assert_close(f64(dq)[sq, 0], g["dq"], dt, "dq", mult=2.0)
    assert_close(f64(dk)[sk, 0], g["dk"], dt, "dk", mult=2.0)
    assert_close(f64(dv)[sk, 0], g["dv"], dt, "dv", mult=2.0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged16"])
@pytest.mark.parametrize("name", _named("hostcpp_M77N300D128_c0.npz", "hostcpp_M1N65D64_c0.npz"))
def test_kvcache_prefilled(name, paged, splits, dt):
    """The cache holds K and V (rows behind cache_seqlens = N hold other numbers), contiguous or in shuffled pages of 16."""
    g = _load(name)
    M, N, D = g["M"], g["N"], g["D"]
    page = 16
    npages = (N + page - 1) // page + 1
    kc = rand16((1, npages * page, 1, D), dt, 21)
    vc = rand16((1, npages * page, 1, D), dt, 22)
    kc[0, :N], vc[0, :N] = _dev(g["k"], dt), _dev(g["v"], dt)
    bt = None
    if paged:
        perm = torch.randperm(npages + 2, generator=torch.Generator().manual_seed(23))[:npages]
        kp, vp = rand16((npages + 2, page, 1, D), dt, 24), rand16((npages + 2, page, 1, D), dt, 25)
        kp[perm.cuda()], vp[perm.cuda()] = kc.view(npages, page, 1, D), vc.view(npages, page, 1, D)
        kc, vc, bt = kp, vp, perm.to(torch.int32)[None].cuda()
    out, lse = _fa().flash_attn_with_kvcache(_dev(g["q"], dt)[None], kc, vc,
                                             cache_seqlens=torch.tensor([N], dtype=torch.int32, device="cuda"),
                                             block_table=bt, softmax_scale=g["scale"], causal=False, num_splits=splits,
                                             return_softmax_lse=True)
    assert_close(f64(out)[0, :, 0], g["o"], dt, "out", mult=1.0)
    assert_lse_close(f64(lse)[0, 0], g["lse"], "lse", atol=LSE_ATOL)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", _named("hostcpp_M200N200D64_c1.npz", "hostcpp_M128N128D128_c1.npz"))
def test_kvcache_append_causal(name, dt):
    """An empty cache (cache_seqlens = 0), K and V appended by the call, causal: afterwards the cache rows are K and V bit
    for bit."""
    g = _load(name)
    N, D = g["N"], g["D"]
    kc, vc = rand16((1, N + 24, 1, D), dt, 31), rand16((1, N + 24, 1, D), dt, 32)
    tail_k, tail_v = kc[0, N:].clone(), vc[0, N:].clone()
    knew, vnew = _dev(g["k"], dt)[None], _dev(g["v"], dt)[None]
    out, lse = _fa().flash_attn_with_kvcache(_dev(g["q"], dt)[None], kc, vc, k=knew, v=vnew,
                                             cache_seqlens=torch.zeros(1, dtype=torch.int32, device="cuda"),
                                             softmax_scale=g["scale"], causal=True, return_softmax_lse=True)
    assert torch.equal(kc[0, :N], knew[0]) and torch.equal(vc[0, :N], vnew[0])
    assert torch.equal(kc[0, N:], tail_k) and torch.equal(vc[0, N:], tail_v)
    assert_close(f64(out)[0, :, 0], g["o"], dt, "out", mult=1.0)
    assert_lse_close(f64(lse)[0, 0], g["lse"], "lse", atol=LSE_ATOL)
