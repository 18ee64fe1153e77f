"""GPU: what the ops do OUTSIDE the elements they are meant to produce (tests/guard.py).

  A. workspace  - every workspace the wrapper hands out is exactly the queried bytes between sentinel bands; the results are
                  bit-identical whether it arrives zeroed, as 0xFF or as random bytes; the route the case exists for was taken.
  B. tensors    - inputs and caller-owned outputs are strided views inside NaN-filled slabs: results against the oracle (the
                  gates and multipliers of the op's own test file), every byte outside the outputs untouched, inputs unchanged.
  C. C ABI      - the outputs the wrapper allocates itself (lse, softmax_d, dsinks, the kv-cache out) as slab views through
                  direct calls of the entry points and their _ext forms.
Every stray access these tests can detect lands in memory the test allocated itself."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import fp8_gate
import guard
import oracle
import sink_ref
import tree_ref as tr
from util import DT, LSE_ATOL_FP8, assert_close, assert_lse_close, f64, rand16

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn
FILLS = ("zeros", "ones", "random")


def _fa():
    import flash_attn
    return flash_attn


def _fi():
    from flash_attn_mi355 import flash_attn_interface as fi
    return fi


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")


def _rotary(seqlen_ro, rd, dt):
    pos = torch.arange(seqlen_ro, dtype=torch.float32)[:, None]
    inv = 1.0 / (10000 ** (torch.arange(0, rd, 2, dtype=torch.float32) / rd))[None, :]
    ang = pos * inv
    return torch.cos(ang).to(DT[dt]).cuda(), torch.sin(ang).to(DT[dt]).cuda()


def _unchanged(buf, snap, name):
    """an input slab: every byte, the view's own included, is what it was"""
    assert torch.equal(guard.bits(buf), snap), f"{name}: an input was written"


def _with_fills(monkeypatch, run):
    """run() once per workspace fill under a guarded _workspace: ({fill: results}, {fill: requested sizes}); the guard bands
    are checked after every run"""
    fi = _fi()
    res, sizes = {}, {}
    for fill in FILLS:
        ws, check = guard.guarded_workspace(fill)
        monkeypatch.setattr(fi, "_workspace", ws)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            res[fill] = run()
        sizes[fill] = check()["sizes"]
    assert sizes["zeros"] == sizes["ones"] == sizes["random"]
    return res, sizes["zeros"]


def _same_bits(res, names):
    for fill in FILLS[1:]:
        for name, a, b in zip(names, res["zeros"], res[fill]):
            assert torch.isfinite(a.float()).all(), f"{name}: non-finite with a zeroed workspace"
            assert torch.equal(a, b), f"{name}: differs between a zeroed workspace and one filled with '{fill}'"


# =====================================================================================================================
# A. workspace: stays inside, contents do not matter
# =====================================================================================================================
def _planes(B, Hq, Sq):
    return 2 * B * Hq * Sq * 4


DENSE_BWD_WS = [
    # id, B, Hq, Hk, Sq, Sk, D, dtype, causal, window, alibi, deterministic, wanted gradients, route
    ("asm-planes-partials", 1, 8, 2, 1100, 1100, 128, "bf16", True, (-1, -1), False, False, "qkv", "split"),
    ("asm-planes-only", 1, 8, 2, 1100, 1100, 128, "bf16", True, (-1, -1), False, True, "qkv", "planes"),
    # (11 stages per workgroup: too few to split on a 256-CU part - the planes alone, 15984 bytes; the left-window case below
    #  has the partials behind planes that are no multiple of 256 bytes)
    ("asm-odd-plane-count", 2, 3, 3, 333, 333, 128, "fp16", True, (-1, -1), False, False, "qkv", "planes"),
    ("gen2part-d64", 1, 14, 2, 900, 900, 64, "bf16", True, (-1, -1), False, False, "qkv", "split"),
    ("gen2part-d40-one-key-block", 2, 4, 4, 1500, 77, 40, "fp16", False, (-1, -1), False, False, "qkv", "split"),
    ("d256-split", 1, 4, 2, 1000, 1000, 256, "bf16", True, (-1, -1), False, False, "qkv", "split"),
    ("d256-split-192", 1, 2, 2, 900, 300, 192, "fp16", False, (-1, -1), False, False, "qkv", "split"),
    ("left-window", 1, 4, 2, 1300, 1300, 128, "bf16", False, (200, 0), False, False, "qkv", "split"),
    ("asm-alibi-no-split", 1, 4, 4, 700, 700, 128, "bf16", True, (-1, -1), True, False, "qkv", "planes"),
    ("q-only", 1, 8, 2, 1100, 1100, 128, "bf16", True, (-1, -1), False, False, "q", "planes"),
    ("kv-only", 1, 8, 2, 1100, 1100, 128, "bf16", True, (-1, -1), False, False, "kv", "split"),
]


@pytest.mark.parametrize("case", DENSE_BWD_WS, ids=lambda c: c[0])
def test_dense_backward_workspace(case, monkeypatch):
    fi = _fi()
    _, B, Hq, Hk, Sq, Sk, D, dt, causal, window, alibi, det, want, route = case
    monkeypatch.setattr(fi, "DS_HANDOFF", False)
    q, k, v = rand16((B, Sq, Hq, D), dt, 521), rand16((B, Sk, Hk, D), dt, 522), rand16((B, Sk, Hk, D), dt, 523)
    do = rand16((B, Sq, Hq, D), dt, 524)
    slopes = (2.0 ** (-8.0 * (torch.arange(Hq) + 1) / Hq)).float().cuda() if alibi else None

    def run(deterministic=det):
        ins = [t.detach().clone().requires_grad_(n in want) for t, n in ((q, "q"), (k, "kv"), (v, "kv"))]
        out = _fa().flash_attn_func(*ins, causal=causal, window_size=window, alibi_slopes=slopes, deterministic=deterministic)
        return torch.autograd.grad(out, [t for t in ins if t.requires_grad], do)

    res, sizes = _with_fills(monkeypatch, run)
    _same_bits(res, [f"grad {i}" for i in range(3)])
    assert len(sizes) == 1
    planes = _planes(B, Hq, Sq) if D == 128 else 0
    if route == "planes":                                    # the statistics planes alone, exactly
        assert sizes[0] == planes > 0
    else:                                                    # partial slabs on top of what the unsplit call asks for
        _, unsplit = _with_fills(monkeypatch, lambda: run(True))
        assert sizes[0] > unsplit[0] and unsplit[0] == planes
        if planes:
            assert sizes[0] > (planes + 255) // 256 * 256   # (the partials lie 256-byte aligned behind the planes)
    if want == "q":                                          # the plan differs with the gradients wanted
        monkeypatch.setattr(fi, "_workspace", lambda n, dev: None)
        assert torch.equal(run()[0], res["zeros"][0])        # (the dQ kernel is the same one without the planes)


@pytest.mark.parametrize("case", [(8, 8, 8, 200, 500, "bf16", False), (8, 8, 8, 200, 1000, "fp16", True)],
                         ids=lambda c: "-".join(map(str, c)))
def test_ds_handoff_workspace(case, monkeypatch):
    """The opt-in dS hand-off (FA_FLAG_DS_HANDOFF): launches that fill the chip (256 workgroups: no split) store packed dS tiles of
    32 x 32 behind the statistics planes, a one-GEMM dQ kernel reads them back; ragged last row tile and key block."""
    fi = _fi()
    B, Hq, Hk, Sq, Sk, dt, causal = case
    D = 128
    monkeypatch.setattr(fi, "DS_HANDOFF", True)
    q, k, v = rand16((B, Sq, Hq, D), dt, 811), rand16((B, Sk, Hk, D), dt, 812), rand16((B, Sk, Hk, D), dt, 813)
    do = rand16((B, Sq, Hq, D), dt, 814)

    def run():
        ins = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
        return torch.autograd.grad(_fa().flash_attn_func(*ins, causal=causal), ins, do)

    res, sizes = _with_fills(monkeypatch, run)
    _same_bits(res, ("dq", "dk", "dv"))
    tiles = B * Hq * ((Sq + 31) // 32) * 4 * ((Sk + 127) // 128) * 2048
    assert sizes == [(_planes(B, Hq, Sq) + 255) // 256 * 256 + tiles], "the hand-off did not run (planes + dS tiles)"


VARLEN_BWD_WS = [
    # lens_q, lens_k, Hq, Hk, D, dtype, route.  A packed launch splits when its flat list of key blocks x kv-heads leaves the chip
    # underfilled and the average pass keeps >= 8 stages x q-heads per split (fa_bwd.hip: dkv_split_factor): one kv-head with a
    # group of 8 does at these lengths; the same lengths at 4 / 2 heads do not (the statistics planes alone).
    ([300, 0, 77, 513], None, 8, 1, 128, "bf16", "split"),                # hand-scheduled kernel: planes + partials
    ([300, 0, 77, 513], None, 8, 1, 64, "fp16", "split"),                 # Gen2Part: partials at offset 0
    ([513, 64, 1], [77, 300, 129], 8, 1, 128, "bf16", "split"),           # lens_q != lens_k
    ([300, 0, 77, 513], None, 4, 2, 128, "bf16", "planes"),
    ([900, 1300, 257], None, 8, 1, 128, "bf16", "split"),                 # 8 splits, a one-row key block at the packed tensor's end
    ([2048, 3, 0, 1400], None, 8, 2, 64, "fp16", "split"),                # empty and tiny sequences next to long ones
    ([1200, 900], None, 4, 2, 256, "bf16", "split"),                      # head dim 256: each role stores its partial
]


@pytest.mark.parametrize("case", VARLEN_BWD_WS, ids=lambda c: "-".join(map(str, c)))
def test_varlen_backward_workspace(case, monkeypatch):
    """The flat work lists: fp32 dK / dV partial slabs of [total_k, Hk, D] rows per split, filled by 128-key blocks that end
    ragged at every sequence's tail - the reduction skips rows past the last sequence, so only the bands can show an overrun."""
    lens_q, lens_k, Hq, Hk, D, dt, route = case
    lens_k = lens_k or lens_q
    Tq, Tk = sum(lens_q), sum(lens_k)
    q, k, v = rand16((Tq, Hq, D), dt, 61), rand16((Tk, Hk, D), dt, 62), rand16((Tk, Hk, D), dt, 63)
    do = rand16((Tq, Hq, D), dt, 64)
    cu_q, cu_k = _cu(lens_q), _cu(lens_k)

    def run(deterministic=False):
        ins = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
        out = _fa().flash_attn_varlen_func(*ins, cu_q, cu_k, max(lens_q), max(lens_k), causal=True, deterministic=deterministic)
        return torch.autograd.grad(out, ins, do)

    res, sizes = _with_fills(monkeypatch, run)
    _same_bits(res, ("dq", "dk", "dv"))
    # (the forward asks too - for nothing: no paged K / V); the backward's request is the last one
    assert len(sizes) == 2 and sizes[0] == 0
    planes = 2 * Hq * Tq * 4 if D == 128 else 0              # [H][total_q] statistics planes of the hand-scheduled kernels
    unsplit_res, unsplit = _with_fills(monkeypatch, lambda: run(True))     # the public switch (FA_FLAG_NO_DKV_SPLIT)
    assert unsplit[-1] == planes
    if route == "planes":
        assert sizes[-1] == planes > 0
    else:
        assert sizes[-1] > unsplit[-1], "the packed launch did not split: the partial slabs are not covered"
        slabs = sizes[-1] - (planes + 255) // 256 * 256      # 2 x splits x total_k x Hk x D floats, 256-byte aligned behind the planes
        per_split = 2 * Tk * Hk * D * 4
        assert slabs % per_split == 0 and slabs // per_split >= 2
        assert torch.equal(res["zeros"][0], unsplit_res["zeros"][0])      # dq: the same kernel with or without the split
    # and run-to-run repeatable
    again, _ = _with_fills(monkeypatch, run)
    for a, b in zip(res["zeros"], again["random"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", [(1, 32, 32, 1900, 1900), (1, 16, 16, 2048, 3000)], ids=lambda c: "-".join(map(str, c)))
def test_forward_key_split_workspace(case, monkeypatch):
    fi = _fi()
    B, Hq, Hk, Sq, Sk = case
    D, dt = 128, "bf16"
    q, k, v = rand16((B, Sq, Hq, D), dt, 31), rand16((B, Sk, Hk, D), dt, 32), rand16((B, Sk, Hk, D), dt, 33)
    monkeypatch.setattr(fi, "FWD_SPLIT", True)
    res, sizes = _with_fills(monkeypatch, lambda: _fa().flash_attn_func(q, k, v, causal=True, return_attn_probs=True)[:2])
    _same_bits(res, ("out", "lse"))
    assert len(sizes) == 1 and sizes[0] > 0, "the key split did not run (it asks for its partial buffers)"
    monkeypatch.setattr(fi, "FWD_SPLIT", False)
    out, lse, _ = _fa().flash_attn_func(q, k, v, causal=True, return_attn_probs=True)
    assert_close(f64(res["zeros"][0]), f64(out), dt, "split vs unsplit")
    assert_lse_close(f64(res["zeros"][1]), f64(lse), "lse split vs unsplit")


def _kv_setup(B, Hk, D, dt, Smax, lens, Tn, page, fp8, seed=0):
    """contiguous caches, or paged ones; fp8 with descales.  Only the `lens` keys each sequence holds are data: the rows behind
    them (the Tn the call appends included), page tails, spare pages and the page that the table's unreferenced entries point
    at hold NaN, so a read past cache_seqlens + Tn or through a stale table entry reaches the result as NaN."""
    scale = 1.5 if fp8 else 1.0
    if page:
        bt, nblk, _ = guard.paged_table([l + Tn for l in lens], page, width=Smax // page, seed=seed)
        shape = (nblk, page, Hk, D)
        valid = torch.zeros(shape[:2], dtype=torch.bool)
        for b, l in enumerate(lens):
            for j in range((l + page - 1) // page):
                valid[int(bt[b, j]), :min(page, l - j * page)] = True
    else:
        bt, shape = None, (B, Smax, Hk, D)
        valid = torch.arange(Smax)[None, :] < torch.tensor(lens)[:, None]
    valid = valid.cuda()
    kd, vd = (0.05, 0.04) if fp8 else (None, None)
    caches = []
    for i, desc in enumerate((kd, vd)):
        data = rand16(shape, dt, 2 + i + seed, scale=scale)
        if fp8:
            data = (data.float() / desc).to(FP8)
        c = guard.fill_nan(torch.empty_like(data))
        guard.bits(c)[valid] = guard.bits(data)[valid]
        caches.append(c)
    return caches[0], caches[1], bt, kd, vd


KV_WS = (
    # id, Tq, Hq, Hk, D, fp8, paged, extra
    [(f"d{D}", 1, 8, 2, D, False, False, None) for D in (64, 96, 128, 256)] +
    [("d128-paged", 1, 8, 2, 128, False, True, None),
     ("tq5-one-row-block", 5, 8, 2, 128, False, False, None),
     ("tq5-paged", 5, 8, 2, 128, False, True, None),
     ("tq70-ragged-fifth-block", 70, 4, 2, 128, False, False, None),
     ("tq70-paged", 70, 4, 2, 128, False, True, None),
     ("fp8-token-major", 1, 16, 8, 128, True, False, None),
     ("fp8-token-major-paged", 1, 16, 8, 128, True, True, None),
     ("fp8-head-per-wave", 2, 32, 8, 128, True, False, None),
     ("fp8-head-per-wave-paged", 2, 32, 8, 128, True, True, None),
     ("tree", 7, 8, 2, 128, False, False, "tree"),
     ("tree-rotary", 7, 8, 2, 128, False, True, "tree-rotary"),
     ("sinks", 1, 8, 2, 128, False, False, "sinks")])


@pytest.mark.parametrize("nsplit", [0, 3, 5])
@pytest.mark.parametrize("case", KV_WS, ids=lambda c: c[0])
def test_kvcache_decode_workspace(case, nsplit, monkeypatch):
    fi = _fi()
    _, Tq, Hq, Hk, D, fp8, paged, extra = case
    B, Smax, dt = 3, 1024, "bf16"
    lens = [777, 1, 1000 - Tq]
    kc, vc, bt, kd, vd = _kv_setup(B, Hk, D, dt, Smax, lens, Tq, 128 if paged else 0, fp8)
    q = rand16((B, Tq, Hq, D), dt, 1)
    knew, vnew = rand16((B, Tq, Hk, D), dt, 4), rand16((B, Tq, Hk, D), dt, 5)
    kw = dict(causal=True)
    if extra and extra.startswith("tree"):
        rng = np.random.default_rng(5)
        pars = [tr.random_parents(Tq, rng) for _ in range(B)]
        kw = dict(tree_mask=torch.from_numpy(np.stack([tr.mask_from_parents(p) for p in pars])).cuda())
        if extra == "tree-rotary":
            cos, sin = _rotary(Smax + 24, D, dt)
            depths = torch.from_numpy(np.stack([tr.depths_from_parents(p) for p in pars]).astype(np.int32)).cuda()
            kw.update(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False, tree_depths=depths)
    if extra == "sinks":
        kw["sinks"] = torch.tensor([0.5 * h - 1.0 for h in range(Hq)], dtype=torch.float32, device="cuda")
    sl = torch.tensor(lens, dtype=torch.int32).cuda()
    btc = None if bt is None else bt.cuda()

    def run():
        k1, v1 = kc.clone(), vc.clone()
        fi._KV_PLANS.clear()                                 # (the cached-plan fast path allocates its workspace directly)
        out, lse = _fa().flash_attn_with_kvcache(q, k1, v1, k=knew, v=vnew, cache_seqlens=sl, block_table=btc, num_splits=nsplit,
                                                 return_softmax_lse=True, k_descale=kd, v_descale=vd, **kw)
        return out, lse, guard.bits(k1), guard.bits(v1)      # (integer views: the caches hold NaN behind the keys)

    res, sizes = _with_fills(monkeypatch, run)
    for fill in FILLS[1:]:
        for name, a, b in zip(("out", "lse", "k_cache", "v_cache"), res["zeros"], res[fill]):
            assert torch.equal(a, b), f"{name}: differs between a zeroed workspace and one filled with '{fill}'"
    assert torch.isfinite(res["zeros"][0].float()).all(), "out: a NaN from behind a sequence's keys or a stale table entry"
    assert torch.isfinite(res["zeros"][1]).all(), "lse: a NaN from behind a sequence's keys or a stale table entry"
    per_part = B * Hq * Tq * (_fi()._padded_head_dim(D) + 1) * 4         # one partial (O row of the kernel width, LSE) per query row
    assert len(sizes) == 1 and sizes[0] > 0, "no split-KV partials were requested: the decode kernels' split path is not covered"
    # include/fa_mi355.h: splits x B x Hq x Tq x (head_dim + 1) x 4.  The token-major kernel (one query token, D 128, groups of 1 / 2,
    # kv-heads a multiple of 8 in an fp8 cache) has one head group of 8 here, so its four waves take key sub-ranges of every grid
    # split and write a partial each: x 4 (fa_decode.hip: gemv_tm_ksub)
    ksub = 4 if fp8 and Tq == 1 else 1
    if nsplit:
        assert sizes[0] == nsplit * ksub * per_part
    else:                                                    # the heuristic's count: whole partials, at least two
        assert sizes[0] % (ksub * per_part) == 0 and sizes[0] // (ksub * per_part) >= (2 if ksub == 1 else 1)


@pytest.mark.parametrize("qlens", [[1] * 5, [3] * 5, [4] * 5, [1, 3, 2, 4, 1, 300]],
                         ids=["decode-1", "decode-3", "decode-4", "mixed-with-a-prefill-chunk"])
def test_varlen_decode_route_workspace(qlens, monkeypatch):
    """Decode through the varlen op: five sequences that all bring the same 1 .. 4 query tokens (the uniform route: ragged
    counts without a long sequence stay on the general kernel, which has no workspace), and sequences of 1 .. 4 tokens next
    to a 300-token prefill chunk (the mixed route: the decode kernels in varlen-q mode + the general kernel)."""
    Hq, Hk, D, dt, page = 8, 2, 128, "bf16", 64
    B = len(qlens)
    lens_k = [max(ql, lk) for ql, lk in zip(qlens, [700, 33, 1024, 4, 257, 513])]
    bt, nblk, nan_page = guard.paged_table(lens_k, page, seed=4)
    kp, vp = rand16((nblk, page, Hk, D), dt, 11), rand16((nblk, page, Hk, D), dt, 12)
    for b, lk in enumerate(lens_k):                          # page tails and the stale entries' page: NaN
        if lk % page:
            last = int(bt[b, lk // page])
            guard.fill_nan(kp[last, lk % page:]); guard.fill_nan(vp[last, lk % page:])
    guard.fill_nan(kp[nan_page]); guard.fill_nan(vp[nan_page])
    q = rand16((sum(qlens), Hq, D), dt, 13)
    cu_q, cu_k = _cu(qlens), _cu(lens_k)
    run = lambda: _fa().flash_attn_varlen_func(q, kp, vp, cu_q, cu_k, max(qlens), max(lens_k), causal=True,
                                               return_attn_probs=True, block_table=bt.cuda())[:2]
    res, sizes = _with_fills(monkeypatch, run)
    _same_bits(res, ("out", "lse"))
    assert len(sizes) == 1 and sizes[0] > 0, "fa_varlen_fwd did not take the decode route (it asks for the split-KV partials)"
    o_ref, lse_ref = oracle.varlen_fwd(f64(q), f64(kp), f64(vp), cu_q.cpu().numpy(), cu_k.cpu().numpy(), max(qlens), max(lens_k),
                                       D ** -0.5, causal=True, block_table=bt.numpy())
    assert_close(f64(res["random"][0]), o_ref, dt, "out")
    assert_lse_close(f64(res["random"][1]), lse_ref, "lse")


# =====================================================================================================================
# B. tensors: stays inside, gaps never reach the result
# =====================================================================================================================
def _in(x, row_dim=-3):
    """an input inside a gapped slab: (buf, view, snapshot)"""
    return guard.guarded(x, gaps=True, row_dim=row_dim)


def _out(shape, dtype):
    return guard.guarded(shape=shape, dtype=dtype, gaps=True, device="cuda")


DENSE_B = ([(B, Hq, Hk, Sq, Sk, D, causal, 0.0, 0.0, False)
            for (B, Hq, Hk, Sq, Sk) in ((2, 4, 2, 77, 300), (1, 2, 2, 257, 129))
            for D in (40, 64, 96, 128, 192, 256) for causal in (False, True)] +
           [(2, 4, 2, 77, 300, 128, True, 0.2, 0.0, False),           # dropout, softcap, ALiBi [B, H]: the compiler-scheduled kernels
            (2, 4, 2, 77, 300, 64, False, 0.0, 30.0, False),
            (2, 4, 2, 77, 300, 128, True, 0.0, 0.0, True)])


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("case", DENSE_B, ids=lambda c: "-".join(map(str, c)))
def test_dense_forward_backward_in_slabs(case, dt):
    fi = _fi()
    B, Hq, Hk, Sq, Sk, D, causal, pdrop, softcap, alibi = case
    torch.manual_seed(1234)
    (qb, q, qs), (kb, k, ks), (vb, v, vs), (dob, do, dos) = (
        _in(rand16(s, dt, 421 + i)) for i, s in enumerate(((B, Sq, Hq, D), (B, Sk, Hk, D), (B, Sk, Hk, D), (B, Sq, Hq, D))))
    (ob, out, osn), (dqb, dq, dqs), (dkb, dk, dks), (dvb, dv, dvs) = (
        _out(s, DT[dt]) for s in ((B, Sq, Hq, D), (B, Sq, Hq, D), (B, Sk, Hk, D), (B, Sk, Hk, D)))
    # ([B, H] slopes: the geometric ALiBi sequence of tests/test_fwd_gpu.py, halved for the second batch entry - the LSE gate is
    #  calibrated for scores of that size, steeper slopes put the bias alone at -100 and its fp32 ulp near the gate)
    slopes = (2.0 ** (-8.0 * (torch.arange(Hq) + 1) / Hq)).float()[None, :] / (1 + torch.arange(B).float())[:, None]
    slopes = slopes.contiguous().cuda() if alibi else None
    res, lse, _, saved, rng, scale = fi._dense_forward(q, k, v, pdrop, None, causal, (-1, -1), softcap, slopes, False, out=out)
    assert res is out and all(a is b for a, b in zip(saved, (q, k, v, out))), "the wrapper copied a slab view"
    fi._dense_backward(do, q, k, v, out, lse, slopes, pdrop, scale, causal, (-1, -1), softcap, rng, dq, dk, dv)
    torch.cuda.synchronize()
    for buf, snap, name in ((qb, qs, "q"), (kb, ks, "k"), (vb, vs, "v"), (dob, dos, "dout")):
        _unchanged(buf, snap, name)
    for buf, view, snap, name in ((ob, out, osn, "out"), (dqb, dq, dqs, "dq"), (dkb, dk, dks, "dk"), (dvb, dv, dvs, "dv")):
        guard.assert_untouched(buf, view, snap, name)
    t = lambda x: f64(x).transpose(0, 2, 1, 3)
    kw = dict(causal=causal, softcap=softcap, alibi_slopes=None if slopes is None else f64(slopes))
    if pdrop:
        kw.update(dropout_p=pdrop, seed=rng[0], offset=rng[1])
    o_ref, lse_ref, _ = oracle.attn_fwd(t(q), t(k), t(v), D ** -0.5, **kw)
    g = oracle.attn_bwd(t(do), t(q), t(k), t(v), o_ref, lse_ref.astype(np.float64), D ** -0.5, **kw)
    # (multipliers: tests/test_fwd_gpu.py and test_bwd_gpu.py - 1 forward, 2 gradients; tests/test_dropout_gpu.py - 1.5 and 3)
    assert_close(t(out), o_ref, dt, "out", mult=1.5 if pdrop else 1.0)
    assert_lse_close(f64(lse), lse_ref, "lse")
    for name, got, ref in (("dq", dq, g[0]), ("dk", dk, g[1]), ("dv", dv, g[2])):
        assert_close(t(got), ref, dt, name, mult=3.0 if pdrop else 2.0)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [40, 64, 128])
def test_varlen_forward_backward_in_slabs(D, dt):
    fi = _fi()
    lens_q, lens_k, Hq, Hk = [0, 1, 77, 300], [5, 0, 129, 257], 4, 2
    Tq, Tk = sum(lens_q), sum(lens_k)
    (qb, q, qs), (kb, k, ks), (vb, v, vs), (dob, do, dos) = (
        _in(rand16(s, dt, 61 + i)) for i, s in enumerate(((Tq, Hq, D), (Tk, Hk, D), (Tk, Hk, D), (Tq, Hq, D))))
    (ob, out, osn), (dqb, dq, dqs), (dkb, dk, dks), (dvb, dv, dvs) = (
        _out(s, DT[dt]) for s in ((Tq, Hq, D), (Tq, Hq, D), (Tk, Hk, D), (Tk, Hk, D)))
    cu_q, cu_k = _cu(lens_q), _cu(lens_k)
    mq, mk = max(lens_q), max(lens_k)
    res, lse, _, saved, rng, scale = fi._varlen_forward(q, k, v, cu_q, cu_k, mq, mk, 0.0, None, True, (-1, -1), 0.0, None, False,
                                                        None, out=out)
    assert res is out and all(a is b for a, b in zip(saved[:4], (q, k, v, out))), "the wrapper copied a slab view"
    fi._varlen_backward(do, q, k, v, out, lse, cu_q, cu_k, None, mq, mk, 0.0, scale, True, (-1, -1), 0.0, rng, dq, dk, dv)
    torch.cuda.synchronize()
    for buf, snap, name in ((qb, qs, "q"), (kb, ks, "k"), (vb, vs, "v"), (dob, dos, "dout")):
        _unchanged(buf, snap, name)
    for buf, view, snap, name in ((ob, out, osn, "out"), (dqb, dq, dqs, "dq"), (dkb, dk, dks, "dk"), (dvb, dv, dvs, "dv")):
        guard.assert_untouched(buf, view, snap, name)
    cq, ck = cu_q.cpu().numpy(), cu_k.cpu().numpy()
    o_ref, lse_ref = oracle.varlen_fwd(f64(q), f64(k), f64(v), cq, ck, mq, mk, D ** -0.5, causal=True)
    g = oracle.varlen_bwd(f64(do), f64(q), f64(k), f64(v), o_ref, lse_ref.astype(np.float64), cq, ck, mq, mk, D ** -0.5, causal=True)
    assert_close(f64(out), o_ref, dt, "out")
    assert_lse_close(f64(lse), lse_ref, "lse")
    for name, got, ref in (("dq", dq, g[0]), ("dk", dk, g[1]), ("dv", dv, g[2])):
        assert_close(f64(got), ref, dt, name, mult=2.0)


@pytest.mark.parametrize("page", [16, 256])
def test_varlen_paged_forward_in_slabs(page):
    fi = _fi()
    lens_q, lens_k, Hq, Hk, D, dt = [70, 1, 300], [200, 513, 300], 4, 2, 128, "fp16"
    bt, nblk, nan_page = guard.paged_table(lens_k, page, seed=5)
    pages = [torch.full((nblk, page, Hk, D), float("nan"), dtype=DT[dt]) for _ in range(2)]
    for i, pg in enumerate(pages):                           # valid rows only: page tails, spare pages and the NaN page stay NaN
        data = rand16((nblk, page, Hk, D), dt, 11 + i, device="cpu")
        for b, lk in enumerate(lens_k):
            for j in range((lk + page - 1) // page):
                n = min(page, lk - j * page)
                pg[int(bt[b, j]), :n] = data[int(bt[b, j]), :n]
    (kb, kp, ks), (vb, vp, vs) = _in(pages[0].cuda()), _in(pages[1].cuda())
    qb, q, qs = _in(rand16((sum(lens_q), Hq, D), dt, 13))
    ob, out, osn = _out((sum(lens_q), Hq, D), DT[dt])
    cu_q, cu_k = _cu(lens_q), _cu(lens_k)
    res, lse = fi._varlen_forward(q, kp, vp, cu_q, cu_k, max(lens_q), max(lens_k), 0.0, None, True, (-1, -1), 0.0, None, False,
                                  bt.cuda(), out=out)[:2]
    torch.cuda.synchronize()
    assert res is out
    for buf, snap, name in ((qb, qs, "q"), (kb, ks, "k pages"), (vb, vs, "v pages")):
        _unchanged(buf, snap, name)
    guard.assert_untouched(ob, out, osn, "out")
    o_ref, lse_ref = oracle.varlen_fwd(f64(q), f64(kp), f64(vp), cu_q.cpu().numpy(), cu_k.cpu().numpy(), max(lens_q), max(lens_k),
                                       D ** -0.5, causal=True, block_table=bt.numpy())
    assert_close(f64(out), o_ref, dt, "out")
    assert_lse_close(f64(lse), lse_ref, "lse")


def _rand8(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(FP8).cuda()


@pytest.mark.parametrize("layout", ["kv-packed", "head-slice"])
@pytest.mark.parametrize("D", [16, 48, 64, 128])
def test_fp8_forward_in_slabs(D, layout):
    fi = _fi()
    B, Hq, Hk, Sq, Sk = 1, 4, 2, 77, 300
    if layout == "kv-packed":                                # k, v = kv[:, :, 0], kv[:, :, 1] of one [B, Sk, 2, Hk, D] slab
        qb, q, qs = _in(_rand8((B, Sq, Hq, D), 10 + D))
        kvb, kv, kvs = _in(_rand8((B, Sk, 2, Hk, D), 20 + D), row_dim=1)           # (bands of 256 key rows, k and v of each)
        k, v = kv[:, :, 0], kv[:, :, 1]
        bufs = ((qb, qs, "q"), (kvb, kvs, "kv"))
    else:                                                    # every other head of slabs twice as wide
        qb, q2, qs = _in(_rand8((B, Sq, 2 * Hq, D), 10 + D))
        kb, k2, ks = _in(_rand8((B, Sk, 2 * Hk, D), 20 + D))
        vb, v2, vs = _in(_rand8((B, Sk, 2 * Hk, D), 30 + D))
        q, k, v = q2[:, :, 1::2], k2[:, :, ::2], v2[:, :, 1::2]
        bufs = ((qb, qs, "q"), (kb, ks, "k"), (vb, vs, "v"))
    for x in (q, k, v):
        assert fi._prep8(x, D) is x                          # (a copy would take the slab out of the test)
    out, lse, _ = _fa().flash_attn_func(q, k, v, causal=True, return_attn_probs=True)
    # the wrapper allocates the fp8 forward's out and lse itself (no out=): the same call through the C ABI writes them into slabs
    from flash_attn_mi355 import _lib
    ob, out_s, osn = _out((B, Sq, Hq, D), torch.bfloat16)
    lb, lse_s, lsn = _f32_slab((B, Hq, Sq))
    p = _abi_params(q, k, v, out_s, lse_s, "bshd", True, D ** -0.5)
    p.dtype = p.kv_dtype = _lib.FA_FP8_E4M3
    p.o_dtype = _lib.FA_BF16
    p.q_descale = 1.0
    _abi("fa_fwd", p)
    torch.cuda.synchronize()
    for buf, snap, name in bufs:
        _unchanged(buf, snap, name)
    guard.assert_untouched(ob, out_s, osn, "out")
    guard.assert_untouched(lb, lse_s, lsn, "lse")
    assert torch.equal(out_s, out) and torch.equal(lse_s, lse), "the C-ABI call on slabs differs from the wrapper's call"
    t = lambda x: x.detach().to(torch.float64).cpu().numpy().transpose(0, 2, 1, 3)
    scale = D ** -0.5
    o_ref, lse_ref, _ = oracle.attn_fwd(t(q), t(k), t(v), scale, causal=True)
    bnd, _ = fp8_gate.dense_bound(t(q), t(k), t(v), scale, True, (-1, -1))
    fp8_gate.check_out(t(out), o_ref, bnd, "out")            # (the fp8 forward's own gate: tests/fp8_gate.py)
    assert_lse_close(f64(lse), lse_ref, "lse")               # (unit-magnitude inputs: LSE_ATOL alone, as tests/test_fp8_fwd_gpu.py)


KV_B = [
    # id, B, Tq, Hq, Hk, D, dtype, fp8, page, rotary, batch_idx, leftpad, num_splits
    ("append", 3, 1, 8, 2, 128, "bf16", False, 0, False, False, False, 0),
    ("append-rotary", 3, 1, 8, 2, 128, "fp16", False, 0, True, False, False, 0),
    ("chunk-rotary-leftpad", 2, 5, 4, 2, 128, "fp16", False, 0, True, False, True, 0),
    ("batch-idx-d64", 2, 3, 4, 4, 64, "bf16", False, 0, True, True, False, 3),
    ("paged-16", 3, 2, 8, 2, 128, "fp16", False, 16, True, False, False, 0),
    ("paged-256-d96", 3, 1, 8, 2, 96, "bf16", False, 256, False, False, False, 5),
    ("chunk-70-rotary-leftpad", 2, 70, 4, 2, 128, "bf16", False, 0, True, False, True, 0),
    ("fp8", 3, 1, 8, 8, 128, "bf16", True, 0, False, False, False, 0),
    ("fp8-rotary-batch-idx", 2, 3, 16, 2, 128, "bf16", True, 0, True, True, False, 3),
    ("fp8-paged", 3, 2, 32, 8, 128, "bf16", True, 64, True, False, False, 0),
]


@pytest.mark.parametrize("case", KV_B, ids=lambda c: c[0])
def test_kvcache_append_in_slabs(case):
    _, B, Tq, Hq, Hk, D, dt, fp8, page, rot, use_bidx, use_lp, nsplit = case
    Smax = 512
    kd, vd = (0.05, 0.04) if fp8 else (None, None)
    lens = [Smax - Tq - 20, 1, 300][:B]
    lp = [7, 0, 16][:B] if use_lp else [0] * B
    bidx = [B + 1 - i for i in range(B)] if use_bidx else list(range(B))
    Bc = B + 2 if use_bidx else B
    if page:
        bt, nblk, nan_page = guard.paged_table([l + Tq for l in lens], page, width=Smax // page, seed=6)
        shape = (nblk, page, Hk, D)
        slot = lambda b, pos: (int(bt[b, pos // page]), pos % page)
    else:
        bt, shape = None, (Bc, Smax, Hk, D)
        slot = lambda b, pos: (bidx[b], pos)
    # the caches: NaN everywhere but the keys each sequence holds before the call
    caches = []
    for i in range(2):
        data = rand16(shape, dt, 2 + i, scale=1.5 if fp8 else 1.0, device="cpu")
        if fp8:
            data = (data.float() / (kd, vd)[i]).to(FP8)
        c = guard.fill_nan(torch.empty(shape, dtype=data.dtype))
        for b in range(B):
            for pos in range(lp[b], lp[b] + lens[b]):
                s = slot(b, pos)
                guard.bits(c)[s] = guard.bits(data)[s]
        caches.append(_in(c.cuda()))
    (kb, kc, ks), (vb, vc, vs) = caches
    qb, q, qs = guard.guarded(rand16((B, Tq, Hq, D), dt, 1), gaps=False)           # (the wrapper wants q / k / v contiguous)
    knb, knew, kns = guard.guarded(rand16((B, Tq, Hk, D), dt, 4), gaps=False)
    vnb, vnew, vns = guard.guarded(rand16((B, Tq, Hk, D), dt, 5), gaps=False)
    cos, sin = _rotary(Smax + 24, D if D != 96 else 32, dt) if rot else (None, None)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    np_cache = lambda c: c.float().double().cpu().numpy().copy()
    kc_ref, vc_ref = np_cache(kc), np_cache(vc)
    pre_k, pre_v = guard.bits(kc).clone(), guard.bits(vc).clone()
    _fi()._KV_PLANS.clear()
    out, lse = _fa().flash_attn_with_kvcache(
        q, kc, vc, k=knew, v=vnew, rotary_cos=cos, rotary_sin=sin, cache_seqlens=i32(lens).cuda(),
        cache_batch_idx=i32(bidx).cuda() if use_bidx else None, cache_leftpad=i32(lp).cuda() if use_lp else None,
        block_table=None if bt is None else bt.cuda(), causal=True, rotary_interleaved=False, num_splits=nsplit,
        return_softmax_lse=True, k_descale=kd, v_descale=vd)
    torch.cuda.synchronize()
    for buf, snap, name in ((qb, qs, "q"), (knb, kns, "k"), (vnb, vns, "v")):
        _unchanged(buf, snap, name)
    guard.assert_untouched(kb, kc, ks, "k_cache")
    guard.assert_untouched(vb, vc, vs, "v_cache")
    o_ref, lse_ref = oracle.kvcache_fwd(
        f64(q), kc_ref, vc_ref, k=f64(knew), v=f64(vnew), rotary_cos=None if cos is None else f64(cos),
        rotary_sin=None if sin is None else f64(sin), cache_seqlens=np.array(lens),
        cache_batch_idx=np.array(bidx) if use_bidx else None, cache_leftpad=np.array(lp) if use_lp else None,
        block_table=None if bt is None else bt.numpy(), causal=True, rotary_interleaved=False, io_dtype=dt,
        k_descale=kd, v_descale=vd)
    # inside the caches: the appended rows and nothing else
    new = torch.zeros(shape[:2], dtype=torch.bool)
    for b in range(B):
        for r in range(Tq):
            new[slot(b, lp[b] + lens[b] + r)] = True
    for name, c, pre in (("k_cache", kc, pre_k), ("v_cache", vc, pre_v)):
        touched = (guard.bits(c) != pre).flatten(2).any(-1).cpu()
        stray = touched & ~new
        assert not bool(stray.any()), f"{name}: rows {torch.nonzero(stray)[:4].tolist()} changed (not appended by this call)"
    got_k, got_v = np_cache(kc)[new.numpy()], np_cache(vc)[new.numpy()]
    ref_k, ref_v = kc_ref[new.numpy()], vc_ref[new.numpy()]
    assert np.isfinite(got_k).all() and np.isfinite(got_v).all(), "an appended row was not written"
    if fp8:      # identical fp8 codes except for fp32-vs-fp64 rounding ties (<= 1 code step): tests/test_kvcache_gpu.py
        assert (np.abs(got_k - ref_k) <= 0.13 * np.maximum(np.abs(ref_k), 2.0 ** -6)).all()
        assert (got_k != ref_k).mean() < 1e-3
        assert np.array_equal(got_v, ref_v)
    else:        # 1-ulp slack for fp32-vs-fp64 rounding ties of the rotation
        tol = 2.0 ** (-7 if dt == "bf16" else -10)
        assert np.abs(got_k - ref_k).max() <= (tol if rot else 0.0) * max(1.0, np.abs(ref_k).max())
        assert np.array_equal(got_v, ref_v)
    assert_close(f64(out), o_ref, dt, "out", mult=1.5 if fp8 else (2.0 if rot else 1.0))
    assert_lse_close(f64(lse), lse_ref, "lse", **(dict(atol=LSE_ATOL_FP8) if fp8 else {}))


# =====================================================================================================================
# C. the outputs the wrapper allocates itself, through the C ABI
# =====================================================================================================================
def _f32_slab(shape):
    buf, view = guard.slab(shape, torch.float32, gaps=True, device="cuda", check_prep=False)
    return buf, view, guard.snapshot(buf)


def _abi(op, p, ext=None):
    from flash_attn_mi355 import _lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = (getattr(_lib.lib, op)(ctypes.byref(p), stream) if not op.endswith("_ext")
          else getattr(_lib.lib, op)(ctypes.byref(p), None if ext is None else ctypes.byref(ext), stream))
    assert rc == 0, _lib.lib.fa_last_error()


def _abi_params(q, k, v, out, lse, layout, causal, scale, cu=None):
    fi = _fi()
    p = fi._base_params(q, out.dtype, scale, causal, (-1, -1), 0.0)      # (16-bit calls: out has q's dtype)
    p.q, p.k, p.v, p.o, p.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr()
    for name, t in (("q", q), ("k", k), ("v", v), ("o", out)):
        fi._set3(p, name, t, layout)
    p.nheads_q, p.nheads_k = q.shape[-2], k.shape[-2]
    fi._set_head_dim(p, q.shape[-1])
    if cu is None:
        p.batch, p.seqlen_q, p.seqlen_k = q.shape[0], q.shape[1], k.shape[1]
        p.lse_batch_stride, p.lse_head_stride = lse.stride(0), lse.stride(1)
    else:
        cu_q, cu_k, mq, mk = cu
        p.batch, p.seqlen_q, p.seqlen_k = cu_q.numel() - 1, mq, mk
        p.cu_seqlens_q, p.cu_seqlens_k = cu_q.data_ptr(), cu_k.data_ptr()
        p.total_q, p.total_k = q.shape[0], k.shape[0]
        p.lse_batch_stride, p.lse_head_stride = 0, lse.stride(0)
    return p


def _abi_backward(p, do, dq, dk, dv, softmax_d, layout):
    fi = _fi()
    p.dout, p.dq, p.dk, p.dv, p.softmax_d = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), softmax_d.data_ptr()
    for name, t in (("do", do), ("dq", dq), ("dk", dk), ("dv", dv)):
        fi._set3(p, name, t, layout)


def _ref_grads(ref_fn, q, k, v, do, sinks):
    """fp64 autograd through tests/sink_ref.py (sinks None: plain attention): out, lse, dq, dk, dv, dsinks, softmax_d"""
    ins = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    s = None if sinks is None else sinks.detach().double().requires_grad_(True)
    o, lse = ref_fn(*ins, s)
    g = torch.autograd.grad(o, ins + ([s] if s is not None else []), do.double())
    return o.detach(), lse.detach(), g[0], g[1], g[2], (g[3] if s is not None else None), (do.double() * o.detach()).sum(-1)


@pytest.mark.parametrize("ext", [False, True], ids=["abi4", "ext-sinks"])
@pytest.mark.parametrize("Sq,Sk,D,dt", [(77, 50, 128, "bf16"), (300, 129, 64, "fp16")])
def test_c_abi_dense_lse_softmax_d_dsinks_in_slabs(Sq, Sk, D, dt, ext):
    """fa_fwd / fa_bwd and their _ext forms with lse and softmax_d strided inside fp32 slabs (lse_head_stride > Sq,
    lse_batch_stride > H x head stride) and dsinks between bands; causal with Sq > Sk: the first Sq - Sk rows have no keys."""
    from flash_attn_mi355 import _lib
    B, Hq, Hk = 2, 4, 2
    scale = D ** -0.5
    q, k, v, do = (rand16(s, dt, 91 + i) for i, s in enumerate(((B, Sq, Hq, D), (B, Sk, Hk, D), (B, Sk, Hk, D), (B, Sq, Hq, D))))
    (ob, out, osn), (dqb, dq, dqs), (dkb, dk, dks), (dvb, dv, dvs) = (
        _out(s, DT[dt]) for s in ((B, Sq, Hq, D), (B, Sq, Hq, D), (B, Sk, Hk, D), (B, Sk, Hk, D)))
    lb, lse, lsn = _f32_slab((B, Hq, Sq))
    sb, sd, ssn = _f32_slab((B, Hq, Sq))
    assert lse.stride(1) > Sq and lse.stride(0) > Hq * lse.stride(1) and sd.stride() == lse.stride()
    sinks = torch.tensor([0.5 * h - 1.0 for h in range(Hq)], dtype=torch.float32, device="cuda") if ext else None
    dsb, dsinks, dssn = _f32_slab((Hq,))
    p = _abi_params(q, k, v, out, lse, "bshd", True, scale)
    _abi("fa_fwd_ext" if ext else "fa_fwd", p, _lib.ext_params(sinks) if ext else None)
    _abi_backward(p, do, dq, dk, dv, sd, "bshd")
    ws = torch.empty(max(1, int(_lib.lib.fa_bwd_workspace_bytes(ctypes.byref(p)))), dtype=torch.uint8, device="cuda")
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    _abi("fa_bwd_ext" if ext else "fa_bwd", p, _lib.ext_params(sinks, dsinks) if ext else None)
    torch.cuda.synchronize()
    for buf, view, snap, name in ((ob, out, osn, "out"), (dqb, dq, dqs, "dq"), (dkb, dk, dks, "dk"), (dvb, dv, dvs, "dv"),
                                  (lb, lse, lsn, "lse"), (sb, sd, ssn, "softmax_d")):
        guard.assert_untouched(buf, view, snap, name)         # (the padding of the planes stays NaN, bit for bit)
    if ext:
        guard.assert_untouched(dsb, dsinks, dssn, "dsinks")
    else:
        assert torch.equal(guard.bits(dsb), dssn)
    o_ref, lse_ref, dq_r, dk_r, dv_r, ds_r, sd_r = _ref_grads(
        lambda a, b, c, s: sink_ref.ref_dense(a, b, c, s, scale, causal=True), q, k, v, do, sinks)
    if not ext:
        assert torch.isneginf(lse[:, :, :Sq - Sk]).all() and torch.isfinite(lse[:, :, Sq - Sk:]).all()      # rows without keys
    assert_close(f64(out), f64(o_ref), dt, "out")
    assert_lse_close(f64(lse), f64(lse_ref), "lse")
    for name, got, ref in (("dq", dq, dq_r), ("dk", dk, dk_r), ("dv", dv, dv_r)):
        assert_close(f64(got), f64(ref), dt, name, mult=2.0)
    assert_close(f64(sd), f64(sd_r).transpose(0, 2, 1), dt, "softmax_d", mult=2.0)
    if ext:
        assert_close(f64(dsinks), f64(ds_r), dt, "dsinks", mult=2.0)


@pytest.mark.parametrize("ext", [False, True], ids=["abi4", "ext-sinks"])
def test_c_abi_varlen_lse_softmax_d_in_slabs(ext):
    """fa_varlen_fwd / fa_varlen_bwd (+ _ext): lse / softmax_d [Hq, Tq] with lse_head_stride > Tq inside fp32 slabs"""
    from flash_attn_mi355 import _lib
    lens_q, lens_k, Hq, Hk, D, dt = [77, 0, 300, 1], [50, 9, 300, 0], 4, 2, 128, "bf16"
    Tq, Tk = sum(lens_q), sum(lens_k)
    scale = D ** -0.5
    q, k, v, do = (rand16(s, dt, 71 + i) for i, s in enumerate(((Tq, Hq, D), (Tk, Hk, D), (Tk, Hk, D), (Tq, Hq, D))))
    (ob, out, osn), (dqb, dq, dqs), (dkb, dk, dks), (dvb, dv, dvs) = (
        _out(s, DT[dt]) for s in ((Tq, Hq, D), (Tq, Hq, D), (Tk, Hk, D), (Tk, Hk, D)))
    lb, lse, lsn = _f32_slab((Hq, Tq))
    sb, sd, ssn = _f32_slab((Hq, Tq))
    assert lse.stride(0) > Tq
    sinks = torch.tensor([0.5 * h - 1.0 for h in range(Hq)], dtype=torch.float32, device="cuda") if ext else None
    dsb, dsinks, dssn = _f32_slab((Hq,))
    cu_q, cu_k = _cu(lens_q), _cu(lens_k)
    p = _abi_params(q, k, v, out, lse, "thd", True, scale, cu=(cu_q, cu_k, max(lens_q), max(lens_k)))
    _abi("fa_varlen_fwd_ext" if ext else "fa_varlen_fwd", p, _lib.ext_params(sinks) if ext else None)
    _abi_backward(p, do, dq, dk, dv, sd, "thd")
    ws = torch.empty(max(1, int(_lib.lib.fa_bwd_workspace_bytes(ctypes.byref(p)))), dtype=torch.uint8, device="cuda")
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    _abi("fa_varlen_bwd_ext" if ext else "fa_varlen_bwd", p, _lib.ext_params(sinks, dsinks) if ext else None)
    torch.cuda.synchronize()
    for buf, view, snap, name in ((ob, out, osn, "out"), (dqb, dq, dqs, "dq"), (dkb, dk, dks, "dk"), (dvb, dv, dvs, "dv"),
                                  (lb, lse, lsn, "lse"), (sb, sd, ssn, "softmax_d")):
        guard.assert_untouched(buf, view, snap, name)
    if ext:
        guard.assert_untouched(dsb, dsinks, dssn, "dsinks")
    cq, ck = cu_q.tolist(), cu_k.tolist()
    o_ref, lse_ref, dq_r, dk_r, dv_r, ds_r, sd_r = _ref_grads(
        lambda a, b, c, s: sink_ref.ref_varlen(a, b, c, cq, ck, s, scale, causal=True), q, k, v, do, sinks)
    assert_close(f64(out), f64(o_ref), dt, "out")
    assert_lse_close(f64(lse), f64(lse_ref), "lse")
    for name, got, ref in (("dq", dq, dq_r), ("dk", dk, dk_r), ("dv", dv, dv_r)):
        assert_close(f64(got), f64(ref), dt, name, mult=2.0)
    assert_close(f64(sd), f64(sd_r).T, dt, "softmax_d", mult=2.0)
    if ext:
        assert_close(f64(dsinks), f64(ds_r), dt, "dsinks", mult=2.0)


@pytest.mark.parametrize("ext", [False, True], ids=["abi4", "ext-sinks"])
@pytest.mark.parametrize("Tq,nsplit", [(1, 3), (5, 0), (77, 1)])
def test_c_abi_kvcache_out_and_lse_in_slabs(Tq, nsplit, ext):
    """fa_fwd_kvcache (+ _ext): out a gapped slab view, lse [B, Hq, Tq] strided inside an fp32 slab; one query token with
    explicit split-KV partials, a 5-token block with the heuristic's, 77 tokens (ten ragged row blocks) written in place.
    The second sequence holds two keys fewer than the query block has rows: rows without keys, LSE = -inf (s_h with sinks)."""
    from flash_attn_mi355 import _lib
    fi = _fi()
    B, Hq, Hk, D, dt, Smax = 3, 8, 2, 128, "bf16", 512
    lens = [Smax - 3, max(1, Tq - 2), 300]
    q = rand16((B, Tq, Hq, D), dt, 1)
    (kb, kc, ks), (vb, vc, vs) = _in(rand16((B, Smax, Hk, D), dt, 2)), _in(rand16((B, Smax, Hk, D), dt, 3))
    for b, l in enumerate(lens):                             # rows past the sequences' keys: NaN
        guard.fill_nan(kc[b, l:]); guard.fill_nan(vc[b, l:])
    ks, vs = guard.snapshot(kb), guard.snapshot(vb)
    ob, out, osn = _out((B, Tq, Hq, D), DT[dt])
    lb, lse, lsn = _f32_slab((B, Hq, Tq))
    sl = torch.tensor(lens, dtype=torch.int32).cuda()
    sinks = torch.tensor([0.5 * h - 1.0 for h in range(Hq)], dtype=torch.float32, device="cuda") if ext else None
    p = _abi_params(q, kc, vc, out, lse, "bshd", True, D ** -0.5)
    p.seqlen_q, p.seqlen_k = Tq, Smax
    p.cache_seqlens = sl.data_ptr()
    p.num_splits = nsplit
    n = int(_lib.lib.fa_fwd_kvcache_workspace_bytes(ctypes.byref(p)))
    ws = torch.empty(max(1, n), dtype=torch.uint8, device="cuda")
    p.workspace, p.workspace_bytes = ws.data_ptr(), n
    _abi("fa_fwd_kvcache_ext" if ext else "fa_fwd_kvcache", p, _lib.ext_params(sinks) if ext else None)
    torch.cuda.synchronize()
    _unchanged(kb, ks, "k_cache"); _unchanged(vb, vs, "v_cache")
    guard.assert_untouched(ob, out, osn, "out")
    guard.assert_untouched(lb, lse, lsn, "lse")
    o_ref, lse_ref = oracle.kvcache_fwd(f64(q), f64(kc), f64(vc), cache_seqlens=np.array(lens), causal=True, io_dtype=dt)
    if ext:
        o_ref, lse_ref = sink_ref.sink_identity_bshd(o_ref, lse_ref.astype(np.float64), f64(sinks))
    elif Tq > lens[1]:
        assert np.isneginf(lse_ref[1, :, :Tq - lens[1]]).all() and torch.isneginf(lse[1, :, :Tq - lens[1]]).all()
    assert_close(f64(out), o_ref, dt, "out")
    assert_lse_close(f64(lse), lse_ref, "lse")
