"""GPU parity: tree attention masks of flash_attn_with_kvcache (speculative decoding: the query tokens are the nodes of a
draft tree) against tests/tree_ref.py, with the gates of the existing kv-cache tests (tests/util.py; fp8 caches: out 1.5 x
the io tolerance and LSE_ATOL_FP8, rotary: 2 x, as tests/test_kvcache_gpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import tree_ref as tr
from util import LSE_ATOL_FP8, DT, assert_close, assert_lse_close, f64, rand16

pytestmark = pytest.mark.gpu


def _fa():
    import flash_attn
    return flash_attn


def _rotary(seqlen_ro, rd, dt):
    pos = torch.arange(seqlen_ro, dtype=torch.float32)[:, None]
    inv = 1.0 / (10000 ** (torch.arange(0, rd, 2, dtype=torch.float32) / rd))[None, :]
    ang = pos * inv
    return torch.cos(ang).to(DT[dt]).cuda(), torch.sin(ang).to(DT[dt]).cuda()


def _tree_masks(B, T, seed, kind="tree", shared=False):
    """bool mask [B, T, T] ([T, T] when shared) and depths; kind 'random': arbitrary, row 0 empty, no diagonal promise"""
    rng = np.random.default_rng(seed)
    n = 1 if shared else B
    if kind == "tree":
        pars = [tr.random_parents(T, rng) for _ in range(n)]
        mask = np.stack([tr.mask_from_parents(p) for p in pars])
        depths = np.stack([tr.depths_from_parents(p) for p in pars])
    else:
        mask = rng.random((n, T, T)) < 0.4
        mask[:, 0] = False
        depths = rng.integers(0, T, size=(n, T)).astype(np.int32)
    return (mask[0], depths[0]) if shared else (mask, depths)


def _setup(B, T, Hq, Hk, D, dt, seqlens, page=0, bidx=False, leftpad=False, fp8=False, Smax=None, seed=0):
    """caches (contiguous, or paged with `page` tokens per page) with room for max(seqlens) + T keys; the last value
    returned is the cache capacity"""
    need = max(seqlens) + T + (16 if leftpad else 0)
    Smax = Smax or -(-(need + 5) // 32) * 32
    g = torch.Generator().manual_seed(100 + seed)
    bt = None
    if page:
        pps = -(-Smax // page)
        nblk = B * pps + 3
        shape = (nblk, page, Hk, D)
        bt = torch.randperm(nblk, generator=g)[: B * pps].reshape(B, pps).to(torch.int32)
    else:
        shape = (B + 2 if bidx else B, Smax, Hk, D)
    kc = rand16(shape, dt, 2 + seed, scale=1.5 if fp8 else 1.0)
    vc = rand16(shape, dt, 3 + seed, scale=1.5 if fp8 else 1.0)
    kd = vd = None
    if fp8:
        kd, vd = 0.05, 0.04
        kc = (kc.float() / kd).to(torch.float8_e4m3fn)
        vc = (vc.float() / vd).to(torch.float8_e4m3fn)
    bi = torch.tensor([shape[0] - 1 - i for i in range(B)], dtype=torch.int32) if bidx else None
    lp = torch.randint(0, 17, (B,), generator=g, dtype=torch.int32) if leftpad else None
    return kc, vc, bt, bi, lp, kd, vd, (bt.shape[1] * page if page else Smax)       # (the cache capacity: rotary tables cover it)


def _np_cache(c):
    return c.float().double().cpu().numpy().copy()


TCASES = [
    # B, T, Hq, Hk, D, dtype, seqlens (cache lengths before the append), page, bidx, leftpad, num_splits, rotary, append,
    # fp8, softcap, sinks, shared mask, mask kind
    (2, 2, 4, 4, 64, "bf16", [45, 300], 0, False, False, 0, None, True, False, 0.0, False, False, "tree"),        # off mid-tile
    (3, 7, 8, 2, 128, "fp16", [64, 0, 509], 16, False, False, 1, "gptj", True, False, 0.0, False, False, "tree"),  # page 16, tile edge, L = 0
    (2, 32, 16, 2, 128, "bf16", [1000, 96], 256, False, False, 4, "neox", True, False, 0.0, False, False, "tree"), # G 8: 8 row blocks, page 256
    (2, 33, 2, 2, 256, "fp16", [64, 333], 0, True, False, 0, None, True, False, 0.0, False, False, "tree"),        # D 256, two words, batch idx
    (2, 64, 8, 2, 96, "bf16", [200, 31], 0, False, True, 4, "gptj", True, False, 0.0, False, False, "tree"),       # narrow width, leftpad
    (2, 64, 16, 2, 128, "fp16", [0, 700], 16, False, False, 0, None, True, False, 0.0, False, True, "tree"),       # 16 row blocks, shared mask
    (2, 7, 8, 2, 128, "bf16", [130, 57], 0, False, False, 1, None, False, False, 0.0, False, False, "tree"),       # K / V already in the cache
    (2, 33, 4, 1, 64, "fp16", [500, 20], 256, False, False, 4, "neox", True, False, 0.0, False, False, "tree"),    # D 64, MQA, paged
    (2, 32, 4, 4, 256, "bf16", [96, 41], 16, False, False, 1, None, True, False, 0.0, False, True, "tree"),        # D 256 paged, exactly one word
    # fp8 caches with descales: head-per-wave route (H_k 8, <= 32 packed rows), the F8M row-block route (H_k 2), D 64
    (2, 7, 32, 8, 128, "bf16", [700, 17], 256, False, False, 0, "neox", True, True, 0.0, False, False, "tree"),
    (2, 33, 8, 2, 128, "bf16", [511, 256], 16, False, False, 4, None, True, True, 0.0, False, False, "tree"),
    (2, 8, 2, 2, 64, "fp16", [100, 64], 0, False, False, 1, "gptj", True, True, 0.0, False, True, "tree"),
    (2, 7, 16, 8, 128, "fp16", [300, 40], 256, False, False, 2, None, False, True, 0.0, True, False, "random"),    # HPW, sinks, no append
    # softcap and sinks (the per-element score path), arbitrary masks with an empty row
    (2, 7, 8, 2, 128, "bf16", [77, 400], 0, False, False, 0, None, True, False, 15.0, False, False, "tree"),
    (2, 32, 4, 4, 64, "fp16", [33, 600], 0, False, False, 1, None, True, False, 0.0, True, False, "tree"),
    (2, 33, 8, 2, 128, "bf16", [0, 250], 16, False, False, 4, "neox", True, False, 0.0, True, False, "random"),    # empty row + sinks + split
    (2, 12, 4, 1, 128, "fp16", [0, 64], 0, False, False, 0, None, True, False, 30.0, False, True, "random"),       # empty row: LSE = -inf
]


@pytest.mark.parametrize("case", TCASES, ids=lambda c: "-".join(map(str, c)))
def test_tree_vs_reference(case):
    B, T, Hq, Hk, D, dt, seqlens, page, bidx, leftpad, nsplit, rot, append, fp8, softcap, use_sinks, shared, kind = case
    kc, vc, bt, bi, lp, kd, vd, Smax = _setup(B, T, Hq, Hk, D, dt, seqlens, page, bidx, leftpad, fp8)
    q = rand16((B, T, Hq, D), dt, 1)
    knew = rand16((B, T, Hk, D), dt, 4) if append else None
    vnew = rand16((B, T, Hk, D), dt, 5) if append else None
    mask, depths = _tree_masks(B, T, 7 + T, kind, shared)
    rd = {64: 32, 128: 128, 256: 64, 96: 32}[D]
    cos, sin = _rotary(Smax + 24, rd, dt) if rot else (None, None)
    # k = None: the nodes are the last T keys of the cache
    sl = torch.tensor([s + (0 if append else T) for s in seqlens], dtype=torch.int32)
    sinks = torch.tensor([0.5 * h - 1.0 for h in range(Hq)], dtype=torch.float32, device="cuda") if use_sinks else None
    kc_ref, vc_ref = _np_cache(kc), _np_cache(vc)
    # half of the cases hand the library the bool matrix, the others the packed words
    tm = torch.from_numpy(mask).cuda() if (T + B) % 2 else torch.from_numpy(tr.pack_mask(mask)).cuda()
    td = torch.from_numpy(depths.astype(np.int32)).cuda()
    out, lse = _fa().flash_attn_with_kvcache(
        q, kc, vc, k=knew, v=vnew, rotary_cos=cos, rotary_sin=sin, cache_seqlens=sl.cuda(),
        cache_batch_idx=None if bi is None else bi.cuda(), cache_leftpad=None if lp is None else lp.cuda(),
        block_table=None if bt is None else bt.cuda(), causal=bool(T % 2), softcap=softcap,
        rotary_interleaved=rot == "gptj", num_splits=nsplit, return_softmax_lse=True, k_descale=kd, v_descale=vd,
        sinks=sinks, tree_mask=tm, tree_depths=td if rot else None)
    o_ref, lse_ref, kc_a, vc_a = tr.ref_tree(
        f64(q), kc_ref, vc_ref, mask, k=None if knew is None else f64(knew), v=None if vnew is None else f64(vnew),
        depths=depths, rotary_cos=None if cos is None else f64(cos), rotary_sin=None if sin is None else f64(sin),
        cache_seqlens=sl.numpy(), cache_batch_idx=None if bi is None else bi.numpy(),
        cache_leftpad=None if lp is None else lp.numpy(), block_table=None if bt is None else bt.numpy(), softcap=softcap,
        rotary_interleaved=rot == "gptj", io_dtype=dt, k_descale=kd, v_descale=vd,
        sinks=None if sinks is None else f64(sinks))
    got_k, got_v = _np_cache(kc), _np_cache(vc)
    if fp8:   # appended rows: identical fp8 codes except for fp32-vs-fp64 rounding ties (<= 1 code step)
        assert (np.abs(got_k - kc_a) <= 0.13 * np.maximum(np.abs(kc_a), 2.0 ** -6)).all()
        assert (got_k != kc_a).mean() < 1e-3
    else:     # 1-ulp slack for fp32-vs-fp64 rounding ties of the rotation
        tol = 2.0 ** (-7 if dt == "bf16" else -10)
        assert np.abs(got_k - kc_a).max() <= (tol if rot else 0.0) * max(1.0, np.abs(kc_a).max())
    assert np.array_equal(got_v, vc_a)
    mr, fro = assert_close(f64(out), o_ref, dt, "out", mult=1.5 if fp8 else (2.0 if rot else 1.0))
    d = assert_lse_close(f64(lse), lse_ref, "lse", **(dict(atol=LSE_ATOL_FP8) if fp8 else {}))
    print(f"tree case: out max-rel {mr:.3e} fro {fro:.3e}  lse max-abs {d:.3e}")
    if kind == "random":
        empty = ~np.isfinite(lse_ref) if sinks is None else None
        if 0 in seqlens and append:
            b0 = seqlens.index(0)
            assert torch.all(out[b0, 0] == 0)
            if sinks is None:
                assert empty[b0, :, 0].all() and torch.all(torch.isneginf(lse[b0, :, 0]))
            else:
                assert torch.allclose(lse[b0, :, 0], sinks, rtol=0, atol=1e-5)       # (a row without keys: LSE = s_h)


@pytest.mark.parametrize("case", [
    # B, T, Hq, Hk, D, dtype, page, num_splits, fp8
    (2, 5, 4, 4, 128, "bf16", 0, 1, False),
    (3, 32, 8, 2, 128, "fp16", 256, 4, False),       # four row blocks, split
    (2, 17, 4, 1, 64, "bf16", 16, 2, False),
    (2, 8, 4, 4, 256, "fp16", 0, 3, False),
    (2, 4, 64, 8, 128, "bf16", 256, 2, True),        # head per wave, fp8
    (2, 24, 8, 2, 128, "fp16", 16, 4, True),         # fp8 row blocks
])
def test_chain_is_bit_identical_to_causal(case):
    """A lower-triangular mask with depths = arange is the causal rule: same kernel, same tiles, same order - out, LSE and
    the appended cache rows carry the same bits as causal=True without a tree (explicit num_splits; at these shapes the
    causal call runs on the decode kernel too)."""
    B, T, Hq, Hk, D, dt, page, nsplit, fp8 = case
    seqlens = [777, 40, 95][:B]
    kc, vc, bt, _, _, kd, vd, Smax = _setup(B, T, Hq, Hk, D, dt, seqlens, page, fp8=fp8)
    q = rand16((B, T, Hq, D), dt, 1)
    knew, vnew = rand16((B, T, Hk, D), dt, 4), rand16((B, T, Hk, D), dt, 5)
    cos, sin = _rotary(Smax + 8, 64, dt)
    sl = torch.tensor(seqlens, dtype=torch.int32).cuda()
    kw = dict(k=knew, v=vnew, rotary_cos=cos, rotary_sin=sin, cache_seqlens=sl, block_table=None if bt is None else bt.cuda(),
              rotary_interleaved=False, num_splits=nsplit, return_softmax_lse=True, k_descale=kd, v_descale=vd)
    kc2, vc2 = kc.clone(), vc.clone()
    o_c, l_c = _fa().flash_attn_with_kvcache(q, kc2, vc2, causal=True, **kw)
    mask = torch.ones(T, T, dtype=torch.bool, device="cuda").tril()
    o_t, l_t = _fa().flash_attn_with_kvcache(q, kc, vc, tree_mask=mask, tree_depths=torch.arange(T, dtype=torch.int32, device="cuda"), **kw)
    assert torch.equal(o_t, o_c) and torch.equal(l_t, l_c)
    bits = torch.int8 if fp8 else torch.int16
    assert torch.equal(kc.view(bits), kc2.view(bits)) and torch.equal(vc.view(bits), vc2.view(bits))


def test_chain_agrees_with_the_general_path():
    """B 8, H 64/8, T_q 64: the causal call runs on the general kernel (16 row blocks against 8 passes, 512 workgroups), the
    tree call on the decode kernel's row blocks; the two agree within the io gates."""
    B, T, Hq, Hk, D, dt = 8, 64, 64, 8, 128, "bf16"
    seqlens = [300, 1, 64, 257, 128, 90, 33, 500]
    kc, vc, _, _, _, _, _, Smax = _setup(B, T, Hq, Hk, D, dt, seqlens)
    q = rand16((B, T, Hq, D), dt, 1)
    knew, vnew = rand16((B, T, Hk, D), dt, 4), rand16((B, T, Hk, D), dt, 5)
    sl = torch.tensor(seqlens, dtype=torch.int32).cuda()
    kc2, vc2 = kc.clone(), vc.clone()
    o_c, l_c = _fa().flash_attn_with_kvcache(q, kc2, vc2, k=knew, v=vnew, cache_seqlens=sl, causal=True, return_softmax_lse=True)
    mask = torch.ones(T, T, dtype=torch.bool, device="cuda").tril()
    o_t, l_t = _fa().flash_attn_with_kvcache(q, kc, vc, k=knew, v=vnew, cache_seqlens=sl, tree_mask=mask, return_softmax_lse=True)
    assert_close(f64(o_t), f64(o_c), dt, "tree (decode row blocks) vs causal (general path)")
    assert_lse_close(f64(l_t), f64(l_c), "lse")
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)


@pytest.mark.parametrize("dt,fp8", [("bf16", False), ("fp16", True)])
def test_appended_rows_equal_a_chain_append_at_the_same_positions(dt, fp8):
    """Node t's cache row (slot L + t) holds the bits a plain append writes for that token at position L + depth[t]."""
    B, T, Hq, Hk, D = 2, 9, 4, 2, 128
    seqlens = [50, 200]
    kc, vc, _, _, _, kd, vd, Smax = _setup(B, T, Hq, Hk, D, dt, seqlens, fp8=fp8)
    q = rand16((B, T, Hq, D), dt, 1)
    knew, vnew = rand16((B, T, Hk, D), dt, 4), rand16((B, T, Hk, D), dt, 5)
    mask, depths = _tree_masks(B, T, 3)
    cos, sin = _rotary(Smax + 8, 128, dt)
    sl = torch.tensor(seqlens, dtype=torch.int32).cuda()
    kc0, vc0 = kc.clone(), vc.clone()
    _fa().flash_attn_with_kvcache(q, kc, vc, k=knew, v=vnew, rotary_cos=cos, rotary_sin=sin, cache_seqlens=sl,
                                  tree_mask=torch.from_numpy(mask).cuda(), tree_depths=torch.from_numpy(depths).cuda(),
                                  k_descale=kd, v_descale=vd)
    bits = torch.int8 if fp8 else torch.int16
    for t in range(T):
        ks, vs = kc0.clone(), vc0.clone()
        pos = sl + torch.from_numpy(depths[:, t]).cuda()
        _fa().flash_attn_with_kvcache(q[:, t:t + 1], ks, vs, k=knew[:, t:t + 1], v=vnew[:, t:t + 1], rotary_cos=cos, rotary_sin=sin,
                                      cache_seqlens=pos.to(torch.int32), causal=True, k_descale=kd, v_descale=vd)
        for b in range(B):
            p_chain, p_tree = int(pos[b]), seqlens[b] + t
            assert torch.equal(kc[b, p_tree].view(bits), ks[b, p_chain].view(bits)), (b, t)
            assert torch.equal(vc[b, p_tree].view(bits), vs[b, p_chain].view(bits)), (b, t)
    # nothing outside the T slots changed
    for b in range(B):
        keep = torch.ones(kc.shape[1], dtype=torch.bool, device="cuda")
        keep[seqlens[b]:seqlens[b] + T] = False
        assert torch.equal(kc[b, keep].view(bits), kc0[b, keep].view(bits))


def test_plan_cache_keeps_tree_and_causal_calls_apart():
    """One geometry, alternating a tree call and a causal call (the second and later calls of each kind take the plan fast
    path): each matches its own reference."""
    from flash_attn_mi355 import flash_attn_interface as fi
    B, T, Hq, Hk, D, dt = 2, 8, 8, 2, 128, "fp16"
    seqlens = [100, 37]
    kc, vc, _, _, _, _, _, Smax = _setup(B, T, Hq, Hk, D, dt, seqlens)
    q = rand16((B, T, Hq, D), dt, 1)
    knew, vnew = rand16((B, T, Hk, D), dt, 4), rand16((B, T, Hk, D), dt, 5)
    mask, _ = _tree_masks(B, T, 11)
    sl = torch.tensor(seqlens, dtype=torch.int32).cuda()
    tm = torch.from_numpy(mask).cuda()
    kc_ref, vc_ref = _np_cache(kc), _np_cache(vc)
    o_tree, l_tree, _, _ = tr.ref_tree(f64(q), kc_ref, vc_ref, mask, k=f64(knew), v=f64(vnew), cache_seqlens=sl.cpu().numpy(), io_dtype=dt)
    o_caus, l_caus = oracle.kvcache_fwd(f64(q), kc_ref.copy(), vc_ref.copy(), k=f64(knew), v=f64(vnew),
                                        cache_seqlens=sl.cpu().numpy(), causal=True, io_dtype=dt)
    n0 = len(fi._KV_PLANS)
    for rep in range(3):
        o, l = _fa().flash_attn_with_kvcache(q, kc, vc, k=knew, v=vnew, cache_seqlens=sl, causal=True, return_softmax_lse=True,
                                             tree_mask=tm)
        assert_close(f64(o), o_tree, dt, f"tree out (call {rep})")
        assert_lse_close(f64(l), l_tree, "tree lse")
        o, l = _fa().flash_attn_with_kvcache(q, kc, vc, k=knew, v=vnew, cache_seqlens=sl, causal=True, return_softmax_lse=True)
        assert_close(f64(o), o_caus, dt, f"causal out (call {rep})")
        assert_lse_close(f64(l), l_caus, "causal lse")
    assert len(fi._KV_PLANS) == n0 + 2
    # and another tree of the same geometry goes through the same plan with its own words
    mask2, _ = _tree_masks(B, T, 12)
    o, l = _fa().flash_attn_with_kvcache(q, kc, vc, k=knew, v=vnew, cache_seqlens=sl, return_softmax_lse=True,
                                         tree_mask=torch.from_numpy(mask2).cuda(), causal=True)
    o2, l2, _, _ = tr.ref_tree(f64(q), kc_ref, vc_ref, mask2, k=f64(knew), v=f64(vnew), cache_seqlens=sl.cpu().numpy(), io_dtype=dt)
    assert_close(f64(o), o2, dt, "second tree out")
    assert_lse_close(f64(l), l2, "second tree lse")
    assert len(fi._KV_PLANS) == n0 + 2


@pytest.mark.parametrize("kind", ["bf16-paged-bool", "fp8-paged-split-words"])
def test_tree_step_replays_in_a_graph(kind):
    """A tree verification step (append T draft tokens with RoPE at their depths, attend under the tree mask) captured in a
    HIP graph: replays with new q / k / v / mask contents give the eager results bit for bit.  A bool mask is packed on the
    device inside the captured region."""
    fa = _fa()
    fp8 = kind.startswith("fp8")
    dt = "bf16"
    B, T, Hq, Hk, D, Smax, page = (4, 8, 16, 4, 128, 1024, 256) if not fp8 else (2, 16, 32, 8, 128, 4096, 256)
    g = torch.Generator().manual_seed(5)
    nblk = B * Smax // page
    kc, vc = rand16((nblk, page, Hk, D), dt, 2), rand16((nblk, page, Hk, D), dt, 3)
    bt = torch.randperm(nblk, generator=g).to(torch.int32).reshape(B, Smax // page).cuda()
    kw = {}
    if fp8:
        kc, vc = (kc.float() * 0.5).to(torch.float8_e4m3fn), (vc.float() * 0.5).to(torch.float8_e4m3fn)
        kw = dict(k_descale=2.0, v_descale=2.0, num_splits=4)
    lens = torch.randint(Smax // 2, Smax - 64, (B,), generator=g, dtype=torch.int32).cuda()
    cos, sin = _rotary(Smax + 8, 64, dt)
    steps = 3
    qs = [rand16((B, T, Hq, D), dt, 10 + i) for i in range(steps)]
    ks = [rand16((B, T, Hk, D), dt, 20 + i) for i in range(steps)]
    vs = [rand16((B, T, Hk, D), dt, 30 + i) for i in range(steps)]
    trees = [_tree_masks(B, T, 50 + i) for i in range(steps)]
    as_mask = (lambda m: torch.from_numpy(m).cuda()) if not fp8 else (lambda m: torch.from_numpy(tr.pack_mask(m)).cuda())
    ms = [as_mask(m) for m, _ in trees]
    ds = [torch.from_numpy(d).cuda() for _, d in trees]

    def make_step(kc_, vc_, q_, k_, v_, m_, d_):
        def step():
            return fa.flash_attn_with_kvcache(q_, kc_, vc_, k=k_, v=v_, rotary_cos=cos, rotary_sin=sin, cache_seqlens=lens,
                                              block_table=bt, rotary_interleaved=False, return_softmax_lse=True,
                                              tree_mask=m_, tree_depths=d_, **kw)
        return step

    kc_e, vc_e = kc.clone(), vc.clone()
    ref = []
    for i in range(steps):
        o, lse = make_step(kc_e, vc_e, qs[i], ks[i], vs[i], ms[i], ds[i])()
        ref.append((o.clone(), lse.clone()))
    torch.cuda.synchronize()
    kc_g, vc_g = kc.clone(), vc.clone()
    q_s, k_s, v_s, m_s, d_s = qs[0].clone(), ks[0].clone(), vs[0].clone(), ms[0].clone(), ds[0].clone()
    graph, (o_s, lse_s) = _capture(make_step(kc_g, vc_g, q_s, k_s, v_s, m_s, d_s))
    kc_g.copy_(kc); vc_g.copy_(vc)
    for i in range(steps):
        q_s.copy_(qs[i]); k_s.copy_(ks[i]); v_s.copy_(vs[i]); m_s.copy_(ms[i]); d_s.copy_(ds[i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_s, ref[i][0]), f"step {i}: out differs from the eager step"
        assert torch.equal(lse_s, ref[i][1]), f"step {i}: lse differs"
    bits = torch.int8 if fp8 else torch.int16
    assert torch.equal(kc_g.view(bits), kc_e.view(bits)) and torch.equal(vc_g.view(bits), vc_e.view(bits))


def test_fake_impl_of_the_tree_op_matches_the_real_one():
    """torch.library.opcheck of fwd_kvcache_tree: schema (the caches are the mutated arguments) and the fake implementation's
    shapes / dtypes against the real op"""
    import flash_attn_mi355.torch_ops  # noqa: F401
    op = torch.ops.flash_attn_mi355.fwd_kvcache_tree
    q = rand16((2, 5, 4, 64), "fp16", 1)
    kc, vc = rand16((2, 128, 2, 64), "fp16", 2), rand16((2, 128, 2, 64), "fp16", 3)
    kn, vn = rand16((2, 5, 2, 64), "fp16", 4), rand16((2, 5, 2, 64), "fp16", 5)
    m = torch.ones(5, 5, dtype=torch.bool, device="cuda").tril()
    sl = torch.tensor([40, 3], dtype=torch.int32, device="cuda")
    torch.library.opcheck(op, (q, kc, vc, kn, vn, sl, None, None, None, None, None, m, None, 0.125, 0.0, True, 0),
                          test_utils=("test_schema", "test_faketensor"))
    cos, sin = _rotary(136, 32, "fp16")
    d = torch.tensor([0, 1, 1, 2, 2], dtype=torch.int32, device="cuda")
    torch.library.opcheck(op, (q, kc, vc, kn, vn, sl, cos, sin, None, None, None, tr_words(m), d, 0.125, 10.0, False, 2),
                          test_utils=("test_schema", "test_faketensor"))


def tr_words(mask):
    return torch.from_numpy(tr.pack_mask(mask.cpu().numpy())).cuda()


def _capture(fn, warm=3):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def test_c_abi_null_tree_equals_fa_fwd_kvcache():
    """fa_fwd_kvcache_tree(p, NULL, NULL) is fa_fwd_kvcache(p), bit for bit (and so is a block whose mask is NULL)."""
    from flash_attn_mi355 import _lib
    B, T, Hq, Hk, D, S = 2, 4, 8, 2, 128, 512
    q = rand16((B, T, Hq, D), "bf16", 1)
    kc, vc = rand16((B, S, Hk, D), "bf16", 2), rand16((B, S, Hk, D), "bf16", 3)
    sl = torch.tensor([300, 77], dtype=torch.int32).cuda()
    p = _lib.FaParams()
    p.q, p.k, p.v = q.data_ptr(), kc.data_ptr(), vc.data_ptr()
    p.q_batch_stride, p.q_row_stride, p.q_head_stride = q.stride(0), q.stride(1), q.stride(2)
    p.o_batch_stride, p.o_row_stride, p.o_head_stride = q.stride(0), q.stride(1), q.stride(2)
    for n, t in (("k", kc), ("v", vc)):
        setattr(p, n + "_batch_stride", t.stride(0)); setattr(p, n + "_row_stride", t.stride(1)); setattr(p, n + "_head_stride", t.stride(2))
    p.lse_batch_stride, p.lse_head_stride = Hq * T, T
    p.batch, p.nheads_q, p.nheads_k, p.seqlen_q, p.seqlen_k, p.head_dim = B, Hq, Hk, T, S, D
    p.dtype = p.kv_dtype = _lib.FA_BF16
    p.softmax_scale = D ** -0.5
    p.is_causal = 1
    p.window_left = p.window_right = -1
    p.cache_seqlens = sl.data_ptr()
    p.k_descale = p.v_descale = 1.0
    p.num_splits = 2
    nbytes = int(_lib.lib.fa_fwd_kvcache_workspace_bytes(ctypes.byref(p)))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    outs = []
    stream = torch.cuda.current_stream().cuda_stream
    empty = _lib.tree_params()
    for how in ("plain", "tree-null", "tree-null-mask"):
        o = torch.zeros_like(q)
        lse = torch.zeros(B, Hq, T, dtype=torch.float32, device="cuda")
        p.o, p.lse = o.data_ptr(), lse.data_ptr()
        if how == "plain":
            _lib.call("fa_fwd_kvcache", p, stream)
        else:
            _lib.call_tree(p, None, None if how == "tree-null" else empty, stream)
        torch.cuda.synchronize()
        outs.append((o, lse))
    for o, lse in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(lse, outs[0][1])
    assert outs[0][0].abs().max() > 0
