"""GPU: fa_kv_store (flash_attn_mi355.kv_store.store_kv_cache) - a ragged packed batch of K / V rows into a paged or contiguous
KV cache.  The caches are pre-filled with random data and the WHOLE cache is compared bit for bit with the torch CPU restatement
(kv_store_ref), so a stray write inside the cache shows as well; the fp8 codes and the rotated bits are pinned to the kv-cache
op's own append and to fa_rotary, bit for bit."""
import numpy as np
import pytest
import torch

import guard
import kv_store_ref as R
import oracle
import rotary_ref
from util import LSE_ATOL_FP8, DT, assert_close, assert_lse_close, f64, rand16

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
HK, PAGE = 2, 16


def _fa():
    import flash_attn
    return flash_attn


def _store(*a, **kw):
    from flash_attn_mi355.kv_store import store_kv_cache
    return store_kv_cache(*a, **kw)


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


def _cu(lens):
    return [0] + np.cumsum(lens).tolist()


def _cache(shape, dt, seed, fp8=False, nan_page=None):
    """a pre-filled cache (random data; fp8: random codes of finite values) with the table's spare page set to NaN"""
    c = rand16(shape, dt, seed, scale=2.0)
    if fp8:
        c = c.to(FP8)
    if nan_page is not None:
        guard.fill_nan(c[nan_page])
    return c


def _rotary(seqlen_ro, rd, dt):
    pos = torch.arange(seqlen_ro, dtype=torch.float32)[:, None]
    inv = 1.0 / (10000 ** (torch.arange(0, rd, 2, dtype=torch.float32) / rd))[None, :]
    return torch.cos(pos * inv).to(DT[dt]).cuda(), torch.sin(pos * inv).to(DT[dt]).cuda()


def _check(kc, vc, want, name):
    torch.cuda.synchronize()
    R.diff_report(kc, want[0], name + " k_cache")
    R.diff_report(vc, want[1], name + " v_cache")


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_sequence_mode_paged(D, dt):
    """new lengths [0, 1, 37, 130] at cache_seqlens [5, 15, 0, 100]: an empty sequence, one token on the last row of a page, a
    sequence that starts a page and one that crosses nine pages from mid-page"""
    lens, L = [0, 1, 37, 130], [5, 15, 0, 100]
    bt, nblk, nanp = guard.paged_table([a + b for a, b in zip(lens, L)], PAGE, seed=1)
    k, v = rand16((sum(lens), HK, D), dt, 1), rand16((sum(lens), HK, D), dt, 2)
    kc, vc = _cache((nblk, PAGE, HK, D), dt, 3, nan_page=nanp), _cache((nblk, PAGE, HK, D), dt, 4, nan_page=nanp)
    cu = _cu(lens)
    want = R.kv_store_ref(k, v, kc, vc, cu_seqlens=cu, cache_seqlens=L, block_table=bt)
    assert not R.same_bits(want[0], kc)
    _store(k, v, kc, vc, cu_seqlens=_i32(cu), cache_seqlens=_i32(L), block_table=bt.cuda())
    _check(kc, vc, want, "paged")
    # cache_seqlens None = zeros
    kc2, vc2 = _cache((nblk, PAGE, HK, D), dt, 5, nan_page=nanp), _cache((nblk, PAGE, HK, D), dt, 6, nan_page=nanp)
    want = R.kv_store_ref(k, v, kc2, vc2, cu_seqlens=cu, block_table=bt)
    _store(k, v, kc2, vc2, cu_seqlens=_i32(cu), block_table=bt.cuda())
    _check(kc2, vc2, want, "paged, no cache_seqlens")


# 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_sequence_mode_contiguous_with_cache_batch_idx(D, dt):
    """S_max 64, a permuted cache_batch_idx into a cache with more slots than sequences; sequence 1 ends 5 tokens past S_max
    (dropped, the neighbouring slot untouched); k / v carry 7 rows more than cu_seqlens[-1] (ignored)"""
    lens, L, Bc, S = [10, 30, 7], [0, 39, 3], 5, 64
    assert L[1] + lens[1] == S + 5
    bidx = [4, 0, 2]
    k, v = rand16((sum(lens) + 7, HK, D), dt, 1), rand16((sum(lens) + 7, HK, D), dt, 2)
    kc, vc = _cache((Bc, S, HK, D), dt, 3), _cache((Bc, S, HK, D), dt, 4)
    cu = _cu(lens)
    want = R.kv_store_ref(k, v, kc, vc, cu_seqlens=cu, cache_seqlens=L, cache_batch_idx=bidx)
    dest, _ = R.destinations(k.shape[0], kc.shape, cu_seqlens=cu, cache_seqlens=L, cache_batch_idx=bidx)
    assert sum(d is None for d in dest) == 5 + 7
    _store(k, v, kc, vc, cu_seqlens=_i32(cu), cache_seqlens=_i32(L), cache_batch_idx=_i32(bidx))
    _check(kc, vc, want, "contiguous")
    # the identity mapping (no cache_batch_idx)
    kc2, vc2 = _cache((Bc, S, HK, D), dt, 5), _cache((Bc, S, HK, D), dt, 6)
    want = R.kv_store_ref(k, v, kc2, vc2, cu_seqlens=cu, cache_seqlens=L)
    _store(k, v, kc2, vc2, cu_seqlens=_i32(cu), cache_seqlens=_i32(L))
    _check(kc2, vc2, want, "contiguous, identity")


# 3 -------------------------------------------------------------------------------------------------------------------------
def _slots(T, n_slots, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.randperm(n_slots, generator=g)[:T].clone()
    drop = torch.randperm(T, generator=g)[:15]
    s[drop[:13]] = -1
    s[drop[13]] = n_slots
    s[drop[14]] = n_slots + 77
    return s


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_slot_mode_from_packed_qkv_views(D, dt):
    """200 rows to a random permutation of slots, 13 padding rows (-1) and 2 slots at / past the end; k and v are the head
    slices of one packed [200, 4 + 2 x 2, D] qkv, taken without a copy; paged cache and a contiguous one seen as page = S_max"""
    from flash_attn_mi355 import flash_attn_interface as fi
    T, nblk = 200, 20
    qkv = rand16((T, 4 + 2 * HK, D), dt, 1)
    k, v = qkv[:, 4:4 + HK], qkv[:, 4 + HK:]
    assert k.data_ptr() == qkv.data_ptr() + 4 * D * 2 and v.data_ptr() == qkv.data_ptr() + (4 + HK) * D * 2
    assert fi._prep(k, D) is k and fi._prep(v, D) is v          # the wrapper takes the views as they are
    slots = _slots(T, nblk * PAGE, 7)
    for shape, name in (((nblk, PAGE, HK, D), "paged"), ((5, 64, HK, D), "contiguous as page = S_max")):
        kc, vc = _cache(shape, dt, 3), _cache(shape, dt, 4)
        want = R.kv_store_ref(k, v, kc, vc, slot_mapping=slots)
        kc32, vc32 = kc.clone(), vc.clone()
        _store(k, v, kc, vc, slot_mapping=slots.cuda())
        _check(kc, vc, want, name)
        _store(k, v, kc32, vc32, slot_mapping=slots.to(torch.int32).cuda())
        _check(kc32, vc32, want, name + ", int32 slots")


# 4 -------------------------------------------------------------------------------------------------------------------------
def _fp8_inputs(T, D, dt, descale, seed):
    """random rows with the special values in front of every row: +0, -0, values below half the smallest e4m3 subnormal times the
    descale, and exact ties (between codes 16 | 18 | 20, 1 | 1.125 | 1.25, and 0 | 2^-9)"""
    x = rand16((T, HK, D), dt, seed, scale=1.0, device="cpu")
    d = descale
    special = [0.0, -0.0, 2.0 ** -11 * d, -(2.0 ** -11) * d, 2.0 ** -10 * d, -(2.0 ** -10) * d, 17 * d, -17 * d, 19 * d, 1.0625 * d,
               1.1875 * d, -1.1875 * d, 3 * 2.0 ** -10 * d]
    s = torch.tensor(special, dtype=torch.float64)
    assert torch.equal(s.to(DT[dt]).double(), s), "the special values must be exact in the io type"
    x[:, :, :len(special)] = s.to(DT[dt])
    return x.cuda()


@pytest.mark.parametrize("layout", ["wide", "narrow"])
@pytest.mark.parametrize("mode", ["seq", "slot"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_fp8_cache_power_of_two_descales(D, dt, mode, layout):
    """power-of-two descales: x / descale is exact, the codes are bit-exact against the reference - zeros of both signs,
    underflow, exact ties; then a data set on which the reference itself saturates.  `narrow`: the cache is a view at an odd
    multiple of 8 bytes with strides that are no multiple of 16 (8-byte stores instead of 16-byte ones)"""
    lens, L = [1, 37, 0, 70], [15, 0, 3, 20]
    T = sum(lens)
    bt, nblk, nanp = guard.paged_table([a + b for a, b in zip(lens, L)], PAGE, seed=2)
    cu = _cu(lens)
    slots = _slots(T, nblk * PAGE, 9)[:T]
    addr = dict(cu_seqlens=cu, cache_seqlens=L, block_table=bt) if mode == "seq" else dict(slot_mapping=slots)
    dev = ({k_: (v_.cuda() if isinstance(v_, torch.Tensor) else _i32(v_)) for k_, v_ in addr.items()})

    def caches(seed):
        if layout == "wide":
            return _cache((nblk, PAGE, HK, D), dt, seed, fp8=True, nan_page=nanp), None
        big = _cache((nblk, PAGE, HK, D + 8), dt, seed, fp8=True)
        return big[..., 8:], big

    for kd, vd, make in ((0.0625, 0.03125, lambda d, s: _fp8_inputs(T, D, dt, d, s)),
                         (2.0 ** -8, 2.0 ** -8, lambda d, s: rand16((T, HK, D), dt, s, scale=1.5))):
        k, v = make(kd, 1), make(vd, 2)
        (kc, kbig), (vc, vbig) = caches(3), caches(4)
        before = None if kbig is None else (kbig.clone(), vbig.clone())
        want = R.kv_store_ref(k, v, kc, vc, k_descale=kd, v_descale=vd, **addr)
        if kd == 2.0 ** -8:                                 # the case cannot pass vacuously: the reference has both kinds of codes
            dest, _ = R.destinations(T, kc.shape, **addr)
            rows = torch.stack([want[0][d[0], d[1]].float() for d in dest if d is not None])
            sat = float((rows.abs() == 448).float().mean())
            assert 0.15 < sat < 0.35, sat
        _store(k, v, kc, vc, k_descale=kd, v_descale=vd, **dev)
        _check(kc, vc, want, f"fp8 {mode} {layout} descale {kd}")
        if kbig is not None:                                # the 8 columns in front of every head are not the cache's
            assert torch.equal(kbig[..., :8].view(torch.uint8), before[0][..., :8].view(torch.uint8))
            assert torch.equal(vbig[..., :8].view(torch.uint8), before[1][..., :8].view(torch.uint8))


# 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ["none", "interleaved-full", "neox-full", "interleaved-32", "neox-32"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_bitwise_equal_to_the_kvcache_ops_append(D, dt, paged, fp8, rot):
    """the arbiter: a uniform batch appended by flash_attn_with_kvcache(k=, v=) on one copy of the cache and stored by
    store_kv_cache on another leaves the same bits - fp8 codes with non-power-of-two descales and rotated rows included"""
    B, Tn, L = 3, 3, [14, 0, 31]
    knew, vnew = rand16((B, Tn, HK, D), dt, 1, scale=1.5), rand16((B, Tn, HK, D), dt, 2, scale=1.5)
    q = rand16((B, Tn, 2 * HK, D), dt, 3)
    if paged:
        bt, nblk, nanp = guard.paged_table([l + Tn for l in L], PAGE, width=3, seed=4)
        shape, btd = (nblk, PAGE, HK, D), bt.cuda()
    else:
        shape, btd, nanp = (B, 48, HK, D), None, None
    kc_a, vc_a = _cache(shape, dt, 5, fp8=fp8, nan_page=nanp), _cache(shape, dt, 6, fp8=fp8, nan_page=nanp)
    kc_b, vc_b = kc_a.clone(), vc_a.clone()
    kw = dict(k_descale=0.05, v_descale=0.04) if fp8 else {}
    if rot != "none":
        rd = D if rot.endswith("full") else 32
        cos, sin = _rotary(56, rd, dt)
        kw.update(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=rot.startswith("interleaved"))
    _fa().flash_attn_with_kvcache(q, kc_a, vc_a, k=knew, v=vnew, cache_seqlens=_i32(L), block_table=btd, causal=True, **kw)
    _store(knew.reshape(-1, HK, D), vnew.reshape(-1, HK, D), kc_b, vc_b, cu_seqlens=_i32([0, 3, 6, 9]), cache_seqlens=_i32(L),
           block_table=btd, **kw)
    torch.cuda.synchronize()
    R.diff_report(kc_b, kc_a, "k_cache vs the append")
    R.diff_report(vc_b, vc_a, "v_cache vs the append")
    assert not R.same_bits(kc_a, _cache(shape, dt, 5, fp8=fp8, nan_page=nanp))      # (the append did write)


# 6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [True, False], ids=["interleaved", "neox"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D,rd", [(64, 64), (128, 128), (128, 32)])
def test_fused_rope_equals_fa_rotary_then_store(D, rd, dt, fp8, interleaved):
    """ragged lengths [1, 17, 40] at cache_seqlens [3, 0, 30]; the table ends 4 tokens before the last sequence does (those rows
    are stored unrotated).  Fused store == apply_rotary_emb + plain store, bit for bit; V unrotated; one bf16 case also within
    the derived bound of the fp64 rotation"""
    from flash_attn.layers.rotary import apply_rotary_emb
    lens, L = [1, 17, 40], [3, 0, 30]
    seqlen_ro = L[2] + lens[2] - 4
    cos, sin = _rotary(seqlen_ro, rd, dt)
    bt, nblk, nanp = guard.paged_table([a + b for a, b in zip(lens, L)], PAGE, seed=6)
    cu = _cu(lens)
    k, v = rand16((sum(lens), HK, D), dt, 1), rand16((sum(lens), HK, D), dt, 2)
    kc_a, vc_a = _cache((nblk, PAGE, HK, D), dt, 3, fp8=fp8, nan_page=nanp), _cache((nblk, PAGE, HK, D), dt, 4, fp8=fp8, nan_page=nanp)
    kc_b, vc_b = kc_a.clone(), vc_a.clone()
    kw = dict(k_descale=0.05, v_descale=0.04) if fp8 else {}
    addr = dict(cu_seqlens=_i32(cu), cache_seqlens=_i32(L), block_table=bt.cuda())
    want_v = R.kv_store_ref(k, v, kc_a, vc_a, cu_seqlens=cu, cache_seqlens=L, block_table=bt, **kw)[1]
    _store(k, v, kc_a, vc_a, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved, **addr, **kw)
    k_rot = apply_rotary_emb(k, cos, sin, interleaved=interleaved, seqlen_offsets=_i32(L), cu_seqlens=_i32(cu), max_seqlen=max(lens))
    assert not torch.equal(k_rot, k) and torch.equal(k_rot[-4:], k[-4:])
    _store(k_rot, v, kc_b, vc_b, **addr, **kw)
    torch.cuda.synchronize()
    R.diff_report(kc_a, kc_b, "fused rope vs fa_rotary + store")
    R.diff_report(vc_a, want_v, "v_cache (never rotated)")
    R.diff_report(vc_b, want_v, "v_cache")
    if dt == "bf16" and not fp8 and D == 128:
        dest, pos = R.destinations(k.shape[0], kc_a.shape, cu_seqlens=cu, cache_seqlens=L, block_table=bt)
        stored = torch.stack([kc_a[d[0], d[1]] for d in dest])
        y64, mag = rotary_ref.rotary_ref(k, cos, sin, np.asarray(pos), interleaved)
        worst = rotary_ref.worst_ratio(stored, y64, mag, DT[dt])
        print(f"stored K vs the fp64 rotation: worst error / bound = {worst:.3f}")
        assert worst <= 1.0


# 7 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fp16", "bf16", "fp8"])
def test_ragged_prefill_then_paged_reads(kind):
    """ragged prefill -> store -> the same attention through the paged cache -> one decode step"""
    fa = _fa()
    fp8 = kind == "fp8"
    dt = "bf16" if fp8 else kind
    lens, Hq, D = [1, 17, 64, 100], 8, 128
    T, B, mx = sum(lens), len(lens), max(lens)
    q, k, v = rand16((T, Hq, D), dt, 1), rand16((T, HK, D), dt, 2), rand16((T, HK, D), dt, 3)
    cu = _i32(_cu(lens))
    cun = np.asarray(_cu(lens))
    bt, nblk, nanp = guard.paged_table(lens, PAGE, seed=8)
    kc = torch.zeros((nblk, PAGE, HK, D), dtype=DT[dt], device="cuda")
    vc = torch.zeros((nblk, PAGE, HK, D), dtype=DT[dt], device="cuda")
    kw, okw = {}, {}
    if fp8:
        kc, vc = kc.to(FP8), vc.to(FP8)
        kw = dict(k_descale=0.0625, v_descale=0.03125)
    guard.fill_nan(kc[nanp]); guard.fill_nan(vc[nanp])
    out_dense, lse_dense, _ = fa.flash_attn_varlen_func(q, k, v, cu, cu, mx, mx, causal=True, return_attn_probs=True)
    _store(k, v, kc, vc, cu_seqlens=cu, block_table=bt.cuda(), **kw)
    out_paged, lse_paged, _ = fa.flash_attn_varlen_func(q, kc, vc, cu, cu, mx, mx, causal=True, return_attn_probs=True,
                                                        block_table=bt.cuda(), **kw)
    o_ref, lse_ref = oracle.varlen_fwd(f64(q), f64(k), f64(v), cun, cun, mx, mx, D ** -0.5, causal=True)
    assert_close(f64(out_dense), o_ref, dt, "dense prefill")
    assert_lse_close(f64(lse_dense), lse_ref, "dense prefill lse")
    q1 = rand16((B, 1, Hq, D), dt, 4)
    out1, lse1 = fa.flash_attn_with_kvcache(q1, kc, vc, cache_seqlens=_i32(lens), block_table=bt.cuda(), return_softmax_lse=True, **kw)
    if not fp8:
        assert_close(f64(out_paged), o_ref, dt, "paged read of the stored cache")
        assert_lse_close(f64(lse_paged), lse_ref, "paged lse")
        kv, vv = np.nan_to_num(f64(kc)), np.nan_to_num(f64(vc))
        o1_ref, lse1_ref = oracle.kvcache_fwd(f64(q1), kv, vv, cache_seqlens=np.asarray(lens), block_table=bt.numpy(), io_dtype=dt)
        assert_close(f64(out1), o1_ref, dt, "decode step")
        assert_lse_close(f64(lse1), lse1_ref, "decode lse")
    else:
        # the oracle gets the dequantised codes actually stored; gates: the existing fp8 kv-cache tests'
        kv, vv = np.nan_to_num(kc.float().double().cpu().numpy()), np.nan_to_num(vc.float().double().cpu().numpy())
        o8_ref, lse8_ref = oracle.varlen_fwd(f64(q), kv * kw["k_descale"], vv * kw["v_descale"], cun, cun, mx, mx, D ** -0.5,
                                             causal=True, block_table=bt.numpy())
        assert_close(f64(out_paged), o8_ref, dt, "paged read of the stored fp8 cache", mult=1.5)
        assert_lse_close(f64(lse_paged), lse8_ref, "paged lse", atol=LSE_ATOL_FP8)
        o1_ref, lse1_ref = oracle.kvcache_fwd(f64(q1), kv, vv, cache_seqlens=np.asarray(lens), block_table=bt.numpy(), io_dtype=dt, **kw)
        assert_close(f64(out1), o1_ref, dt, "decode step", mult=1.5)
        assert_lse_close(f64(lse1), lse1_ref, "decode lse", atol=LSE_ATOL_FP8)


# 8 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["paged-16bit", "contiguous-16bit", "paged-fp8"])
def test_guard_bands(case):
    """inputs and caches are views with gaps inside NaN-filled slabs: nothing outside a tensor's logical elements is written,
    and a read past k / v would carry NaN into the cache and fail the equality"""
    dt, D = "bf16", 128
    fp8 = case.endswith("fp8")
    lens, L = [3, 0, 41, 20], [14, 7, 0, 30]
    cu = _cu(lens)
    kw = dict(k_descale=0.0625, v_descale=0.03125) if fp8 else {}
    if case.startswith("paged"):
        bt, nblk, nanp = guard.paged_table([a + b for a, b in zip(lens, L)], PAGE, seed=10)
        shape, addr = (nblk, PAGE, HK, D), dict(cu_seqlens=cu, cache_seqlens=L, block_table=bt)
    else:
        shape, nanp, addr = (6, 64, HK, D), None, dict(cu_seqlens=cu, cache_seqlens=L, cache_batch_idx=[5, 1, 3, 0])
    kb, k, ks = guard.guarded(rand16((sum(lens), HK, D), dt, 1))
    vb, v, vs = guard.guarded(rand16((sum(lens), HK, D), dt, 2))
    kcb, kc, kcs = guard.guarded(_cache(shape, dt, 3, fp8=fp8, nan_page=nanp))
    vcb, vc, vcs = guard.guarded(_cache(shape, dt, 4, fp8=fp8, nan_page=nanp))
    want = R.kv_store_ref(k, v, kc, vc, **addr, **kw)
    dev = {k_: (v_.cuda() if isinstance(v_, torch.Tensor) else _i32(v_)) for k_, v_ in addr.items()}
    _store(k, v, kc, vc, **dev, **kw)
    _check(kc, vc, want, case)
    for buf, view, snap, name in ((kb, k, ks, "k"), (vb, v, vs, "v"), (kcb, kc, kcs, "k_cache"), (vcb, vc, vcs, "v_cache")):
        guard.assert_untouched(buf, view, snap, name)
    assert torch.equal(guard.bits(kb), ks) and torch.equal(guard.bits(vb), vs)      # the inputs themselves are read only
    # slot mode on the same slabs
    slots = _slots(sum(lens), shape[0] * shape[1], 12)[:sum(lens)]
    want = R.kv_store_ref(k, v, kc, vc, slot_mapping=slots, **kw)
    _store(k, v, kc, vc, slot_mapping=slots.cuda(), **kw)
    _check(kc, vc, want, case + " slots")
    for buf, view, snap, name in ((kcb, kc, kcs, "k_cache"), (vcb, vc, vcs, "v_cache")):
        guard.assert_untouched(buf, view, snap, name + " (slot mode)")


# 9 -------------------------------------------------------------------------------------------------------------------------
def test_store_and_decode_replay_in_a_graph():
    """store_kv_cache (slot mode, one padding row) followed by a decode call, captured in one graph on one stream; replayed after
    k, v, slot_mapping, q and the lengths were overwritten in place: cache and output equal the eager results bit for bit"""
    fa = _fa()
    dt, D, Hq, B = "bf16", 128, 8, 2
    lens0 = [20, 33]
    bt, nblk, nanp = guard.paged_table([l + 4 for l in lens0], PAGE, seed=14)
    kc0, vc0 = _cache((nblk, PAGE, HK, D), dt, 1, nan_page=nanp), _cache((nblk, PAGE, HK, D), dt, 2, nan_page=nanp)
    btd = bt.cuda()
    steps = 3
    ks = [rand16((B + 1, HK, D), dt, 10 + i) for i in range(steps)]
    vs = [rand16((B + 1, HK, D), dt, 20 + i) for i in range(steps)]
    qs = [rand16((B, 1, Hq, D), dt, 30 + i) for i in range(steps)]
    slots = [torch.tensor([int(bt[b, (l + i) // PAGE]) * PAGE + (l + i) % PAGE for b, l in enumerate(lens0)] + [-1], device="cuda")
             for i in range(steps)]
    lens = [_i32([l + i + 1 for l in lens0]) for i in range(steps)]

    def make_step(kc, vc, k, v, slot, q, n):
        def step():
            _store(k, v, kc, vc, slot_mapping=slot)
            return fa.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=n, block_table=btd, return_softmax_lse=True)
        return step

    kc_e, vc_e = kc0.clone(), vc0.clone()
    ref = []
    for i in range(steps):
        o, lse = make_step(kc_e, vc_e, ks[i], vs[i], slots[i], qs[i], lens[i])()
        ref.append((o.clone(), lse.clone()))
    torch.cuda.synchronize()
    kc_g, vc_g = kc0.clone(), vc0.clone()
    k_s, v_s, slot_s, q_s, n_s = ks[0].clone(), vs[0].clone(), slots[0].clone(), qs[0].clone(), lens[0].clone()
    step = make_step(kc_g, vc_g, k_s, v_s, slot_s, q_s, n_s)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_s, lse_s = step()
    kc_g.copy_(kc0); vc_g.copy_(vc0)
    for i in range(steps):
        k_s.copy_(ks[i]); v_s.copy_(vs[i]); slot_s.copy_(slots[i]); q_s.copy_(qs[i]); n_s.copy_(lens[i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_s, ref[i][0]), f"step {i}: out differs from the eager step"
        assert torch.equal(lse_s, ref[i][1]), f"step {i}: lse differs"
    R.diff_report(kc_g, kc_e, "k_cache after the replays")
    R.diff_report(vc_g, vc_e, "v_cache after the replays")


# 10 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["slot", "seq-rope-fp8"])
def test_torch_op_gives_the_same_bits(mode):
    import flash_attn_mi355.torch_ops  # noqa: F401  (registers the ops)
    dt, D = "fp16", 64
    lens, L = [5, 0, 30], [2, 9, 16]
    bt, nblk, nanp = guard.paged_table([a + b for a, b in zip(lens, L)], PAGE, seed=16)
    fp8 = mode.endswith("fp8")
    k, v = rand16((sum(lens), HK, D), dt, 1), rand16((sum(lens), HK, D), dt, 2)
    kc_a, vc_a = _cache((nblk, PAGE, HK, D), dt, 3, fp8=fp8, nan_page=nanp), _cache((nblk, PAGE, HK, D), dt, 4, fp8=fp8, nan_page=nanp)
    kc_b, vc_b = kc_a.clone(), vc_a.clone()
    if mode == "slot":
        slots = _slots(sum(lens), nblk * PAGE, 18)[:sum(lens)].cuda()
        _store(k, v, kc_a, vc_a, slot_mapping=slots)
        r = torch.ops.flash_attn_mi355.kv_store(k, v, kc_b, vc_b, slots, None, None, None, None, None, None, True, 1.0, 1.0)
    else:
        cos, sin = _rotary(64, 32, dt)
        cu, Ld, btd = _i32(_cu(lens)), _i32(L), bt.cuda()
        _store(k, v, kc_a, vc_a, cu_seqlens=cu, cache_seqlens=Ld, block_table=btd, rotary_cos=cos, rotary_sin=sin,
               rotary_interleaved=False, k_descale=0.05, v_descale=0.04)
        r = torch.ops.flash_attn_mi355.kv_store(k, v, kc_b, vc_b, None, cu, Ld, btd, None, cos, sin, False, 0.05, 0.04)
    assert r is None
    torch.cuda.synchronize()
    assert not R.same_bits(kc_a, _cache((nblk, PAGE, HK, D), dt, 3, fp8=fp8, nan_page=nanp))
    R.diff_report(kc_b, kc_a, "torch op k_cache")
    R.diff_report(vc_b, vc_a, "torch op v_cache")
