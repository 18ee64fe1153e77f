"""GPU: fa_rope_store (flash_attn_mi355.rope_store.rope_and_store_kv) - q and k rotated at per-token positions and K / V stored
into a KV cache by slot, in one launch.  The arbiters are the library's existing ops, bit for bit: per-token rotation is
apply_rotary_emb on the rows seen as T sequences of length 1 with seqlen_offsets = positions, and the cache is what
store_kv_cache(slot_mapping=) leaves of that rotated K (with kv_store_ref's CPU restatement for the whole-cache comparison).
Every case uses the same positions - a ragged-batch run, a block of repeated and decreasing values (tree depths) and three
out-of-table values - and the same kind of slots: a random permutation with 5 padding rows and 2 slots at / past the end."""
import numpy as np
import pytest
import torch

import guard
import kv_store_ref as R
import rotary_ref
from util import LSE_ATOL, LSE_ATOL_FP8, DT, assert_close, assert_lse_close, f64, rand16

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
T, HQ, HK, PAGE, NBLK, SEQLEN_RO = 77, 4, 2, 16, 10, 56
NANP = NBLK - 1                                            # the page no slot names: filled with NaN
N_SLOTS = NBLK * PAGE
ROTS = ["interleaved-full", "neox-full", "interleaved-32", "neox-32"]


def _fa():
    import flash_attn
    return flash_attn


def _rs(*a, **kw):
    from flash_attn_mi355.rope_store import rope_and_store_kv
    return rope_and_store_kv(*a, **kw)


def _store(*a, **kw):
    from flash_attn_mi355.kv_store import store_kv_cache
    return store_kv_cache(*a, **kw)


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


def _positions():
    """77 positions: a ragged batch (lengths 20, 1, 25 at offsets 3, 40, 7), 28 tree nodes at len + depth (repeated and
    decreasing values), then -1, seqlen_ro and seqlen_ro + 5.  No position is 0: the rotation by 0 is the identity."""
    ragged = [3 + i for i in range(20)] + [40] + [7 + i for i in range(25)]
    tree = [30, 31, 31, 32, 32, 32, 31, 30, 30, 29, 33, 33, 32, 31, 34, 34, 33, 30, 29, 28, 28, 31, 32, 35, 35, 34, 33, 30]
    pos = ragged + tree + [-1, SEQLEN_RO, SEQLEN_RO + 5]
    assert len(pos) == T and 0 not in pos
    return torch.tensor(pos, dtype=torch.int64)


def _slots(seed):
    """a random permutation of the slots of the pages 0 .. NBLK - 2 with 5 entries of -1, one n_slots and one n_slots + 77"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randperm(NANP * PAGE, generator=g)[:T].clone()
    drop = torch.randperm(T - 3, generator=g)[:7]          # (the three out-of-table rows keep their slots)
    s[drop[:5]] = -1
    s[drop[5]] = N_SLOTS
    s[drop[6]] = N_SLOTS + 77
    return s


def _tables(rot, D, dt):
    rd = D if rot.endswith("full") else int(rot.split("-")[1])
    pos = torch.arange(SEQLEN_RO, dtype=torch.float32)[:, None]
    inv = 1.0 / (10000 ** (torch.arange(0, rd, 2, dtype=torch.float32) / rd))[None, :]
    return torch.cos(pos * inv).to(DT[dt]).cuda(), torch.sin(pos * inv).to(DT[dt]).cuda(), rot.startswith("interleaved")


def _cache(D, dt, seed, kind="16bit"):
    """a pre-filled cache [NBLK, PAGE, HK, D] (random data; fp8: random codes of finite values) whose last page is NaN.
    kind 'fp8-narrow': a view at an odd multiple of 8 bytes with strides that are no multiple of 16 (8-byte stores); returns
    (cache, the tensor it is a view of or None)"""
    wide = D + 8 if kind == "fp8-narrow" else D
    c = rand16((NBLK, PAGE, HK, wide), dt, seed, scale=2.0)
    if kind != "16bit":
        c = c.to(FP8)
    guard.fill_nan(c[NANP])
    return (c[..., 8:], c) if kind == "fp8-narrow" else (c, None)


def _arbiter(x, cos, sin, interleaved, positions):
    """per-token rotation on the existing op: every row a sequence of length 1 at offset positions[r]"""
    from flash_attn.layers.rotary import apply_rotary_emb
    y = apply_rotary_emb(x.unsqueeze(1), cos, sin, interleaved=interleaved, seqlen_offsets=positions.to(torch.int32).cuda())
    return y.squeeze(1)


def _check_arbiter_rotates(x, y):
    """the reference itself rotates at least 60 rows and leaves exactly the 3 out-of-table rows as they were"""
    same = [bool(torch.equal(x[r], y[r])) for r in range(T)]
    assert sum(not s for s in same) >= 60 and same[-3:] == [True] * 3 and sum(same) == 3, same


def _bits(t):
    return t.contiguous().view(torch.int16)


def _eq(got, want, name):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    ne = _bits(got) != _bits(want)
    if ne.any():
        first = tuple(int(i) for i in torch.nonzero(ne)[0])
        raise AssertionError(f"{name}: {int(ne.sum())} of {ne.numel()} elements differ; first at (row, head, col) = {first}: "
                             f"got {float(got[first])}, expected {float(want[first])}")


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", ["16bit", "fp8-wide", "fp8-narrow"])
@pytest.mark.parametrize("rot", ROTS)
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_bits_against_the_composition(D, dt, rot, cache):
    """q_out, k_out, the whole k_cache and the whole v_cache == apply_rotary_emb per token + store_kv_cache by slot, bit for bit
    (fp8: the non-power-of-two descales 0.05 / 0.04; narrow: 8-byte stores, the 8 columns in front of every head untouched)"""
    cos, sin, il = _tables(rot, D, dt)
    pos, slots = _positions(), _slots(7)
    q, k, v = rand16((T, HQ, D), dt, 1), rand16((T, HK, D), dt, 2), rand16((T, HK, D), dt, 3)
    q0, k0, v0 = q.clone(), k.clone(), v.clone()
    (kc, kbig), (vc, vbig) = _cache(D, dt, 4, cache), _cache(D, dt, 5, cache)
    (kc_b, _), (vc_b, _) = _cache(D, dt, 4, cache), _cache(D, dt, 5, cache)
    before = None if kbig is None else (kbig.clone(), vbig.clone())
    kw = dict(k_descale=0.05, v_descale=0.04) if cache != "16bit" else {}
    q_ref, k_ref = _arbiter(q, cos, sin, il, pos), _arbiter(k, cos, sin, il, pos)
    _check_arbiter_rotates(q, q_ref)
    _check_arbiter_rotates(k, k_ref)
    want = R.kv_store_ref(k_ref, v, kc_b, vc_b, slot_mapping=slots, **kw)
    _store(k_ref, v, kc_b, vc_b, slot_mapping=slots.cuda(), **kw)
    q_out, k_out = _rs(q, k, v, pos.cuda(), cos, sin, kc, vc, slots.cuda(), interleaved=il, inplace=False, **kw)
    torch.cuda.synchronize()
    _eq(q_out, q_ref, "q_out")
    _eq(k_out, k_ref, "k_out")
    R.diff_report(kc, kc_b, "k_cache vs apply_rotary_emb + store_kv_cache")
    R.diff_report(vc, vc_b, "v_cache vs store_kv_cache")
    R.diff_report(kc, want[0], "k_cache vs kv_store_ref")
    R.diff_report(vc, want[1], "v_cache vs kv_store_ref")
    assert not R.same_bits(kc, _cache(D, dt, 4, cache)[0]) and not R.same_bits(vc, _cache(D, dt, 5, cache)[0])   # the call did write
    _eq(q, q0, "q (read only)"); _eq(k, k0, "k (read only)"); _eq(v, v0, "v (read only)")
    if kbig is not None:                                    # the 8 columns in front of every head are not the cache's
        assert torch.equal(kbig[..., :8].view(torch.uint8), before[0][..., :8].view(torch.uint8))
        assert torch.equal(vbig[..., :8].view(torch.uint8), before[1][..., :8].view(torch.uint8))


@pytest.mark.parametrize("cache", ["16bit", "fp8-wide"])
@pytest.mark.parametrize("rot", ["interleaved-16", "neox-16", "interleaved-48", "neox-48"])
def test_rotary_dims_that_are_no_multiple_of_32(rot, cache):
    """rotary_dim 16 and 48 of D 64: a NeoX half of 8 or 24 columns holds no whole 16-column runs, so an fp8 cache that could
    take 16-byte stores gets 8-byte ones there (interleaved keeps the 16-byte stores); the same bits as the composition"""
    D, dt = 64, "bf16"
    cos, sin, il = _tables(rot, D, dt)
    pos, slots = _positions(), _slots(9)
    q, k, v = rand16((T, HQ, D), dt, 1), rand16((T, HK, D), dt, 2), rand16((T, HK, D), dt, 3)
    (kc, _), (vc, _) = _cache(D, dt, 4, cache), _cache(D, dt, 5, cache)
    kc_b, vc_b = kc.clone(), vc.clone()
    kw = dict(k_descale=0.05, v_descale=0.04) if cache != "16bit" else {}
    q_ref, k_ref = _arbiter(q, cos, sin, il, pos), _arbiter(k, cos, sin, il, pos)
    _check_arbiter_rotates(k, k_ref)
    _store(k_ref, v, kc_b, vc_b, slot_mapping=slots.cuda(), **kw)
    q_out, k_out = _rs(q, k, v, pos.cuda(), cos, sin, kc, vc, slots.cuda(), interleaved=il, inplace=False, **kw)
    torch.cuda.synchronize()
    _eq(q_out, q_ref, "q_out")
    _eq(k_out, k_ref, "k_out")
    R.diff_report(kc, kc_b, "k_cache")
    R.diff_report(vc, vc_b, "v_cache")
    qi, ki = q.clone(), k.clone()
    _rs(qi, ki, None, pos.cuda(), cos, sin, interleaved=il)           # and in place, rotate only
    torch.cuda.synchronize()
    _eq(qi, q_ref, "q in place")
    _eq(ki, k_ref, "k in place")


# 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ROTS)
@pytest.mark.parametrize("D", [64, 128])
def test_in_place_on_one_packed_qkv(D, rot):
    """q, k and v are the head slices of one packed [77, 4 + 2 x 2, D] qkv, taken without a copy and rotated where they are: the
    q and k heads equal the out-of-place result bit for bit (one lane owns both partner pieces of a NeoX pair: nothing is read
    after its partner was written), the v heads are unchanged, and with rotary_dim 32 the columns 32.. are untouched in place and
    copied out of place"""
    from flash_attn_mi355 import flash_attn_interface as fi
    dt = "bf16"
    cos, sin, il = _tables(rot, D, dt)
    rd = 2 * cos.shape[1]
    pos, slots = _positions().cuda(), _slots(11).cuda()
    qkv = rand16((T, HQ + 2 * HK, D), dt, 1)
    qkv0 = qkv.clone()
    q, k, v = qkv[:, :HQ], qkv[:, HQ:HQ + HK], qkv[:, HQ + HK:]
    assert k.data_ptr() == qkv.data_ptr() + HQ * D * 2 and v.data_ptr() == qkv.data_ptr() + (HQ + HK) * D * 2
    assert fi._prep(q, D) is q and fi._prep(k, D) is k and fi._prep(v, D) is v      # the wrapper takes the views as they are
    (kc_a, _), (vc_a, _) = _cache(D, dt, 4), _cache(D, dt, 5)
    kc_b, vc_b = kc_a.clone(), vc_a.clone()
    q_out, k_out = _rs(q, k, v, pos, cos, sin, kc_a, vc_a, slots, interleaved=il, inplace=False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(qkv), _bits(qkv0))                 # out of place: the packed buffer is read only
    _eq(q_out, _arbiter(qkv0[:, :HQ], cos, sin, il, pos.cpu()), "q_out vs the arbiter")
    _eq(q_out[..., rd:], qkv0[:, :HQ, rd:], "q_out columns behind rotary_dim (copied)")
    _eq(k_out[..., rd:], qkv0[:, HQ:HQ + HK, rd:], "k_out columns behind rotary_dim (copied)")
    rq, rk = _rs(q, k, v, pos, cos, sin, kc_b, vc_b, slots, interleaved=il)
    torch.cuda.synchronize()
    assert rq.data_ptr() == q.data_ptr() and rk.data_ptr() == k.data_ptr() and rq.stride() == q.stride()
    _eq(qkv[:, :HQ], q_out, "q heads in place")
    _eq(qkv[:, HQ:HQ + HK], k_out, "k heads in place")
    _eq(qkv[:, HQ + HK:], qkv0[:, HQ + HK:], "v heads (unchanged)")
    _eq(qkv[:, :HQ + HK, rd:], qkv0[:, :HQ + HK, rd:], "columns behind rotary_dim (untouched in place)")
    assert not torch.equal(_bits(qkv[:, :HQ + HK]), _bits(qkv0[:, :HQ + HK]))
    R.diff_report(kc_b, kc_a, "k_cache, in place vs out of place")
    R.diff_report(vc_b, vc_a, "v_cache, in place vs out of place")


# 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("il", [True, False], ids=["interleaved", "neox"])
def test_optional_forms(il):
    """q=None; k_out=False (k unchanged, the cache still rotated); rotate only (no caches); int32 positions / slot_mapping"""
    D, dt = 128, "fp16"
    cos, sin, _ = _tables("neox-32", D, dt)
    pos, slots = _positions(), _slots(13)
    q, k, v = rand16((T, HQ, D), dt, 1), rand16((T, HK, D), dt, 2), rand16((T, HK, D), dt, 3)
    q_ref, k_ref = _arbiter(q, cos, sin, il, pos), _arbiter(k, cos, sin, il, pos)
    (kc0, _), (vc0, _) = _cache(D, dt, 4), _cache(D, dt, 5)
    kc_w, vc_w = kc0.clone(), vc0.clone()
    _store(k_ref, v, kc_w, vc_w, slot_mapping=slots.cuda())
    # the full call with int32 ids, in place
    qa, ka, kc, vc = q.clone(), k.clone(), kc0.clone(), vc0.clone()
    r = _rs(qa, ka, v, pos.to(torch.int32).cuda(), cos, sin, kc, vc, slots.to(torch.int32).cuda(), interleaved=il)
    torch.cuda.synchronize()
    assert r[0] is qa and r[1] is ka
    _eq(qa, q_ref, "q (int32 ids)"); _eq(ka, k_ref, "k (int32 ids)")
    R.diff_report(kc, kc_w, "k_cache (int32 ids)"); R.diff_report(vc, vc_w, "v_cache (int32 ids)")
    # q=None
    ka, kc, vc = k.clone(), kc0.clone(), vc0.clone()
    r = _rs(None, ka, v, pos.cuda(), cos, sin, kc, vc, slots.cuda(), interleaved=il)
    torch.cuda.synchronize()
    assert r[0] is None and r[1] is ka
    _eq(ka, k_ref, "k (q=None)")
    R.diff_report(kc, kc_w, "k_cache (q=None)"); R.diff_report(vc, vc_w, "v_cache (q=None)")
    # k_out=False, in place and out of place
    for inplace in (True, False):
        qa, ka, kc, vc = q.clone(), k.clone(), kc0.clone(), vc0.clone()
        r = _rs(qa, ka, v, pos.cuda(), cos, sin, kc, vc, slots.cuda(), interleaved=il, k_out=False, inplace=inplace)
        torch.cuda.synchronize()
        assert r[1] is None and (r[0] is qa) == inplace
        _eq(r[0], q_ref, "q_out (k_out=False)")
        _eq(ka, k, "k (k_out=False: unchanged)")
        R.diff_report(kc, kc_w, "k_cache (k_out=False: still rotated)"); R.diff_report(vc, vc_w, "v_cache (k_out=False)")
    # rotate only
    qa, ka = q.clone(), k.clone()
    r = _rs(qa, ka, None, pos.cuda(), cos, sin, interleaved=il)
    torch.cuda.synchronize()
    _eq(qa, q_ref, "q (rotate only, in place)"); _eq(ka, k_ref, "k (rotate only, in place)")
    r = _rs(q, k, None, pos.cuda(), cos, sin, interleaved=il, inplace=False)
    torch.cuda.synchronize()
    _eq(r[0], q_ref, "q_out (rotate only)"); _eq(r[1], k_ref, "k_out (rotate only)")
    r = _rs(None, k, None, pos.cuda(), cos, sin, interleaved=il, inplace=False)
    torch.cuda.synchronize()
    assert r[0] is None
    _eq(r[1], k_ref, "k_out (rotate only, q=None)")


# 4 -------------------------------------------------------------------------------------------------------------------------
def test_padding_rows_are_rotated_and_unnamed_slots_untouched():
    """rows with slot -1 (and the two slots at / past the end) still get their q_out / k_out; the cache keeps its bits at every
    slot that no row names"""
    D, dt = 128, "bf16"
    cos, sin, il = _tables("neox-full", D, dt)
    pos, slots = _positions(), _slots(15)
    q, k, v = rand16((T, HQ, D), dt, 1), rand16((T, HK, D), dt, 2), rand16((T, HK, D), dt, 3)
    (kc, _), (vc, _) = _cache(D, dt, 4), _cache(D, dt, 5)
    kc0, vc0 = kc.clone(), vc.clone()
    q_out, k_out = _rs(q, k, v, pos.cuda(), cos, sin, kc, vc, slots.cuda(), interleaved=il, inplace=False)
    torch.cuda.synchronize()
    pad = [r for r in range(T) if not 0 <= int(slots[r]) < N_SLOTS]
    assert len(pad) == 7 and sum(int(slots[r]) == -1 for r in pad) == 5
    q_ref, k_ref = _arbiter(q, cos, sin, il, pos), _arbiter(k, cos, sin, il, pos)
    for r in pad:
        assert torch.equal(q_out[r], q_ref[r]) and torch.equal(k_out[r], k_ref[r]), r
        assert not torch.equal(q_out[r], q[r]) and not torch.equal(k_out[r], k[r]), r
    named = torch.zeros(N_SLOTS, dtype=torch.bool)
    named[slots[(slots >= 0) & (slots < N_SLOTS)]] = True
    assert int(named.sum()) == T - 7
    un = ~named.cuda()
    for c, c0, name in ((kc, kc0, "k_cache"), (vc, vc0, "v_cache")):
        a, b = c.view(torch.int16).reshape(N_SLOTS, -1), c0.view(torch.int16).reshape(N_SLOTS, -1)
        assert torch.equal(a[un], b[un]), f"{name}: a slot that no row names was written"
        assert not (a[~un] == b[~un]).all(dim=1).any(), f"{name}: a named slot kept its pre-fill"


# 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("il", [True, False], ids=["interleaved", "neox"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_equal_to_the_kvcache_ops_fused_append(paged, fp8, il):
    """a uniform batch (B 3, T_new 3, lengths 14, 0, 31): rope_and_store_kv at positions cache_seqlens[b] + i and the slots those
    positions map to leaves the cache flash_attn_with_kvcache(k=, v=, rotary_cos=) leaves, bit for bit; and the kv-cache op on
    the pre-rotated q, without k / v and with advanced lengths, agrees with the fused-append call within the dtype gate"""
    fa = _fa()
    dt, D, B, Tn, L = "bf16", 128, 3, 3, [14, 0, 31]
    knew, vnew = rand16((B, Tn, HK, D), dt, 1, scale=1.5), rand16((B, Tn, HK, D), dt, 2, scale=1.5)
    q = rand16((B, Tn, 2 * HK, D), dt, 3)
    if paged:
        bt, nblk, nanp = guard.paged_table([l + Tn for l in L], PAGE, width=3, seed=4)
        shape, btd = (nblk, PAGE, HK, D), bt.cuda()
        slot = lambda b, p: int(bt[b, p // PAGE]) * PAGE + p % PAGE       # noqa: E731
    else:
        shape, btd, nanp = (B, 48, HK, D), None, None
        slot = lambda b, p: b * 48 + p                                     # noqa: E731  (a contiguous cache: page = S_max)
    kc_a = rand16(shape, dt, 5, scale=2.0)
    vc_a = rand16(shape, dt, 6, scale=2.0)
    if fp8:
        kc_a, vc_a = kc_a.to(FP8), vc_a.to(FP8)
    if nanp is not None:
        guard.fill_nan(kc_a[nanp]); guard.fill_nan(vc_a[nanp])
    kc0, kc_b, vc_b = kc_a.clone(), kc_a.clone(), vc_a.clone()
    kw = dict(k_descale=0.05, v_descale=0.04) if fp8 else {}
    cos, sin, _ = _tables("neox-full", D, dt)
    out_a, lse_a = fa.flash_attn_with_kvcache(q, kc_a, vc_a, k=knew, v=vnew, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=il,
                                              cache_seqlens=_i32(L), block_table=btd, causal=True, return_softmax_lse=True, **kw)
    pos = torch.tensor([L[b] + i for b in range(B) for i in range(Tn)], device="cuda")
    slots = torch.tensor([slot(b, L[b] + i) for b in range(B) for i in range(Tn)], device="cuda")
    q_rot, _ = _rs(q.view(-1, 2 * HK, D), knew.view(-1, HK, D), vnew.view(-1, HK, D), pos, cos, sin, kc_b, vc_b, slots,
                   interleaved=il, inplace=False, k_out=False, **kw)
    torch.cuda.synchronize()
    assert not R.same_bits(kc_a, kc0)                            # (the append did write)
    R.diff_report(kc_b, kc_a, "k_cache vs the fused append")
    R.diff_report(vc_b, vc_a, "v_cache vs the fused append")
    out_b, lse_b = fa.flash_attn_with_kvcache(q_rot.view(B, Tn, 2 * HK, D), kc_b, vc_b, cache_seqlens=_i32([l + Tn for l in L]),
                                              block_table=btd, causal=True, return_softmax_lse=True, **kw)
    assert_close(f64(out_b), f64(out_a), dt, "pre-rotated q on the stored cache vs the fused append", mult=1.5 if fp8 else 1.0)
    assert_lse_close(f64(lse_b), f64(lse_a), "lse", atol=LSE_ATOL_FP8 if fp8 else LSE_ATOL)


# 6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("il", [True, False], ids=["interleaved", "neox"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_within_the_derived_bound_of_the_fp64_rotation(dt, il):
    """q_out and the stored 16-bit K against rotary_ref.rotary_ref: worst error / rotary_ref.bound <= 1 (one rounding of the exact
    result to the io type plus the fp32 evaluation: the derived bound, not a tuned one)"""
    D = 128
    cos, sin, _ = _tables("neox-full", D, dt)
    pos, slots = _positions(), _slots(17)
    q, k, v = rand16((T, HQ, D), dt, 1), rand16((T, HK, D), dt, 2), rand16((T, HK, D), dt, 3)
    (kc, _), (vc, _) = _cache(D, dt, 4), _cache(D, dt, 5)
    q_out, _ = _rs(q, k, v, pos.cuda(), cos, sin, kc, vc, slots.cuda(), interleaved=il, inplace=False, k_out=False)
    torch.cuda.synchronize()
    y64, mag = rotary_ref.rotary_ref(q, cos, sin, pos.numpy(), il)
    assert np.abs(y64 - f64(q)).max() > 0.5                      # (the reference rotates)
    worst_q = rotary_ref.worst_ratio(q_out, y64, mag, DT[dt])
    rows = [r for r in range(T) if 0 <= int(slots[r]) < N_SLOTS]
    stored = torch.stack([kc[int(slots[r]) // PAGE, int(slots[r]) % PAGE] for r in rows])
    y64, mag = rotary_ref.rotary_ref(k[rows], cos, sin, pos.numpy()[rows], il)
    worst_k = rotary_ref.worst_ratio(stored, y64, mag, DT[dt])
    print(f"worst error / bound: q_out {worst_q:.3f}, stored K {worst_k:.3f}")
    assert worst_q <= 1.0 and worst_k <= 1.0


# 7 -------------------------------------------------------------------------------------------------------------------------
def _guarded_ids(x):
    """an int64 tensor of exactly len(x) elements in the middle of a larger buffer, which must come back unchanged"""
    buf = torch.full((4096 + len(x) + 4096,), -1, dtype=torch.int64, device="cuda")
    view = buf[4096:4096 + len(x)]
    view.copy_(x)
    return buf, view


@pytest.mark.parametrize("case", ["16bit-neox", "fp8-interleaved", "16bit-neox-32-inplace"])
def test_guard_bands(case):
    """q, k, v, the outputs and the caches are views with gaps inside NaN-filled slabs: nothing outside a tensor's logical
    elements is written, a read past an input would carry NaN into the results, and the inputs are bit-unchanged out of place;
    positions / slot_mapping are exactly T long inside guarded buffers"""
    dt, D = "bf16", 128
    fp8, inplace = case.startswith("fp8"), case.endswith("inplace")
    cos, sin, il = _tables("interleaved-full" if "interleaved" in case else ("neox-32" if "32" in case else "neox-full"), D, dt)
    pos, slots = _positions(), _slots(19)
    kw = dict(k_descale=0.05, v_descale=0.04) if fp8 else {}
    qb, q, qs = guard.guarded(rand16((T, HQ, D), dt, 1))
    kb, k, ks = guard.guarded(rand16((T, HK, D), dt, 2))
    vb, v, vs = guard.guarded(rand16((T, HK, D), dt, 3))
    kcb, kc, kcs = guard.guarded(_cache(D, dt, 4, "fp8-wide" if fp8 else "16bit")[0])
    vcb, vc, vcs = guard.guarded(_cache(D, dt, 5, "fp8-wide" if fp8 else "16bit")[0])
    pb, pv = _guarded_ids(pos)
    sb, sv = _guarded_ids(slots)
    pb0, sb0 = pb.clone(), sb.clone()
    q_ref, k_ref = _arbiter(q, cos, sin, il, pos), _arbiter(k, cos, sin, il, pos)
    want = R.kv_store_ref(k_ref, v, kc, vc, slot_mapping=slots, **kw)
    checks = [(vb, v, vs, "v"), (kcb, kc, kcs, "k_cache"), (vcb, vc, vcs, "v_cache")]
    if inplace:
        r = _rs(q, k, v, pv, cos, sin, kc, vc, sv, interleaved=il, **kw)
        assert r[0] is q and r[1] is k
        q_out, k_out = q, k
        checks += [(qb, q, qs, "q (in place)"), (kb, k, ks, "k (in place)")]
    else:
        qob, q_out, qos = guard.guarded(shape=(T, HQ, D), dtype=DT[dt], device="cuda")
        kob, k_out, kos = guard.guarded(shape=(T, HK, D), dtype=DT[dt], device="cuda")
        _call_into(q, k, v, q_out, k_out, pv, sv, cos, sin, kc, vc, il, kw)
        checks += [(qb, q, qs, "q"), (kb, k, ks, "k"), (qob, q_out, qos, "q_out"), (kob, k_out, kos, "k_out")]
    torch.cuda.synchronize()
    _eq(q_out, q_ref, "q_out")
    _eq(k_out, k_ref, "k_out")
    R.diff_report(kc, want[0], case + " k_cache")
    R.diff_report(vc, want[1], case + " v_cache")
    for buf, view, snap, name in checks:
        guard.assert_untouched(buf, view, snap, name)
    assert torch.equal(guard.bits(vb), vs)                       # v itself is read only
    if not inplace:
        assert torch.equal(guard.bits(qb), qs) and torch.equal(guard.bits(kb), ks)
    assert torch.equal(pb, pb0) and torch.equal(sb, sb0)


def _call_into(q, k, v, q_out, k_out, pos, slots, cos, sin, kc, vc, il, kw):
    """fa_rope_store with caller-owned strided outputs (the Python function allocates contiguous ones): the C ABI through the
    ctypes mirror, filled the way rope_and_store_kv fills it"""
    import ctypes
    from flash_attn_mi355 import _lib
    from flash_attn_mi355 import flash_attn_interface as fi
    s = _lib.FaRopeStoreParams()
    s.struct_size = ctypes.sizeof(_lib.FaRopeStoreParams)
    s.q, s.k, s.v, s.q_out, s.k_out = q.data_ptr(), k.data_ptr(), v.data_ptr(), q_out.data_ptr(), k_out.data_ptr()
    s.q_row_stride, s.q_head_stride = q.stride(0), q.stride(1)
    s.k_row_stride, s.k_head_stride = k.stride(0), k.stride(1)
    s.v_row_stride, s.v_head_stride = v.stride(0), v.stride(1)
    s.qo_row_stride, s.qo_head_stride = q_out.stride(0), q_out.stride(1)
    s.ko_row_stride, s.ko_head_stride = k_out.stride(0), k_out.stride(1)
    s.positions, s.slot_mapping = pos.data_ptr(), slots.data_ptr()
    s.rotary_cos, s.rotary_sin = cos.data_ptr(), sin.data_ptr()
    s.rotary_dim, s.seqlen_ro, s.rotary_interleaved = 2 * cos.shape[1], cos.shape[0], int(il)
    s.total_rows, s.nheads_q, s.nheads_k, s.head_dim = q.shape[0], q.shape[1], k.shape[1], q.shape[2]
    s.dtype = fi._DTYPES[q.dtype]
    s.cache_dtype = _lib.FA_FP8_E4M3 if kc.dtype == FP8 else s.dtype
    s.k_cache, s.v_cache = kc.data_ptr(), vc.data_ptr()
    s.kc_batch_stride, s.kc_row_stride, s.kc_head_stride = kc.stride(0), kc.stride(1), kc.stride(2)
    s.vc_batch_stride, s.vc_row_stride, s.vc_head_stride = vc.stride(0), vc.stride(1), vc.stride(2)
    s.num_blocks, s.page_block_size = kc.shape[0], kc.shape[1]
    s.k_descale, s.v_descale = kw.get("k_descale", 0.0), kw.get("v_descale", 0.0)
    _lib.call_rope_store(s, fi._stream(q.device))


# 8 -------------------------------------------------------------------------------------------------------------------------
def test_prologue_and_decode_replay_in_a_graph():
    """rope_and_store_kv (in place on a packed qkv, one padding row) followed by a decode call, captured in one graph on one
    stream; replayed after qkv, positions, slot_mapping and the lengths were overwritten in place: q, the caches and the output
    equal the eager results bit for bit"""
    fa = _fa()
    dt, D, Hq, B = "bf16", 128, 8, 2
    lens0 = [20, 33]
    bt, nblk, nanp = guard.paged_table([l + 4 for l in lens0], PAGE, seed=14)
    kc0, vc0 = rand16((nblk, PAGE, HK, D), dt, 1, scale=2.0), rand16((nblk, PAGE, HK, D), dt, 2, scale=2.0)
    guard.fill_nan(kc0[nanp]); guard.fill_nan(vc0[nanp])
    btd = bt.cuda()
    cos, sin, _ = _tables("neox-full", D, dt)
    steps = 3
    qkvs = [rand16((B + 1, Hq + 2 * HK, D), dt, 10 + i) for i in range(steps)]
    poss = [torch.tensor([l + i for l in lens0] + [0], device="cuda") for i in range(steps)]
    slots = [torch.tensor([int(bt[b, (l + i) // PAGE]) * PAGE + (l + i) % PAGE for b, l in enumerate(lens0)] + [-1], device="cuda")
             for i in range(steps)]
    lens = [_i32([l + i + 1 for l in lens0]) for i in range(steps)]

    def make_step(kc, vc, qkv, pos, slot, n):
        q, k, v = qkv[:, :Hq], qkv[:, Hq:Hq + HK], qkv[:, Hq + HK:]

        def step():
            _rs(q, k, v, pos, cos, sin, kc, vc, slot)
            return fa.flash_attn_with_kvcache(q[:B].unsqueeze(1), kc, vc, cache_seqlens=n, block_table=btd, return_softmax_lse=True)
        return step

    kc_e, vc_e = kc0.clone(), vc0.clone()
    ref = []
    for i in range(steps):
        x = qkvs[i].clone()
        o, lse = make_step(kc_e, vc_e, x, poss[i], slots[i], lens[i])()
        ref.append((o.clone(), lse.clone(), x))
    torch.cuda.synchronize()
    assert not torch.equal(ref[0][2][:B, :Hq + HK], qkvs[0][:B, :Hq + HK])      # (the eager steps rotate)
    kc_g, vc_g = kc0.clone(), vc0.clone()
    x_s, p_s, slot_s, n_s = qkvs[0].clone(), poss[0].clone(), slots[0].clone(), lens[0].clone()
    step = make_step(kc_g, vc_g, x_s, p_s, slot_s, n_s)
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
        x_s.copy_(qkvs[i]); p_s.copy_(poss[i]); slot_s.copy_(slots[i]); n_s.copy_(lens[i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_s, ref[i][0]), f"step {i}: out differs from the eager step"
        assert torch.equal(lse_s, ref[i][1]), f"step {i}: lse differs"
        assert torch.equal(_bits(x_s), _bits(ref[i][2])), f"step {i}: the rotated qkv differs"
    R.diff_report(kc_g, kc_e, "k_cache after the replays")
    R.diff_report(vc_g, vc_e, "v_cache after the replays")


# 9 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_torch_op_gives_the_same_bits(fp8):
    import flash_attn_mi355.torch_ops  # noqa: F401  (registers the ops)
    dt, D = "fp16", 64
    cos, sin, il = _tables("neox-32" if fp8 else "interleaved-full", D, dt)
    pos, slots = _positions().cuda(), _slots(21).cuda()
    kind = "fp8-wide" if fp8 else "16bit"
    qkv_a = rand16((T, HQ + 2 * HK, D), dt, 1)
    qkv_b = qkv_a.clone()
    (kc_a, _), (vc_a, _) = _cache(D, dt, 4, kind), _cache(D, dt, 5, kind)
    kc_b, vc_b = kc_a.clone(), vc_a.clone()
    kw = dict(k_descale=0.05, v_descale=0.04) if fp8 else {}
    _rs(qkv_a[:, :HQ], qkv_a[:, HQ:HQ + HK], qkv_a[:, HQ + HK:], pos, cos, sin, kc_a, vc_a, slots, interleaved=il, **kw)
    r = torch.ops.flash_attn_mi355.rope_store_(qkv_b[:, :HQ], qkv_b[:, HQ:HQ + HK], qkv_b[:, HQ + HK:], pos, cos, sin, kc_b, vc_b,
                                               slots, il, kw.get("k_descale", 1.0), kw.get("v_descale", 1.0))
    assert r is None
    torch.cuda.synchronize()
    assert not torch.equal(_bits(qkv_a), _bits(rand16((T, HQ + 2 * HK, D), dt, 1)))
    assert not R.same_bits(kc_a, _cache(D, dt, 4, kind)[0])
    assert torch.equal(_bits(qkv_b), _bits(qkv_a))
    R.diff_report(kc_b, kc_a, "torch op k_cache")
    R.diff_report(vc_b, vc_a, "torch op v_cache")
