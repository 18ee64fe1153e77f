"""GPU: fa_qk_norm_rope_store (flash_attn_mi355.qk_norm) - a per-head RMSNorm of q and k, the rotation at per-token positions and
the K / V store by slot, in one launch.  The norm alone is held against the fp64 restatement (qk_norm_ref) within a derived bound;
everything else is held against the library's own ops, bit for bit: the fused call == qk_rms_norm followed by rope_and_store_kv.
Every case uses T = 77 rows, Hq 4, Hk 2, pages of 16 rows, 10 pages (the last one NaN and named by no slot), the positions of a
ragged batch, a block of tree depths and three out-of-table values, slots that are a random permutation with 5 padding rows and 2
slots at / past the end (the patterns of test_rope_store_gpu.py), and weights 1 + 0.2 randn."""
import numpy as np
import pytest
import torch

import guard
import kv_store_ref as R
import qk_norm_ref as N
from util import DT, rand16

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
T, HQ, HK, PAGE, NBLK, SEQLEN_RO = 77, 4, 2, 16, 10, 56
NANP = NBLK - 1                                            # the page no slot names: filled with NaN
N_SLOTS = NBLK * PAGE
ROTS = ["interleaved-full", "neox-full", "interleaved-32", "neox-32"]
EPS = 1e-6
DESCALES = dict(k_descale=0.05, v_descale=0.04)


def _fused(*a, **kw):
    from flash_attn_mi355.qk_norm import qk_norm_rope_and_store_kv
    return qk_norm_rope_and_store_kv(*a, **kw)


def _norm(*a, **kw):
    from flash_attn_mi355.qk_norm import qk_rms_norm
    return qk_rms_norm(*a, **kw)


def _rs(*a, **kw):
    from flash_attn_mi355.rope_store import rope_and_store_kv
    return rope_and_store_kv(*a, **kw)


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


def _cache(D, dt, seed, fp8=False):
    """a pre-filled cache [NBLK, PAGE, HK, D] (random data; fp8: random codes of finite values) whose last page is NaN"""
    c = rand16((NBLK, PAGE, HK, D), dt, seed, scale=2.0)
    if fp8:
        c = c.to(FP8)
    guard.fill_nan(c[NANP])
    return c


def _weights(D, dt, fp32=False, seed=31):
    """q_weight, k_weight = 1 + 0.2 randn, of the io dtype or fp32"""
    g = torch.Generator().manual_seed(seed)
    w = 1.0 + 0.2 * torch.randn(2, D, generator=g)
    w = w if fp32 else w.to(DT[dt])
    return w[0].cuda().contiguous(), w[1].cuda().contiguous()


def _inputs(D, dt, hq=HQ):
    return rand16((T, hq, D), dt, 1), rand16((T, HK, D), dt, 2), rand16((T, HK, D), dt, 3)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _eq(got, want, name):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    ne = _bits(got) != _bits(want)
    if ne.any():
        first = tuple(int(i) for i in torch.nonzero(ne)[0])
        raise AssertionError(f"{name}: {int(ne.sum())} of {ne.numel()} elements differ; first at (row, head, col) = {first}: "
                             f"got {float(got[first])}, expected {float(want[first])}")


def _nan_page_kept(c, name):
    assert torch.equal(guard.bits(c[NANP]), guard.bits(guard.fill_nan(torch.empty_like(c[NANP])))), f"{name}: the NaN page was written"


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0.0, 1.0])
@pytest.mark.parametrize("wdt", ["io", "fp32"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 96, 128, 256])
def test_norm_only_within_the_derived_bound_of_fp64(D, dt, wdt, offset):
    """qk_rms_norm against qk_norm_ref.rms_norm_ref: |got - ref| <= 0.5 ulp16(ref) + 2^-16 |ref| (qk_norm_ref.bound: one rounding
    to the io type plus the fp32 evaluation - derived, not measured).  D 64 / 96 / 128 / 256: 8, 12 of 16, 16 and 32 lanes a head"""
    q, k, _ = _inputs(D, dt)
    qw, kw = _weights(D, dt, wdt == "fp32")
    q0, k0 = q.clone(), k.clone()
    q_out, k_out = _norm(q, k, qw, kw, EPS, weight_offset=offset)
    torch.cuda.synchronize()
    _eq(q, q0, "q (read only)"); _eq(k, k0, "k (read only)")
    for got, x, w, name in ((q_out, q, qw, "q"), (k_out, k, kw, "k")):
        ref = N.rms_norm_ref(x, w, EPS, offset)
        changed = np.abs(ref - x.double().cpu().numpy()).max(axis=-1)
        assert (changed > 1e-2).all(), f"{name}: the reference leaves a head as it was"     # (the arbiter normalises)
        worst = N.worst_ratio(got, ref, DT[dt])
        print(f"{name}: worst error / bound {worst:.3f}")
        assert worst <= 1.0, f"{name}: worst error / bound {worst:.3f}"


# 2 -------------------------------------------------------------------------------------------------------------------------
_MAIN = [(D, rot) for D in (64, 128) for rot in ROTS] + [(96, "neox-32"), (256, "neox-32")]


@pytest.mark.parametrize("cache", ["16bit", "fp8"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D,rot", _MAIN)
def test_fused_equals_norm_then_rope_store_bit_for_bit(D, rot, dt, cache):
    """q_out, k_out, the whole k_cache and the whole v_cache of the fused call == qk_rms_norm(inplace=False) followed by
    rope_and_store_kv, bit for bit (fp8: the non-power-of-two descales 0.05 / 0.04); the NaN page stays as it was"""
    fp8 = cache == "fp8"
    cos, sin, il = _tables(rot, D, dt)
    pos, slots = _positions().cuda(), _slots(7).cuda()
    q, k, v = _inputs(D, dt)
    qw, kw = _weights(D, dt, fp32=(D == 128))
    off = 1.0 if D == 64 else 0.0
    q0, k0, v0 = q.clone(), k.clone(), v.clone()
    kc, vc, kc_b, vc_b = _cache(D, dt, 4, fp8), _cache(D, dt, 5, fp8), _cache(D, dt, 4, fp8), _cache(D, dt, 5, fp8)
    kwd = DESCALES if fp8 else {}
    qn, kn = _norm(q, k, qw, kw, EPS, weight_offset=off, inplace=False)
    q_ref, k_ref = _rs(qn, kn, v, pos, cos, sin, kc_b, vc_b, slots, interleaved=il, inplace=False, **kwd)
    q_out, k_out = _fused(q, k, v, pos, cos, sin, kc, vc, slots, q_weight=qw, k_weight=kw, eps=EPS, weight_offset=off,
                          interleaved=il, inplace=False, **kwd)
    torch.cuda.synchronize()
    assert not torch.equal(_bits(qn), _bits(q)) and not torch.equal(_bits(q_ref), _bits(qn))     # (the composition does both)
    _eq(q_out, q_ref, "q_out")
    _eq(k_out, k_ref, "k_out")
    R.diff_report(kc, kc_b, "k_cache vs qk_rms_norm + rope_and_store_kv")
    R.diff_report(vc, vc_b, "v_cache vs rope_and_store_kv")
    assert not R.same_bits(kc, _cache(D, dt, 4, fp8)) and not R.same_bits(vc, _cache(D, dt, 5, fp8))   # the call did write
    _nan_page_kept(kc, "k_cache"); _nan_page_kept(vc, "v_cache")
    _eq(q, q0, "q (read only)"); _eq(k, k0, "k (read only)"); _eq(v, v0, "v (read only)")


# 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", ["16bit", "fp8"])
@pytest.mark.parametrize("rot", ["interleaved-full", "neox-32"])
def test_without_weights_the_bits_of_rope_and_store_kv(rot, cache):
    """no weight: rope_and_store_kv's bits, caches included; only q_weight: k is the rotate-only k; only k_weight: q is the
    rotate-only q (and the other tensor is the fully fused one)"""
    D, dt, fp8 = 128, "bf16", cache == "fp8"
    cos, sin, il = _tables(rot, D, dt)
    pos, slots = _positions().cuda(), _slots(9).cuda()
    q, k, v = _inputs(D, dt)
    qw, kw = _weights(D, dt)
    kwd = DESCALES if fp8 else {}
    kc_r, vc_r = _cache(D, dt, 4, fp8), _cache(D, dt, 5, fp8)
    q_rot, k_rot = _rs(q, k, v, pos, cos, sin, kc_r, vc_r, slots, interleaved=il, inplace=False, **kwd)
    kc_f, vc_f = _cache(D, dt, 4, fp8), _cache(D, dt, 5, fp8)
    q_full, k_full = _fused(q, k, v, pos, cos, sin, kc_f, vc_f, slots, q_weight=qw, k_weight=kw, interleaved=il, inplace=False, **kwd)
    kc, vc = _cache(D, dt, 4, fp8), _cache(D, dt, 5, fp8)
    q_out, k_out = _fused(q, k, v, pos, cos, sin, kc, vc, slots, interleaved=il, inplace=False, **kwd)
    torch.cuda.synchronize()
    _eq(q_out, q_rot, "q_out (no weights)"); _eq(k_out, k_rot, "k_out (no weights)")
    R.diff_report(kc, kc_r, "k_cache (no weights)"); R.diff_report(vc, vc_r, "v_cache (no weights)")
    assert not torch.equal(_bits(q_full), _bits(q_rot)) and not torch.equal(_bits(k_full), _bits(k_rot))
    kc, vc = _cache(D, dt, 4, fp8), _cache(D, dt, 5, fp8)
    q_out, k_out = _fused(q, k, v, pos, cos, sin, kc, vc, slots, q_weight=qw, interleaved=il, inplace=False, **kwd)
    torch.cuda.synchronize()
    _eq(q_out, q_full, "q_out (q_weight only)"); _eq(k_out, k_rot, "k_out (q_weight only: rotated only)")
    R.diff_report(kc, kc_r, "k_cache (q_weight only)"); R.diff_report(vc, vc_r, "v_cache (q_weight only)")
    kc, vc = _cache(D, dt, 4, fp8), _cache(D, dt, 5, fp8)
    q_out, k_out = _fused(q, k, v, pos, cos, sin, kc, vc, slots, k_weight=kw, interleaved=il, inplace=False, **kwd)
    torch.cuda.synchronize()
    _eq(q_out, q_rot, "q_out (k_weight only: rotated only)"); _eq(k_out, k_full, "k_out (k_weight only)")
    R.diff_report(kc, kc_f, "k_cache (k_weight only)"); R.diff_report(vc, vc_f, "v_cache (k_weight only)")


# 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ROTS)
@pytest.mark.parametrize("D", [64, 128])
def test_in_place_on_one_packed_qkv(D, rot):
    """q, k and v are the head slices of one packed [77, 4 + 2 x 2, D] qkv, taken without a copy and changed where they are: the
    q and k heads equal the out-of-place result bit for bit (a lane only ever loads its own columns; the partner piece of a NeoX
    pair comes from the partner lane's registers), the v heads are unchanged"""
    from flash_attn_mi355 import flash_attn_interface as fi
    dt = "bf16"
    cos, sin, il = _tables(rot, D, dt)
    pos, slots = _positions().cuda(), _slots(11).cuda()
    qw, kw = _weights(D, dt)
    qkv = rand16((T, HQ + 2 * HK, D), dt, 1)
    qkv0 = qkv.clone()
    q, k, v = qkv[:, :HQ], qkv[:, HQ:HQ + HK], qkv[:, HQ + HK:]
    assert fi._prep(q, D) is q and fi._prep(k, D) is k and fi._prep(v, D) is v      # the wrapper takes the views as they are
    kc_a, vc_a = _cache(D, dt, 4), _cache(D, dt, 5)
    kc_b, vc_b = kc_a.clone(), vc_a.clone()
    q_out, k_out = _fused(q, k, v, pos, cos, sin, kc_a, vc_a, slots, q_weight=qw, k_weight=kw, interleaved=il, inplace=False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(qkv), _bits(qkv0))                 # out of place: the packed buffer is read only
    rq, rk = _fused(q, k, v, pos, cos, sin, kc_b, vc_b, slots, q_weight=qw, k_weight=kw, interleaved=il)
    torch.cuda.synchronize()
    assert rq.data_ptr() == q.data_ptr() and rk.data_ptr() == k.data_ptr() and rq.stride() == q.stride()
    _eq(qkv[:, :HQ], q_out, "q heads in place")
    _eq(qkv[:, HQ:HQ + HK], k_out, "k heads in place")
    _eq(qkv[:, HQ + HK:], qkv0[:, HQ + HK:], "v heads (unchanged)")
    assert not torch.equal(_bits(qkv[:, :HQ + HK]), _bits(qkv0[:, :HQ + HK]))
    R.diff_report(kc_b, kc_a, "k_cache, in place vs out of place")
    R.diff_report(vc_b, vc_a, "v_cache, in place vs out of place")


# 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("il", [True, False], ids=["interleaved", "neox"])
def test_optional_forms(il):
    """q=None; k_out=False (k unchanged, the cache still normalised and rotated); norm + store without rotation; int32 positions
    / slot_mapping"""
    D, dt = 128, "fp16"
    cos, sin, _ = _tables("neox-32", D, dt)
    pos, slots = _positions().cuda(), _slots(13).cuda()
    q, k, v = _inputs(D, dt)
    qw, kw = _weights(D, dt)
    nw = dict(q_weight=qw, k_weight=kw, eps=EPS)
    kc0, vc0 = _cache(D, dt, 4), _cache(D, dt, 5)
    kc_w, vc_w = kc0.clone(), vc0.clone()
    q_ref, k_ref = _fused(q, k, v, pos, cos, sin, kc_w, vc_w, slots, interleaved=il, inplace=False, **nw)
    qn, kn = _norm(q, k, qw, kw, EPS)
    torch.cuda.synchronize()
    # the full call with int32 ids, in place
    qa, ka, kc, vc = q.clone(), k.clone(), kc0.clone(), vc0.clone()
    r = _fused(qa, ka, v, pos.to(torch.int32), cos, sin, kc, vc, slots.to(torch.int32), interleaved=il, **nw)
    torch.cuda.synchronize()
    assert r[0] is qa and r[1] is ka
    _eq(qa, q_ref, "q (int32 ids)"); _eq(ka, k_ref, "k (int32 ids)")
    R.diff_report(kc, kc_w, "k_cache (int32 ids)"); R.diff_report(vc, vc_w, "v_cache (int32 ids)")
    # q=None
    ka, kc, vc = k.clone(), kc0.clone(), vc0.clone()
    r = _fused(None, ka, v, pos, cos, sin, kc, vc, slots, interleaved=il, k_weight=kw, eps=EPS)
    torch.cuda.synchronize()
    assert r[0] is None and r[1] is ka
    _eq(ka, k_ref, "k (q=None)")
    R.diff_report(kc, kc_w, "k_cache (q=None)"); R.diff_report(vc, vc_w, "v_cache (q=None)")
    # k_out=False, in place and out of place
    for inplace in (True, False):
        qa, ka, kc, vc = q.clone(), k.clone(), kc0.clone(), vc0.clone()
        r = _fused(qa, ka, v, pos, cos, sin, kc, vc, slots, interleaved=il, k_out=False, inplace=inplace, **nw)
        torch.cuda.synchronize()
        assert r[1] is None and (r[0] is qa) == inplace
        _eq(r[0], q_ref, "q_out (k_out=False)")
        _eq(ka, k, "k (k_out=False: unchanged)")
        R.diff_report(kc, kc_w, "k_cache (k_out=False: still normalised and rotated)"); R.diff_report(vc, vc_w, "v_cache (k_out=False)")
    # norm + store without rotation: the cache holds what store_kv_cache leaves of the normalised k
    from flash_attn_mi355.kv_store import store_kv_cache
    kc_n, vc_n = kc0.clone(), vc0.clone()
    store_kv_cache(kn, v, kc_n, vc_n, slot_mapping=slots)
    kc, vc = kc0.clone(), vc0.clone()
    r = _fused(q, k, v, None, None, None, kc, vc, slots, inplace=False, **nw)
    torch.cuda.synchronize()
    _eq(r[0], qn, "q_out (no rotation)"); _eq(r[1], kn, "k_out (no rotation)")
    R.diff_report(kc, kc_n, "k_cache (no rotation)"); R.diff_report(vc, vc_n, "v_cache (no rotation)")
    assert not R.same_bits(kc, kc_w)
    # norm only, in place
    qa, ka = q.clone(), k.clone()
    r = _norm(qa, ka, qw, kw, EPS, inplace=True)
    torch.cuda.synchronize()
    assert r[0] is qa and r[1] is ka
    _eq(qa, qn, "q (norm only, in place)"); _eq(ka, kn, "k (norm only, in place)")


# 6 -------------------------------------------------------------------------------------------------------------------------
def test_batch_invariance():
    """the same rows in reversed order and a sub-batch of 5 rows give the same bits per row, caches included; Hq = 1 gives the bits
    Hq = 4 gives for that head: a head's sum never sees another row or head"""
    D, dt = 96, "bf16"
    cos, sin, il = _tables("neox-32", D, dt)
    pos, slots = _positions().cuda(), _slots(15).cuda()
    q, k, v = _inputs(D, dt)
    qw, kw = _weights(D, dt)
    nw = dict(q_weight=qw, k_weight=kw, eps=EPS, interleaved=il, inplace=False)
    kc, vc = _cache(D, dt, 4), _cache(D, dt, 5)
    q_out, k_out = _fused(q, k, v, pos, cos, sin, kc, vc, slots, **nw)
    kc_r, vc_r = _cache(D, dt, 4), _cache(D, dt, 5)
    fl = lambda t: t.flip(0).contiguous()                  # noqa: E731
    q_rev, k_rev = _fused(fl(q), fl(k), fl(v), fl(pos), cos, sin, kc_r, vc_r, fl(slots), **nw)
    torch.cuda.synchronize()
    _eq(q_rev.flip(0), q_out, "q_out, rows reversed"); _eq(k_rev.flip(0), k_out, "k_out, rows reversed")
    R.diff_report(kc_r, kc, "k_cache, rows reversed"); R.diff_report(vc_r, vc, "v_cache, rows reversed")
    sub = slice(10, 15)
    kc_s, vc_s = _cache(D, dt, 4), _cache(D, dt, 5)
    q_sub, k_sub = _fused(q[sub], k[sub], v[sub], pos[sub], cos, sin, kc_s, vc_s, slots[sub], **nw)
    q_one, _ = _fused(q[:, 2:3], k, v, pos, cos, sin, _cache(D, dt, 4), _cache(D, dt, 5), slots, **nw)
    torch.cuda.synchronize()
    _eq(q_sub, q_out[sub], "q_out, 5 rows"); _eq(k_sub, k_out[sub], "k_out, 5 rows")
    for r in range(10, 15):
        s = int(slots[r])
        if 0 <= s < N_SLOTS:
            assert torch.equal(_bits(kc_s[s // PAGE, s % PAGE]), _bits(kc[s // PAGE, s % PAGE])), r
    _eq(q_one, q_out[:, 2:3], "q_out, Hq = 1")


# 7 -------------------------------------------------------------------------------------------------------------------------
def test_range_large_fp16_values_and_an_all_zero_head():
    """a head of fp16 values near +-60000 (their squares overflow 16 bits, not fp32) stays finite and inside test 1's bound; an
    all-zero head gives zeros with eps > 0"""
    D, dt = 128, "fp16"
    g = torch.Generator().manual_seed(5)
    sign = torch.where(torch.rand(T, HQ, D, generator=g) < 0.5, -1.0, 1.0)
    q = (sign * (60000.0 - 2000.0 * torch.rand(T, HQ, D, generator=g))).to(torch.float16).cuda()
    k = rand16((T, HK, D), dt, 2)
    k[3] = 0
    k[:, 1, :] *= 0.001
    k[40, 1] = 0
    qw, kw = _weights(D, dt)
    q_out, k_out = _norm(q, k, qw, kw, EPS)
    torch.cuda.synchronize()
    assert float(q.float().abs().min()) > 57000
    for got, x, w, name in ((q_out, q, qw, "q"), (k_out, k, kw, "k")):
        worst = N.worst_ratio(got, N.rms_norm_ref(x, w, EPS), DT[dt])
        print(f"{name}: worst error / bound {worst:.3f}")
        assert worst <= 1.0, f"{name}: worst error / bound {worst:.3f}"
    assert float(q_out.float().abs().max()) > 0.5
    assert not k_out[3].any() and not k_out[40, 1].any() and k_out[40, 0].any()


# 8 -------------------------------------------------------------------------------------------------------------------------
def test_padding_rows_and_out_of_table_rows():
    """rows with slot -1 (and the two slots at / past the end) are normalised and rotated, and the cache keeps its bits at every
    slot that no row names; rows whose position is outside the table are normalised and left unrotated"""
    D, dt = 128, "bf16"
    cos, sin, il = _tables("neox-full", D, dt)
    pos, slots = _positions(), _slots(17)
    q, k, v = _inputs(D, dt)
    qw, kw = _weights(D, dt)
    kc, vc = _cache(D, dt, 4), _cache(D, dt, 5)
    kc0, vc0 = kc.clone(), vc.clone()
    q_out, k_out = _fused(q, k, v, pos.cuda(), cos, sin, kc, vc, slots.cuda(), q_weight=qw, k_weight=kw, interleaved=il, inplace=False)
    qn, kn = _norm(q, k, qw, kw)
    q_ref, k_ref = _rs(qn, kn, None, pos.cuda(), cos, sin, interleaved=il, inplace=False)
    torch.cuda.synchronize()
    pad = [r for r in range(T) if not 0 <= int(slots[r]) < N_SLOTS]
    assert len(pad) == 7 and sum(int(slots[r]) == -1 for r in pad) == 5
    for r in pad:
        assert torch.equal(q_out[r], q_ref[r]) and torch.equal(k_out[r], k_ref[r]), r
        assert not torch.equal(q_out[r], qn[r]) and not torch.equal(k_out[r], kn[r]), r        # (rotated)
    for r in (T - 3, T - 2, T - 1):                        # positions -1, seqlen_ro, seqlen_ro + 5
        assert torch.equal(q_out[r], qn[r]) and torch.equal(k_out[r], kn[r]), r
        assert not torch.equal(q_out[r], q[r]) and not torch.equal(k_out[r], k[r]), r          # (normalised)
    named = torch.zeros(N_SLOTS, dtype=torch.bool)
    named[slots[(slots >= 0) & (slots < N_SLOTS)]] = True
    assert int(named.sum()) == T - 7
    un = ~named.cuda()
    for c, c0, name in ((kc, kc0, "k_cache"), (vc, vc0, "v_cache")):
        a, b = c.view(torch.int16).reshape(N_SLOTS, -1), c0.view(torch.int16).reshape(N_SLOTS, -1)
        assert torch.equal(a[un], b[un]), f"{name}: a slot that no row names was written"
        assert not (a[~un] == b[~un]).all(dim=1).any(), f"{name}: a named slot kept its pre-fill"


# 9 -------------------------------------------------------------------------------------------------------------------------
def _guarded_1d(x):
    """a tensor of exactly len(x) elements in the middle of a larger buffer, which must come back unchanged"""
    buf = torch.full((4096 + len(x) + 4096,), -1, dtype=x.dtype, device="cuda")
    view = buf[4096:4096 + len(x)]
    view.copy_(x)
    return buf, view


def _call_into(q, k, v, q_out, k_out, pos, slots, cos, sin, kc, vc, il, qw, kw, kwd):
    """fa_qk_norm_rope_store with caller-owned strided outputs (the Python function allocates contiguous ones): the C ABI through
    the ctypes mirror, filled the way qk_norm_rope_and_store_kv fills it"""
    import ctypes
    from flash_attn_mi355 import _lib
    from flash_attn_mi355 import flash_attn_interface as fi
    s = _lib.FaQkNormRopeStoreParams()
    s.struct_size = ctypes.sizeof(_lib.FaQkNormRopeStoreParams)
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
    s.k_descale, s.v_descale = kwd.get("k_descale", 0.0), kwd.get("v_descale", 0.0)
    s.q_weight, s.k_weight = qw.data_ptr(), kw.data_ptr()
    s.weight_dtype = _lib.FA_FP32 if qw.dtype == torch.float32 else s.dtype
    s.eps = EPS
    _lib.call_qk_norm_rope_store(s, fi._stream(q.device))


@pytest.mark.parametrize("case", ["16bit-neox", "fp8-interleaved", "16bit-neox-32-inplace"])
def test_guard_bands(case):
    """q, k, v, the outputs and the caches are views with gaps inside NaN-filled slabs, the weights, positions and slot_mapping
    sit exactly sized inside guarded buffers: nothing outside a tensor's logical elements is written, a read past an input would
    carry NaN into the results, and the inputs are bit-unchanged out of place"""
    dt, D = "bf16", 128
    fp8, inplace = case.startswith("fp8"), case.endswith("inplace")
    cos, sin, il = _tables("interleaved-full" if "interleaved" in case else ("neox-32" if "32" in case else "neox-full"), D, dt)
    pos, slots = _positions().cuda(), _slots(19).cuda()
    kwd = DESCALES if fp8 else {}
    q_d, k_d, v_d = _inputs(D, dt)
    w_q, w_k = _weights(D, dt, fp32=fp8)
    kc_d, vc_d = _cache(D, dt, 4, fp8), _cache(D, dt, 5, fp8)
    kc_w, vc_w = kc_d.clone(), vc_d.clone()
    q_ref, k_ref = _fused(q_d, k_d, v_d, pos, cos, sin, kc_w, vc_w, slots, q_weight=w_q, k_weight=w_k, eps=EPS, interleaved=il,
                          inplace=False, **kwd)
    qb, q, qs = guard.guarded(q_d)
    kb, k, ks = guard.guarded(k_d)
    vb, v, vs = guard.guarded(v_d)
    kcb, kc, kcs = guard.guarded(kc_d)
    vcb, vc, vcs = guard.guarded(vc_d)
    (pb, pv), (sb, sv), (qwb, qw), (kwb, kw) = _guarded_1d(pos), _guarded_1d(slots), _guarded_1d(w_q), _guarded_1d(w_k)
    side0 = [b.clone() for b in (pb, sb, qwb, kwb)]
    checks = [(vb, v, vs, "v"), (kcb, kc, kcs, "k_cache"), (vcb, vc, vcs, "v_cache")]
    if inplace:
        r = _fused(q, k, v, pv, cos, sin, kc, vc, sv, q_weight=qw, k_weight=kw, eps=EPS, interleaved=il, **kwd)
        assert r[0] is q and r[1] is k
        q_out, k_out = q, k
        checks += [(qb, q, qs, "q (in place)"), (kb, k, ks, "k (in place)")]
    else:
        qob, q_out, qos = guard.guarded(shape=(T, HQ, D), dtype=DT[dt], device="cuda")
        kob, k_out, kos = guard.guarded(shape=(T, HK, D), dtype=DT[dt], device="cuda")
        _call_into(q, k, v, q_out, k_out, pv, sv, cos, sin, kc, vc, il, qw, kw, kwd)
        checks += [(qb, q, qs, "q"), (kb, k, ks, "k"), (qob, q_out, qos, "q_out"), (kob, k_out, kos, "k_out")]
    torch.cuda.synchronize()
    _eq(q_out, q_ref, "q_out")
    _eq(k_out, k_ref, "k_out")
    R.diff_report(kc, kc_w, case + " k_cache")
    R.diff_report(vc, vc_w, case + " v_cache")
    for buf, view, snap, name in checks:
        guard.assert_untouched(buf, view, snap, name)
    assert torch.equal(guard.bits(vb), vs)                       # v itself is read only
    if not inplace:
        assert torch.equal(guard.bits(qb), qs) and torch.equal(guard.bits(kb), ks)
    for b, b0 in zip((pb, sb, qwb, kwb), side0):
        assert torch.equal(b, b0)


# 10 ------------------------------------------------------------------------------------------------------------------------
def test_prologue_and_decode_replay_in_a_graph():
    """qk_norm_rope_and_store_kv (in place on a packed qkv, one padding row) followed by a decode call, captured in one graph on
    one stream; replayed after qkv, positions, slot_mapping and the lengths were overwritten in place: the qkv, the caches and the
    output equal the eager results bit for bit"""
    import flash_attn as fa
    dt, D, Hq, B = "bf16", 128, 8, 2
    lens0 = [20, 33]
    bt, nblk, nanp = guard.paged_table([l + 4 for l in lens0], PAGE, seed=14)
    kc0, vc0 = rand16((nblk, PAGE, HK, D), dt, 1, scale=2.0), rand16((nblk, PAGE, HK, D), dt, 2, scale=2.0)
    guard.fill_nan(kc0[nanp]); guard.fill_nan(vc0[nanp])
    btd = bt.cuda()
    cos, sin, _ = _tables("neox-full", D, dt)
    qw, kw = _weights(D, dt)
    steps = 3
    qkvs = [rand16((B + 1, Hq + 2 * HK, D), dt, 10 + i) for i in range(steps)]
    poss = [torch.tensor([l + i for l in lens0] + [0], device="cuda") for i in range(steps)]
    slots = [torch.tensor([int(bt[b, (l + i) // PAGE]) * PAGE + (l + i) % PAGE for b, l in enumerate(lens0)] + [-1], device="cuda")
             for i in range(steps)]
    lens = [torch.tensor([l + i + 1 for l in lens0], dtype=torch.int32, device="cuda") for i in range(steps)]

    def make_step(kc, vc, qkv, pos, slot, n):
        q, k, v = qkv[:, :Hq], qkv[:, Hq:Hq + HK], qkv[:, Hq + HK:]

        def step():
            _fused(q, k, v, pos, cos, sin, kc, vc, slot, q_weight=qw, k_weight=kw, eps=EPS)
            return fa.flash_attn_with_kvcache(q[:B].unsqueeze(1), kc, vc, cache_seqlens=n, block_table=btd, return_softmax_lse=True)
        return step

    kc_e, vc_e = kc0.clone(), vc0.clone()
    ref = []
    for i in range(steps):
        x = qkvs[i].clone()
        o, lse = make_step(kc_e, vc_e, x, poss[i], slots[i], lens[i])()
        ref.append((o.clone(), lse.clone(), x))
    torch.cuda.synchronize()
    assert not torch.equal(ref[0][2][:B, :Hq + HK], qkvs[0][:B, :Hq + HK])      # (the eager steps change q and k)
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
        assert torch.equal(_bits(x_s), _bits(ref[i][2])), f"step {i}: the normalised, rotated qkv differs"
    R.diff_report(kc_g, kc_e, "k_cache after the replays")
    R.diff_report(vc_g, vc_e, "v_cache after the replays")


# 11 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_torch_op_gives_the_same_bits(fp8):
    import flash_attn_mi355.torch_ops  # noqa: F401  (registers the ops)
    dt, D = "fp16", 64
    cos, sin, il = _tables("neox-32" if fp8 else "interleaved-full", D, dt)
    pos, slots = _positions().cuda(), _slots(21).cuda()
    qw, kw = _weights(D, dt, fp32=fp8)
    qkv_a = rand16((T, HQ + 2 * HK, D), dt, 1)
    qkv_b = qkv_a.clone()
    kc_a, vc_a = _cache(D, dt, 4, fp8), _cache(D, dt, 5, fp8)
    kc_b, vc_b = kc_a.clone(), vc_a.clone()
    kwd = DESCALES if fp8 else {}
    _fused(qkv_a[:, :HQ], qkv_a[:, HQ:HQ + HK], qkv_a[:, HQ + HK:], pos, cos, sin, kc_a, vc_a, slots, q_weight=qw, k_weight=kw,
           eps=1e-5, weight_offset=1.0, interleaved=il, **kwd)
    r = torch.ops.flash_attn_mi355.qk_norm_rope_store_(qkv_b[:, :HQ], qkv_b[:, HQ:HQ + HK], qkv_b[:, HQ + HK:], pos, cos, sin, kc_b,
                                                       vc_b, slots, qw, kw, 1e-5, 1.0, il, kwd.get("k_descale", 1.0),
                                                       kwd.get("v_descale", 1.0))
    assert r is None
    torch.cuda.synchronize()
    assert not torch.equal(_bits(qkv_a), _bits(rand16((T, HQ + 2 * HK, D), dt, 1)))
    assert not R.same_bits(kc_a, _cache(D, dt, 4, fp8))
    assert torch.equal(_bits(qkv_b), _bits(qkv_a))
    R.diff_report(kc_b, kc_a, "torch op k_cache")
    R.diff_report(vc_b, vc_a, "torch op v_cache")
