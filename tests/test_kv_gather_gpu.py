"""GPU: fa_kv_gather (flash_attn_mi355.kv_gather.gather_kv_cache / move_kv_cache) - ragged K / V rows out of a paged or contiguous
KV cache into packed tensors.  Everything is compared bit for bit with the torch CPU restatement (kv_gather_ref): no tolerance
anywhere.  The outputs start as NaN, so a row that was not written shows; the block tables' spare page holds NaN, so a wrong page
lookup shows."""
import numpy as np
import pytest
import torch

import guard
import kv_gather_ref as G
import kv_store_ref as R
from util import DT, rand16

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
HK, PAGE = 2, 16


def _gather(*a, **kw):
    from flash_attn_mi355.kv_gather import gather_kv_cache
    return gather_kv_cache(*a, **kw)


def _move(*a, **kw):
    from flash_attn_mi355.kv_gather import move_kv_cache
    return move_kv_cache(*a, **kw)


def _store(*a, **kw):
    from flash_attn_mi355.kv_store import store_kv_cache
    return store_kv_cache(*a, **kw)


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


def _cu(lens):
    return [0] + np.cumsum(lens).tolist()


def _cache(shape, dt, seed, nan_page=None):
    c = rand16(shape, dt, seed, scale=2.0)
    if nan_page is not None:
        guard.fill_nan(c[nan_page])
    return c


def _cache8(shape, seed, nan_page=None):
    """an fp8 cache over random BYTES with the two NaN codes replaced: every finite code occurs, -0 and the subnormals included"""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    b[b == 0x7F] = 0x7E
    b[b == 0xFF] = 0x80
    assert len(torch.unique(b)) == 254
    c = b.view(FP8).cuda()
    if nan_page is not None:
        guard.fill_nan(c[nan_page])
    return c


def _nan_out(T, D, dt, hk=HK):
    """an output pair that starts as NaN: an unwritten element shows"""
    k = guard.fill_nan(torch.empty((T, hk, D), dtype=DT[dt], device="cuda"))
    return k, k.clone()


def _dev(addr):
    return {k_: (v_.cuda() if isinstance(v_, torch.Tensor) else _i32(v_)) for k_, v_ in addr.items()}


def _check(got, want, name):
    torch.cuda.synchronize()
    G.diff_report(got[0], want[0], name + " k")
    G.diff_report(got[1], want[1], name + " v")


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_sequence_mode_paged(D, dt):
    """lengths [0, 1, 37, 130] at seq_offsets [5, 15, 0, 100]: an empty sequence, the last row of a page, a page start and nine
    pages from mid-page"""
    lens, off = [0, 1, 37, 130], [5, 15, 0, 100]
    T = sum(lens)
    bt, nblk, nanp = guard.paged_table([a + b for a, b in zip(lens, off)], PAGE, seed=1)
    kc, vc = _cache((nblk, PAGE, HK, D), dt, 3, nan_page=nanp), _cache((nblk, PAGE, HK, D), dt, 4, nan_page=nanp)
    cu = _cu(lens)
    want = G.kv_gather_ref(kc, vc, cu_seqlens=cu, seq_offsets=off, block_table=bt, total_rows=T)
    assert not torch.isnan(want[0].float()).any() and float(want[0].float().abs().sum()) > 0
    snap = kc.clone(), vc.clone()
    got = _gather(kc, vc, cu_seqlens=_i32(cu), seq_offsets=_i32(off), block_table=bt.cuda(), out=_nan_out(T, D, dt))
    _check(got, want, "paged")
    got = _gather(kc, vc, cu_seqlens=_i32(cu), seq_offsets=_i32(off), block_table=bt.cuda(), total_rows=T)     # fresh tensors
    assert got[0].is_contiguous() and got[0].dtype == DT[dt] and tuple(got[1].shape) == (T, HK, D)
    _check(got, want, "paged, no out")
    # seq_offsets None = zeros
    want0 = G.kv_gather_ref(kc, vc, cu_seqlens=cu, block_table=bt, total_rows=T)
    assert not G.same_bits(want0[0], want[0])
    got = _gather(kc, vc, cu_seqlens=_i32(cu), block_table=bt.cuda(), out=_nan_out(T, D, dt))
    _check(got, want0, "paged, no seq_offsets")
    assert R.same_bits(kc, snap[0]) and R.same_bits(vc, snap[1])                  # the caches are read only


# 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_sequence_mode_contiguous_with_cache_batch_idx(D, dt):
    """S_max 64, a permuted cache_batch_idx into a cache with more slots than sequences; sequence 1 runs 5 positions past S_max
    (those rows are exactly zero, the neighbouring slot is not read); the output has 7 rows more than cu_seqlens[-1] (zero too)"""
    lens, off, Bc, S = [10, 30, 7], [0, 39, 3], 5, 64
    assert off[1] + lens[1] == S + 5
    bidx = [4, 0, 2]
    T = sum(lens) + 7
    kc, vc = _cache((Bc, S, HK, D), dt, 3), _cache((Bc, S, HK, D), dt, 4)
    cu = _cu(lens)
    want = G.kv_gather_ref(kc, vc, cu_seqlens=cu, seq_offsets=off, cache_batch_idx=bidx, total_rows=T)
    src = G.sources(T, kc.shape, cu_seqlens=cu, seq_offsets=off, cache_batch_idx=bidx)
    assert [r for r, s in enumerate(src) if s is None] == list(range(35, 40)) + list(range(47, 54))
    assert want[0].view(torch.int16)[35:40].eq(0).all() and want[1].view(torch.int16)[47:].eq(0).all()
    got = _gather(kc, vc, cu_seqlens=_i32(cu), seq_offsets=_i32(off), cache_batch_idx=_i32(bidx), out=_nan_out(T, D, dt))
    _check(got, want, "contiguous")
    # the identity mapping (no cache_batch_idx)
    want = G.kv_gather_ref(kc, vc, cu_seqlens=cu, seq_offsets=off, total_rows=T)
    got = _gather(kc, vc, cu_seqlens=_i32(cu), seq_offsets=_i32(off), out=_nan_out(T, D, dt))
    _check(got, want, "contiguous, identity")


def test_no_sequences_and_no_slots_give_zero_rows():
    """sequence mode with batch 0 and total_rows > 0 zero-fills the rows; so does a cache without a single slot (num_blocks 0
    through the C ABI - an empty torch tensor has no address to pass): nothing is read through k_cache / v_cache then"""
    import ctypes
    from flash_attn_mi355 import _lib
    kc = _cache((3, PAGE, HK, 64), "bf16", 1)
    got = _gather(kc, kc.clone(), cu_seqlens=_i32([0]), out=_nan_out(5, 64, "bf16"))
    torch.cuda.synchronize()
    assert got[0].view(torch.int16).eq(0).all() and got[1].view(torch.int16).eq(0).all()
    k, v = _nan_out(40, 64, "bf16")
    slots = torch.arange(40, device="cuda")
    s = _lib.FaKvGatherParams()
    s.struct_size = ctypes.sizeof(_lib.FaKvGatherParams)
    s.k_cache = s.v_cache = kc.data_ptr()
    s.kc_batch_stride = s.vc_batch_stride = PAGE * HK * 64
    s.kc_row_stride = s.vc_row_stride = s.k_row_stride = s.v_row_stride = HK * 64
    s.kc_head_stride = s.vc_head_stride = s.k_head_stride = s.v_head_stride = 64
    s.k, s.v = k.data_ptr(), v.data_ptr()
    s.total_rows, s.nheads, s.head_dim = 40, HK, 64
    s.dtype = s.cache_dtype = _lib.FA_BF16
    s.num_blocks, s.page_block_size = 0, PAGE
    s.slot_mapping = slots.data_ptr()
    _lib.call_kv_gather(s, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert k.view(torch.int16).eq(0).all() and v.view(torch.int16).eq(0).all()


# 3 -------------------------------------------------------------------------------------------------------------------------
def _slots(T, n_slots, seed, usable=None):
    """T slots of a cache with n_slots: a random permutation of the first `usable` (default: all), 13 of them replaced by -1 and 2
    by slots at / past the end"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randperm(n_slots if usable is None else usable, generator=g)[:T].clone()
    drop = torch.randperm(T, generator=g)[:15]
    s[drop[:13]] = -1
    s[drop[13]] = n_slots
    s[drop[14]] = n_slots + 77
    return s


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_slot_mode_into_packed_qkv_views(D, dt):
    """200 rows from a random permutation of slots, 13 slots of -1 and 2 at / past the end (zero rows); int64 and int32 slots;
    the outputs are the K / V head slices of one packed [200, 4 + 2 x 2, D] qkv buffer, written where they lie: the query heads
    stay untouched; a paged cache and a contiguous one seen as page = S_max"""
    T, nblk = 200, 20
    slots = _slots(T, nblk * PAGE, 7)
    for shape, name in (((nblk, PAGE, HK, D), "paged"), ((5, 64, HK, D), "contiguous as page = S_max")):
        kc, vc = _cache(shape, dt, 3), _cache(shape, dt, 4)
        want = G.kv_gather_ref(kc, vc, slot_mapping=slots)
        assert sum(int(want[0].view(torch.int16)[r].eq(0).all()) for r in range(T)) == 15
        for sl, tag in ((slots.cuda(), ""), (slots.to(torch.int32).cuda(), ", int32 slots")):
            qkv = rand16((T, 4 + 2 * HK, D), dt, 1)
            before = qkv.clone()
            k, v = qkv[:, 4:4 + HK], qkv[:, 4 + HK:]
            got = _gather(kc, vc, slot_mapping=sl, out=(k, v))
            assert got[0] is k and got[1] is v                                    # no copy
            torch.cuda.synchronize()
            G.diff_report(qkv[:, 4:4 + HK], want[0], name + tag + " k")
            G.diff_report(qkv[:, 4 + HK:], want[1], name + tag + " v")
            assert R.same_bits(qkv[:, :4].contiguous(), before[:, :4].contiguous()), "the query heads were written"
        got = _gather(kc, vc, slot_mapping=slots.cuda())
        _check(got, want, name + ", no out")


def test_slot_mode_past_the_grid_cap():
    """4096 x 16 + 37 rows (Hk 2, D 64: 16 rows per workgroup step): more groups than the capped grid holds, so workgroups take a
    second group; slots repeat (a gather may read a row many times).  The expectation is torch indexing on the CPU"""
    T, nblk, D = 4096 * 16 + 37, 24, 64
    g = torch.Generator().manual_seed(3)
    slots = torch.randint(-2, nblk * PAGE + 2, (T,), generator=g)
    kc, vc = _cache((nblk, PAGE, HK, D), "bf16", 1), _cache((nblk, PAGE, HK, D), "bf16", 2)
    ok = (slots >= 0) & (slots < nblk * PAGE)
    idx = slots.clamp(0, nblk * PAGE - 1)
    want = [torch.where(ok[:, None, None], c.cpu().view(-1, HK, D)[idx], torch.zeros((), dtype=c.dtype)) for c in (kc, vc)]
    got = _gather(kc, vc, slot_mapping=slots.cuda(), out=_nan_out(T, D, "bf16"))
    _check(got, want, "past the grid cap")


@pytest.mark.parametrize("kind,D", [("bf16", 128), ("fp16", 256), ("fp8", 72), ("fp8", 256)])
def test_rows_of_many_items(kind, D):
    """Hk 8: a group of rows has more items than one pass of the workgroup takes (16-bit D 128: 2048 items, four full passes;
    D 256: 8 rows per group; fp8 D 72: 1152 items, the third pass partly filled)"""
    hk, lens, off = 8, [37, 5, 20], [3, 15, 0]
    T = sum(lens) + 3
    bt, nblk, nanp = guard.paged_table([a + b for a, b in zip(lens, off)], PAGE, seed=5)
    if kind == "fp8":
        kc, vc = _cache8((nblk, PAGE, hk, D), 3, nanp), _cache8((nblk, PAGE, hk, D), 4, nanp)
        kw, dt = dict(dtype=torch.bfloat16, k_descale=0.05, v_descale=0.04), "bf16"
    else:
        kc, vc = _cache((nblk, PAGE, hk, D), kind, 3, nanp), _cache((nblk, PAGE, hk, D), kind, 4, nanp)
        kw, dt = {}, kind
    cu = _cu(lens)
    want = G.kv_gather_ref(kc, vc, cu_seqlens=cu, seq_offsets=off, block_table=bt, total_rows=T, **kw)
    got = _gather(kc, vc, cu_seqlens=_i32(cu), seq_offsets=_i32(off), block_table=bt.cuda(), out=_nan_out(T, D, dt, hk), **kw)
    _check(got, want, f"Hk 8 {kind} D {D}")


# 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descales", [(0.05, 0.04), (1.0, 1.0)])
@pytest.mark.parametrize("mode", ["seq", "slot"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("layout", ["D128-wide", "D72-narrow", "D128-misaligned"])
def test_fp8_cache(layout, dt, mode, descales):
    """fp8 caches over random bytes (all 254 finite codes): out = (code.float() * descale).to(dtype) bit for bit.  D 128 takes
    16 codes per load; D 72 (head_dim % 16 != 0) and a D 128 view whose base is 8 but not 16 bytes aligned take 8; the same
    problem through both widths gives the same bits"""
    D = 72 if layout.startswith("D72") else 128
    lens, off = [1, 37, 0, 70], [15, 0, 3, 20]
    T = sum(lens) + 2
    bt, nblk, nanp = guard.paged_table([a + b for a, b in zip(lens, off)], PAGE, seed=2)
    cu = _cu(lens)
    # (slots stay off the spare page: the NaN codes dequantise to NaN, whose bits are not pinned)
    addr = dict(cu_seqlens=cu, seq_offsets=off, block_table=bt) if mode == "seq" else dict(slot_mapping=_slots(T, nblk * PAGE, 9, usable=nanp * PAGE))
    kd, vd = descales
    kw = dict(dtype=DT[dt], k_descale=kd, v_descale=vd)

    def cache(seed):
        if layout.endswith("misaligned"):
            big = _cache8((nblk, PAGE, HK, D + 8), seed, nanp)
            view = big[..., 8:]
            assert view.data_ptr() % 16 == 8 and view.stride(2) % 16 == 8
            return view
        return _cache8((nblk, PAGE, HK, D), seed, nanp)

    kc, vc = cache(3), cache(4)
    want = G.kv_gather_ref(kc, vc, total_rows=T, **addr, **kw)
    assert not torch.isnan(want[0].float()).any()
    got = _gather(kc, vc, out=_nan_out(T, D, dt), **_dev(addr), **kw)
    _check(got, want, f"fp8 {layout} {mode} {descales}")
    if layout.endswith("misaligned"):                      # the same codes in an aligned cache: the wide path, the same bits
        kca, vca = kc.contiguous(), vc.contiguous()
        assert kca.data_ptr() % 16 == 0 and R.same_bits(kca, kc)
        wide = _gather(kca, vca, out=_nan_out(T, D, dt), **_dev(addr), **kw)
        torch.cuda.synchronize()
        assert G.same_bits(wide[0], got[0]) and G.same_bits(wide[1], got[1]), "16 and 8 codes per load give different bits"


# 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["seq-paged", "seq-contiguous", "slot"])
@pytest.mark.parametrize("kind", ["fp16", "bf16", "fp8"])
def test_inverse_of_the_store(kind, mode):
    """store_kv_cache then gather_kv_cache with the same addressing returns the source rows bit for bit (16-bit caches), or the
    reference's dequantise(quantise(x)) (fp8); storing the gathered rows into a second fp8 cache with the same descales leaves
    identical codes: the round trip on the device"""
    fp8 = kind == "fp8"
    dt, D = ("bf16" if fp8 else kind), 128
    lens, off = [3, 0, 41, 20], [14, 7, 0, 30]
    T = sum(lens)
    cu = _cu(lens)
    if mode == "seq-contiguous":
        shape, nanp = (6, 64, HK, D), None
        st, ga = dict(cu_seqlens=cu, cache_seqlens=off, cache_batch_idx=[5, 1, 3, 0]), dict(cu_seqlens=cu, seq_offsets=off, cache_batch_idx=[5, 1, 3, 0])
    else:
        bt, nblk, nanp = guard.paged_table([a + b for a, b in zip(lens, off)], PAGE, seed=10)
        shape = (nblk, PAGE, HK, D)
        if mode == "slot":
            slots = torch.randperm(nblk * PAGE, generator=torch.Generator().manual_seed(4))[:T]
            st = ga = dict(slot_mapping=slots)
        else:
            st, ga = dict(cu_seqlens=cu, cache_seqlens=off, block_table=bt), dict(cu_seqlens=cu, seq_offsets=off, block_table=bt)
    k, v = rand16((T, HK, D), dt, 1, scale=1.5), rand16((T, HK, D), dt, 2, scale=1.5)
    k[3, 0, 0] = -0.0
    if fp8:
        kc, vc = _cache8(shape, 3, nanp), _cache8(shape, 4, nanp)
        kw, gkw = dict(k_descale=0.05, v_descale=0.04), dict(k_descale=0.05, v_descale=0.04, dtype=DT[dt])
        want = (G.dequantise(R.quantise(k.cpu(), 0.05), 0.05, DT[dt]), G.dequantise(R.quantise(v.cpu(), 0.04), 0.04, DT[dt]))
    else:
        kc, vc = _cache(shape, dt, 3, nanp), _cache(shape, dt, 4, nanp)
        kw, gkw, want = {}, {}, (k, v)
    kc2, vc2 = kc.clone(), vc.clone()
    _store(k, v, kc, vc, **_dev(st), **kw)
    got = _gather(kc, vc, out=_nan_out(T, D, dt), **_dev(ga), **gkw)
    _check(got, want, f"store -> gather {kind} {mode}")
    if fp8:
        _store(got[0], got[1], kc2, vc2, **_dev(st), **kw)
        torch.cuda.synchronize()
        R.diff_report(kc2, kc, "codes after store(gather(store(x)))")
        R.diff_report(vc2, vc, "codes after store(gather(store(x)))")


# 6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["paged-16bit", "contiguous-16bit", "paged-fp8"])
def test_guard_bands(case):
    """the outputs are views with gaps inside NaN-filled slabs, the caches too: nothing outside the logical output elements
    changes, both caches are bit-identical to their snapshots, and a read past a cache would carry NaN into the output"""
    dt, D = "bf16", 128
    fp8 = case.endswith("fp8")
    lens, off = [3, 0, 41, 20], [14, 7, 0, 30]
    T = sum(lens) + 4
    cu = _cu(lens)
    kw = dict(k_descale=0.0625, v_descale=0.04, dtype=DT[dt]) if fp8 else {}
    if case.startswith("paged"):
        bt, nblk, nanp = guard.paged_table([a + b for a, b in zip(lens, off)], PAGE, seed=10)
        shape, addr = (nblk, PAGE, HK, D), dict(cu_seqlens=cu, seq_offsets=off, block_table=bt)
    else:
        shape, nanp, addr = (6, 64, HK, D), None, dict(cu_seqlens=cu, seq_offsets=off, cache_batch_idx=[5, 1, 3, 0])
    mk = (lambda s: _cache8(shape, s, nanp)) if fp8 else (lambda s: _cache(shape, dt, s, nanp))
    kcb, kc, kcs = guard.guarded(mk(3))
    vcb, vc, vcs = guard.guarded(mk(4))
    usable = None if nanp is None else nanp * PAGE         # (slots stay off the spare page: an fp8 NaN's bits are not pinned)
    for name, a in (("sequence mode", addr), ("slot mode", dict(slot_mapping=_slots(T, shape[0] * shape[1], 12, usable=usable)))):
        kb, k, ks = guard.guarded(shape=(T, HK, D), dtype=DT[dt], device="cuda")
        vb, v, vs = guard.guarded(shape=(T, HK, D), dtype=DT[dt], device="cuda")
        want = G.kv_gather_ref(kc, vc, total_rows=T, **a, **kw)
        got = _gather(kc, vc, out=(k, v), **_dev(a), **kw)
        _check(got, want, f"{case} {name}")
        for buf, view, snap, n in ((kb, k, ks, "k"), (vb, v, vs, "v"), (kcb, kc, kcs, "k_cache"), (vcb, vc, vcs, "v_cache")):
            guard.assert_untouched(buf, view, snap, f"{n} ({name})")
        assert torch.equal(guard.bits(kcb), kcs) and torch.equal(guard.bits(vcb), vcs)      # the caches are read only


# 7 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp8"])
def test_move_commits_an_accepted_tree_path(kind):
    """B 2, T 6 draft nodes appended at L + t; the accepted nodes [0, 2, 5] and [0, 1, 3] move to L + 0 .. 2: overlapping source
    and destination sets (slot L + 2 is read for one row and written for another).  The whole cache equals the torch-built
    expectation bit for bit; an fp8 cache keeps its codes.  Then a page copy: 2 pages to 2 other pages, through the torch op"""
    import flash_attn_mi355.torch_ops  # noqa: F401  (registers the ops)
    D, L, acc = 128, [13, 30], [[0, 2, 5], [0, 1, 3]]        # the nodes cross a page boundary in both sequences
    bt, nblk, nanp = guard.paged_table([l + 6 for l in L], PAGE, seed=6)
    shape = (nblk, PAGE, HK, D)
    if kind == "fp8":
        kc, vc = _cache8(shape, 3, nanp), _cache8(shape, 4, nanp)
    else:
        kc, vc = _cache(shape, kind, 3, nanp), _cache(shape, kind, 4, nanp)
    slot = lambda b, p: int(bt[b, p // PAGE]) * PAGE + p % PAGE              # noqa: E731
    src = [slot(b, L[b] + t) for b in range(2) for t in acc[b]]
    dst = [slot(b, L[b] + i) for b in range(2) for i in range(3)]
    assert set(src) & set(dst) and src != dst
    # a padding pair in the middle (skipped) and a source out of range (stores zeros)
    spare = slot(0, L[0] + 5)
    src, dst = src + [src[0], -1], dst + [-1, spare]

    def expect(c):
        e = guard.bits(c.cpu().clone()).view(-1, HK, D)
        rows = [e[s].clone() if s >= 0 else torch.zeros_like(e[0]) for s in src]          # every read before any write
        for r, d in zip(rows, dst):
            if d >= 0:
                e[d] = r
        return e.view(shape)

    want_k, want_v = expect(kc), expect(vc)
    assert not torch.equal(want_k, guard.bits(kc.cpu()))
    assert _move(kc, vc, torch.tensor(src, device="cuda"), torch.tensor(dst, device="cuda")) is None
    torch.cuda.synchronize()
    assert torch.equal(guard.bits(kc.cpu()), want_k), "k_cache after the move"
    assert torch.equal(guard.bits(vc.cpu()), want_v), "v_cache after the move"
    # page copy: pages (p0, p1) -> (p2, p3)
    p = [int(bt[0, 0]), int(bt[1, 1]), int(bt[1, 0]), int(bt[0, 1])]
    src = torch.cat([torch.arange(PAGE) + p[0] * PAGE, torch.arange(PAGE) + p[1] * PAGE]).to(torch.int32)
    dst = torch.cat([torch.arange(PAGE) + p[2] * PAGE, torch.arange(PAGE) + p[3] * PAGE]).to(torch.int32)
    want_k, want_v = guard.bits(kc.cpu().clone()), guard.bits(vc.cpu().clone())
    for w in (want_k, want_v):
        w[p[2]], w[p[3]] = w[p[0]].clone(), w[p[1]].clone()
    assert torch.ops.flash_attn_mi355.kv_move(kc, vc, src.cuda(), dst.cuda()) is None
    torch.cuda.synchronize()
    assert torch.equal(guard.bits(kc.cpu()), want_k), "k_cache after the page copy"
    assert torch.equal(guard.bits(vc.cpu()), want_v), "v_cache after the page copy"


# 8 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fp16", "bf16", "fp8"])
def test_shared_prefix_out_of_a_paged_cache(kind):
    """a 48-token prefix gathered out of three pages (sequence mode, batch 1, one block-table row) and handed to
    flash_attn_with_shared_prefix: out and lse equal the call with the torch-indexed prefix bit for bit; for an fp8 cache the
    gathered bf16 prefix against (pages.float() * descale).to(bf16)"""
    from flash_attn_mi355.cascade import flash_attn_with_shared_prefix
    fp8 = kind == "fp8"
    dt, D, Hq, B, Sp = ("bf16" if fp8 else kind), 128, 4, 3, 48
    bt, nblk, nanp = guard.paged_table([Sp], PAGE, seed=8)
    if fp8:
        kc, vc = _cache8((nblk, PAGE, HK, D), 3, nanp), _cache8((nblk, PAGE, HK, D), 4, nanp)
        kd, vd = 0.01, 0.008
        kw = dict(dtype=DT[dt], k_descale=kd, v_descale=vd)
        f32 = lambda x: torch.tensor(x, dtype=torch.float32, device="cuda")       # noqa: E731
        pk_t = (kc[bt[0].long().cuda()].float() * f32(kd)).to(DT[dt]).reshape(Sp, HK, D)
        pv_t = (vc[bt[0].long().cuda()].float() * f32(vd)).to(DT[dt]).reshape(Sp, HK, D)
    else:
        kc, vc = _cache((nblk, PAGE, HK, D), dt, 3, nanp), _cache((nblk, PAGE, HK, D), dt, 4, nanp)
        kw = {}
        pk_t, pv_t = kc[bt[0].long().cuda()].reshape(Sp, HK, D), vc[bt[0].long().cuda()].reshape(Sp, HK, D)
    pk, pv = _gather(kc, vc, cu_seqlens=_i32([0, Sp]), block_table=bt.cuda(), total_rows=Sp, **kw)
    torch.cuda.synchronize()
    assert G.same_bits(pk, pk_t) and G.same_bits(pv, pv_t)
    q = rand16((B, 1, Hq, D), dt, 5)
    ks, vs = rand16((B, 64, HK, D), dt, 6), rand16((B, 64, HK, D), dt, 7)
    lens = _i32([0, 17, 64])
    out_a, lse_a = flash_attn_with_shared_prefix(q, pk, pv, ks, vs, cache_seqlens=lens, return_softmax_lse=True)
    out_b, lse_b = flash_attn_with_shared_prefix(q, pk_t, pv_t, ks, vs, cache_seqlens=lens, return_softmax_lse=True)
    torch.cuda.synchronize()
    assert torch.isfinite(out_a.float()).all() and torch.isfinite(lse_a).all()
    assert torch.equal(out_a.view(torch.int16), out_b.view(torch.int16)), "out differs from the torch-indexed prefix"
    assert torch.equal(lse_a.view(torch.int32), lse_b.view(torch.int32)), "lse differs from the torch-indexed prefix"


# 9 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_gather_and_store_replay_in_a_graph(kind):
    """gather_kv_cache (slot mode, one padding slot) followed by store_kv_cache into a second cache, captured in one graph on one
    stream; replayed after the source cache and the slots were overwritten in place: the gathered rows and the second cache
    equal the eager results bit for bit"""
    fp8 = kind == "fp8"
    dt, D, nblk, T, steps = "bf16", 128, 6, 9, 3
    shape = (nblk, PAGE, HK, D)
    mk = (lambda s: _cache8(shape, s)) if fp8 else (lambda s: _cache(shape, dt, s))
    gkw = dict(dtype=DT[dt], k_descale=0.05, v_descale=0.04) if fp8 else {}
    skw = dict(k_descale=0.05, v_descale=0.04) if fp8 else {}
    srcs = [(mk(10 + i), mk(20 + i)) for i in range(steps)]
    g = torch.Generator().manual_seed(1)
    s_src, s_dst = [], []
    for i in range(steps):
        a, b = torch.randperm(nblk * PAGE, generator=g)[:T], torch.randperm(nblk * PAGE, generator=g)[:T]
        a[i + 2] = -1                                       # a zero row
        b[i + 4] = -1                                       # a skipped row
        s_src.append(a.cuda()); s_dst.append(b.cuda())
    dst0 = mk(30), mk(31)

    def make_step(kc, vc, kc2, vc2, a, b, out):
        def step():
            k, v = _gather(kc, vc, slot_mapping=a, out=out, **gkw)
            _store(k, v, kc2, vc2, slot_mapping=b, **skw)
        return step

    ref = []
    for i in range(steps):
        out = _nan_out(T, D, dt)
        d = dst0[0].clone(), dst0[1].clone()
        make_step(*srcs[i], *d, s_src[i], s_dst[i], out)()
        torch.cuda.synchronize()
        ref.append((out, d))
    assert not G.same_bits(ref[0][0][0], ref[1][0][0]) and not R.same_bits(ref[0][1][0], dst0[0])
    kc_s, vc_s = srcs[0][0].clone(), srcs[0][1].clone()
    kc2_s, vc2_s = dst0[0].clone(), dst0[1].clone()
    a_s, b_s = s_src[0].clone(), s_dst[0].clone()
    out_s = _nan_out(T, D, dt)
    step = make_step(kc_s, vc_s, kc2_s, vc2_s, a_s, b_s, out_s)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for i in range(steps):
        kc_s.copy_(srcs[i][0]); vc_s.copy_(srcs[i][1]); kc2_s.copy_(dst0[0]); vc2_s.copy_(dst0[1])
        a_s.copy_(s_src[i]); b_s.copy_(s_dst[i])
        guard.fill_nan(out_s[0]); guard.fill_nan(out_s[1])
        graph.replay()
        torch.cuda.synchronize()
        G.diff_report(out_s[0], ref[i][0][0], f"step {i}: gathered k")
        G.diff_report(out_s[1], ref[i][0][1], f"step {i}: gathered v")
        R.diff_report(kc2_s, ref[i][1][0], f"step {i}: second k_cache")
        R.diff_report(vc2_s, ref[i][1][1], f"step {i}: second v_cache")


# 10 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["slot", "seq-fp8"])
def test_torch_op_gives_the_same_bits(mode):
    import flash_attn_mi355.torch_ops  # noqa: F401  (registers the ops)
    dt, D = "fp16", 64
    lens, off = [5, 0, 30], [2, 9, 16]
    T = sum(lens) + 1
    bt, nblk, nanp = guard.paged_table([a + b for a, b in zip(lens, off)], PAGE, seed=16)
    if mode == "slot":
        kc, vc = _cache((nblk, PAGE, HK, D), dt, 3, nanp), _cache((nblk, PAGE, HK, D), dt, 4, nanp)
        slots = _slots(T, nblk * PAGE, 18, usable=nanp * PAGE).cuda()
        want = _gather(kc, vc, slot_mapping=slots)
        got = torch.ops.flash_attn_mi355.kv_gather(kc, vc, slots, None, None, None, None, T, DT[dt], 1.0, 1.0)
    else:
        kc, vc = _cache8((nblk, PAGE, HK, D), 3, nanp), _cache8((nblk, PAGE, HK, D), 4, nanp)
        cu, offd, btd = _i32(_cu(lens)), _i32(off), bt.cuda()
        want = _gather(kc, vc, cu_seqlens=cu, seq_offsets=offd, block_table=btd, total_rows=T, dtype=DT[dt], k_descale=0.05, v_descale=0.04)
        got = torch.ops.flash_attn_mi355.kv_gather(kc, vc, None, cu, offd, btd, None, T, DT[dt], 0.05, 0.04)
    torch.cuda.synchronize()
    assert len(got) == 2 and got[0].dtype == DT[dt] and tuple(got[0].shape) == (T, HK, D)
    assert float(want[0].float().abs().sum()) > 0
    assert G.same_bits(got[0], want[0]) and G.same_bits(got[1], want[1])
