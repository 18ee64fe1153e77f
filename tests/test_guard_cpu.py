"""CPU: the guard-band helpers (tests/guard.py) detect what tests/test_guard_bands_gpu.py relies on them to detect - planted
writes outside a slab's view, a one-byte workspace overrun - and build slabs the wrappers take without a copy."""
import pytest
import torch

import guard

FP8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def fi():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import flash_attn_interface
    return flash_attn_interface


def _plant(buf, off):
    """flip one element of the 1-D allocation"""
    b = guard.bits(buf)
    b[off] = b[off] ^ 1


SHAPE = (2, 5, 3, 40)          # B, S, H, D


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, FP8, torch.float32])
@pytest.mark.parametrize("gaps", [True, False])
def test_slab_layout_bands_and_fill(dtype, gaps):
    shape = (2, 5, 3, 48)
    buf, view = guard.slab(shape, dtype, gaps=gaps, device="cpu", check_prep=False)
    item = buf.element_size()
    bs, rs, hs, cs = view.stride()
    assert tuple(view.shape) == shape and cs == 1 and view.data_ptr() % 16 == 0
    if gaps:
        a = 16 if dtype == FP8 else 8
        assert hs > shape[3] and rs > shape[2] * hs and bs > shape[1] * rs
        assert all(s % a == 0 for s in (bs, rs, hs))
    else:
        assert view.is_contiguous()
    head = view.storage_offset()
    last = head + sum((n - 1) * s for n, s in zip(shape, view.stride()))
    tail = buf.numel() - 1 - last
    for band in (head, tail):
        assert band >= 256 * rs and band * item >= 64 * 1024
    # every element - bands, gaps and the view - holds the dtype's NaN pattern
    assert bool((guard.bits(buf) == guard._NAN_BITS[dtype]).all())
    if dtype != FP8:
        assert bool(torch.isnan(buf).all())
    else:
        assert bool(torch.isnan(buf.float()).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, FP8, torch.float32])
def test_assert_untouched_finds_a_planted_write_in_every_region(dtype):
    buf, view = guard.slab(SHAPE, dtype, gaps=True, device="cpu", check_prep=False)
    snap = guard.snapshot(buf)
    B, S, H, D = SHAPE
    bs, rs, hs, _ = view.stride()
    base = view.storage_offset()
    guard.assert_untouched(buf, view, snap, "clean")
    spots = {
        "head band, first element": 0,
        "head band, one before the view": base - 1,
        "tail band, one past the view": base + (B - 1) * bs + (S - 1) * rs + (H - 1) * hs + D,
        "tail band, last element": buf.numel() - 1,
        "row gap": base + 1 * bs + 2 * rs + H * hs,                   # behind the last head of row 2
        "batch gap": base + S * rs,                                   # behind the last row of batch 0
        "head gap / columns between D and the head stride": base + 3 * rs + 1 * hs + D,
        "last column of the head stride": base + 4 * rs + 2 * hs + hs - 1,
    }
    for where, off in spots.items():
        assert 0 <= off < buf.numel()
        _plant(buf, off)
        with pytest.raises(AssertionError) as e:
            guard.assert_untouched(buf, view, snap, where)
        assert where in str(e.value) and "1 elements" in str(e.value), where
        assert f"offset {off - base} " in str(e.value)
        _plant(buf, off)                                              # (undo)
        guard.assert_untouched(buf, view, snap, where)


def test_assert_untouched_reports_first_and_last_in_rows_heads_columns():
    buf, view = guard.slab(SHAPE, torch.float16, gaps=True, device="cpu", check_prep=False)
    snap = guard.snapshot(buf)
    bs, rs, hs, _ = view.stride()
    base = view.storage_offset()
    _plant(buf, base + 1 * bs + 2 * rs + 1 * hs + 41)                 # column 41 of a 40-column head
    _plant(buf, base + 1 * bs + 7 * rs + 3)                           # two rows past the last row of batch 1 (tail band)
    with pytest.raises(AssertionError) as e:
        guard.assert_untouched(buf, view, snap, "dq")
    msg = str(e.value)
    assert "dq: 2 elements" in msg
    assert "first at" in msg and "batch 1, row 2, head 1, col 41 (outside 0..39)" in msg
    assert "last at" in msg and "batch 1, row 7 (outside 0..4), head 0, col 3" in msg


def test_assert_untouched_accepts_writes_inside_the_view():
    for dtype in (torch.bfloat16, torch.float16, torch.float32, FP8):
        buf, view = guard.slab(SHAPE, dtype, gaps=True, device="cpu", check_prep=False)
        snap = guard.snapshot(buf)
        guard.bits(view).fill_(3)                                     # every logical element, and nothing else
        guard.assert_untouched(buf, view, snap, "inside")
        inside = guard._inside(buf, view)
        assert int(inside.sum()) == view.numel()
        assert bool((guard.bits(buf)[inside] == 3).all()) and bool((guard.bits(buf)[~inside] == snap[~inside]).all())


@pytest.mark.parametrize("D", [40, 64, 96, 128, 192, 256])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_slab_passes_prep_without_a_copy(fi, D, dtype):
    for shape in ((2, 7, 3, D), (11, 3, D)):                          # [B, S, H, D] and the packed [T, H, D]
        for gaps in (True, False):
            buf, view = guard.slab(shape, dtype, gaps=gaps, device="cpu")       # (asserts _prep(view, D) is view itself)
            assert fi._prep(view, D) is view
            assert view.stride(-1) == 1 and view.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in view.stride()[:-1])
            if gaps:
                assert view.stride(-2) > D and not view.is_contiguous()
            # and as a caller-allocated output the wrappers write it in place
            assert fi._usable_out(view, D, D)


@pytest.mark.parametrize("D", [16, 48, 64, 128])
def test_fp8_slab_passes_prep8_without_a_copy(fi, D):
    for shape in ((2, 7, 3, D), (11, 3, D)):
        buf, view = guard.slab(shape, FP8, gaps=True, device="cpu")
        assert fi._prep8(view, D) is view
        assert all(s % 16 == 0 for s in view.stride()[:-1]) and view.stride(-2) > D


def test_slab_refuses_a_layout_prep_would_copy(fi):
    with pytest.raises(AssertionError):
        guard.slab((2, 7, 3, 44), torch.float16, gaps=True, device="cpu")        # D = 44 is padded to 48: a copy


def test_slab_row_dim_sizes_the_bands_of_a_kv_packed_slab():
    """[B, S, 2, H, D]: the rows are dimension 1 - 256 of them span k and v of 256 keys, twice what dimension -3 spans"""
    shape = (1, 9, 2, 300, 128)
    buf, view = guard.slab(shape, FP8, gaps=True, device="cpu", check_prep=False, row_dim=1)
    assert view.storage_offset() >= 256 * view.stride(1) > 256 * view.stride(2)
    last = view.storage_offset() + sum((n - 1) * st for n, st in zip(shape, view.stride()))
    assert buf.numel() - 1 - last >= 256 * view.stride(1)


def test_guarded_copies_the_data_and_nothing_else():
    x = torch.randn(3, 4, 2, 64).to(torch.bfloat16)
    buf, view, snap = guard.guarded(x, gaps=True)
    assert torch.equal(view, x)
    inside = guard._inside(buf, view)
    assert bool((guard.bits(buf)[~inside] == 0x7FC1).all())
    guard.assert_untouched(buf, view, snap, "x")
    x8 = torch.randn(3, 4, 2, 64).to(FP8)
    buf, view, snap = guard.guarded(x8, gaps=True)
    assert torch.equal(view.view(torch.uint8), x8.view(torch.uint8))


@pytest.mark.parametrize("fill", ["zeros", "ones", "random"])
def test_guarded_workspace_sizes_alignment_fill_and_overrun(fill):
    ws_fn, check = guard.guarded_workspace(fill)
    sizes = [70400, 1, 0, 3 * (1 << 20) + 17, 255]
    got = [ws_fn(n, torch.device("cpu")) for n in sizes]
    assert got[2] is None                                              # _workspace's contract: nothing for 0 bytes
    for n, ws in zip(sizes, got):
        if n:
            assert ws.dtype == torch.uint8 and ws.numel() == n and ws.data_ptr() % 256 == 0 and ws.is_contiguous()
            if fill == "zeros":
                assert bool((ws == 0).all())
            elif fill == "ones":
                assert bool((ws == 0xFF).all()) and bool(torch.isnan(ws[: n // 4 * 4].view(torch.float32)).all())
    if fill == "random":
        assert len(torch.unique(got[0])) > 200 and not torch.equal(got[0][:255], got[4])
        again = guard.guarded_workspace("random")[0](sizes[0], torch.device("cpu"))
        assert torch.equal(again, got[0])                              # seeded: the same bytes in every run
    rep = check()
    assert rep == {"requests": 5, "sizes": sizes}
    # writes inside are fine; one byte past the end, or one before the start, is caught
    got[0].fill_(7)
    check()
    for k, (ws, off, text) in enumerate(((got[0], sizes[0], "0 bytes past the end"), (got[3], -1, "1 bytes before the start"),
                                         (got[1], 1 + (1 << 20) - 1, "past the end"))):
        base = ws.untyped_storage()
        whole = torch.empty(0, dtype=torch.uint8).set_(base)
        pos = ws.storage_offset() + off
        old = int(whole[pos])
        assert old == guard.WS_SENTINEL
        whole[pos] = old ^ 0x10
        with pytest.raises(AssertionError) as e:
            check()
        assert text in str(e.value) and "1 guard bytes" in str(e.value)
        whole[pos] = old
        check()


def test_guarded_workspace_bands_are_at_least_the_request_and_a_mebibyte():
    ws_fn, check = guard.guarded_workspace("zeros")
    for n in (100, 5 << 20):
        ws = ws_fn(n, torch.device("cpu"))
        total = ws.untyped_storage().nbytes()
        lo = ws.storage_offset()
        assert lo >= max(n, 1 << 20) and total - lo - n >= max(n, 1 << 20)
    check()


def test_paged_table_points_unreferenced_entries_at_the_nan_page():
    lens, page = [300, 0, 77, 513], 64
    bt, nblk, nan_page = guard.paged_table(lens, page, width=10, seed=3)
    assert bt.dtype == torch.int32 and tuple(bt.shape) == (4, 10) and nan_page == nblk - 1
    used = []
    for b, l in enumerate(lens):
        n = (l + page - 1) // page
        used += bt[b, :n].tolist()
        assert bool((bt[b, n:] == nan_page).all())
    assert len(set(used)) == len(used) and nan_page not in used and all(0 <= p < nblk - 1 for p in used)
