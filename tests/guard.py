"""Guard bands for the tests that check what an op does OUTSIDE the elements it is meant to produce (a plain helper module, like
tree_ref.py: no fixtures, no pytest settings).

  slab()               a tensor view of the requested logical shape inside one larger 1-D allocation: a head band and a tail band
                       around it (each >= 256 rows of the view's row stride - the largest tile any kernel here works in - and
                       >= 64 KiB), optionally with gaps between columns, heads, rows and batch entries.  Everything is filled
                       with a NaN bit pattern, so a read past an input poisons the result and an unwritten output element shows.
  snapshot() /         bit-exact comparison (integer views: NaN != NaN) of every byte outside the view's logical elements, with
  assert_untouched()   the first and last changed offsets reported in rows / heads / columns of the view.
  guarded_workspace()  a replacement for flash_attn_interface._workspace: exactly the queried bytes, 256-byte aligned, between
                       two sentinel bands of max(n, 1 MiB); the interior zeroed, 0xFF (fp32 NaN, integer -1) or seeded random.
  paged_table()        block tables whose unreferenced entries point at one dedicated page the caller fills with NaN: integer side
                       tables never hold wild values, so a read through a stale entry stays in memory the test owns.

Works on CPU tensors (tests/test_guard_cpu.py) and on the GPU."""
import numpy as np
import torch

FP8 = torch.float8_e4m3fn
# NaN bit patterns per dtype (a quiet NaN with a payload bit: never produced by arithmetic on finite data)
_INT_OF = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, FP8: torch.uint8,
           torch.uint8: torch.uint8}
_NAN_BITS = {torch.float16: 0x7FC1, torch.bfloat16: 0x7FC1, torch.float32: 0x7FC00001, FP8: 0x7F}
MAX_TILE_ROWS = 256
MIN_BAND_BYTES = 64 * 1024
WS_MIN_BAND = 1 << 20
WS_SENTINEL = 0xA5


def _up(x, a):
    return (x + a - 1) // a * a


def bits(t):
    """integer view of a tensor's bytes (same shape and strides)"""
    return t.view(_INT_OF[t.dtype])


def fill_nan(t):
    """every element of `t` (a view is fine) becomes the dtype's NaN bit pattern"""
    bits(t).fill_(_NAN_BITS[t.dtype])
    return t


def slab_strides(shape, dtype, gaps):
    """element strides of a slab view: contiguous, or with gaps - every stride a multiple of 8 elements (16 for fp8), the head
    stride > D, the row stride > H x head stride, the batch stride > S x row stride"""
    a = 16 if dtype == FP8 else 8
    strides = [1]
    extent = shape[-1]
    for n in reversed(shape[:-1]):
        st = _up(extent, a) + a if gaps else extent
        strides.insert(0, st)
        extent = st * n
    return tuple(strides)


def slab(shape, dtype, *, gaps, device, check_prep=None, row_dim=-3):
    """(buf, view): `view` has the logical `shape` ([..., S, H, D]; the row stride is the S stride - `row_dim` names another
    dimension as the rows, e.g. 1 for a kv-packed [B, S, 2, H, D]) and lies inside the 1-D
    allocation `buf` between two bands; every element of buf - bands, gaps and the view itself - holds the dtype's NaN pattern
    (inputs: view.copy_(data) afterwards).  16-bit and fp8 slabs must pass flash_attn_interface._prep / _prep8 WITHOUT a copy
    (asserted: a silent copy would turn a guard test into a no-op); check_prep=False for tensors that never go through them."""
    shape = tuple(int(s) for s in shape)
    strides = slab_strides(shape, dtype, gaps)
    item = torch.empty((), dtype=dtype).element_size()
    row_stride = strides[row_dim] if len(shape) >= 3 else strides[0]
    band = _up(max(MAX_TILE_ROWS * row_stride, MIN_BAND_BYTES // item), 16)          # (a multiple of 16 elements: 16-byte aligned start)
    span = sum((n - 1) * st for n, st in zip(shape, strides)) + 1 if all(shape) else 0
    buf = torch.empty(band + span + band, dtype=dtype, device=device)
    fill_nan(buf)
    view = buf.as_strided(shape, strides, band)
    assert view.data_ptr() % 16 == 0
    if check_prep is None:
        check_prep = dtype in (torch.float16, torch.bfloat16, FP8) and len(shape) >= 3
    if check_prep:
        from flash_attn_mi355 import flash_attn_interface as fi
        prep, mult = (fi._prep8, 16) if dtype == FP8 else (fi._prep, 8)
        assert shape[-1] % mult == 0, f"head dim {shape[-1]}: the wrapper pads it to a multiple of {mult} (a copy)"
        assert prep(view, shape[-1]) is view, f"slab {shape} strides {strides}: _prep would copy it"
    return buf, view


def snapshot(buf):
    return bits(buf).clone()


def _inside(buf, view):
    """bool [buf.numel()]: the logical elements of `view`"""
    m = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    m.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(True)
    return m


def describe_offset(off, view):
    """an element offset relative to view[0, ..., 0] as batch / row / head / column of the view's strides"""
    names = {2: ("row", "col"), 3: ("row", "head", "col"), 4: ("batch", "row", "head", "col")}.get(
        view.dim(), tuple(f"dim{i}" for i in range(view.dim())))
    parts, rem = [], int(off)
    for d, (name, st, n) in enumerate(zip(names, view.stride(), view.shape)):
        i = rem // st if st else 0
        if d == 0 and view.dim() >= 4:
            i = min(max(i, 0), n - 1)                     # (the bands count as rows before batch 0 / past the last batch)
        rem -= i * st
        parts.append(f"{name} {i}" + ("" if 0 <= i < n else f" (outside 0..{n - 1})"))
    row_stride = view.stride(-3) if view.dim() >= 3 else view.stride(0)
    return f"offset {int(off)} = " + ", ".join(parts) + f" [{off / max(row_stride, 1):+.2f} rows from the view's start]"


def changed_outside(buf, view, snap):
    """offsets (relative to the view's first element) of the elements outside the view that differ from the snapshot"""
    diff = (bits(buf) != snap) & ~_inside(buf, view)
    return torch.nonzero(diff).flatten() - (view.storage_offset() - buf.storage_offset())


def assert_untouched(buf, view, snap, name):
    """every byte of `buf` outside the logical elements of `view` is bit-identical to `snap` (synchronise first on the GPU)"""
    idx = changed_outside(buf, view, snap)
    if idx.numel():
        first, last = int(idx[0]), int(idx[-1])
        raise AssertionError(f"{name}: {idx.numel()} elements outside the tensor were written; first at "
                             f"{describe_offset(first, view)}; last at {describe_offset(last, view)}")


def guarded(data=None, *, shape=None, dtype=None, gaps=True, device=None, row_dim=-3):
    """slab + copy + snapshot in one: (buf, view, snap).  `data` (a tensor: an input) is copied into the view; without data
    (an output) the view keeps its NaN fill."""
    if data is not None:
        shape, dtype, device = data.shape, data.dtype, data.device
    buf, view = slab(shape, dtype, gaps=gaps, device=device, row_dim=row_dim)
    if data is not None:
        if dtype == FP8:
            view.view(torch.uint8).copy_(data.view(torch.uint8))
        else:
            view.copy_(data)
    return buf, view, snapshot(buf)


def guarded_workspace(fill):
    """(workspace(nbytes, device), check): workspace() has _workspace's signature; each request of n > 0 bytes gets a 256-byte
    aligned uint8 slice of exactly n bytes inside its own buffer, with max(n, 1 MiB) of sentinel bytes on both sides and the
    interior set by `fill`: 'zeros', 'ones' (0xFF) or 'random' (seeded).  check() synchronises, asserts that every band of every
    workspace handed out still holds the sentinel and returns the sizes requested (zero-byte requests included)."""
    assert fill in ("zeros", "ones", "random")
    handed, sizes = [], []

    def workspace(nbytes, device):
        nbytes = int(nbytes)
        sizes.append(nbytes)
        if nbytes <= 0:
            return None
        band = _up(max(nbytes, WS_MIN_BAND), 256)
        buf = torch.empty(band + nbytes + band + 256, dtype=torch.uint8, device=device)
        lo = band + (-(buf.data_ptr() + band)) % 256
        buf.fill_(WS_SENTINEL)
        ws = buf[lo:lo + nbytes]
        if fill == "zeros":
            ws.zero_()
        elif fill == "ones":
            ws.fill_(0xFF)
        else:
            g = torch.Generator(device="cpu").manual_seed(977 + len(handed))
            ws.copy_(torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8))
        assert ws.data_ptr() % 256 == 0 and ws.numel() == nbytes
        handed.append((buf, lo, nbytes))
        return ws

    def check():
        if any(b.is_cuda for b, _, _ in handed):
            torch.cuda.synchronize()
        for i, (buf, lo, n) in enumerate(handed):
            bad = buf != WS_SENTINEL
            bad[lo:lo + n] = False
            idx = torch.nonzero(bad).flatten()
            if idx.numel():
                first, last = int(idx[0]) - lo, int(idx[-1]) - lo
                where = lambda o: f"{-o} bytes before the start" if o < 0 else f"{o - n} bytes past the end (byte {o} of {n})"
                raise AssertionError(f"workspace {i} ({n} bytes, fill '{fill}'): {idx.numel()} guard bytes were written; first "
                                     f"{where(first)}, last {where(last)}")
        return {"requests": len(sizes), "sizes": list(sizes)}

    return workspace, check


def paged_table(lens, page, width=None, spare=2, seed=0):
    """Block table for sequences of `lens` tokens in pages of `page`: (table int32 [B, width] on the CPU, number of pages, index
    of the NaN page).  The referenced pages are a seeded permutation; every unreferenced table entry points at one dedicated
    page (the last) that the caller fills with NaN and no sequence owns."""
    need = [(int(l) + page - 1) // page for l in lens]
    width = max(max(need), 1) if width is None else width
    assert width >= max(need)
    nblk = sum(need) + spare + 1
    nan_page = nblk - 1
    perm = iter(np.random.default_rng(seed).permutation(nblk - 1).tolist())
    bt = torch.full((len(lens), width), nan_page, dtype=torch.int32)
    for b, n in enumerate(need):
        for j in range(n):
            bt[b, j] = next(perm)
    return bt, nblk, nan_page
