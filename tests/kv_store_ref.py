"""Torch CPU restatement of fa_kv_store for its tests (a plain helper module, like merge_ref.py: no fixtures).

  destinations()   where every source row goes: a list of (block, row) or None (dropped), for slot mode and sequence mode.
  quantise()       the fp8-e4m3 rule in fp32: (x.float() * (float32(1) / float32(descale))).clamp(-448, 448).to(float8_e4m3fn).
                   torch's cast is round-to-nearest-even (17 -> 16, 19 -> 20, 2^-10 -> 0, -0 keeps its sign; NaN above 464
                   without the clamp, 448 with it), and on 400 000 random fp16 and bf16 values with descales 0.0625, 0.03125,
                   0.05, 0.04 and 0.013 the expression agreed code for code with oracle.kvcache.round_e4m3(x / d).
  kv_store_ref()   the expected (k_cache, v_cache) as CPU tensors of the cache dtype; the caches passed in are not modified.
                   With rotary tables K is rotated by rotary_ref.rotary_ref (fp64, one rounding to the 16-bit type): that is a
                   reference within rotary_ref.bound, not bit for bit - the bitwise checks of the rotated store go against the
                   library's own kernels.
  same_bits()      bit-exact equality of two caches (integer views: -0 != +0, NaN == NaN)."""
import numpy as np
import torch

import rotary_ref

FP8 = torch.float8_e4m3fn
_INT_OF = {torch.float16: torch.int16, torch.bfloat16: torch.int16, FP8: torch.uint8}


def _list(t):
    return None if t is None else [int(x) for x in (t.tolist() if isinstance(t, torch.Tensor) else list(t))]


def destinations(total_rows, cache_shape, *, slot_mapping=None, cu_seqlens=None, cache_seqlens=None, block_table=None,
                 cache_batch_idx=None):
    """(dest, pos): dest[r] = (block, row) of source row r in a cache of `cache_shape` ([nblk, page, ...] or [Bc, S_max, ...]) or
    None when the row is dropped; pos[r] = its position inside its sequence's cache (sequence mode; -1 for rows of no sequence)"""
    nblk, page = int(cache_shape[0]), int(cache_shape[1])
    dest, pos = [None] * total_rows, [-1] * total_rows
    if slot_mapping is not None:
        assert cu_seqlens is None
        for r, s in enumerate(_list(slot_mapping)):
            if 0 <= s < nblk * page:
                dest[r] = (s // page, s % page)
        return dest, pos
    cu = _list(cu_seqlens)
    L = _list(cache_seqlens) or [0] * (len(cu) - 1)
    bt = None if block_table is None else np.asarray(block_table.cpu() if isinstance(block_table, torch.Tensor) else block_table)
    cbi = _list(cache_batch_idx)
    capacity = bt.shape[1] * page if bt is not None else page
    for b in range(len(cu) - 1):
        for r in range(cu[b], min(cu[b + 1], total_rows)):
            p = L[b] + (r - cu[b])
            pos[r] = p
            if not 0 <= p < capacity:
                continue                                   # dropped: past the capacity
            if bt is not None:
                dest[r] = (int(bt[b, p // page]), p % page)
            else:
                dest[r] = (cbi[b] if cbi is not None else b, p)
    return dest, pos


def quantise(x, descale):
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(descale), dtype=torch.float32)
    return (x.float() * inv).clamp(-448, 448).to(FP8)


def kv_store_ref(k, v, k_cache, v_cache, *, slot_mapping=None, cu_seqlens=None, cache_seqlens=None, block_table=None,
                 cache_batch_idx=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=True, k_descale=None, v_descale=None):
    k, v = k.detach().cpu(), v.detach().cpu()
    kc, vc = k_cache.detach().cpu().clone(), v_cache.detach().cpu().clone()
    T = k.shape[0]
    dest, pos = destinations(T, kc.shape, slot_mapping=slot_mapping, cu_seqlens=cu_seqlens, cache_seqlens=cache_seqlens,
                             block_table=block_table, cache_batch_idx=cache_batch_idx)
    if rotary_cos is not None:
        assert cu_seqlens is not None
        y64, _ = rotary_ref.rotary_ref(k, rotary_cos.cpu(), rotary_sin.cpu(), np.asarray(pos), rotary_interleaved)
        k = torch.from_numpy(y64).to(k.dtype)
    if kc.dtype == FP8:
        k = quantise(k, 1.0 if k_descale is None else k_descale)
        v = quantise(v, 1.0 if v_descale is None else v_descale)
    kci, vci = kc.view(_INT_OF[kc.dtype]), vc.view(_INT_OF[vc.dtype])
    ki, vi = k.contiguous().view(_INT_OF[k.dtype]), v.contiguous().view(_INT_OF[v.dtype])
    for r, d in enumerate(dest):
        if d is not None:
            kci[d[0], d[1]] = ki[r]
            vci[d[0], d[1]] = vi[r]
    return kc, vc


def same_bits(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(_INT_OF[a.dtype]), b.view(_INT_OF[b.dtype])))


def diff_report(got, want, name):
    """assert same_bits with the first differing element named"""
    g, w = got.detach().cpu(), want.detach().cpu()
    assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
    ne = g.view(_INT_OF[g.dtype]) != w.view(_INT_OF[w.dtype])
    if ne.any():
        idx = torch.nonzero(ne)
        first = tuple(int(i) for i in idx[0])
        raise AssertionError(f"{name}: {idx.shape[0]} of {ne.numel()} elements differ; first at (block, row, head, col) = {first}: "
                             f"got {float(g[first].float())}, expected {float(w[first].float())}")
