"""Torch CPU restatement of fa_kv_gather for its tests (a plain helper module, like kv_store_ref.py: no fixtures).

  sources()        where every output row comes from: kv_store_ref.destinations with seq_offsets in the place of cache_seqlens -
                   the addressing is the store's rule read backwards: a list of (block, row) or None (a row of zeros).
  dequantise()     the fp8-e4m3 way back: (code.float() * float32(descale)).to(dtype) - the exact conversion of the code, one
                   fp32 multiply, one rounding (torch's casts are round-to-nearest-even).
  kv_gather_ref()  the expected (k, v) as contiguous CPU tensors [total_rows, Hk, D] of `dtype`: a bit copy of a 16-bit cache,
                   dequantise() of an fp8 one, +0 for rows that name nothing.
  same_bits() / diff_report()   bit-exact comparison (integer views: -0 != +0, NaN == NaN), kv_store_ref's."""
import torch

import kv_store_ref

FP8 = kv_store_ref.FP8
_INT_OF = kv_store_ref._INT_OF
same_bits = kv_store_ref.same_bits


def sources(total_rows, cache_shape, *, slot_mapping=None, cu_seqlens=None, seq_offsets=None, block_table=None, cache_batch_idx=None):
    return kv_store_ref.destinations(total_rows, cache_shape, slot_mapping=slot_mapping, cu_seqlens=cu_seqlens,
                                     cache_seqlens=seq_offsets, block_table=block_table, cache_batch_idx=cache_batch_idx)[0]


def dequantise(codes, descale, dtype):
    return (codes.float() * torch.tensor(float(descale), dtype=torch.float32)).to(dtype)


def kv_gather_ref(k_cache, v_cache, *, slot_mapping=None, cu_seqlens=None, seq_offsets=None, block_table=None, cache_batch_idx=None,
                  total_rows=None, dtype=None, k_descale=None, v_descale=None):
    kc, vc = k_cache.detach().cpu(), v_cache.detach().cpu()
    if total_rows is None:
        total_rows = len(kv_store_ref._list(slot_mapping))
    if kc.dtype == FP8:
        assert dtype in (torch.float16, torch.bfloat16)
        kc = dequantise(kc, 1.0 if k_descale is None else k_descale, dtype)
        vc = dequantise(vc, 1.0 if v_descale is None else v_descale, dtype)
    else:
        assert dtype in (None, kc.dtype)
    src = sources(total_rows, kc.shape, slot_mapping=slot_mapping, cu_seqlens=cu_seqlens, seq_offsets=seq_offsets,
                  block_table=block_table, cache_batch_idx=cache_batch_idx)
    k = torch.zeros((total_rows,) + tuple(kc.shape[2:]), dtype=kc.dtype)
    v = torch.zeros_like(k)
    ki, vi, kci, vci = (t.view(_INT_OF[t.dtype]) for t in (k, v, kc, vc))
    for r, s in enumerate(src):
        if s is not None:
            ki[r] = kci[s[0], s[1]]
            vi[r] = vci[s[0], s[1]]
    return k, v


def diff_report(got, want, name):
    """assert same_bits with the first differing element named"""
    g, w = got.detach().cpu(), want.detach().cpu()
    assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
    ne = g.contiguous().view(_INT_OF[g.dtype]) != w.contiguous().view(_INT_OF[w.dtype])
    if ne.any():
        idx = torch.nonzero(ne)
        first = tuple(int(i) for i in idx[0])
        raise AssertionError(f"{name}: {idx.shape[0]} of {ne.numel()} elements differ; first at {first}: "
                             f"got {float(g[first].float())}, expected {float(w[first].float())}")
