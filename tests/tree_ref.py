"""Two independent fp64 formulations of tree attention over a KV cache (speculative decoding: the T_q query tokens of a
call are the nodes of a draft tree), used as the checker of the tree tests:

  (a) `ref_tree`: direct.  The cache is gathered (paged or contiguous), the new K / V are appended at slots L + t with
      `oracle.kvcache.apply_rope` at the DEPTH positions L + leftpad + depth[t] (e4m3 rounding for fp8 caches), scores are
      built with the explicit visibility matrix - the committed cache for every row, new key c for row t iff mask[t, c] -
      then softcap, then softmax.  Covers arbitrary masks, rows without a visible key included.
  (b) `ref_tree_chains`: the ancestor-chain identity on the existing, reference-pinned oracle.  For node t the visible new
      keys are collected in index order and `oracle.kvcache.kvcache_fwd(causal=True)` runs on a fresh copy of the cache
      with that chain as the new tokens, t last; row t of the tree result is the last row of that call.  Holds for masks
      in which every node sees itself and whose visible sets are ancestor-closed (trees from parent arrays with
      parent[t] < t): the chain's position i is then depth of its i-th node.

Both mutate nothing: they work on copies and return the appended caches next to out / LSE.
"""
import numpy as np

from oracle.attention import round_to
from oracle.kvcache import apply_rope, kvcache_fwd, round_e4m3


# ---- trees ---------------------------------------------------------------------------------------------------------
def random_parents(T, rng, chain_bias=0.3):
    """parent[t] < t (-1: a root, child of the committed context); node 0 is a root"""
    par = np.full(T, -1, dtype=np.int64)
    for t in range(1, T):
        par[t] = t - 1 if rng.random() < chain_bias else int(rng.integers(-1, t))
    return par


def mask_from_parents(par):
    """bool [T, T]: row t sees itself and its ancestors"""
    T = len(par)
    m = np.zeros((T, T), dtype=bool)
    for t in range(T):
        c = t
        while c >= 0:
            m[t, c] = True
            c = par[c]
    return m


def depths_from_parents(par):
    T = len(par)
    d = np.zeros(T, dtype=np.int32)
    for t in range(T):
        d[t] = 0 if par[t] < 0 else d[par[t]] + 1
    return d


def pack_mask(mask):
    """bool [..., T, T] -> int32 [..., T, ceil(T / 32)]: bit c & 31 of word c >> 5 = column c"""
    mask = np.asarray(mask, dtype=bool)
    T = mask.shape[-1]
    W = (T + 31) // 32
    words = np.zeros(mask.shape[:-1] + (W,), dtype=np.uint32)
    for c in range(T):
        words[..., c >> 5] |= mask[..., c].astype(np.uint32) << np.uint32(c & 31)
    return words.view(np.int32)


def unpack_mask(words, T):
    w = np.asarray(words).view(np.uint32)
    cols = [(w[..., c >> 5] >> np.uint32(c & 31)) & np.uint32(1) for c in range(T)]
    return np.stack(cols, axis=-1).astype(bool)


# ---- (a) -----------------------------------------------------------------------------------------------------------
def _per_batch(x, b, nd):
    x = np.asarray(x)
    return x[b] if x.ndim == nd + 1 else x


def ref_tree(q, k_cache, v_cache, mask, k=None, v=None, depths=None, rotary_cos=None, rotary_sin=None,
             cache_seqlens=None, cache_batch_idx=None, cache_leftpad=None, block_table=None, scale=None, softcap=0.0,
             rotary_interleaved=True, io_dtype="fp16", k_descale=None, v_descale=None, sinks=None):
    """q [B, T, Hq, D]; caches as in oracle.kvcache.kvcache_fwd (fp64 arrays of the stored values); mask bool [B, T, T] or
    [T, T]; depths int [B, T] or [T] (needed with rotary).  Returns out [B, T, Hq, D], LSE [B, Hq, T] (fp64; with sinks
    [Hq] the sink-inclusive one) and the caches after the append."""
    q = np.asarray(q, dtype=np.float64)
    kc = np.array(k_cache, dtype=np.float64, copy=True)
    vc = np.array(v_cache, dtype=np.float64, copy=True)
    B, T, Hq, D = q.shape
    Hk = kc.shape[2]
    G = Hq // Hk
    paged = block_table is not None
    page = kc.shape[1]
    scale = D ** -0.5 if scale is None else scale
    t_new = 0 if k is None else k.shape[1]
    assert t_new in (0, T)
    kd = 1.0 if k_descale is None else float(k_descale)
    vd = 1.0 if v_descale is None else float(v_descale)
    out = np.zeros((B, T, Hq, D))
    lse = np.full((B, Hq, T), -np.inf)

    def slot(b, pos):
        if paged:
            return int(np.asarray(block_table)[b, pos // page]), pos % page
        return (int(cache_batch_idx[b]) if cache_batch_idx is not None else b), pos

    for b in range(B):
        lp = int(cache_leftpad[b]) if cache_leftpad is not None else 0
        L = int(cache_seqlens[b]) if cache_seqlens is not None else 0
        mb = _per_batch(mask, b, 2)
        db = None if depths is None else _per_batch(depths, b, 1)
        for r in range(t_new):
            i0, i1 = slot(b, L + lp + r)                               # the SLOT is L + r ...
            kr = np.asarray(k[b, r], dtype=np.float64)
            if rotary_cos is not None:                                 # ... the POSITION L + depth[r]
                kr = apply_rope(kr, rotary_cos, rotary_sin, L + lp + int(db[r]), rotary_interleaved, io_dtype)
            vr = np.asarray(v[b, r], dtype=np.float64)
            kc[i0, i1] = round_e4m3(kr / kd) if k_descale is not None else kr
            vc[i0, i1] = round_e4m3(vr / vd) if v_descale is not None else vr
        sk = L + t_new
        off = sk - T
        idx = [slot(b, lp + j) for j in range(sk)]
        i0 = np.array([a for a, _ in idx], dtype=np.int64)
        i1 = np.array([c for _, c in idx], dtype=np.int64)
        kk = kc[i0, i1] * kd if sk else np.zeros((0, Hk, D))
        vv = vc[i0, i1] * vd if sk else np.zeros((0, Hk, D))
        vis = np.ones((T, sk), dtype=bool)
        for j in range(sk):
            if j >= off:
                vis[:, j] = mb[:, j - off]
        for h in range(Hq):
            g = h // G
            qq = q[b, :, h].copy()
            if rotary_cos is not None:
                for t in range(T):
                    qq[t] = apply_rope(qq[t], rotary_cos, rotary_sin, L + lp + int(db[t]), rotary_interleaved, io_dtype)
            s = (qq @ kk[:, g].T) * scale
            if softcap and softcap > 0.0:
                s = softcap * np.tanh(s / softcap)
            s = np.where(vis, s, -np.inf)
            sh = -np.inf if sinks is None else float(sinks[h])
            m = np.maximum(s.max(axis=1) if sk else np.full(T, -np.inf), sh)
            m_safe = np.where(np.isfinite(m), m, 0.0)
            e = np.where(vis, np.exp(s - m_safe[:, None]), 0.0)
            l = e.sum(axis=1) + (np.exp(sh - m_safe) if np.isfinite(sh) else 0.0)
            has = l > 0
            p = np.where(has[:, None], e / np.where(has, l, 1.0)[:, None], 0.0)
            out[b, :, h] = p @ vv[:, g]
            lse[b, h] = np.where(has, m_safe + np.log(np.where(has, l, 1.0)), -np.inf)
    return out, lse, kc, vc


# ---- (b) -----------------------------------------------------------------------------------------------------------
def ref_tree_chains(q, k_cache, v_cache, mask, k, v, rotary_cos=None, rotary_sin=None, cache_seqlens=None,
                    cache_batch_idx=None, cache_leftpad=None, block_table=None, scale=None, softcap=0.0,
                    rotary_interleaved=True, io_dtype="fp16", k_descale=None, v_descale=None):
    """(b): one causal oracle call per (batch entry, node) on a fresh copy of the cache.  Needs the new K / V (k, v) and a
    mask whose rows contain the diagonal and are ancestor-closed.  Returns out [B, T, Hq, D] fp64, LSE [B, Hq, T] (the
    oracle's fp32 values)."""
    q = np.asarray(q, dtype=np.float64)
    B, T, Hq, D = q.shape
    out = np.zeros((B, T, Hq, D))
    lse = np.zeros((B, Hq, T))
    sl = lambda x, b: None if x is None else np.asarray(x)[b:b + 1]
    # (the one-sequence call is batch entry 0 of the oracle: name the cache row of entry b)
    bidx = lambda b: None if block_table is not None else np.array([b if cache_batch_idx is None else cache_batch_idx[b]])
    for b in range(B):
        mb = _per_batch(mask, b, 2)
        for t in range(T):
            chain = [c for c in range(T) if mb[t, c]]
            assert chain and chain[-1] == t, "identity (b): every node sees itself, and nothing after itself"
            kc = np.array(k_cache, dtype=np.float64, copy=True)
            vc = np.array(v_cache, dtype=np.float64, copy=True)
            o, l = kvcache_fwd(q[b:b + 1, chain], kc, vc, k=np.asarray(k)[b:b + 1, chain], v=np.asarray(v)[b:b + 1, chain],
                               rotary_cos=rotary_cos, rotary_sin=rotary_sin, cache_seqlens=sl(cache_seqlens, b),
                               cache_batch_idx=bidx(b), cache_leftpad=sl(cache_leftpad, b),
                               block_table=sl(block_table, b), scale=scale, causal=True, softcap=softcap,
                               rotary_interleaved=rotary_interleaved, io_dtype=io_dtype, k_descale=k_descale,
                               v_descale=v_descale)
            out[b, t] = o[0, -1]
            lse[b, :, t] = l[0, :, -1]
    return out, lse


__all__ = ["random_parents", "mask_from_parents", "depths_from_parents", "pack_mask", "unpack_mask", "ref_tree",
           "ref_tree_chains", "round_to"]
