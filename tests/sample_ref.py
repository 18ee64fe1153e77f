"""The fp64 yardstick of fa_sample (include/fa_mi355.h: the rules 1 - 6) and the builder of DECISIVE inputs for its tests.

The rules, per row: v_j = float(logits_j) with a NaN read as -inf; the order "larger value, then lower index"; x_j = v_j / T;
e_j = exp(x_j - x_j*); the integer mass q_j = floor(e_j 2^40); top_k, min_p and top_p each keep a prefix of the order; the draw
is an inverse CDF over the kept masses in INDEX order.  Everything behind the q_j is integer arithmetic, here on numpy uint64
(sums of 2^20 masses of at most 2^40 fit) and Python ints - exact.

So device and reference can differ only in the bits of e_j: the device rounds 1 / T, x_j = v_j (1 / T), x_j - m and the product
with log2(e) to fp32 and takes the hardware's exp2.  With a = the relative error of 1 / T and b the one of a product, x' - m' =
(x - m)(1 + a) + x b_j - m b_m, then one rounding of the difference and one of the product with (a rounded) log2(e); the error of
the exponent is the relative error of the mass:

    mass_rel_bound(x, m) = 2^-24 (2 |x| + 2 |x - m|) + 2^-23          (the last term: exp2 to one ulp)

below 2^-15 for |v / T| <= 64, which `build` asserts.  The floor adds at most one unit of 2^-40 per token: 2^-20 of the mass of
j* for a whole row of 2^20 tokens - counted in DELTA's slack.  No row is ever left out of a test: `build` chooses min_p, top_p
and u such that every decision has a margin DELTA = 2^-13 = 4 x 2^-15 in normalised mass:

    min_p   the geometric midpoint of two adjacent distinct masses whose log gap exceeds 4 DELTA
    top_p   the midpoint of the cumulative interval (in the order, over the mass that min_p and top_k leave) of a token whose
            normalised mass exceeds 4 DELTA
    u       the midpoint of the index-order interval of a kept token whose normalised mass exceeds 4 DELTA

top_k needs no margin (it counts keys).  `emulate=True` computes e_j with the device's fp32 roundings and a correctly rounded
exp2 instead: the CPU tests hold the reference against it on decisive inputs."""
import hashlib
import math

import numpy as np
import torch

DELTA = 2.0 ** -13
MASS_BOUND = 2.0 ** -15
SCALE = float(2 ** 40)
LOG2E32 = np.float32(1.4426950408889634)
THREADS = 1024                                               # csrc/fa_sample.hip: lanes per row
STEP = 8 * THREADS                                           # columns the workgroup takes per sweep step


CHUNK = 16384                                                # csrc/fa_sample.hip: columns per workgroup of the split plan
SPLIT_MIN = 2 * CHUNK                                        # the split plan serves V >= SPLIT_MIN, one workgroup per row below


def chunks(V):
    """workgroups per row"""
    return -(-V // CHUNK) if V >= SPLIT_MIN else 1


def iters(V):
    """csrc/fa_sample.hip: the trip count of every sweep, a function of V alone"""
    return CHUNK // 8 // THREADS if V >= SPLIT_MIN else -(-(-(-V // 8)) // THREADS)


def wave_run(V):
    """the columns a wave owns: run g of the row has [g * wave_run, (g + 1) * wave_run)"""
    return iters(V) * 64 * 8


def workspace_bytes(rows, V):
    """fa_sample_workspace_bytes: per row a 256-byte record, the masses' sums, 256 bins of counts (u32) and masses (u64), a
    32-byte partial per chunk and a u64 total per run, rounded up to 256 bytes; nothing for one workgroup per row"""
    if V < SPLIT_MIN or rows <= 0:
        return 0
    C = chunks(V)
    return rows * ((3392 + 32 * C + 8 * 16 * C + 255) // 256 * 256)


def f32(x):
    return float(np.float32(x))


def values(row):
    """a row of logits (a 1-D tensor of any of the three dtypes) as the fp64 values of the rules: NaN -> -inf, -0 -> +0"""
    v = row.detach().cpu().double().numpy().copy()
    v[np.isnan(v)] = -np.inf
    return v + 0.0


def order(v):
    """the token indices in the order: larger value first, then lower index"""
    return _memo("order", v, None, lambda: np.lexsort((np.arange(v.size), -v)))


def mass_rel_bound(x, m):
    return 2.0 ** -24 * (2.0 * np.abs(x) + 2.0 * np.abs(x - m)) + 2.0 ** -23


_MEMO = {}


def _memo(kind, v, extra, make):
    """the last few (order / masses) results, keyed by the row's bytes: the tests run many parameter sets over one row.  What is
    returned is shared - never written to"""
    key = (kind, hashlib.blake2b(v.tobytes(), digest_size=16).digest(), extra)
    if key not in _MEMO:
        if len(_MEMO) >= 16:
            _MEMO.clear()
        _MEMO[key] = make()
    return _MEMO[key]


def masses(v, T, emulate=False):
    """(e fp64 array, q uint64 array, lse) of a sampled row (T > 0, a finite maximum).  emulate: the device's fp32 roundings"""
    return _memo("masses", v, (float(T), emulate), lambda: _masses(v, T, emulate))


def _masses(v, T, emulate):
    jstar = int(order(v)[0])
    with np.errstate(over="ignore", invalid="ignore"):
        if emulate:
            inv_t = np.float32(1.0) / np.float32(T)
            x = (v.astype(np.float32) * inv_t).astype(np.float32)
            t = (x - x[jstar]).astype(np.float32)
            e = np.exp2((t * LOG2E32).astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
        else:
            x = v * (1.0 / f32(T))
            e = np.exp(x - x[jstar])
        x = x.astype(np.float64)
        e[np.isneginf(v)] = 0.0
        q = np.floor(e * SCALE).astype(np.uint64)
        fin = np.isfinite(x)
        lse = float(x[jstar] + math.log(float(np.exp(x[fin] - x[jstar]).sum())))
    return e, q, lse


def plain_lse(v):
    """lse at inv_t = 1 (greedy rows): -inf for an empty row, NaN for a row that holds +inf"""
    if not (v > -np.inf).any():
        return -math.inf
    if np.isposinf(v).any():
        return math.nan
    m = v.max()
    return float(m + math.log(float(np.exp(v[np.isfinite(v)] - m).sum())))


def row_ref(row, T, k=0, top_p=1.0, min_p=0.0, u=0.0, emulate=False):
    """The rules on one row: dict(id, n_kept, kept (bool [V]), lse, sampled)"""
    v = values(row)
    V = v.size
    T, top_p, min_p, u, k = f32(T), f32(top_p), f32(min_p), f32(u), int(k)
    kept = np.zeros(V, dtype=bool)
    n0 = int((v > -np.inf).sum())
    if n0 == 0:
        return dict(id=-1, n_kept=0, kept=kept, lse=-math.inf, sampled=False)
    o = order(v)
    with np.errstate(over="ignore", divide="ignore"):
        overflow = T > 0 and np.isfinite(v[o[0]]) and not np.isfinite(np.float32(v[o[0]]) * (np.float32(1.0) / np.float32(T)))
    if not (T > 0) or v[o[0]] == np.inf or overflow:                # (overflow: 1 / T takes x_j* out of fp32)
        kept[o[0]] = True
        return dict(id=int(o[0]), n_kept=1, kept=kept, lse=None if overflow else plain_lse(v), sampled=False)   # (None: not specified)
    e, q, lse = masses(v, T, emulate)
    es, qs = e[o], q[o]
    n = k if 1 <= k < n0 else n0
    if min_p > 0:
        n = int((es[:n] >= min(min_p, 1.0)).sum())
    if top_p < 1:
        Q2 = int(qs[:n].sum())
        Tq = max(1, math.ceil(top_p * float(Q2)))
        n = int(np.searchsorted(np.cumsum(qs[:n]), np.uint64(Tq), side="left")) + 1
    kept[o[:n]] = True
    idx = np.flatnonzero(kept)
    cq = np.cumsum(q[idx])
    Q = int(cq[-1])
    uu = u if u > 0 else 0.0
    d = math.floor(uu * float(Q)) if uu * float(Q) < 2.0 ** 64 else Q
    rr = min(d, Q - 1)
    tok = int(idx[int(np.searchsorted(cq, np.uint64(rr), side="right"))])
    return dict(id=tok, n_kept=n, kept=kept, lse=lse, sampled=True)


def filtered_ref(row, kept):
    """the logit's own bits where kept, -inf elsewhere"""
    out = torch.full_like(row, float("-inf"))
    m = torch.from_numpy(kept).to(row.device)
    out[m] = row[m]
    return out


def lse_bound(row, T, lse):
    """|device lse - reference lse|: the masses' bound on s, the fp32 roundings of m = v_j* (1 / T) (two) and of m + log(s), the
    library logf to 2 ulp, and the fixed-order sum of s: 8 columns, iters pieces, 6 butterfly steps, 16 waves, the chunks - each
    one rounding of a partial sum that is at most s"""
    v = values(row)
    m = abs(float(v.max()) / f32(T)) if T > 0 else abs(float(v.max()))
    adds = 8 + iters(v.size) + 6 + 16 + chunks(v.size)
    return MASS_BOUND + adds * 2.0 ** -24 + (m + abs(lse) + 1.0) * 2.0 ** -22


def build(row, T, k=0, *, want_min_p=False, want_top_p=False, seed=0, cut_index=None, draw_index=None):
    """min_p, top_p and u (fp32 values; 0.0 / 1.0 where not wanted) that make every decision on this row clear by DELTA, and what
    they decide: dict(min_p, top_p, u, id, n_kept, margins).  cut_index: the token that top_p's cut falls on; draw_index: the
    token that is drawn - both must carry more than 4 DELTA of the mass they are measured in (an AssertionError otherwise: no case
    is ever skipped)"""
    rng = np.random.default_rng(seed)
    v = values(row)
    T = f32(T)
    assert T > 0 and np.isfinite(v.max())
    fin = np.isfinite(v)
    x = v[fin] / T
    assert np.abs(x).max() <= 64.0, "the builder's range: |v / T| <= 64"
    assert mass_rel_bound(x, x.max()).max() < MASS_BOUND
    e, q, _ = masses(v, T)
    o = order(v)
    n0 = int(fin.sum())
    n = k if 1 <= k < n0 else n0
    margins = {}
    min_p = 0.0
    if want_min_p:
        es = e[o[:n]]
        with np.errstate(divide="ignore"):
            gap = np.log(es[:-1]) - np.log(es[1:])
        cand = np.flatnonzero((gap > 4 * DELTA) & (es[1:] > 0))
        assert cand.size, "no two adjacent masses with a log gap above 4 DELTA"
        i = int(cand[rng.integers(cand.size)]) + 1              # the first token that min_p drops
        min_p = f32(math.sqrt(es[i - 1] * es[i]))
        assert 0 < min_p <= 1 and es[i - 1] / min_p > 1 + 1.5 * DELTA and min_p / es[i] > 1 + 1.5 * DELTA
        margins["min_p"] = min(math.log(es[i - 1] / min_p), math.log(min_p / es[i]))
        n = i
    top_p = 1.0
    if want_top_p:
        qs = q[o[:n]].astype(np.float64)
        norm = qs / qs.sum()
        if cut_index is None:
            cand = np.flatnonzero(norm > 4 * DELTA)
            pos = int(cand[rng.integers(cand.size)])
        else:
            pos = int(np.flatnonzero(o[:n] == cut_index)[0])
            assert norm[pos] > 4 * DELTA, "the planted cut token carries too little mass"
        c = np.cumsum(norm)
        top_p = f32(c[pos] - norm[pos] / 2)
        assert 0 < top_p < 1
        margins["top_p"] = min(top_p - (c[pos] - norm[pos]), c[pos] - top_p)
        assert margins["top_p"] > 1.5 * DELTA
        n = pos + 1
    idx = np.sort(o[:n])
    qk = q[idx].astype(np.float64)
    norm = qk / qk.sum()
    if draw_index is None:
        cand = np.flatnonzero(norm > 4 * DELTA)
        pos = int(cand[rng.integers(cand.size)])
    else:
        pos = int(np.flatnonzero(idx == draw_index)[0])
        assert norm[pos] > 4 * DELTA, "the planted draw token carries too little mass"
    c = np.cumsum(norm)
    u = f32(c[pos] - norm[pos] / 2)
    assert 0 < u < 1
    margins["u"] = min(u - (c[pos] - norm[pos]), c[pos] - u)
    assert margins["u"] > 1.5 * DELTA
    return dict(min_p=min_p, top_p=top_p, u=u, id=int(idx[pos]), n_kept=n, margins=margins)


def randn_row(V, dtype, seed, spread=3.0, plant=(), lift=4.0):
    """a seeded randn row times `spread`, rounded to dtype; plant: indices that get the values max + lift - n / 8 (distinct in
    every dtype below 32), so that each of them carries more than 4 DELTA of the row's mass at T = 1"""
    g = torch.Generator().manual_seed(seed)
    row = (torch.randn(V, generator=g, dtype=torch.float32) * spread)
    top = float(row.max())
    for n, i in enumerate(plant):
        row[i] = top + lift - 0.125 * n
    return row.to(dtype)
