"""The fp64 yardstick of fa_spec_accept / fa_spec_walk (include/fa_mi355.h) and the builder of DECISIVE uniform numbers for their
tests.  It reuses sample_ref's values / order / masses: the target row's v_j, the order, j* and the masses e_j ARE fa_sample's.

The rules, per node with target row v, draft row q (as it is) and draft token d:
    empty row: (accept, recovered) = (0, -1);   greedy row (!(T > 0), v_j* = +inf, x_j* not finite): (d == j*, j*)
    p_j = e_j / s,  s = sum e_j;   accept = (uu q_d < p_d), d outside [0, V): 0
    r_j = min(max(p_j - q_j, 0), 1) (a NaN: 0),  R_j = floor(r_j 2^40),  R = sum R_j;   R == 0: R_j = floor(e_j 2^40)
    rr = min(floor(uu_r R), R - 1);   recovered = the smallest index whose index-order running sum of R_j exceeds rr
Behind the R_j everything is integer arithmetic (numpy uint64 and Python ints: exact), so device and reference can differ only in
the bits of p_j, of r_j and of the product uu q_d.

The margin.  sample_ref.mass_rel_bound: the device's e_j is within 2^-15 relative for |v / T| <= 64.  The device's s is a fixed-
order fp32 sum of those e_j: the same 2^-15 from its terms plus one rounding per addition on a path from a term to the total - 8
columns, 2 pieces, 6 butterfly steps, 16 waves, at most 64 chunks, each with a merge product: < 200 roundings of 2^-24 < 2^-16.
1.0f / s is one correctly rounded division (2^-24) and p_j = e_j * (1 / s) one product (2^-24).  Together
    |p_j' / p_j - 1|  <=  2^-15 + 2^-15 + 2^-16 + 2^-23  <  2^-13 = DELTA_P
The subtraction p_j - q_j is one rounding of the difference: relative 2^-24 of r_j, far inside the slack of the line above.  So
sum_j |r_j' - r_j| <= DELTA_P sum_j p_j = DELTA_P, the floor adds at most 2^-40 per token, and with tau = sum r_j (the total-
variation distance) both the numerator and the denominator of a normalised running residual mass move by at most DELTA_P +
V 2^-40: a threshold in normalised residual mass moves by at most
    margin_r(V, tau) = 2 (DELTA_P + V 2^-40) / tau
(the issue's count gives (2 DELTA_P + V 2^-40) / tau; this one carries the floor term in both places and is the larger).  The
rounding of floor(uu_r R) is one unit of R >= tau 2^40: nothing.  `build` places u_recover at the midpoint of the interval of a
token whose normalised residual mass exceeds 4 margins and asserts 1.5 margins on both sides; the test rows have tau >= 1/4, so
a margin is at most 2^-10 + V 2^-37.  Where R == 0 the draw is fa_sample's over the e_j: sample_ref.DELTA, and the branch itself
is decisive only where every q_j >= 1 >= p_j, which `build` asserts.  The accept test compares uu q_d (one product: 2^-24) with
p_d (DELTA_P): `build` puts uu q_d a factor 2 away from p_d where it can and asserts a factor 1 + 8 DELTA_P in every case.

`emulate=True` computes p_j, r_j and uu q_d with the device's fp32 roundings (s as numpy's pairwise fp32 sum - another order than
the device's, inside the same bound): the CPU tests hold the reference against it on every case the GPU tests run."""
import math

import numpy as np
import torch

import sample_ref as R

DELTA_P = 2.0 ** -13
SCALE = R.SCALE
CHUNK = 16384                                                # csrc/fa_spec_verify.hip: columns per workgroup
NODES_MAX = 64


def chunks(V):
    return -(-V // CHUNK)


def workspace_bytes(rows, V):
    """fa_spec_accept_workspace_bytes: per node a 32-byte partial and two u64 sums per chunk, rounded up to 64 bytes"""
    return 0 if rows <= 0 else rows * ((48 * chunks(V) + 63) // 64 * 64)


def margin_r(V, tau):
    return 2.0 * (DELTA_P + V * 2.0 ** -40) / tau


def _state(trow, T):
    """('empty' | 'greedy' | 'sampled', v, j*)"""
    v = R.values(trow)
    if not (v > -np.inf).any():
        return "empty", v, -1
    o = R.order(v)
    T = R.f32(T)
    with np.errstate(over="ignore", divide="ignore"):
        overflow = T > 0 and np.isfinite(v[o[0]]) and not np.isfinite(np.float32(v[o[0]]) * (np.float32(1.0) / np.float32(T)))
    if not (T > 0) or v[o[0]] == np.inf or overflow:
        return "greedy", v, int(o[0])
    return "sampled", v, int(o[0])


def probs(v, T, emulate=False):
    """(p, e-masses q uint64) of a sampled target row; emulate: fp32 e_j, s, 1 / s and product"""
    e, qm, _ = R.masses(v, R.f32(T), emulate)
    if emulate:
        e32 = e.astype(np.float32)
        inv_s = np.float32(1.0) / e32.sum(dtype=np.float32)
        return (e32 * inv_s).astype(np.float32).astype(np.float64), qm
    return e / e.sum(), qm


def residual(p, q, emulate=False):
    """(r fp64 array, R_j uint64 array)"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = (p.astype(np.float32) - q.astype(np.float32)).astype(np.float64) if emulate else p - q
    r = np.where(r > 0, r, 0.0)                              # (a NaN: 0)
    r = np.minimum(r, 1.0)
    return r, np.floor(r * SCALE).astype(np.uint64)


def _draft(qrow):
    return qrow.detach().cpu().double().numpy()


def _uu(u):
    u = R.f32(u)
    return u if u > 0 else 0.0


def accept_ref(trow, qrow, d, T, u_accept, u_recover, emulate=False):
    """The rules on one node: (accept, recovered)"""
    kind, v, jstar = _state(trow, T)
    d = int(d)
    if kind == "empty":
        return 0, -1
    if kind == "greedy":
        return int(d == jstar), jstar
    q = _draft(qrow)
    p, qm = probs(v, T, emulate)
    acc = 0
    if 0 <= d < v.size:
        lhs = _uu(u_accept) * q[d]
        if emulate:
            with np.errstate(over="ignore", invalid="ignore"):
                lhs = float(np.float32(_uu(u_accept)) * np.float32(q[d]))
        acc = int(lhs < p[d])
    _, Rj = residual(p, q, emulate)
    Rt = int(Rj.sum())
    if Rt == 0:
        Rj, Rt = qm, int(qm.sum())
    x = _uu(u_recover) * float(Rt)
    rr = min(math.floor(x) if x < 2.0 ** 64 else Rt, Rt - 1)
    rec = int(np.searchsorted(np.cumsum(Rj), np.uint64(rr), side="right"))
    return acc, rec


def build(trow, qrow, d, T, *, want_accept, recover_index=None, seed=0):
    """u_accept and u_recover (fp32 values) for which both decisions of this node are clear of the device's rounding, and what
    they decide: dict(u_accept, u_recover, accept, recovered, tau, margins).  want_accept: the side of p_d / q_d that u_accept is
    put on; recover_index: the token that is recovered - it must carry more than 4 margins of normalised residual mass.  An
    AssertionError where a case cannot be made decisive: no case is ever skipped."""
    rng = np.random.default_rng(seed)
    kind, v, _ = _state(trow, T)
    assert kind == "sampled"
    V = v.size
    x = v[np.isfinite(v)] / R.f32(T)
    assert np.abs(x).max() <= 64.0, "the builder's range: |v / T| <= 64"
    assert R.mass_rel_bound(x, x.max()).max() < R.MASS_BOUND
    q = _draft(qrow)
    p, qm = probs(v, T)
    d = int(d)
    margins = {}
    # ---- the accept test
    slack = 1.0 + 8.0 * DELTA_P
    if not (0 <= d < V):
        assert not want_accept
        u_accept = 0.5
    elif want_accept:
        assert p[d] > 0 and q[d] >= 0
        u_accept = 0.5 if q[d] == 0 else R.f32(min(p[d] / q[d], 1.0) * 0.5)
        assert u_accept * q[d] * slack < p[d]
        margins["accept"] = math.inf if q[d] == 0 else p[d] / (u_accept * q[d])
    else:
        if p[d] == 0:
            u_accept = 0.5
            margins["accept"] = math.inf
        else:
            ratio = p[d] / q[d]
            assert q[d] > 0 and ratio * slack * slack < 1.0, "no u in [0, 1) rejects this token decisively"
            u_accept = R.f32(min(2.0 * ratio, (1.0 + ratio) / 2.0))
            assert u_accept < 1.0 and u_accept * q[d] > p[d] * slack
            margins["accept"] = u_accept * q[d] / p[d]
    # ---- the recovered token
    r, Rj = residual(p, q)
    tau = float(r.sum())
    if int(Rj.sum()) == 0:
        assert (q >= 1.0).all(), "R == 0 is decisive only where q covers every p_j <= 1"
        w, m = qm.astype(np.float64), R.DELTA
    else:
        assert tau >= 0.25, f"the test rows are built with tau >= 1/4, got {tau}"
        w, m = r, margin_r(V, tau)
    norm = w / w.sum()
    if recover_index is None:
        cand = np.flatnonzero(norm > 4 * m)
        pos = int(cand[rng.integers(cand.size)])
    else:
        pos = int(recover_index)
        assert norm[pos] > 4 * m, f"the planted recovered token carries {norm[pos]} of the residual mass, 4 margins are {4 * m}"
    c = np.cumsum(norm)
    u_recover = R.f32(c[pos] - norm[pos] / 2)
    assert 0 < u_recover < 1
    margins["recover"] = min(u_recover - (c[pos] - norm[pos]), c[pos] - u_recover) / m
    assert margins["recover"] > 1.5
    return dict(u_accept=u_accept, u_recover=u_recover, accept=int(want_accept), recovered=pos, tau=tau, margins=margins)


# ---- the constructed rows ------------------------------------------------------------------------------------------------
def plants(V):
    """index 0, V - 1 and both sides of every chunk boundary"""
    return sorted({0, V - 1} | {c for w in range(1, chunks(V)) for c in (w * CHUNK - 1, w * CHUNK)})


def target_row(V, dtype, seed):
    """a seeded randn row (spread 2) with every plant lifted so that it carries mass at T = 1"""
    return R.randn_row(V, dtype, seed, spread=2.0, plant=plants(V), lift=6.0)


def draft_row(trow, T, qdtype, rec, d, want_accept):
    """a draft row for the target row: q_j = p_j everywhere (residual ~ 0) except on the plants - every second plant, and `rec`,
    gets q = 0 (its residual is its p_j: tau >= 1/4), the others q = 2 p_j (residual 0) -, and q_d = p_d / 2 (accept) or 2 p_d
    (reject); rounded to qdtype"""
    v = R.values(trow)
    p, _ = probs(v, T)
    q = p.copy()
    pl = plants(v.size)
    for n, j in enumerate(pl):
        q[j] = 0.0 if (n % 2 == 0 or j == rec) else 2.0 * p[j]
    if rec is not None:
        q[rec] = 0.0
    if 0 <= d < v.size and d != rec:
        q[d] = p[d] / 2 if want_accept else 2.0 * p[d]
    return torch.from_numpy(q).to(qdtype)


# ---- the walk ------------------------------------------------------------------------------------------------------------
def valid_parent(par, t):
    return t >= 1 and 0 <= int(par[t]) < t


def walk_ref(parents, draft_ids, target_ids, accept=None, recovered=None):
    """one request: (out_tokens [T], num_out, path_nodes [T]) - lists padded with -1.  parents None: the chain; target_ids: a list
    of T ids, or one number that serves every node"""
    T = len(draft_ids)
    par = list(range(-1, T - 1)) if parents is None else [int(x) for x in parents]
    tid = (lambda c: int(target_ids[c])) if hasattr(target_ids, "__len__") else (lambda c: int(target_ids))
    kids = lambda c: [t for t in range(1, T) if valid_parent(par, t) and par[t] == c]   # noqa: E731
    out, path, c = [], [0], 0
    while True:
        if accept is None:
            y = tid(c)
            out.append(y)
            nxt = [t for t in kids(c) if int(draft_ids[t]) == y] if y != -1 else []
            if not nxt:
                break
            c = nxt[0]
        else:
            k = kids(c)
            if not k:
                out.append(tid(c))
                break
            t = k[0]
            if int(accept[t]) != 0:
                out.append(int(draft_ids[t]))
                c = t
            else:
                out.append(int(recovered[t]))
                break
        path.append(c)
    n = len(out)
    assert 1 <= n <= T and len(path) <= T
    return out + [-1] * (T - n), n, path + [-1] * (T - len(path))


def commit_ref(path_nodes, cache_seqlens, *, block_table=None, page_block_size=None, cache_batch_idx=None, seqlen_cache=None):
    """commit_slots as a Python loop: (src, dst) lists of B T slots"""
    src, dst = [], []
    for b, path in enumerate(path_nodes):
        for i, t in enumerate(path):
            if t < 0:
                src.append(-1)
                dst.append(-1)
                continue
            L = int(cache_seqlens[b])
            pair = []
            for pos in (L + int(t), L + i):
                if block_table is not None:
                    pair.append(int(block_table[b][pos // page_block_size]) * page_block_size + pos % page_block_size)
                else:
                    row = b if cache_batch_idx is None else int(cache_batch_idx[b])
                    pair.append(row * seqlen_cache + pos)
            src.append(pair[0])
            dst.append(pair[1])
    return src, dst


# ---- the batches the GPU tests run (and the CPU tests check the margins of) -------------------------------------------------
ACCEPT_V = [1, 7, 8, 9, 264, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 32769, 49153, 151936]
_DT = [torch.bfloat16, torch.float16, torch.float32]


def dtype_pairs(V):
    """(logits dtype, draft_probs dtype): every pair at V = 264 and 16385, one pair in rotation elsewhere"""
    if V in (264, 16385):
        return [(a, b) for a in _DT for b in _DT]
    n = ACCEPT_V.index(V)
    return [(_DT[n % 3], _DT[(n // 3 + n) % 3])]


def tree_parents(T):
    """[3, T]: a chain, a star, and a binary tree whose last node is a padding node"""
    par = np.full((3, T), -1, dtype=np.int32)
    for t in range(1, T):
        par[0, t], par[1, t], par[2, t] = t - 1, 0, (t - 1) // 2
    if T > 1:
        par[2, T - 1] = -1
    return par


def batch_case(V, tdtype, qdtype):
    """B = 3 requests (T = 5 nodes, more where the plants need them: 1 + ceil((plants + 1) / 3)) over tree_parents, per-request
    temperatures 1 / 0.7 / 0.5.  Every child node gets its own draft row; the recovered token and the draft token walk through
    the plants (index 0, V - 1, both sides of every chunk boundary), accept and reject alternate.  Returns a dict of CPU tensors:
    target [B, T, V], draft [B, T, V] (row 0 and padding rows: NaN), draft_ids, parents, temperature, u_accept, u_recover and the
    reference's accept / recovered [B, T]."""
    pl = plants(V)
    N = len(pl)
    B, T = 3, max(5, 1 + -(-(N + 1) // 3))
    par = tree_parents(T)
    temps = [1.0, 0.7, 0.5]
    target = torch.stack([torch.stack([target_row(V, tdtype, 1000 * V % 99991 + 10 * b + t) for t in range(T)]) for b in range(B)])
    draft = torch.full((B, T, V), float("nan"), dtype=qdtype)
    ids = torch.full((B, T), -7, dtype=torch.int32)
    ua = torch.full((B, T), float("nan"), dtype=torch.float32)
    ur = torch.full((B, T), float("nan"), dtype=torch.float32)
    acc = torch.zeros((B, T), dtype=torch.int32)
    rec = torch.full((B, T), -1, dtype=torch.int32)
    n = 0
    for b in range(B):
        for t in range(1, T):
            if not valid_parent(par[b], t):
                continue
            trow = target[b, int(par[b, t])]
            r, want = pl[n % N], (n // N + n % N) % 2 == 0
            d = pl[(n + 1) % N]
            if N == 1:                                           # V = 1: accept with the residual draw, reject with the fallback draw
                r = 0 if want else None
            qrow = draft_row(trow, temps[b], qdtype, r, d, want)
            bd = build(trow, qrow, d, temps[b], want_accept=want, recover_index=0 if r is None else r, seed=n)
            draft[b, t], ids[b, t] = qrow, d
            ua[b, t], ur[b, t], acc[b, t], rec[b, t] = bd["u_accept"], bd["u_recover"], bd["accept"], bd["recovered"]
            n += 1
    assert n >= N
    return dict(target=target, draft=draft, draft_ids=ids, parents=torch.from_numpy(par), temperature=torch.tensor(temps),
                u_accept=ua, u_recover=ur, accept=acc, recovered=rec)
