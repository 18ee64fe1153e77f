"""Witness data: attention inputs on which ONE wrongly masked key changes a row's result by tens of per cent.

The 16-bit attention tests draw N(0, 1) inputs and gate on max error / max |ref| over the whole tensor.  There a key far
from the diagonal carries a probability of 1e-3, so a mask mistake confined to a few rows (a ragged last block, the
unpaired middle block, one part of a key split, a stale cache row) moves a bf16 gradient by less than its gate.  The data
of this module puts all of a row's probability on keys chosen at the mask's edges, with exact values, so that the same
gates (tests/util.py) become decisive.  Pure numpy / torch on the CPU; the GPU tests (tests/test_witness_gpu.py) feed it
to the kernels, tests/test_witness_cpu.py proves the design conditions and the sensitivity on the oracle.

Key code.  h = (D - 2) // 3; key j < h * h carries 1.0 in dims  j % h,  h + j // h  and  2 h + (j % h + j // h) % h.
Any two of the three digits fix the third, so two different keys agree in at most one digit.  Dims D - 2 and D - 1 stay
free for the poison.  All values (0, 1, U, 2 U, 8 U; U = 256) are exact in fp16 and bf16.

Pair rows (wrongful exclusion).  q_i = U (code(a_i) + code(b_i)): both targets score U (3 + m) scale (m = 0 / 1 shared
digits), any other key at most 2 U scale - 16 nats or more behind even at D 256 - so P = 1/2, 1/2 to 1e-6, O is
(V_a + V_b) / 2 and dS, dQ, dK, dV all need both targets seen.  One visible key: one target; none: q = 0.
Three ways to pick (a, b): `edges` (first and last visible key), `random` (seeded per batch and head), `tiles` (the
visible keys nearest a multiple of 32 / 64 / 128 / 256 and that multiple minus 1).

Decoy rows (wrongful inclusion).  q_i = U (code(dL_i) + code(dR_i)), the first invisible keys left and right of the
row's visible range: a leaked decoy scores 3 U against at most 2 U for every visible key and takes the row.

Poison (memory no query may see).  Such rows carry 1.0 in the free dims and V = 64 in every column; the queries that
must not see them carry 8 U in a free dim.  In varlen, sequence b's queries carry 8 U in dim D - 2 + b % 2 and its keys
1.0 in the other free dim, so each neighbouring sequence is poison to it.

v and dO are N(0, 1) and N(0, 1) / 8 rounded to bf16, values below 2^-14 flushed to zero: exact in both io types, so one
forward reference serves both.  On pair rows dO is (N(0, 1) / 8 + (V_a - V_b) / 16) / 128 (see aim()).
"""
import numpy as np
import torch

import oracle
import oracle.attention as _oa
from util import DT, LSE_ATOL, TOL_MAXREL, rand16

U = 256.0
POISON_Q = 8 * U
POISON_V = 64.0
GRAD_CAP = 65504.0 / 8                                            # every reference gradient stays below this
TILES = (32, 64, 128, 256)
VARIANTS = ("edges", "random", "tiles", "decoy")


def digits(D):
    return (D - 2) // 3


def capacity(D):
    return digits(D) ** 2


def code(j, D):
    """[len(j), D] fp64: the three-digit code of keys j (all < capacity(D)); j < 0 gives a zero row"""
    j = np.atleast_1d(np.asarray(j, dtype=np.int64))
    h = digits(D)
    assert (j < h * h).all(), f"key {int(j.max())} exceeds the code capacity {h * h} of head dim {D}"
    c = np.zeros((j.size, D))
    ok = np.nonzero(j >= 0)[0]
    x, y = j[ok] % h, j[ok] // h
    c[ok, x] = 1.0
    c[ok, h + y] = 1.0
    c[ok, 2 * h + (x + y) % h] = 1.0
    return c


def shared16(shape, seed, scale=1.0):
    """rand16 in bf16 with |x| < 2^-14 flushed to zero: exact in fp16 too.  fp64 numpy."""
    x = rand16(shape, "bf16", seed, scale=scale, device="cpu").to(torch.float64).numpy()
    return np.where(np.abs(x) < 2.0 ** -14, 0.0, x)


def snap16(x):
    """round fp64 to bf16 and flush |x| < 2^-14: exact in both io types"""
    x = torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()
    return np.where(np.abs(x) < 2.0 ** -14, 0.0, x)


def aim(do, v, a, b):
    """dO [sq, D] of one head's pair rows, every row made to count: dO_i = (N(0, 1) / 8 + (V_a - V_b) / 16) / 128.
    dP_a - dP_b = dO_i . (V_a - V_b) then has the same size, D / 1024, in EVERY row; with the N(0, 1) part alone a row
    has a small difference now and then, and a mistake in just that row would change dQ little (dQ_i is dS_ia
    (code(a) - code(b))).  The sign is the same in all rows, so dK and dV of a key that many rows aim at - key 0 under a
    causal mask, 5200 rows at S 1300 with four heads - are sums WITHOUT cancellation (alternating signs were tried: the
    16-bit rounding of dS then shows in dK at 1 - 3 x the gate, a property of the data, not of a kernel); the factor
    1 / 128 keeps those sums below GRAD_CAP."""
    two = (b >= 0)[:, None]
    return snap16(np.where(two, (do + (v[np.maximum(a, 0)] - v[np.maximum(b, 0)]) / 16) / 128, do))


def to_dev(x, dt, device="cuda"):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DT[dt]).to(device)


def lse_atol(lse_ref):
    """util.LSE_ATOL was calibrated on |LSE| of a few units; witness scores reach 4 U scale (128 at D 64, LSE up to
    about 140).  The gate grows with the fp32 ulp: x 2 in [64, 128), x 4 in [128, 256) - what the fp8 one-hot test uses."""
    fin = np.abs(lse_ref[np.isfinite(lse_ref)])
    top = float(fin.max()) if fin.size else 0.0
    return LSE_ATOL * max(1.0, 2.0 ** (np.floor(np.log2(max(top, 1.0))) - 5))


# ------------------------------------------------------------------------------------------------ masks and targets
def visible(sq, sk, causal, window, norm_q=None, norm_k=None, kvcache=False, alibi=False):
    """The oracle's mask [sq, sk], flags normalised as its entry points do (varlen: by the maximal lengths)"""
    c, wl, wr = oracle.normalize_flags(sq if norm_q is None else norm_q, sk if norm_k is None else norm_k, causal,
                                       window[0], window[1], alibi, kvcache=kvcache)
    return _oa.visible_mask(sq, sk, c, wl, wr)


def _range(vis):
    """first / last visible key per row (-1, -1 for none) and the count"""
    n = vis.sum(axis=1)
    lo = np.where(n > 0, vis.argmax(axis=1), -1)
    hi = np.where(n > 0, vis.shape[1] - 1 - vis[:, ::-1].argmax(axis=1), -1)
    return lo, hi, n


def pick_targets(vis, variant, rng=None, head=0):
    """(a, b) [sq] int64: the two targets of each pair row; b = -1 with one visible key, both -1 with none"""
    sq, sk = vis.shape
    lo, hi, n = _range(vis)
    a, b = lo.copy(), np.where(n > 1, hi, -1)
    if variant == "edges":
        return a, b
    for i in np.nonzero(n > 1)[0]:
        if variant == "random":
            ks = np.nonzero(vis[i])[0]
            a[i], b[i] = rng.choice(ks, size=2, replace=False)
        elif variant == "tiles":
            t = TILES[(i + head) % 4]
            m = (hi[i] // t) * t if (i // 4 + head) % 2 == 0 else (lo[i] // t + 1) * t
            x, y = np.clip(m, lo[i], hi[i]), np.clip(m - 1, lo[i], hi[i])
            if x != y and vis[i, x] and vis[i, y]:
                a[i], b[i] = x, y
        else:
            raise ValueError(variant)
    return a, b


def pick_decoys(vis):
    """(dL, dR) [sq]: the first invisible key left / right of each row's visible range (-1 where there is none).  A row
    without visible keys takes the key nearest its diagonal j = i + sk - sq on either side."""
    sq, sk = vis.shape
    lo, hi, n = _range(vis)
    diag = np.arange(sq) + (sk - sq)
    lo = np.where(n > 0, lo, np.clip(diag + 1, 0, sk))
    hi = np.where(n > 0, hi, np.clip(diag, -1, sk - 1))
    dl = np.where(lo - 1 >= 0, lo - 1, -1)
    dr = np.where(hi + 1 < sk, hi + 1, -1)
    return dl, dr


def query_rows(a, b, D):
    return U * (code(a, D) + code(np.where(b == a, -1, b), D))


def mutate_mask(vis, kind, rows, keys=None):
    """A copy of `vis` with one localised mistake in `rows` (a 32-row band or a single row):
       lose_first / lose_last  the row's first / last visible key goes
       lose                    key `keys[i]` goes (a tile-edge target)
       gain_left / gain_right  the first invisible key left / right of the visible range appears
    Rows where the mistake is impossible (no such key) stay as they are."""
    out = vis.copy()
    lo, hi, n = _range(vis)
    dl, dr = pick_decoys(vis)
    for i in np.atleast_1d(rows):
        j = {"lose_first": lo[i] if n[i] else -1, "lose_last": hi[i] if n[i] else -1,
             "lose": -1 if keys is None else keys[i], "gain_left": dl[i], "gain_right": dr[i]}[kind]
        if j >= 0:
            out[i, j] = kind.startswith("gain")
    return out


def _rows(valid):
    """(a 32-row band, a single row) among the rows where `valid`: the band around the middle valid row, cut to the
    valid rows, and the last valid row"""
    idx = np.nonzero(valid)[0]
    if not idx.size:
        return None, None
    r0 = (idx[idx.size // 2] // 32) * 32
    band = idx[(idx >= r0) & (idx < r0 + 32)]
    return band, idx[-1:]


def mistakes(vis, variant, a=None, b=None):
    """[(name, mask)]: every localised mistake that bites on this data.  Pair rows lose one of their two targets (the
    boundary keys for `edges`: lose_first / lose_last; the tile-edge or random targets otherwise), decoy rows gain the
    first invisible key on either side; each in one 32-row band and in one single row."""
    out = []
    if variant == "decoy":
        dl, dr = pick_decoys(vis)
        for kind, d in (("gain_left", dl), ("gain_right", dr)):
            for where, rows in zip(("band", "row"), _rows(d >= 0)):
                if rows is not None:
                    out.append((f"{kind}-{where}{rows[0]}", mutate_mask(vis, kind, rows)))
        return out
    pair = vis.sum(axis=1) >= 2
    for where, rows in zip(("band", "row"), _rows(pair)):
        if rows is None:
            continue
        if variant == "edges":
            out += [(f"{kind}-{where}{rows[0]}", mutate_mask(vis, kind, rows)) for kind in ("lose_first", "lose_last")]
        else:
            out += [(f"lose_{n}-{where}{rows[0]}", mutate_mask(vis, "lose", rows, keys=t)) for n, t in (("a", a), ("b", b))]
    return out


def leak_forward(q, k, v, vis, scale, rows=None, k_leak=None, v_leak=None):
    """One head's forward (q [sq, D], k / v [sk, D]) in which `rows` also see one row of memory they must not: a stale
    or unreferenced cache row, a key past seqused_k, a neighbouring sequence's key.  rows None: the clean forward."""
    if rows is not None:
        k, v = np.concatenate([k, k_leak[None]]), np.concatenate([v, v_leak[None]])
        col = np.zeros((vis.shape[0], 1), dtype=bool)
        col[rows] = True
        vis = np.concatenate([vis, col], axis=1)
    with patched_mask(vis):
        o, lse, _ = oracle.attn_fwd(q[None, None], k[None, None], v[None, None], scale, normalize=False)
    return o[0, 0], lse[0, 0]


class patched_mask:
    """Within the block the oracle's masks of shape `vis.shape` are replaced by `vis` (a mutate_mask result): the oracle
    itself computes what a kernel with that mistake would.  Run only the backward inside to put the mistake into its P."""
    def __init__(self, vis):
        self.vis = vis

    def __enter__(self):
        self.orig = _oa.visible_mask
        _oa.visible_mask = lambda sq, sk, *a: self.vis if (sq, sk) == self.vis.shape else self.orig(sq, sk, *a)

    def __exit__(self, *exc):
        _oa.visible_mask = self.orig


# ------------------------------------------------------------------------------------------------ dense
class Dense:
    """q [B, Hq, Sq, D], k / v [B, Hk, Sk, D], do (fp64, the oracle's layout), the mask and the targets [B, Hq, Sq]"""

    def __init__(self, sq, sk, D, hq, hk, causal, window, variant, B=1, seed=0, alibi=None):
        assert sk <= capacity(D), (sk, D, capacity(D))
        self.sq, self.sk, self.D, self.hq, self.hk, self.B = sq, sk, D, hq, hk, B
        self.causal, self.window, self.variant, self.alibi = causal, window, variant, alibi
        self.scale = D ** -0.5
        self.vis = visible(sq, sk, causal, window, alibi=alibi is not None)
        self.k = np.broadcast_to(code(np.arange(sk), D), (B, hk, sk, D)).copy()
        self.v = shared16((B, hk, sk, D), seed + 1)
        self.do = shared16((B, hq, sq, D), seed + 2, scale=0.125)
        self.q = np.zeros((B, hq, sq, D))
        self.a = np.full((B, hq, sq), -1)
        self.b = np.full((B, hq, sq), -1)
        for bi in range(B):
            for h in range(hq):
                if variant == "decoy":
                    a, b = pick_decoys(self.vis)
                else:
                    a, b = pick_targets(self.vis, variant, np.random.default_rng([seed, bi, h]), h)
                self.a[bi, h], self.b[bi, h] = a, b
                self.q[bi, h] = query_rows(a, b, D)
                if variant != "decoy":
                    self.do[bi, h] = aim(self.do[bi, h], self.v[bi, h // (hq // hk)], a, b)
        self.kw = dict(causal=causal, window=window, alibi_slopes=alibi)

    def forward(self):
        o, lse, _ = oracle.attn_fwd(self.q, self.k, self.v, self.scale, **self.kw)
        return o, lse

    def backward(self, o, lse, dt):
        g = oracle.attn_bwd(self.do, self.q, self.k, self.v, oracle.round_to(o, dt), lse.astype(np.float64), self.scale,
                            **self.kw)[:3]
        check_grad_cap(g)
        return g

    def pair_out(self, magnitude=False):
        """(V_a + V_b) / 2 (V_a with one target, 0 with none) [B, Hq, Sq, D] - pair variants only.
        magnitude: (|V_a| + |V_b|) / 2 instead, the scale of the operands where they cancel"""
        g = self.hq // self.hk
        o = np.zeros_like(self.q)
        for bi in range(self.B):
            for h in range(self.hq):
                a, b, v = self.a[bi, h], self.b[bi, h], self.v[bi, h // g]
                v = np.abs(v) if magnitude else v
                va, vb = np.where(a[:, None] >= 0, v[a], 0.0), v[b]
                o[bi, h] = np.where(b[:, None] >= 0, (va + vb) / 2, va)
        return o

    def design(self):
        """Integer score matrix check: (rows with two targets, rows among them where the tie or the one-unit margin fails)"""
        g = self.hq // self.hk
        pairs = bad = 0
        if self.variant == "decoy":
            return 0, 0
        for bi in range(self.B):
            for h in range(self.hq):
                s = np.rint(self.q[bi, h] @ self.k[bi, h // g].T / U).astype(np.int64)
                s = np.where(self.vis, s, -1)
                a, b = self.a[bi, h], self.b[bi, h]
                rows = np.nonzero(b >= 0)[0]
                pairs += rows.size
                sa, sb = s[rows, a[rows]], s[rows, b[rows]]
                s[rows, a[rows]] = -1
                s[rows, b[rows]] = -1
                bad += int(((sa != sb) | (sa < 3) | (s[rows].max(axis=1) > sa - 1)).sum())
                assert ((self.vis.sum(axis=1) >= 2) == (b >= 0)).all()
        return pairs, bad


def check_grad_cap(grads):
    for name, x in zip(("dq", "dk", "dv"), grads):
        top = float(np.abs(x).max(initial=0.0))
        assert top < GRAD_CAP, f"witness {name} reaches {top:.0f}: beyond 1/8 of the fp16 range"


# ------------------------------------------------------------------------------------------------ varlen
class Varlen:
    """Packed q [Tq, Hq, D], k / v [Tk, Hk, D] (or paged [nblk, page, Hk, D] with block_table), causal.  Each sequence
    is poison to its neighbours; keys past seqused_k, page tails and unreferenced pages are poison to everyone."""

    def __init__(self, lens_q, lens_k, D, hq, hk, variant, causal=True, seed=0, used=None, page=0):
        assert max(lens_k) <= capacity(D)
        self.lens_q, self.lens_k, self.D, self.hq, self.hk = list(lens_q), list(lens_k), D, hq, hk
        self.variant, self.causal, self.used, self.page = variant, causal, used, page
        self.scale = D ** -0.5
        self.cu_q = np.concatenate([[0], np.cumsum(lens_q)]).astype(np.int32)
        self.cu_k = np.concatenate([[0], np.cumsum(lens_k)]).astype(np.int32)
        self.mq, self.mk = max(lens_q), max(lens_k)
        tq, tk = int(self.cu_q[-1]), int(self.cu_k[-1])
        self.q = np.zeros((tq, hq, D))
        self.do = shared16((tq, hq, D), seed + 2, scale=0.125)
        k = np.zeros((tk, hk, D))
        v = shared16((tk, hk, D), seed + 1)
        self.vis, self.a, self.b = [], [], []
        for s, (lq, lk) in enumerate(zip(lens_q, lens_k)):
            q0, k0 = int(self.cu_q[s]), int(self.cu_k[s])
            eff = lk if used is None else (min(lk, used[s]) if used[s] > 0 else 0)
            vis = visible(lq, eff, causal, (-1, -1), norm_q=self.mq, norm_k=self.mk)
            self.vis.append(vis)
            k[k0:k0 + eff] = code(np.arange(eff), D)[:, None, :]
            if used is None:
                k[k0:k0 + lk, :, D - 2 + (s + 1) % 2] = 1.0
            else:
                k[k0 + eff:k0 + lk, :, D - 2:] = 1.0
                v[k0 + eff:k0 + lk] = POISON_V
            aa, bb = [], []
            for h in range(hq):
                if variant == "decoy":
                    a, b = pick_decoys(vis) if eff else (np.full(lq, -1), np.full(lq, -1))
                else:
                    a, b = pick_targets(vis, variant, np.random.default_rng([seed, s, h]), h) if eff else \
                        (np.full(lq, -1), np.full(lq, -1))
                aa.append(a), bb.append(b)
                self.q[q0:q0 + lq, h] = query_rows(a, b, D)
                if variant != "decoy" and eff:
                    self.do[q0:q0 + lq, h] = aim(self.do[q0:q0 + lq, h], v[k0:k0 + eff, h // (hq // hk)], a, b)
            self.a.append(aa), self.b.append(bb)
            if used is None:
                self.q[q0:q0 + lq, :, D - 2 + s % 2] = POISON_Q
            else:
                self.q[q0:q0 + lq, :, D - 2:] = POISON_Q
        self.block_table = None
        if page:
            per = [(l + page - 1) // page for l in lens_k]
            nblk = sum(per) + 3
            perm = np.random.default_rng(seed).permutation(nblk)
            self.block_table = np.zeros((len(lens_k), max(max(per), 1)), dtype=np.int32)
            kp, vp = np.zeros((nblk, page, hk, D)), np.full((nblk, page, hk, D), POISON_V)
            kp[..., D - 2:] = 1.0
            it = iter(perm)
            for s, lk in enumerate(lens_k):
                k0 = int(self.cu_k[s])
                for j in range(per[s]):
                    blk = self.block_table[s, j] = next(it)
                    n = min(page, lk - j * page)
                    kp[blk, :n], vp[blk, :n] = k[k0 + j * page:k0 + j * page + n], v[k0 + j * page:k0 + j * page + n]
            self.spare = [int(x) for x in it]
            k, v = kp, vp
        self.k, self.v = k, v
        self.kw = dict(causal=causal)

    def forward(self, **over):
        kw = dict(self.kw, seqused_k=None if self.used is None else np.asarray(self.used, dtype=np.int32),
                  block_table=self.block_table)
        kw.update(over)
        cu_k = kw.pop("cu_k", self.cu_k)
        return oracle.varlen_fwd(self.q, self.k, self.v, self.cu_q, cu_k, self.mq, self.mk, self.scale, **kw)

    def backward(self, o, lse, dt, cu_k=None):
        g = oracle.varlen_bwd(self.do, self.q, self.k, self.v, oracle.round_to(o, dt), lse.astype(np.float64), self.cu_q,
                              self.cu_k if cu_k is None else cu_k, self.mq, self.mk, self.scale, **self.kw)[:3]
        check_grad_cap(g)
        return g

    def design(self):
        pairs = bad = 0
        g = self.hq // self.hk
        for s, vis in enumerate(self.vis):
            q0, k0 = int(self.cu_q[s]), int(self.cu_k[s])
            if self.page or not vis.size:
                continue
            for h in range(self.hq):
                sc = np.rint(self.q[q0:q0 + vis.shape[0], h] @ self.k[k0:k0 + vis.shape[1], h // g].T / U).astype(np.int64)
                sc = np.where(vis, sc, -1)
                a, b = self.a[s][h], self.b[s][h]
                if self.variant == "decoy":
                    continue
                rows = np.nonzero(b >= 0)[0]
                assert ((vis.sum(axis=1) >= 2) == (b >= 0)).all()
                pairs += rows.size
                sa, sb = sc[rows, a[rows]], sc[rows, b[rows]]
                sc[rows, a[rows]] = -1
                sc[rows, b[rows]] = -1
                bad += int(((sa != sb) | (sa < 3) | (sc[rows].max(axis=1) > sa - 1)).sum())
        return pairs, bad


# ------------------------------------------------------------------------------------------------ kv-cache decode
class KVCache:
    """q [B, Tq, Hq, D], caches [B, Smax, Hk, D] or paged, an append of Tn = Tq rows (no rotary).  Row i's targets are
    its first and last visible key: with a causal mask the first cached key and the last appended key it may see, which
    lie in different key splits.  Every stale row (at or past cache_seqlens + Tn), every row below cache_leftpad and
    every unreferenced page is poison; all queries carry 8 U in both free dims.  Where the keys outnumber the code
    capacity (D 64: 400) positions reuse codes modulo the capacity, and a key that would repeat the code of one of the
    batch's targets is zero (a non-target needs no code: it only has to stay a unit behind)."""

    def __init__(self, D, hq, hk, tq, causal, window, seqlens=(1, 63, 700, 1000), smax=1024, page=0, leftpad=None,
                 fp8=False, seed=0):
        B = len(seqlens)
        self.D, self.hq, self.hk, self.tq, self.B, self.smax, self.page = D, hq, hk, tq, B, smax, page
        self.causal, self.window, self.fp8 = causal, window, fp8
        self.scale = D ** -0.5
        self.seqlens = np.asarray(seqlens, dtype=np.int32)
        self.leftpad = None if leftpad is None else np.asarray(leftpad, dtype=np.int32)
        self.kd, self.vd = (0.5, 2.0) if fp8 else (None, None)
        cap = capacity(D)
        tn = tq
        kc = np.zeros((B, smax, hk, D))
        kc[..., D - 2:] = 1.0
        vc = np.full((B, smax, hk, D), POISON_V)
        rnd = shared16((B, smax, hk, D), seed + 1)
        if fp8:                                               # values whose codes (x / descale) are exact in e4m3
            rnd = oracle.kvcache.round_e4m3(rnd) * self.vd
        self.q = np.zeros((B, tq, hq, D))
        self.knew, self.vnew = np.zeros((B, tn, hk, D)), np.zeros((B, tn, hk, D))
        self.vis, self.a, self.b = [], [], []
        for s in range(B):
            L = int(seqlens[s])
            lp = 0 if leftpad is None else int(leftpad[s])
            sk = L + tn
            assert lp + sk <= smax
            vis = visible(tq, sk, causal, window, norm_k=smax, kvcache=True)
            a, b = pick_targets(vis, "edges")
            tg = set((np.concatenate([a, b]) % cap).tolist()) if sk > cap else set()
            kk = code(np.arange(sk) % cap, D)
            for j in range(sk if tg else 0):
                if j % cap in tg and j not in a and j not in b:
                    kk[j] = 0.0
            kc[s, lp:lp + L] = kk[:L, None, :]
            vc[s, lp:lp + L] = rnd[s, lp:lp + L]
            self.knew[s] = kk[L:, None, :]
            self.vnew[s] = rnd[s, lp + L:lp + sk]
            self.q[s] = (U * (kk[a] + np.where((b >= 0)[:, None], kk[np.maximum(b, 0)], 0.0)))[:, None, :]
            self.vis.append(vis), self.a.append(a), self.b.append(b)
        self.q[..., D - 2:] = POISON_Q
        self.block_table = None
        if page:
            pps = smax // page
            nblk = B * pps + 3
            perm = np.random.default_rng(seed).permutation(nblk)
            self.block_table = perm[:B * pps].reshape(B, pps).astype(np.int32)
            self.spare = [int(x) for x in perm[B * pps:]]
            kp, vp = np.zeros((nblk, page, hk, D)), np.full((nblk, page, hk, D), POISON_V)
            kp[..., D - 2:] = 1.0
            kp[self.block_table.reshape(-1)] = kc.reshape(B * pps, page, hk, D)
            vp[self.block_table.reshape(-1)] = vc.reshape(B * pps, page, hk, D)
            kc, vc = kp, vp
        if fp8:                                               # the caches hold the codes' values
            kc, vc = kc / self.kd, vc / self.vd
        self.kc, self.vc = kc, vc

    def forward(self, **over):
        """(out [B, Tq, Hq, D], lse [B, Hq, Tq], k cache, v cache after the append) on fresh copies of the caches"""
        kc, vc = self.kc.copy(), self.vc.copy()
        kw = dict(k=self.knew, v=self.vnew, cache_seqlens=self.seqlens, cache_leftpad=self.leftpad,
                  block_table=self.block_table, causal=self.causal, window=self.window, io_dtype="bf16",
                  k_descale=self.kd, v_descale=self.vd)
        kw.update(over)
        o, lse = oracle.kvcache_fwd(self.q, kc, vc, **kw)
        return o, lse, kc, vc

    def design(self):
        pairs = bad = 0
        kc = self.forward()[2] * (self.kd or 1.0)
        for s, vis in enumerate(self.vis):
            lp = 0 if self.leftpad is None else int(self.leftpad[s])
            sk = vis.shape[1]
            if self.page:
                pos = lp + np.arange(sk)
                kk = kc[self.block_table[s, pos // self.page], pos % self.page, 0]
            else:
                kk = kc[s, lp:lp + sk, 0]
            sc = np.rint(self.q[s, :, 0, :self.D - 2] @ kk[:, :self.D - 2].T / U).astype(np.int64)
            sc = np.where(vis, sc, -1)
            a, b = self.a[s], self.b[s]
            rows = np.nonzero(b >= 0)[0]
            assert ((vis.sum(axis=1) >= 2) == (b >= 0)).all()
            pairs += rows.size
            sa, sb = sc[rows, a[rows]], sc[rows, b[rows]]
            sc[rows, a[rows]] = -1
            sc[rows, b[rows]] = -1
            bad += int(((sa != sb) | (sa < 3) | (sc[rows].max(axis=1) > sa - 1)).sum())
            assert not kk[:, self.D - 2:].any(), "a visible key carries poison"
        return pairs, bad


# ------------------------------------------------------------------------------------------------ gates
def ratio(got, ref, dt, mult=1.0):
    """max error / max |ref| over util's gate for it (what assert_close allows is 1.0)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max(initial=0.0) / max(np.abs(ref).max(initial=0.0), 1e-30) / (TOL_MAXREL[dt] * mult))


def lse_ratio(got, ref, atol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if (np.isneginf(got) != np.isneginf(ref)).any():
        return np.inf
    fin = np.isfinite(ref)
    return float(np.abs(got[fin] - ref[fin]).max(initial=0.0) / atol)


# ------------------------------------------------------------------------------------------------ the cases
CAUSAL, W300, W64, W100 = (True, (-1, -1)), (False, (300, 0)), (False, (64, 32)), (False, (100, 0))
_MASK_ID = {CAUSAL: "causal", W300: "w300_0", W64: "w64_32", W100: "w100_0"}
ALIBI = (0.5, 0.25, 0.125, 0.0625)


def _dense_cases():
    """(id, family, Dense kwargs, FA_ASM_FORCE).  The family names the forward and dQ kernels a case reaches in the built
    library: `hip` the compiler-scheduled ones (short lengths, and every length at D 64: the D 64 bodies of the
    hand-scheduled forward exist in experiment builds only), `asm` the hand-scheduled 256-row ones (D 128, 192 rows or
    more, FA_ASM_FORCE=1 to switch the length heuristic off).  The dK/dV pass at D 128 is the hand-scheduled kernel in
    BOTH families - it has no length test - so the `hip` D 128 dk / dv results are that kernel's on short shapes."""
    out = []

    def add(fam, sq, sk, D, hq, hk, mask, variant, force, B=1, alibi=None):
        cid = f"{fam}-{sq}x{sk}-D{D}-H{hq}_{hk}-{_MASK_ID[mask]}-{variant}" + ("-alibi" if alibi else "") + \
              ("" if force or fam != "asm" else "-noforce")
        out.append((cid, fam, dict(sq=sq, sk=sk, D=D, hq=hq, hk=hk, causal=mask[0], window=mask[1], variant=variant, B=B,
                                   seed=len(out) * 7, alibi=None if alibi is None else np.asarray(alibi[:hq])), force))

    for D in (64, 128):                                       # compiler-scheduled forward and dQ (short lengths)
        for sq, sk in ((77, 300), (257, 129)):
            for mask in (CAUSAL, W64, W100):
                for variant in ("edges", "random", "decoy"):
                    add("hip", sq, sk, D, 4, 2, mask, variant, False, B=2)
    for sq, sk in ((520, 520), (300, 520), (520, 300), (1300, 1300)):   # hand-scheduled forward, dQ and dK/dV (256-row blocks)
        for mask in (CAUSAL, W300, W64):
            for variant in VARIANTS:
                for hq, hk in ((2, 2), (4, 1)):
                    add("asm", sq, sk, 128, hq, hk, mask, variant, True)
    add("asm", 1300, 1300, 128, 2, 2, CAUSAL, "edges", False)
    # ALiBi bodies: forward and dQ take them with any head grouping, dK/dV only with one q-head per kv-head (2/2)
    add("asm", 1300, 1300, 128, 4, 1, CAUSAL, "decoy", True, alibi=ALIBI)
    add("asm", 1300, 1300, 128, 2, 2, CAUSAL, "decoy", True, alibi=ALIBI)
    for sq, sk in ((520, 300), (400, 400)):                   # D 64 at these lengths (code capacity 400): compiler kernels
        for mask in (CAUSAL, W64):
            for variant in ("edges", "tiles", "decoy"):
                add("hip", sq, sk, 64, 2, 2, mask, variant, False)
    for sq, sk, D in ((300, 520, 256), (520, 300, 256), (513, 513, 160)):   # head dim 256 and the 129..256 kernels
        for mask in (CAUSAL, W64):
            for variant in ("edges", "tiles", "decoy"):
                add("d256", sq, sk, D, 2, 1, mask, variant, False)
    return out


def _varlen_cases():
    """(id, family, Varlen kwargs, FA_ASM_FORCE).  Packed input reaches the hand-scheduled forward and dQ (the flat work
    list of 256-row blocks, its ragged blocks, its paged and seqused_k bodies) only at D 128 and when the sequences
    average 256 rows or more (total_q >= 256 batch); the paged bodies also want pages of 64 * 2^n keys.  The `varlen`
    family (lengths 0, 1, 2, 300, 520: 823 rows in 5 sequences) therefore runs the compiler-scheduled forward and dQ,
    `varlen_asm` (300, 520, 257) the hand-scheduled ones.  FA_ASM_FORCE is not read for packed input today; the long
    cases set it so that a length heuristic added later cannot take them off that path unnoticed."""
    lens, lens64, long = [0, 1, 2, 300, 520], [0, 1, 2, 300, 400], [300, 520, 257]
    out = []

    def add(cid, fam, **kw):
        out.append((cid, fam, dict(D=128, hq=4, hk=2, seed=len(out) + 3, **kw), fam == "varlen_asm"))

    for D, ls in ((128, lens), (64, lens64)):
        for variant in ("edges", "decoy"):
            add(f"D{D}-{variant}", "varlen", lens_q=ls, lens_k=ls, variant=variant)
            out[-1][2]["D"] = D
    add("D128-edges-H2_2", "varlen", lens_q=lens, lens_k=lens, variant="edges")
    out[-1][2].update(hq=2, hk=2)
    add("D128-edges-lens_k", "varlen", lens_q=lens, lens_k=[5, 0, 130, 520, 300], variant="edges")
    add("D128-decoy-lens_k", "varlen", lens_q=lens, lens_k=[5, 0, 130, 520, 300], variant="decoy")
    add("D128-seqused", "varlen", lens_q=lens, lens_k=lens, variant="edges", used=[0, 1, 1, 257, 300])
    for page in (16, 256):
        add(f"D128-paged{page}", "varlen", lens_q=lens, lens_k=lens, variant="edges", page=page)
    for variant in ("edges", "decoy"):
        add(f"long-{variant}", "varlen_asm", lens_q=long, lens_k=long, variant=variant)
    add("long-edges-H2_2", "varlen_asm", lens_q=long, lens_k=long, variant="edges")
    out[-1][2].update(hq=2, hk=2)
    add("long-edges-lens_k", "varlen_asm", lens_q=long, lens_k=[520, 300, 400], variant="edges")
    add("long-seqused", "varlen_asm", lens_q=long, lens_k=long, variant="edges", used=[257, 300, 1])
    for page in (64, 256):
        add(f"long-paged{page}", "varlen_asm", lens_q=long, lens_k=long, variant="edges", page=page)
    return out


def _kvcache_cases():
    """(id, KVCache kwargs); every case runs with num_splits 0, 1, 3 and 5"""
    out = []
    for D, hq, hk in ((128, 8, 8), (128, 16, 8), (128, 64, 8), (64, 4, 4)):
        for tq in (1, 5):
            for page in (0, 16, 256):
                for mask in (CAUSAL, W100):
                    out.append((f"D{D}-H{hq}_{hk}-Tq{tq}-page{page}-{_MASK_ID[mask]}",
                                dict(D=D, hq=hq, hk=hk, tq=tq, causal=mask[0], window=mask[1], page=page, seed=len(out))))
    out.append(("D128-H16_8-Tq5-leftpad", dict(D=128, hq=16, hk=8, tq=5, causal=True, window=(-1, -1), leftpad=[0, 3, 16, 7],
                                                  seed=101)))
    for D, hq, hk in ((128, 16, 8), (64, 4, 4)):
        out.append((f"D{D}-H{hq}_{hk}-Tq1-fp8", dict(D=D, hq=hq, hk=hk, tq=1, causal=True, window=(-1, -1), fp8=True, seed=102)))
    return out


DENSE_CASES, VARLEN_CASES, KVCACHE_CASES = _dense_cases(), _varlen_cases(), _kvcache_cases()
SPLITS = (0, 1, 3, 5)
