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

Sinks, tree masks, shared-prefix decode (the second half of the module).  A head's sink is the fp32 value of 3 U scale
and every row ties with it (tie_rows: rows whose targets share a digit are multiplied by 3/4, so that all targets score
3 U): the sink carries 1/3 of a two-target row and 1/2 of a one-target row, next to heads whose sink is -inf or 16 nats
behind (sink_values, SinkDense, SinkVarlen, KVCache(sinks=True)).  Tree puts the pair rows on a committed key and a
visible tree column and the decoy rows on two invisible columns, with the word boundaries of the packed mask (columns 31,
32, 63) pinned in the tree; SharedPrefix puts the targets on both sides of the merge, or on one side in neighbouring
sequences.  KVCache also takes cache_batch_idx (unreferenced batch rows are poison) and k=None.

Out of scope, on purpose, and no weaker variant of these exists here: softcap (tanh squeezes the one-unit margin: at D 128
and softcap 30 the targets sit 2 nats ahead instead of 16), rotary (rotated values are not exact in the io types), ALiBi
together with sinks, the fp8 q / k / v forward (it has its own gate in tests/fp8_gate.py), and dropout: a keep bit is not
a mask edge, and two targets per row cannot show WHICH bit of a row a kernel replayed wrongly - tests/dropout_readout.py
reads the whole keep mask out of O, dQ, dK and dV element by element instead.
"""
import numpy as np
import torch

import oracle
import oracle.attention as _oa
import sink_ref
import tree_ref
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


def aim(do, v, a, b, part=16):
    """dO [sq, D] of one head's pair rows, every row made to count: dO_i = (N(0, 1) / 8 + (V_a - V_b) / 16) / 128.
    dP_a - dP_b = dO_i . (V_a - V_b) then has the same size, D / 1024, in EVERY row; with the N(0, 1) part alone a row
    has a small difference now and then, and a mistake in just that row would change dQ little (dQ_i is dS_ia
    (code(a) - code(b))).  The sign is the same in all rows, so dK and dV of a key that many rows aim at - key 0 under a
    causal mask, 5200 rows at S 1300 with four heads - are sums WITHOUT cancellation (alternating signs were tried: the
    16-bit rounding of dS then shows in dK at 1 - 3 x the gate, a property of the data, not of a kernel); the factor
    1 / 128 keeps those sums below GRAD_CAP.  part: the sink cases take (V_a - V_b) / 4 (see sink_dout)."""
    two = (b >= 0)[:, None]
    return snap16(np.where(two, (do + (v[np.maximum(a, 0)] - v[np.maximum(b, 0)]) / part) / 128, do))


def to_dev(x, dt, device="cuda"):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DT[dt]).to(device)


def lse_atol(lse_ref, base=LSE_ATOL):
    """util.LSE_ATOL was calibrated on |LSE| of a few units; witness scores reach 4 U scale (128 at D 64, LSE up to
    about 140).  The gate grows with the fp32 ulp: x 2 in [64, 128), x 4 in [128, 256) - what the fp8 one-hot test uses."""
    fin = np.abs(lse_ref[np.isfinite(lse_ref)])
    top = float(fin.max()) if fin.size else 0.0
    return base * max(1.0, 2.0 ** (np.floor(np.log2(max(top, 1.0))) - 5))


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
def poison_cache(rows, smax, hk, D):
    """k / v caches [rows, smax, hk, D] in which every row is poison"""
    kc = np.zeros((rows, smax, hk, D))
    kc[..., D - 2:] = 1.0
    return kc, np.full((rows, smax, hk, D), POISON_V)


def paginate(kc, vc, page, seed):
    """contiguous caches [B, smax, Hk, D] -> (k pages, v pages, block_table, spare): the pages in a shuffled table, three
    spare pages that no table entry names and that hold poison"""
    B, smax, hk, D = kc.shape
    pps = smax // page
    nblk = B * pps + 3
    perm = np.random.default_rng(seed).permutation(nblk)
    table = perm[:B * pps].reshape(B, pps).astype(np.int32)
    kp, vp = poison_cache(nblk, page, hk, D)
    kp[table.reshape(-1)] = kc.reshape(B * pps, page, hk, D)
    vp[table.reshape(-1)] = vc.reshape(B * pps, page, hk, D)
    return kp, vp, table, [int(x) for x in perm[B * pps:]]


class KVCache:
    """q [B, Tq, Hq, D], caches [B, Smax, Hk, D] or paged, an append of Tn = Tq rows (no rotary).  Row i's targets are
    its first and last visible key: with a causal mask the first cached key and the last appended key it may see, which
    lie in different key splits.  Every stale row (at or past cache_seqlens + Tn), every row below cache_leftpad and
    every unreferenced page is poison; all queries carry 8 U in both free dims.  Where the keys outnumber the code
    capacity (D 64: 400) positions reuse codes modulo the capacity, and a key that would repeat the code of one of the
    batch's targets is zero (a non-target needs no code: it only has to stay a unit behind)."""

    def __init__(self, D, hq, hk, tq, causal, window, seqlens=(1, 63, 700, 1000), smax=1024, page=0, leftpad=None,
                 fp8=False, seed=0, batch_idx=False, append=True, sinks=False):
        """batch_idx: the caches hold B + 2 rows, sequence s lives in row B + 1 - s and the two unreferenced rows are
        poison; append False: the Tq newest rows already sit in the cache (k=None, cache_seqlens counts them); sinks:
        the tie / -inf / far mix of sink_values(), every row tied with it (tie_rows)"""
        B = len(seqlens)
        assert not (batch_idx and page)
        self.append = append
        self.bidx = np.array([B + 1 - s for s in range(B)], dtype=np.int32) if batch_idx else None
        self.D, self.hq, self.hk, self.tq, self.B, self.smax, self.page = D, hq, hk, tq, B, smax, page
        self.causal, self.window, self.fp8 = causal, window, fp8
        self.scale = D ** -0.5
        self.seqlens = np.asarray(seqlens, dtype=np.int32)
        self.leftpad = None if leftpad is None else np.asarray(leftpad, dtype=np.int32)
        self.kd, self.vd = (0.5, 2.0) if fp8 else (None, None)
        cap = capacity(D)
        tn = tq
        kc, vc = poison_cache(B + 2 if batch_idx else B, smax, hk, D)
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
            n = L if append else sk
            kc[self.row(s), lp:lp + n] = kk[:n, None, :]
            vc[self.row(s), lp:lp + n] = rnd[s, lp:lp + n]
            self.knew[s] = kk[L:, None, :]
            self.vnew[s] = rnd[s, lp + L:lp + sk]
            self.q[s] = (U * (kk[a] + np.where((b >= 0)[:, None], kk[np.maximum(b, 0)], 0.0)))[:, None, :]
            self.vis.append(vis), self.a.append(a), self.b.append(b)
        self.q[..., D - 2:] = POISON_Q
        self.sinks = None
        if sinks:
            tie_rows(self.q)
            self.sinks = sink_values(hq, D)
        self.block_table = None
        if page:
            kc, vc, self.block_table, self.spare = paginate(kc, vc, page, seed)
        if fp8:                                               # the caches hold the codes' values
            kc, vc = kc / self.kd, vc / self.vd
        self.kc, self.vc = kc, vc

    def forward(self, **over):
        """(out [B, Tq, Hq, D], lse [B, Hq, Tq], k cache, v cache after the append) on fresh copies of the caches"""
        kc, vc = self.kc.copy(), self.vc.copy()
        kw = dict(k=self.knew, v=self.vnew, cache_seqlens=self.seqlens, cache_leftpad=self.leftpad,
                  block_table=self.block_table, causal=self.causal, window=self.window, io_dtype="bf16",
                  k_descale=self.kd, v_descale=self.vd)
        if not self.append:
            kw.update(k=None, v=None, cache_seqlens=self.seqlens + self.tq)
        if self.bidx is not None:
            kw["cache_batch_idx"] = self.bidx
        kw.update(over)
        o, lse = oracle.kvcache_fwd(self.q, kc, vc, **kw)
        if self.sinks is not None:
            o, lse = sink_ref.sink_identity_bshd(o, lse.astype(np.float64), self.sinks)
        return o, lse, kc, vc

    def row(self, s):
        """the cache row of sequence s (contiguous caches)"""
        return s if self.bidx is None else int(self.bidx[s])

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
                kk = kc[self.row(s), lp:lp + sk, 0]
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


# ================================================================================================ sinks, trees, shared prefix
def tie_rows(q):
    """In place, on the code dims of q [..., D]: a pair row whose targets share a code digit holds 2 U in that dim and would
    score 4 U on its targets; such rows are multiplied by 3/4 (192 and 384 are exact in both io types).  Every row with a
    target then scores exactly 3 U on its targets and 2 U at most on any other key (1.5 U in a scaled row)."""
    c = q[..., :q.shape[-1] - 2]
    c[c.max(axis=-1) == 2 * U] *= 0.75
    return q


def sink_tie(D):
    """the sink logit that ties with the targets of every row: 3 U scale as the fp32 value the kernels read"""
    return float(np.float32(3 * U * D ** -0.5))


def sink_values(hq, D):
    """[hq] fp64: head h takes the tie value, -inf (must reproduce the no-sink result) or 2 U scale (16 nats or more
    behind: must change nothing), in turn.  On a tie head the sink carries 1/3 of a two-target row and 1/2 of a
    one-target row; a kernel that adds it n times (once per key split or row block) gives it n / (n + 2).
    sink_dout() shapes dO for these heads."""
    far = float(np.float32(2 * U * D ** -0.5))
    return np.array([(sink_tie(D), -np.inf, far)[h % 3] for h in range(hq)])


def sink_dout(do, v, a, b, tie):
    """dO [rows, D] of one head of a sink case, from the N(0, 1) / 8 draw `do`.  With P = 1/3 a tie head's dS_a is
    (2 dP_a - dP_b) / 9 against (dP_a - dP_b) / 4 on the other heads, and it holds dP_a + dP_b, which aim() does not steer: at
    D 64 a row's dQ then ranges over a factor of 2.5 and a mistake in a weak row counts for less.  So: the aimed part is
    (V_a - V_b) / 4 in place of / 16, times 2 D / |V_a - V_b|^2 so that dP_a - dP_b is the same in every row and not
    chi-square distributed (the rows' dQ then agree within a few per cent), dO is doubled on the tie heads (max |ref| is
    then not set by the other heads alone), and dO of a one-target row - dS = 0 without a sink, dP_a / 4 with one - is
    divided by 128 like the pair rows' instead of left at N(0, 1) / 8."""
    d2 = ((v[np.maximum(a, 0)] - v[np.maximum(b, 0)]) ** 2).sum(axis=-1, keepdims=True)
    do = aim(do, v, a, b, part=4 * np.maximum(d2, 1.0) / (2 * v.shape[-1]))
    one = (a >= 0) & (b < 0)
    do[one] = snap16(do[one] / 128)
    return do * (2.0 if tie else 1.0)


def sink_shares(sinks, D, a, b):
    """[..., Hq, rows] the factor a tie sink puts on a row's sink-free result: 2/3 with two targets, 1/2 with one, 1
    without a target or on the other heads.  a, b [..., Hq, rows]"""
    tie = (np.asarray(sinks) == sink_tie(D)).reshape((-1, 1))
    return np.where(tie & (b >= 0), 2.0 / 3, np.where(tie & (a >= 0), 0.5, 1.0))


def sink_grads(do, o16, lse, sinks, head_axis, rows=None, kind=None):
    """(the LSE the backward builds its P from, dsinks [Hq]) - dsinks = -sum exp(s_h - LSE) rowsum(dO o O16) over all rows
    of a head.  do / o16 [..., D] with lse [...] (the head at `head_axis` of lse).  rows (bool, lse's shape) and kind put
    one mistake into them: `drop` - the sink is missing from those rows' P (their LSE is the sink-free one) and from
    dsinks; `twice` - it is counted twice."""
    sh = [1] * lse.ndim
    sh[head_axis] = -1
    s = np.broadcast_to(np.asarray(sinks, dtype=np.float64).reshape(sh), lse.shape)
    lse = lse.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = np.where(np.isneginf(s) | np.isneginf(lse), 0.0, np.exp(s - lse))
        lp = lse
        if kind == "drop":
            lp = np.where(rows, np.where(w < 1.0, lse + np.log1p(-np.minimum(w, 1.0)), -np.inf), lse)
            w = np.where(rows, 0.0, w)
        elif kind == "twice":
            lp = np.where(rows & ~np.isneginf(s), np.logaddexp(lse, s), lse)
            w = np.where(rows, np.where(np.isneginf(s), 0.0, np.exp(s - lp)), w)
    d = (np.asarray(do) * np.asarray(o16)).sum(axis=-1)
    other = tuple(i for i in range(lse.ndim) if i != head_axis)
    return lp, -(w * d).sum(axis=other)


def _tie_design(qc, kk, vis, a, b):
    """(rows with two targets, rows that miss the design) from the exact score matrix in units of U: every row with a
    target scores 3 on each target and 2 at most on any other visible key.  qc [rows, D], kk [sk, D] code dims only."""
    s = np.where(vis, qc @ kk.T / U, -1.0)
    rows = np.nonzero(a >= 0)[0]
    sa = s[rows, a[rows]]
    sb = np.where(b[rows] >= 0, s[rows, np.maximum(b[rows], 0)], 3.0)
    s = s.copy()
    s[rows, a[rows]] = -1.0
    two = rows[b[rows] >= 0]
    s[two, b[two]] = -1.0
    bad = (sa != 3.0) | (sb != 3.0) | (s[rows].max(axis=1, initial=-1.0) > 2.0)
    assert ((vis.sum(axis=1) >= 2) >= (b >= 0)).all()
    return int((b >= 0).sum()), int(bad.sum())


class SinkDense(Dense):
    """Dense with per-head sinks: tie_rows() on q, sink_values() per head.  The forward reference is sink_ref.ref_dense in
    fp64; the backward is the oracle's on the sink-inclusive LSE (P = exp(S - LSE) then holds the sink's share) plus the
    closed form of dsinks - tests/test_witness_cpu.py holds both to ref_dense's autograd."""

    def __init__(self, **kw):
        super().__init__(**kw)
        assert self.variant != "decoy" and self.alibi is None
        tie_rows(self.q)
        self.sinks = sink_values(self.hq, self.D)
        raw = shared16(self.do.shape, kw.get("seed", 0) + 2, scale=0.125)
        for bi in range(self.B):
            for h in range(self.hq):
                self.do[bi, h] = sink_dout(raw[bi, h], self.v[bi, h // (self.hq // self.hk)], self.a[bi, h], self.b[bi, h],
                                           self.sinks[h] == sink_tie(self.D))

    def torch_inputs(self):
        return [torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1, 3))) for x in (self.q, self.k, self.v, self.do)] + \
               [torch.from_numpy(self.sinks)]

    def forward(self):
        q, k, v, _, s = self.torch_inputs()
        o, lse = sink_ref.ref_dense(q, k, v, s, self.scale, causal=self.causal, window=self.window)
        return o.numpy().transpose(0, 2, 1, 3), lse.numpy()

    def backward(self, o, lse, dt, rows=None, kind=None):
        """(dq, dk, dv, dsinks); rows [B, Hq, Sq] bool + kind: one mistake of sink_grads() in the backward's P"""
        o16 = o if dt is None else oracle.round_to(o, dt)         # (None: the exact O, to compare with autograd)
        lp, ds = sink_grads(self.do, o16, lse, self.sinks, 1, rows, kind)
        g = oracle.attn_bwd(self.do, self.q, self.k, self.v, o16, lp, self.scale, **self.kw)[:3]
        check_grad_cap(g)
        return g + (ds,)

    def pair_out(self, magnitude=False):
        return super().pair_out(magnitude) * sink_shares(self.sinks, self.D, self.a, self.b)[..., None]

    def design(self):
        g = self.hq // self.hk
        pairs = bad = 0
        for bi in range(self.B):
            for h in range(self.hq):
                p, x = _tie_design(self.q[bi, h, :, :self.D - 2], self.k[bi, h // g, :, :self.D - 2], self.vis,
                                   self.a[bi, h], self.b[bi, h])
                pairs, bad = pairs + p, bad + x
        return pairs, bad


class SinkVarlen(Varlen):
    """Varlen with per-head sinks (tie_rows, sink_values).  Forward: the oracle + sink_ref's identity (paged too);
    backward: the oracle's on the sink-inclusive LSE + the closed form of dsinks, held to ref_varlen's autograd on the CPU."""

    def __init__(self, **kw):
        super().__init__(**kw)
        assert self.variant != "decoy" and self.used is None
        tie_rows(self.q)
        self.sinks = sink_values(self.hq, self.D)
        raw = shared16(self.do.shape, kw.get("seed", 0) + 2, scale=0.125)
        for s, (lq, lk) in enumerate(zip(self.lens_q, self.lens_k)):
            q0, k0 = int(self.cu_q[s]), int(self.cu_k[s])
            for h in range(self.hq if lq and not self.page else 0):
                self.do[q0:q0 + lq, h] = sink_dout(raw[q0:q0 + lq, h], self.v[k0:k0 + lk, h // (self.hq // self.hk)], self.a[s][h],
                                                   self.b[s][h], self.sinks[h] == sink_tie(self.D))

    def forward(self, **over):
        o, lse = super().forward(**over)
        return sink_ref.sink_identity_thd(o, lse.astype(np.float64), self.sinks)

    def backward(self, o, lse, dt, rows=None, kind=None):
        """(dq, dk, dv, dsinks); rows [Hq, Tq] bool + kind: one mistake of sink_grads()"""
        o16 = o if dt is None else oracle.round_to(o, dt)         # (None: the exact O, to compare with autograd)
        lp, ds = sink_grads(self.do.transpose(1, 0, 2), o16.transpose(1, 0, 2), lse, self.sinks, 0, rows, kind)
        g = oracle.varlen_bwd(self.do, self.q, self.k, self.v, o16, lp, self.cu_q, self.cu_k, self.mq, self.mk, self.scale,
                              **self.kw)[:3]
        check_grad_cap(g)
        return g + (ds,)

    def targets(self):
        """a, b [Hq, Tq]"""
        cat = lambda x: np.concatenate([np.stack(s) if len(s[0]) else np.zeros((self.hq, 0), dtype=np.int64) for s in x], axis=1)
        return cat(self.a), cat(self.b)

    def pair_out(self, magnitude=False):
        """[Tq, Hq, D]: (V_a + V_b) / 2 or V_a of each row's own sequence, times the sink's share (contiguous K / V);
        magnitude: from |V|"""
        a, b = self.targets()
        g = self.hq // self.hk
        o = np.zeros_like(self.q)
        for s in range(len(self.lens_q)):
            q0, q1, k0 = int(self.cu_q[s]), int(self.cu_q[s + 1]), int(self.cu_k[s])
            for h in range(self.hq):
                v = self.v[k0:k0 + max(self.lens_k[s], 1), h // g]
                v = np.abs(v) if magnitude else v
                aa, bb = a[h, q0:q1], b[h, q0:q1]
                va = np.where(aa[:, None] >= 0, v[np.maximum(aa, 0)], 0.0)
                o[q0:q1, h] = np.where(bb[:, None] >= 0, (va + v[np.maximum(bb, 0)]) / 2, va)
        return o * sink_shares(self.sinks, self.D, a, b).T[..., None]

    def design(self):
        pairs = bad = 0
        g = self.hq // self.hk
        for s, vis in enumerate(self.vis):
            q0, k0 = int(self.cu_q[s]), int(self.cu_k[s])
            if self.page or not vis.size:
                continue
            for h in range(self.hq):
                p, x = _tie_design(self.q[q0:q0 + vis.shape[0], h, :self.D - 2], self.k[k0:k0 + vis.shape[1], h // g, :self.D - 2],
                                   vis, self.a[s][h], self.b[s][h])
                pairs, bad = pairs + p, bad + x
        return pairs, bad


def with_sink(o, lse, sink):
    """one head's sink-free (out [rows, D], LSE [rows]) with the sink logit `sink` (None: as they are), fp64"""
    lse = np.asarray(lse, dtype=np.float64)
    if sink is None:
        return o, lse
    o, lse = sink_ref.sink_identity(o[None], lse[None], np.array([sink]), 0)
    return o[0], lse[0]


def masked_forward(q, k, v, vis, scale, sink=None):
    """one head under an explicit mask: q [rows, D], k / v [sk, D] -> out [rows, D], LSE [rows] (fp64), with one sink logit"""
    return with_sink(*leak_forward(q, k, v, vis, scale), sink)


def sink_mistake(o, lse, sink, rows, kind):
    """one head's sink-inclusive forward (out [rows, D], LSE [rows]) in which `rows` dropped the sink or counted it twice"""
    with np.errstate(divide="ignore", over="ignore"):
        w = np.exp(sink - lse)
        f, l = (1.0 / (1.0 - w), lse + np.log1p(-w)) if kind == "drop" else (1.0 / (1.0 + w), np.logaddexp(lse, sink))
    o, lse = o.copy(), lse.copy()
    o[rows], lse[rows] = (o * f[:, None])[rows], l[rows]
    return o, lse


def gather_cache(c, s, kc, vc, sk):
    """the first sk logical keys of sequence s, K / V [sk, Hk, D] with the fp8 descales applied, from caches in c's layout"""
    lp = 0 if c.leftpad is None else int(c.leftpad[s])
    pos = lp + np.arange(sk)
    if c.block_table is not None:
        page = kc.shape[1]
        kk, vv = (x[c.block_table[s, pos // page], pos % page] for x in (kc, vc))
    else:
        kk, vv = kc[c.row(s), pos], vc[c.row(s), pos]
    return kk * (c.kd or 1.0), vv * (c.vd or 1.0)


def cache_pair_out(c, vs, magnitude=False):
    """[B, T, Hq, D]: (V_a + V_b) / 2 or V_a per row of a cache case, times the sink's share; vs[s] [sk, Hk, D] the values of
    sequence s's keys.  magnitude: from |V|, the scale of the operands where they cancel"""
    g = c.hq // c.hk
    o = np.zeros_like(c.q)
    for s in range(c.B):
        a, b = c.a[s], c.b[s]
        for h in range(c.hq):
            v = np.abs(vs[s][:, h // g]) if magnitude else vs[s][:, h // g]
            va = np.where(a[:, None] >= 0, v[np.maximum(a, 0)], 0.0)
            o[s, :, h] = np.where(b[:, None] >= 0, (va + v[np.maximum(b, 0)]) / 2, va)
    if c.sinks is not None:
        a, b = (np.broadcast_to(np.stack(x)[:, None, :], (c.B, c.hq, o.shape[1])) for x in (c.a, c.b))
        o = o * sink_shares(c.sinks, c.D, a, b).transpose(0, 2, 1)[..., None]
    return o


# ------------------------------------------------------------------------------------------------ tree masks
def tree_parents(T, rng):
    """tree_ref.random_parents with the word boundaries of the packed mask pinned: node 32's parent is 30 (column 31 is the
    highest non-ancestor below it: its decoy, one bit left of word 1), node 33's parent is 32 (bit 0 of word 1 visible next
    to bit 31 of word 0 hidden), node 63's parent is 31 (bit 31 of word 0 visible from the last row of word 1; 62 its decoy)"""
    par = tree_ref.random_parents(T, rng)
    for t, p in ((32, 30), (33, 32), (63, 31)):
        if t < T:
            par[t] = p
    return par


class Tree:
    """flash_attn_with_kvcache(tree_mask=): q [B, T, Hq, D] are the T nodes of a draft tree appended at cache_seqlens
    (slot L + t), parents as in tree_ref.py; row t sees the L committed keys and the columns of its ancestors and itself.
    No rotary, no softcap.  Reference: tree_ref.ref_tree.

      own / root  pair rows: target a is a committed key - the first one for even t, the last one (L - 1, next to the first
                  tree column) for odd t -, target b a visible tree column: the node's own (`own`) or its farthest
                  ancestor's (`root`);
      decoy       q aims at two INVISIBLE tree columns: the highest non-ancestor below t and column t + 1 (a descendant or
                  a sibling); one leaked mask bit takes the row.

    Stale rows at and past L + T, rows below the left pad and unreferenced pages are poison, as in KVCache.  The keys
    fit the code capacity (L + T <= capacity(D)), so no code repeats."""

    def __init__(self, D, hq, hk, T, variant, seqlens, page=0, leftpad=None, fp8=False, sinks=False, append=True,
                 shared=False, packed=False, seed=0):
        B = len(seqlens)
        self.D, self.hq, self.hk, self.T, self.B, self.page, self.variant = D, hq, hk, T, B, page, variant
        self.fp8, self.append, self.shared, self.packed, self.bidx = fp8, append, shared, packed, None
        self.scale = D ** -0.5
        self.seqlens = np.asarray(seqlens, dtype=np.int32)
        self.leftpad = None if leftpad is None else np.asarray(leftpad, dtype=np.int32)
        self.kd, self.vd = (0.5, 2.0) if fp8 else (None, None)
        assert max(seqlens) + T <= capacity(D) and min(seqlens) >= 1
        unit = max(page, 32)
        smax = -(-(max(seqlens) + T + (0 if leftpad is None else max(leftpad)) + 8) // unit) * unit
        self.smax = smax
        rng = np.random.default_rng(seed)
        pars = [tree_parents(T, rng) for _ in range(1 if shared else B)]
        self.par = [pars[0 if shared else s] for s in range(B)]
        self.mask = np.stack([tree_ref.mask_from_parents(p) for p in self.par])
        kc, vc = poison_cache(B, smax, hk, D)
        rnd = shared16((B, smax, hk, D), seed + 1)
        if fp8:
            rnd = oracle.kvcache.round_e4m3(rnd) * self.vd
        self.q = np.zeros((B, T, hq, D))
        self.knew, self.vnew = np.zeros((B, T, hk, D)), np.zeros((B, T, hk, D))
        self.vis, self.a, self.b = [], [], []
        for s in range(B):
            L = int(seqlens[s])
            lp = 0 if leftpad is None else int(leftpad[s])
            sk = L + T
            vis = np.ones((T, sk), dtype=bool)
            vis[:, L:] = self.mask[s]
            a, b = np.full(T, -1), np.full(T, -1)
            for t in range(T):
                if variant == "decoy":
                    below = [c for c in range(t) if not self.mask[s, t, c]]
                    a[t] = L + below[-1] if below else -1
                    b[t] = L + t + 1 if t + 1 < T else -1
                else:
                    root = t
                    while self.par[s][root] >= 0:
                        root = self.par[s][root]
                    a[t], b[t] = (0 if t % 2 == 0 else L - 1), L + (t if variant == "own" else root)
            kk = code(np.arange(sk), D)
            n = L if append else sk
            kc[s, lp:lp + n] = kk[:n, None, :]
            vc[s, lp:lp + n] = rnd[s, lp:lp + n]
            self.knew[s], self.vnew[s] = kk[L:, None, :], rnd[s, lp + L:lp + sk]
            self.q[s] = (U * (code(a, D) + code(b, D)))[:, None, :]
            self.vis.append(vis), self.a.append(a), self.b.append(b)
        tie_rows(self.q)
        self.q[..., D - 2:] = POISON_Q
        self.sinks = sink_values(hq, D) if sinks else None
        self.block_table = None
        if page:
            kc, vc, self.block_table, self.spare = paginate(kc, vc, page, seed)
        if fp8:
            kc, vc = kc / self.kd, vc / self.vd
        self.kc, self.vc = kc, vc

    def row(self, s):
        return s

    def call_mask(self):
        """the mask as the call passes it: bool or packed words, [T, T(words)] when shared, else per batch entry"""
        m = self.mask[0] if self.shared else self.mask
        return tree_ref.pack_mask(m) if self.packed else m

    def forward(self, mask=None, caches=None):
        """(out [B, T, Hq, D], lse [B, Hq, T], k cache, v cache after the append).  mask: a mistaken mask [B, T, T] in place
        of the case's; caches: (k, v) caches that already hold the nodes, in place of the case's caches and its append"""
        if mask is None and caches is None:                   # the clean reference, computed once and left unchanged
            if not hasattr(self, "_ref"):
                self._ref = self.forward(mask=self.mask)
            return self._ref
        done = caches is not None or not self.append
        kw = dict(cache_seqlens=self.seqlens + (self.T if done else 0), cache_leftpad=self.leftpad,
                  block_table=self.block_table, io_dtype="bf16", k_descale=self.kd, v_descale=self.vd, sinks=self.sinks)
        k, v = (None, None) if done else (self.knew, self.vnew)
        kc, vc = (self.kc, self.vc) if caches is None else caches
        return tree_ref.ref_tree(self.q, kc, vc, self.mask if mask is None else mask, k=k, v=v, **kw)

    def pair_out(self, magnitude=False):
        """(V_a + V_b) / 2 per row, times the sink's share [B, T, Hq, D] (own / root)"""
        kc, vc = self.forward()[2:]
        return cache_pair_out(self, [gather_cache(self, s, kc, vc, v.shape[1])[1] for s, v in enumerate(self.vis)], magnitude)

    def slot(self, s, j):
        """the index of logical key j of sequence s in the caches"""
        pos = j + (0 if self.leftpad is None else int(self.leftpad[s]))
        return (int(self.block_table[s, pos // self.page]), pos % self.page) if self.page else (s, pos)

    def design(self):
        kc = self.forward()[2]
        pairs = bad = 0
        for s, vis in enumerate(self.vis):
            kk = gather_cache(self, s, kc, kc, vis.shape[1])[0][:, 0]
            assert not kk[:, self.D - 2:].any(), "a visible key carries poison"
            qc, kk = self.q[s, :, 0, :self.D - 2], kk[:, :self.D - 2]
            if self.variant == "decoy":                       # each decoy scores 3, every visible key 2 at most
                sc = qc @ kk.T / U
                for d in (self.a[s], self.b[s]):
                    r = np.nonzero(d >= 0)[0]
                    bad += int((sc[r, d[r]] != 3.0).sum() + (vis[r, d[r]]).sum())
                bad += int((np.where(vis, sc, -1.0).max(axis=1) > 2.0).sum())
                continue
            p, x = _tie_design(qc, kk, vis, self.a[s], self.b[s])
            pairs, bad = pairs + p, bad + x
        return pairs, bad


# ------------------------------------------------------------------------------------------------ shared prefix
SUFFIX = (0, 5, 130)


class SharedPrefix:
    """flash_attn_with_shared_prefix: prefix keys carry codes 0 .. S_p - 1, the suffix keys of every sequence continue from
    S_p (cached keys, then the T appended ones); q [B, T, Hq, D].  Every row sees the whole prefix and the suffix keys up to
    its own token.  Reference: fp64 attention over the concatenated keys under that explicit mask.

      split   a is the first prefix key for even rows and the last one for odd rows, b the last suffix key the row may see:
              the merge weights are 1/2, 1/2 and out is (V_a + V_b) / 2;
      prefix  both targets in the prefix (first and last key); the suffix is 16 nats behind, or empty (LSE -inf);
      suffix  both targets in the suffix (its first key and the row's last);
      mixed   sequence s takes prefix / split / suffix in turn: neighbouring sequences merge with different weights;
      decoy   q aims at the appended token t + 1 and, like every query here, at the poison.

    A row whose part holds one key only (or none) falls back to one target (or to the other part's).  Suffix rows at and
    past cache_seqlens + T, spare pages and unreferenced batch rows are poison."""

    def __init__(self, T, S_p, variant, D=128, hq=8, hk=2, layout="contig", fp8=False, sinks=False, append=True, seed=0):
        B, smax = len(SUFFIX), 160
        self.T, self.S_p, self.variant, self.D, self.hq, self.hk, self.B = T, S_p, variant, D, hq, hk, B
        self.layout, self.fp8, self.append, self.leftpad = layout, fp8, append, None
        self.scale = D ** -0.5
        self.seqlens = np.asarray(SUFFIX, dtype=np.int32)
        self.kd, self.vd = (0.5, 2.0) if fp8 else (None, None)
        tn = T if append else 0
        assert S_p + max(SUFFIX) + tn <= capacity(D)
        self.bidx = np.array([B + 1 - s for s in range(B)], dtype=np.int32) if layout == "batch_idx" else None
        self.pk = np.broadcast_to(code(np.arange(S_p), D)[:, None, :], (S_p, hk, D)).copy()
        self.pv = shared16((S_p, hk, D), seed + 3)
        kc, vc = poison_cache(B + 2 if self.bidx is not None else B, smax, hk, D)
        rnd = shared16((B, smax, hk, D), seed + 1)
        if fp8:
            rnd = oracle.kvcache.round_e4m3(rnd) * self.vd
        self.q = np.zeros((B, T, hq, D))
        self.knew, self.vnew = np.zeros((B, tn, hk, D)), np.zeros((B, tn, hk, D))
        self.vis, self.a, self.b = [], [], []
        for s in range(B):
            L = int(SUFFIX[s])
            sk = L + tn
            kk = code(S_p + np.arange(sk), D)
            kc[self.row(s), :L], vc[self.row(s), :L] = kk[:L, None, :], rnd[s, :L]
            self.knew[s], self.vnew[s] = kk[L:, None, :], rnd[s, L:sk]
            last = sk - T + np.arange(T)                      # the last suffix key row t may see (< 0: none)
            vis = np.ones((T, S_p + sk), dtype=bool)
            vis[:, S_p:] = np.arange(sk)[None, :] <= last[:, None]
            a, b = np.full(T, -1), np.full(T, -1)
            kind = ("prefix", "split", "suffix")[s % 3] if variant == "mixed" else variant
            for t in range(T):
                pre = (0, S_p - 1 if S_p > 1 else -1)
                if kind == "decoy":
                    a[t] = S_p + last[t] + 1 if last[t] + 1 < sk else -1
                elif kind == "split":
                    a[t], b[t] = (0 if t % 2 == 0 else S_p - 1), (S_p + last[t] if last[t] >= 0 else -1)
                elif kind == "suffix" and last[t] >= 0:
                    a[t], b[t] = S_p, (S_p + last[t] if last[t] > 0 else -1)
                else:
                    a[t], b[t] = pre
            allk = np.concatenate([self.pk[:, 0], kk])
            self.q[s] = (U * (allk[np.maximum(a, 0)] * (a >= 0)[:, None] + allk[np.maximum(b, 0)] * (b >= 0)[:, None]))[:, None, :]
            self.vis.append(vis), self.a.append(a), self.b.append(b)
        tie_rows(self.q)
        self.q[..., D - 2:] = POISON_Q
        self.sinks = sink_values(hq, D) if sinks else None
        self.block_table = None
        if layout == "paged":
            kc, vc, self.block_table, self.spare = paginate(kc, vc, 16, seed)
        if fp8:
            kc, vc = kc / self.kd, vc / self.vd
        self.kc, self.vc = kc, vc

    def row(self, s):
        return s if self.bidx is None else int(self.bidx[s])

    def after(self):
        """the suffix caches after the append (fresh copies)"""
        kc, vc = self.kc.copy(), self.vc.copy()
        for s in range(self.B):
            for r in range(self.knew.shape[1]):
                pos = int(SUFFIX[s]) + r
                i = (int(self.block_table[s, pos // 16]), pos % 16) if self.block_table is not None else (self.row(s), pos)
                kc[i], vc[i] = self.knew[s, r] / (self.kd or 1.0), self.vnew[s, r] / (self.vd or 1.0)
        return kc, vc

    def keys(self, s):
        """([prefix ; suffix] K, V [S_p + sk, Hk, D], S_p) of sequence s, descaled"""
        kc, vc = self.after()
        kk, vv = gather_cache(self, s, kc, vc, self.vis[s].shape[1] - self.S_p)
        return np.concatenate([self.pk, kk]), np.concatenate([self.pv, vv])

    def forward(self, parts=False):
        """out [B, T, Hq, D], lse [B, Hq, T] over the concatenated keys.  parts: instead the two partial results the operator
        merges, (o_p, lse_p, o_s, lse_s) - the prefix pass without sink, the suffix pass with it"""
        g = self.hq // self.hk
        res = [np.zeros((self.B, self.T, self.hq, self.D)), np.zeros((self.B, self.hq, self.T)),
               np.zeros((self.B, self.T, self.hq, self.D)), np.zeros((self.B, self.hq, self.T))]
        for s in range(self.B):
            kk, vv = self.keys(s)
            for h in range(self.hq):
                sink = None if self.sinks is None else self.sinks[h]
                args = (self.q[s, :, h], kk[:, h // g], vv[:, h // g])
                if not parts:
                    res[0][s, :, h], res[1][s, h] = masked_forward(*args, self.vis[s], self.scale, sink)
                    continue
                P = self.S_p
                res[0][s, :, h], res[1][s, h] = masked_forward(args[0], args[1][:P], args[2][:P], self.vis[s][:, :P], self.scale)
                res[2][s, :, h], res[3][s, h] = masked_forward(args[0], args[1][P:], args[2][P:], self.vis[s][:, P:], self.scale, sink)
        return tuple(res) if parts else (res[0], res[1])

    def pair_out(self, magnitude=False):
        """(V_a + V_b) / 2 or V_a per row, times the sink's share [B, T, Hq, D] (pair variants); magnitude: from |V|"""
        return cache_pair_out(self, [self.keys(s)[1] for s in range(self.B)], magnitude)

    def design(self):
        pairs = bad = 0
        for s, vis in enumerate(self.vis):
            kk = self.keys(s)[0][:, 0]
            assert not kk[:, self.D - 2:].any(), "a visible key carries poison"
            qc, kk = self.q[s, :, 0, :self.D - 2], kk[:, :self.D - 2]
            if self.variant == "decoy":
                continue
            p, x = _tie_design(qc, kk, vis, self.a[s], self.b[s])
            pairs, bad = pairs + p, bad + x
        return pairs, bad


def merge_states(o_p, l_p, o_s, l_s):
    """what fa_merge_states computes: out [..., T, Hq, D], lse [..., Hq, T] of two partial results over disjoint keys"""
    with np.errstate(invalid="ignore"):
        l = np.logaddexp(l_p, l_s)
        wp = np.where(np.isneginf(l_p), 0.0, np.exp(l_p - l))
        ws = np.where(np.isneginf(l_s), 0.0, np.exp(l_s - l))
    sw = lambda w: np.swapaxes(w, -1, -2)[..., None]
    return o_p * sw(wp) + o_s * sw(ws), l


# ------------------------------------------------------------------------------------------------ the new cases
def _sink_dense_cases():
    """(id, family, SinkDense kwargs, FA_ASM_FORCE).  The sink forward always runs fa_fwd_kernel, the compiler-scheduled
    kernel: the hand-scheduled forward declines a call with sinks (its epilogue has no sink term).  The backward reads the
    sink-inclusive LSE and is the plain one; the `asm` case (D 128, 520 rows, FA_ASM_FORCE=1) therefore reaches the
    hand-scheduled dQ and dK/dV kernels, the others the compiler-scheduled dQ (and, at D 128, the hand-scheduled dK/dV).
    Targets are `random` or `tiles`, or the mask is a window: with `edges` under a causal mask key 0's dK sets max |ref| and
    a band that forgets the sink moves dk / dv by less than the gate."""
    out = []

    def add(fam, sq, sk, D, hq, hk, mask, variant, force, B=1):
        cid = f"sink-{fam}-{sq}x{sk}-D{D}-H{hq}_{hk}-{_MASK_ID[mask]}-{variant}"
        out.append((cid, fam, dict(sq=sq, sk=sk, D=D, hq=hq, hk=hk, causal=mask[0], window=mask[1], variant=variant, B=B,
                                   seed=1000 + len(out) * 7), force))

    add("hip", 300, 520, 128, 4, 2, W64, "random", False)     # GQA
    add("hip", 400, 400, 64, 4, 1, CAUSAL, "random", False, B=2)  # MQA, D 64 (`tiles` here: a band moves dq by 2.4 x its gate only)
    add("hip", 520, 300, 64, 4, 2, CAUSAL, "random", False)   # Sq > Sk: 220 rows without a key (out 0, LSE = s_h)
    add("d256", 300, 520, 256, 4, 1, W64, "random", False)    # D 256, MQA
    add("asm", 520, 520, 128, 4, 2, W64, "random", True)      # hand-scheduled dQ and dK/dV on the sink-inclusive LSE
    return out


def _sink_varlen_cases():
    """(id, SinkVarlen kwargs): lengths 0, 1, 2, 300, 520 forward and backward (`random` targets, GQA and one q-head per
    kv-head), one paged forward"""
    lens = [0, 1, 2, 300, 520]
    base = dict(lens_q=lens, lens_k=lens, D=128, hq=4, hk=2, variant="random")
    return [("sink-varlen-D128-random", dict(base, seed=2001)),
            ("sink-varlen-D128-random-H2_2", dict(base, hq=2, hk=2, seed=2002)),
            ("sink-varlen-D128-paged16", dict(base, variant="edges", page=16, seed=2003))]


def _sink_kvcache_cases():
    """(id, KVCache kwargs), each with num_splits 0, 1, 3 and 5: a 16-bit and an fp8 cache"""
    return [("sink-D128-H16_8-Tq5", dict(D=128, hq=16, hk=8, tq=5, causal=True, window=(-1, -1), sinks=True, seed=3001)),
            ("sink-D64-H4_4-Tq1-page16", dict(D=64, hq=4, hk=4, tq=1, causal=True, window=(-1, -1), page=16, sinks=True, seed=3002)),
            ("sink-D128-H16_8-Tq1-fp8", dict(D=128, hq=16, hk=8, tq=1, causal=True, window=(-1, -1), fp8=True, sinks=True, seed=3003)),
            ("sink-D128-H8_2-Tq5-fp8", dict(D=128, hq=8, hk=2, tq=5, causal=True, window=(-1, -1), fp8=True, sinks=True, seed=3004))]


def _route_cases():
    """(id, KVCache kwargs, num_splits to run).  The route is read from decode_takes() / launch_decode_td() in
    csrc/fa_decode.hip."""
    c = dict(causal=True, window=(-1, -1))
    return [
        # fa_decode_kernel<D 128, 16-bit>, a workgroup per kv-head; the caches hold B + 2 rows, two of them unreferenced
        ("route-batch_idx-D128-H16_8-Tq5", dict(D=128, hq=16, hk=8, tq=5, batch_idx=True, seed=4001, **c), SPLITS),
        # D 256: the NARROW instantiation with head_dim_v = 256, four waves
        ("route-D256-H4_2-Tq5", dict(D=256, hq=4, hk=2, tq=5, seed=4002, **c), SPLITS),
        ("route-D256-H4_2-Tq1-page16", dict(D=256, hq=4, hk=2, tq=1, page=16, seed=4003, **c), (0, 3)),
        # D 96: padded to the 128-wide kernel, NARROW with 96 valid columns, eight waves
        ("route-D96-H8_2-Tq5", dict(D=96, hq=8, hk=2, tq=5, seed=4004, **c), SPLITS),
        # fp8, H_k 8, 5 x 4 = 20 packed rows: decode_hpw() - a head per wave, F8M
        ("route-fp8-hpw-D128-H32_8-Tq5", dict(D=128, hq=32, hk=8, tq=5, fp8=True, seed=4005, **c), SPLITS),
        # fp8, H_k 2: decode_hpw() says no (H_k < 8), the eight-wave F8M row-block form of fa_decode_kernel
        ("route-fp8-f8m-D128-H8_2-Tq5", dict(D=128, hq=8, hk=2, tq=5, fp8=True, seed=4006, **c), SPLITS),
        ("route-fp8-f8m-D128-H8_2-Tq5-page16", dict(D=128, hq=8, hk=2, tq=5, fp8=True, page=16, seed=4007, **c), (0, 3)),
        # k=None: the five newest rows already sit in the cache
        ("route-noappend-D128-H16_8-Tq5", dict(D=128, hq=16, hk=8, tq=5, append=False, seed=4008, **c), SPLITS),
        ("route-noappend-D64-H4_4-Tq1-page256", dict(D=64, hq=4, hk=4, tq=1, append=False, page=256, seed=4009, **c), (0, 3)),
        # decode_takes() declines: G 8, T_q 130 -> 33 row blocks of 32 packed rows against 8 x 2 = 16 passes of the general
        # kernel, and 4 x 64 x 2 = 512 general workgroups = 2 x 256 CUs give factor 1 (33 > 16): fa_fwd_kernel reads the cache
        ("route-general-D128-H64_8-Tq130", dict(D=128, hq=64, hk=8, tq=130, seqlens=(1, 63, 700, 894), seed=4010, **c), (0,)),
    ]


def _tree_cases():
    """(id, Tree kwargs, num_splits), each in the variants own / root / decoy.  Routes from launch_decode_td(): every tree
    call runs fa_decode_kernel (decode_takes() returns true on FA_FLAG_TREE_MASK), in row blocks of 32 packed rows."""
    cases = [
        # 16-bit D 64, one row block (T 2 x G 1), bool mask per batch entry
        ("tree-D64-H4_4-T2", dict(D=64, hq=4, hk=4, T=2, seqlens=(1, 63, 330)), 0),
        # 16-bit D 128, G 8 x T 32 = 8 row blocks, pages of 256, packed words per batch entry, split
        ("tree-D128-H16_2-T32-page256-words", dict(D=128, hq=16, hk=2, T=32, seqlens=(1, 95, 1000), page=256, packed=True), 4),
        # D 256 (NARROW instantiation, four waves), two mask words, one shared bool mask
        ("tree-D256-H2_2-T33-shared", dict(D=256, hq=2, hk=2, T=33, seqlens=(64, 333), shared=True), 1),
        # D 96 (NARROW, 96 valid columns), T 64 x G 4 = 8 row blocks, shared packed words, left pad, split
        ("tree-D96-H8_2-T64-leftpad-words", dict(D=96, hq=8, hk=2, T=64, seqlens=(200, 31, 700), leftpad=[3, 16, 0], shared=True,
                                                 packed=True), 4),
        # fp8, H_k 8, 7 x 4 = 28 packed rows: a head per wave (decode_hpw), pages of 256
        ("tree-fp8-hpw-D128-H32_8-T7-page256", dict(D=128, hq=32, hk=8, T=7, seqlens=(700, 17), page=256, fp8=True), 0),
        # fp8, H_k 2: the F8M row blocks (33 x 4 = 132 packed rows, 5 blocks), pages of 16, packed words, split
        ("tree-fp8-f8m-D128-H8_2-T33-page16-words", dict(D=128, hq=8, hk=2, T=33, seqlens=(511, 256), page=16, fp8=True,
                                                         packed=True), 4),
        # tie sinks: the per-element score path of fa_decode_kernel
        ("tree-sinks-D128-H8_2-T7", dict(D=128, hq=8, hk=2, T=7, seqlens=(130, 57, 1), sinks=True), 1),
        ("tree-sinks-D128-H8_2-T33-split", dict(D=128, hq=8, hk=2, T=33, seqlens=(700, 57), sinks=True, packed=True), 4),
        # k=None: the nodes already sit in the cache, pages of 16, 64 x 4 packed rows
        ("tree-noappend-D128-H8_2-T64-page16", dict(D=128, hq=8, hk=2, T=64, seqlens=(130, 57), page=16, append=False), 0),
    ]
    return [(f"{cid}-{variant}", dict(kw, variant=variant, seed=5000 + 10 * i + j), splits)
            for i, (cid, kw, splits) in enumerate(cases) for j, variant in enumerate(("own", "root", "decoy"))]


def _prefix_cases():
    """(id, SharedPrefix kwargs): S_p 1 / 200 / 257, suffixes 0 / 5 / 130, T 1 and 3"""
    cases = [("Sp200-T3-split", dict(T=3, S_p=200, variant="split")),
             ("Sp257-T1-mixed", dict(T=1, S_p=257, variant="mixed")),
             ("Sp1-T3-mixed", dict(T=3, S_p=1, variant="mixed")),
             ("Sp200-T3-mixed-paged", dict(T=3, S_p=200, variant="mixed", layout="paged")),
             ("Sp257-T3-suffix", dict(T=3, S_p=257, variant="suffix")),
             ("Sp200-T1-prefix-noappend", dict(T=1, S_p=200, variant="prefix", append=False)),    # sequence 0: suffix LSE -inf
             ("Sp257-T3-decoy-batch_idx", dict(T=3, S_p=257, variant="decoy", layout="batch_idx")),
             ("Sp200-T1-decoy-paged", dict(T=1, S_p=200, variant="decoy", layout="paged")),
             ("Sp200-T1-split-fp8", dict(T=1, S_p=200, variant="split", fp8=True)),
             ("Sp257-T3-mixed-fp8-paged", dict(T=3, S_p=257, variant="mixed", fp8=True, layout="paged")),
             ("Sp200-T3-split-sinks", dict(T=3, S_p=200, variant="split", sinks=True)),
             ("Sp257-T1-mixed-sinks-D64", dict(T=1, S_p=257, variant="mixed", sinks=True, D=64, hq=4, hk=1))]
    return [("prefix-" + cid, dict(kw, seed=6000 + i)) for i, (cid, kw) in enumerate(cases)]


SINK_DENSE_CASES, SINK_VARLEN_CASES, SINK_KVCACHE_CASES = _sink_dense_cases(), _sink_varlen_cases(), _sink_kvcache_cases()
ROUTE_CASES, TREE_CASES, PREFIX_CASES = _route_cases(), _tree_cases(), _prefix_cases()
