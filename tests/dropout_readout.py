"""Read-out data: attention inputs on which every dropout keep bit of every kernel shows in one output element.

Three separately written kernels replay the Philox keep mask - the forward, the dQ kernel and a dK/dV kernel, which
applies it twice (to P for dV, to dP for dS).  On N(0, 1) data one wrong bit moves a gradient by a fraction of its gate
(tests/test_dropout_readout_cpu.py measures it).  Here Q and K live in disjoint halves of the head dim, so every score
is exactly 0 and P is uniform over a row's visible keys (or exactly the ALiBi profile), and the other tensors are
one-hot: each output element is ONE term rp keep_ij P_ij of the sum it belongs to.  Pure numpy on the CPU; the GPU tests
(tests/test_dropout_readout_gpu.py) feed it to the kernels.

h = D // 2 (D the caller's head dim).  A pass is one (batch, head) slice.  The dense mask has no batch or head term and
the varlen mask no head term, so passes ride on the batch dimension of a dense call and on the head dimension of a varlen
call, and one launch reads the whole mask.

Call A, the dS paths.  Pass t lights query rows [t h, (t + 1) h) with Q_i = e_{i - t h} and key columns [t h, (t + 1) h)
with K_j = e_{h + j - t h}; V = 1, dO_i = e_0 for every row, so dP_ij = 1 and dS_ij = P_ij (rp keep_ij - D_i) scale:
    dQ_i[h + d] = dS_{i, t h + d}     every row i        - the dQ kernel's mask
    dK_j[d]     = dS_{t h + d, j}     every column j     - the dK/dV kernel's dS-side mask
A row with ONE visible key has P = 1 and D_i = rp keep, so its dS is 0 whatever the bit is: there the dS channels show
only a forward / backward disagreement, the bit itself is read by call B.

Call B, the P paths.  Pass t has dO_i = e_{i - t D} on rows [t D, (t + 1) D) and V_j = e_{j - t D} on columns
[t D, (t + 1) D) (Q and K as in call A):
    O_i[d]  = rp keep P at (i, t D + d)     - the bits multiplied into P V (and they must be the bits written to dmask)
    dV_j[d] = rp keep P at (t D + d, j)     - the dK/dV kernel's P-side mask

All inputs are 0 or 1, exact in fp16 and bf16, so one reference serves both io types.  With GQA every query head of a
group carries the same data: dK and dV are group x the level, and a head-dependent mistake lands between levels.

Decoder.  The reference of every read-out element comes from oracle.attn_bwd / varlen_bwd with the true mask (fed the
oracle's own unrounded forward).  Flipping that element's own bit moves it by delta_ij = rp P_ij c_ij (c: 1 for O and
dV, dP_ij scale = scale for the dS channels, summed over the query heads of a group for dK and dV); the gate is a
quarter of that, derived from the oracle alone.  decode() returns, per channel, the mask the kernel output implies
(nearer the keep level or the drop level) and the worst |got - ref| / gate.
"""
import contextlib

import numpy as np

import oracle
import oracle.attention as _oa
import oracle.varlen as _ov

SEED = 20261020
CHANNELS = {"A": ("dq", "dk"), "B": ("o", "dv")}


@contextlib.contextmanager
def flipped(elem):
    """Inside, the oracle's dense and varlen entry points see the keep mask with ONE bit flipped: elem = (first query row of
    the sequence - 0 in a dense call -, i, j); None changes nothing.  How the CPU tests make a forward-only or a
    backward-only mistake."""
    true = oracle.dropout_keep_mask

    def bad(seed, offset, p_dropout, rows, n_cols, row0=0, col0=0, n_glob=None):
        m = true(seed, offset, p_dropout, rows, n_cols, row0=row0, col0=col0, n_glob=n_glob)
        if elem is not None and row0 == elem[0]:
            m[elem[1], elem[2]] ^= True
        return m

    _oa.dropout_keep_mask = _ov.dropout_keep_mask = bad
    try:
        yield
    finally:
        _oa.dropout_keep_mask = _ov.dropout_keep_mask = true


class Case:
    """One read-out case.  Dense: Sq x Sk, `heads` query heads (all with the same data) over heads // group kv heads.
    Varlen (lens_q given): passes ride on the kv heads, each with `group` query heads; max_seqlen_k = max(lens_k) +
    extra_k.  alibi: None, 'H' (slopes [Hq]) or 'BH' (slopes [B, Hq]); every slope is at most 2^-7."""

    def __init__(self, name, D, Sq=None, Sk=None, causal=False, window=(-1, -1), p=0.25, heads=2, group=1, alibi=None,
                 lens_q=None, lens_k=None, extra_k=0, offset=None):
        self.name, self.D, self.h, self.p = name, D, D // 2, p
        self.causal, self.window, self.group, self.alibi = causal, tuple(window), group, alibi
        self.varlen = lens_q is not None
        self.offset = offset                                       # generator offset forced before each call (counter carry)
        if self.varlen:
            self.lens_q, self.lens_k = list(lens_q), list(lens_k)
            self.cu_q = np.concatenate([[0], np.cumsum(lens_q)]).astype(np.int32)
            self.cu_k = np.concatenate([[0], np.cumsum(lens_k)]).astype(np.int32)
            self.max_q, self.max_k = max(lens_q), max(lens_k) + extra_k
            self.Sq, self.Sk = max(lens_q), max(lens_k)
        else:
            self.Sq, self.Sk, self.heads = Sq, Sk, heads
            assert heads % group == 0
        self.scale = D ** -0.5
        self.rp = 1.0 / (1.0 - p)

    def __repr__(self):
        return self.name

    # ---- geometry
    def width(self, call):
        return self.h if call == "A" else self.D

    def passes(self, call):
        w = self.width(call)
        return max(-(-self.Sq // w), -(-self.Sk // w), 1)

    def dims(self, call):
        """(batch, Hq, Hk) of the call"""
        n = self.passes(call)
        if self.varlen:
            return len(self.lens_q), n * self.group, n
        return n, self.heads, self.heads // self.group

    def slopes(self, call):
        """fp32 ALiBi slopes ([Hq] or [B, Hq]) or None: 2^-7 / (1, 2, 3, 1, ...), different in neighbouring heads"""
        if self.alibi is None:
            return None
        B, Hq, _ = self.dims(call)
        if self.alibi == "H":
            return np.array([2.0 ** -7 / (1 + hq % 3) for hq in range(Hq)], dtype=np.float32)
        return np.array([[2.0 ** -7 / (1 + (b + hq) % 3) for hq in range(Hq)] for b in range(B)], dtype=np.float32)

    def seqs(self):
        """(q0, sq, k0, sk) per sequence; a dense case is one sequence"""
        if not self.varlen:
            return [(0, self.Sq, 0, self.Sk)]
        return [(int(self.cu_q[b]), self.lens_q[b], int(self.cu_k[b]), self.lens_k[b]) for b in range(len(self.lens_q))]

    def flags(self):
        """(causal, wl, wr) as the oracle's entry points normalise them (varlen: by the maximal lengths)"""
        sq, sk = (self.max_q, self.max_k) if self.varlen else (self.Sq, self.Sk)
        return oracle.normalize_flags(sq, sk, self.causal, self.window[0], self.window[1], self.alibi is not None)

    def visible(self):
        """[sq, sk] bool per sequence"""
        c, wl, wr = self.flags()
        return [_oa.visible_mask(sq, sk, c, wl, wr) for _, sq, _, sk in self.seqs()]

    def expected(self, seed, offset):
        """oracle.dropout_keep_mask AND visible, [sq, sk] per sequence: what every channel must read"""
        out = []
        for (q0, sq, _, sk), vis in zip(self.seqs(), self.visible()):
            n_glob = self.max_k if self.varlen else None
            out.append(oracle.dropout_keep_mask(seed, offset, self.p, sq, sk, row0=q0, n_glob=n_glob) & vis)
        return out

    # ---- inputs
    def build(self, call):
        """dict of fp64 q, k, v, do in the op's layout: dense [B, S, H, D], varlen [T, H, D]"""
        B, Hq, Hk = self.dims(call)
        D, h, w = self.D, self.h, self.width(call)
        if self.varlen:
            Tq, Tk = int(self.cu_q[-1]), int(self.cu_k[-1])
            q, do = np.zeros((Tq, Hq, D)), np.zeros((Tq, Hq, D))
            k, v = np.zeros((Tk, Hk, D)), np.zeros((Tk, Hk, D))
        else:
            q, do = np.zeros((B, self.Sq, Hq, D)), np.zeros((B, self.Sq, Hq, D))
            k, v = np.zeros((B, self.Sk, Hk, D)), np.zeros((B, self.Sk, Hk, D))
        if call == "A":
            v[...] = 1.0
            do[..., 0] = 1.0
        G = self.group

        def light(x, t, off, n, width, d0, heads):
            """x[row, :, d0 + row - t width] = 1 for the rows [t width, (t + 1) width) below n of pass t"""
            r = np.arange(t * width, min((t + 1) * width, n))
            if self.varlen:                                        # pass t: kv head t and its G query heads
                x[off + r, heads, d0 + r - t * width] = 1.0
            else:                                                  # pass t: batch t, every head
                x[t, r, :, d0 + r - t * width] = 1.0

        for t in range(self.passes(call)):
            for q0, sq, k0, sk in self.seqs():
                for r in range(G if self.varlen else 1):
                    light(q, t, q0, sq, h, 0, t * G + r)
                    if call == "B":
                        light(do, t, q0, sq, w, 0, t * G + r)
                light(k, t, k0, sk, h, h, t)
                if call == "B":
                    light(v, t, k0, sk, w, 0, t)
        return {"q": q, "k": k, "v": v, "do": do}

    # ---- the oracle
    def oracle_kw(self, call, seed, offset):
        s = self.slopes(call)
        return dict(causal=self.causal, window=self.window, alibi_slopes=None if s is None else s.astype(np.float64),
                    dropout_p=self.p, seed=seed, offset=offset)

    def reference(self, call, seed, offset, o_dtype=None, flip_fwd=None, flip_bwd=None):
        """dict o, lse, dq, dk, dv (fp64, the op's layout) from the oracle with the true mask.  o_dtype: the io type the
        SAVED O is rounded to before the backward (None: unrounded - the reference of the decoder).  flip_fwd / flip_bwd
        = (sequence, i, j): the forward / the backward sees that bit flipped (the CPU tests' mistakes)."""
        x = self.build(call)
        kw = self.oracle_kw(call, seed, offset)
        el = lambda f: None if f is None else (self.seqs()[f[0]][0], f[1], f[2])
        if self.varlen:
            with flipped(el(flip_fwd)):
                o, lse = oracle.varlen_fwd(x["q"], x["k"], x["v"], self.cu_q, self.cu_k, self.max_q, self.max_k, self.scale,
                                           **kw)
            with flipped(el(flip_bwd)):
                g = oracle.varlen_bwd(x["do"], x["q"], x["k"], x["v"], oracle.round_to(o, o_dtype), lse.astype(np.float64),
                                      self.cu_q, self.cu_k, self.max_q, self.max_k, self.scale, **kw)
            return {"o": o, "lse": lse, "dq": g[0], "dk": g[1], "dv": g[2]}
        t = lambda a: a.transpose(0, 2, 1, 3)
        with flipped(el(flip_fwd)):
            o, lse, _ = oracle.attn_fwd(t(x["q"]), t(x["k"]), t(x["v"]), self.scale, **kw)
        with flipped(el(flip_bwd)):
            g = oracle.attn_bwd(t(x["do"]), t(x["q"]), t(x["k"]), t(x["v"]), oracle.round_to(o, o_dtype),
                                lse.astype(np.float64), self.scale, **kw)
        return {"o": t(o), "lse": lse, "dq": t(g[0]), "dk": t(g[1]), "dv": t(g[2])}

    def probs(self, call):
        """P [B, Hq, sq, sk] per sequence (dense: one entry), restated from the oracle's score_matrix on zero scores:
        uniform over the visible keys, or the ALiBi profile.  (tests/test_dropout_readout_cpu.py holds it to the oracle's
        own return_p.)"""
        B, Hq, _ = self.dims(call)
        c, wl, wr = self.flags()
        s = self.slopes(call)
        out = []
        for b, (_, sq, _, sk) in enumerate(self.seqs()):
            nb = 1 if self.varlen else B
            P = np.zeros((nb, Hq, sq, sk))
            for bb in range(nb):
                for hq in range(Hq):
                    sl = None if s is None else float(s[hq] if s.ndim == 1 else s[b if self.varlen else bb, hq])
                    if sq == 0 or sk == 0:
                        continue
                    sc, vis = _oa.score_matrix(np.zeros((sq, 1)), np.zeros((sk, 1)), 1.0, c, wl, wr, 0.0, sl)
                    m = np.max(sc, axis=1, keepdims=True)
                    e = np.where(vis, np.exp(sc - np.where(np.isfinite(m), m, 0.0)), 0.0)
                    l = e.sum(axis=1, keepdims=True)
                    P[bb, hq] = np.where(l > 0, e / np.where(l > 0, l, 1.0), 0.0)
            out.append(P)
        return out

    # ---- the read-out
    def gather(self, ch, x):
        """The elements of tensor x (o / dq: query layout, dk / dv: key layout) that read the mask, as [R, sq, sk] per
        sequence: R readings of every (i, j) - the query heads (dense o, dq), the kv heads (dense dk, dv), the query heads
        of the pass's group (varlen o, dq) or one (varlen dk, dv)."""
        w = self.D if ch in ("o", "dv") else self.h
        base = self.h if ch == "dq" else 0
        out = []
        for q0, sq, k0, sk in self.seqs():
            i, j = np.arange(sq)[:, None], np.arange(sk)[None, :]
            i, j = np.broadcast_arrays(i, j)
            if ch in ("o", "dq"):
                t, row, d = j // w, i, base + j % w                # pass from the column, one row of x per query
            else:
                t, row, d = i // w, j, i % w                       # pass from the row, one row of x per key
            if self.varlen:
                off, R = (q0, self.group) if ch in ("o", "dq") else (k0, 1)      # pass t: kv head t, query heads t R + r
                out.append(np.stack([x[off + row, t * R + r, d] for r in range(R)]) if sq and sk else np.zeros((R, sq, sk)))
            else:
                out.append(np.stack([x[t, row, r, d] for r in range(x.shape[2])]))
        return out

    def delta(self, ch, call):
        """What flipping element (i, j)'s own bit does to its read-out element: rp P_ij c_ij, in the layout of gather()"""
        w = self.width(call)
        c = self.rp * (self.scale if call == "A" else 1.0)
        out = []
        for (q0, sq, k0, sk), P in zip(self.seqs(), self.probs(call)):
            i, j = np.broadcast_arrays(np.arange(sq)[:, None], np.arange(sk)[None, :])
            t = j // w if ch in ("o", "dq") else i // w
            G = self.group
            if self.varlen:                                        # P [1, Hq, sq, sk], pass t = kv head t
                if ch in ("o", "dq"):
                    d = np.stack([P[0, t * G + r, i, j] for r in range(G)]) if sq and sk else np.zeros((G, sq, sk))
                else:
                    d = sum(P[0, t * G + r, i, j] for r in range(G))[None] if sq and sk else np.zeros((1, sq, sk))
            else:                                                  # P [B, Hq, sq, sk], pass t = batch t
                Hq = P.shape[1]
                if ch in ("o", "dq"):
                    d = np.stack([P[t, hq, i, j] for hq in range(Hq)])
                else:
                    d = np.stack([sum(P[t, hk * G + r, i, j] for r in range(G)) for hk in range(Hq // G)])
            out.append(c * d)
        return out

    def decode(self, call, ref, got, keep, ignore=()):
        """ref / got: dicts of fp64 tensors in the op's layout; keep: expected() for the call's (seed, offset).
        Returns {channel: (implied, worst, at)}: implied - the keep mask [R, sq, sk] per sequence each reading implies
        (the expected value where nothing is visible); worst - the largest |got - ref| / gate over the visible elements;
        at - (sequence, reading, i, j) of the worst.  `ignore`: channels to leave out (the sensitivity tests' control)."""
        res = {}
        vis = self.visible()
        for ch in CHANNELS[call]:
            if ch in ignore:
                continue
            implied, worst, at = [], 0.0, None
            for b, (g, r, dl) in enumerate(zip(self.gather(ch, got[ch]), self.gather(ch, ref[ch]), self.delta(ch, call))):
                k, v = keep[b][None], vis[b][None]
                lvl_keep = r + np.where(k, 0.0, dl)                # the element had the bit been 1 / 0
                lvl_drop = r - np.where(k, dl, 0.0)
                imp = np.abs(g - lvl_keep) < np.abs(g - lvl_drop)
                implied.append(np.where(v, imp, k))
                ratio = np.where(v, np.abs(g - r) / np.where(v, dl / 4, 1.0), 0.0)
                if ratio.size and ratio.max() > worst:
                    worst = float(ratio.max())
                    at = (b, *(int(a) for a in np.unravel_index(ratio.argmax(), ratio.shape)))
            res[ch] = (implied, worst, at)
        return res


def wrong_bits(implied, keep):
    """[(sequence, reading, i, j)] where a channel's implied mask differs from the expected one"""
    out = []
    for b, (imp, k) in enumerate(zip(implied, keep)):
        out += [(b, int(r), int(i), int(j)) for r, i, j in np.argwhere(imp != k[None])]
    return out


# ------------------------------------------------------------------------------------------------ the cases
# Shapes: the smallest that cross more than one 128-row query block and more than one key block, ragged tails,
# Sk % 4 in {1, 2, 3} (dropout_keep4's two-counter path) and Sk < 4.
LQ, LK = [70, 0, 5, 130], [33, 7, 131, 64]

DENSE = [
    Case("d32_70x50_causal", 32, 70, 50, causal=True, p=0.25),                 # pads to 64; rows 0..19 see nothing
    Case("d64_200x200_causal", 64, 200, 200, causal=True, p=0.1),
    Case("d64_130x203_full", 64, 130, 203, p=0.25),
    Case("d64_9x3_full", 64, 9, 3, p=0.5),
    Case("d96_130x131_win40_7", 96, 130, 131, window=(40, 7), p=0.25),
    Case("d128_96x130_causal", 128, 96, 130, causal=True, p=0.5),
    Case("d128_257x259_causal", 128, 257, 259, causal=True, p=0.1),
    Case("d128_129x66_win20_0", 128, 129, 66, window=(20, 0), p=0.3),
    Case("d160_130x131_causal", 160, 130, 131, causal=True, p=0.25),
    Case("d192_130x131_causal", 192, 130, 131, causal=True, p=0.25),
    Case("d256_130x203_causal", 256, 130, 203, causal=True, p=0.3),
    Case("d256_257x65_full", 256, 257, 65, p=0.1),
]
ALIBI = [Case(f"alibi_d{D}_130x131_{'causal' if c else 'full'}", D, 130, 131, causal=c, p=0.25, alibi="H")
         for D in (64, 128, 256) for c in (True, False)] + [
    Case("alibi_bh_d128_130x131_causal", 128, 130, 131, causal=True, p=0.25, alibi="BH"),
    # the narrow instantiations with a bias (head dims 96 and 160 run the D 128 / D 256 kernels with DV 96 / 192)
    Case("alibi_d96_130x131_causal", 96, 130, 131, causal=True, p=0.25, alibi="H"),
    Case("alibi_d160_130x131_full", 160, 130, 131, p=0.25, alibi="H"),
]
GQA = [
    Case("gqa4_d64_200x200_causal", 64, 200, 200, causal=True, p=0.1, heads=4, group=4),
    Case("gqa4_d64_130x203_full", 64, 130, 203, p=0.25, heads=4, group=4),
    Case("mqa8_d64_200x200_causal", 64, 200, 200, causal=True, p=0.1, heads=8, group=8),
    Case("mqa8_d64_130x203_full", 64, 130, 203, p=0.25, heads=8, group=8),
    Case("gqa4_d128_96x130_causal", 128, 96, 130, causal=True, p=0.5, heads=4, group=4),
    Case("gqa4_d128_129x66_win20_0", 128, 129, 66, window=(20, 0), p=0.3, heads=4, group=4),
    Case("mqa8_d128_257x259_causal", 128, 257, 259, causal=True, p=0.1, heads=8, group=8),
    Case("mqa8_d128_129x66_full", 128, 129, 66, p=0.3, heads=8, group=8),
]
# offset + (flat >> 2) crosses 2^32 at flat = 256, inside the second row
CARRY = [
    Case("carry_d64_130x203_full", 64, 130, 203, p=0.25, offset=2 ** 32 - 64),
    Case("carry_d128_96x130_causal", 128, 96, 130, causal=True, p=0.5, offset=2 ** 32 - 64),
]
VARLEN = [Case(f"varlen_d{D}_{'causal' if c else 'full'}", D, causal=c, p=0.25, lens_q=LQ, lens_k=LK)
          for D in (64, 128, 256) for c in (True, False)] + [
    Case("varlen_gqa2_d64_causal", 64, causal=True, p=0.25, lens_q=LQ, lens_k=LK, group=2),
    Case("varlen_alibi_d128_causal", 128, causal=True, p=0.25, lens_q=LQ, lens_k=LK, alibi="H"),
    Case("varlen_maxk_d64_causal", 64, causal=True, p=0.25, lens_q=LQ, lens_k=LK, extra_k=6),   # N_glob = 137, odd
    Case("varlen_maxk_d128_full", 128, p=0.25, lens_q=LQ, lens_k=LK, extra_k=29),
]
CASES = DENSE + ALIBI + GQA + CARRY + VARLEN
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FAMILY = {c.name: f for f, cs in (("dense", DENSE), ("alibi", ALIBI), ("gqa", GQA), ("carry", CARRY), ("varlen", VARLEN))
          for c in cs}


def offsets(case):
    """(offset of call A, offset of call B) after torch.manual_seed: a call advances the generator by batch x Hq x 32"""
    if case.offset is not None:
        return case.offset, case.offset
    B, Hq, _ = case.dims("A")
    return 0, B * Hq * 32
