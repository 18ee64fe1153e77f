"""The fp64 / exact-integer restatement of the five fa_moe_* ops (flash_attn_mi355.moe, csrc/fa_moe.hip) and the error bounds
the GPU tests hold the kernels to.  A plain helper module, like act_mul_ref.py: no fixtures, no pytest settings; numpy only.

Every function takes the values the kernel sees (16-bit inputs already widened) as float64 arrays.  `variant` builds a
deliberately WRONG reference - tests/test_moe_cpu.py shows that the checks tell each of them from the right one:
    "tie_high"         the highest index wins a tie            (route)
    "bias_in_weight"   the sigmoid weight keeps the bias       (route)
    "unstable"         a segment's slots descend               (sort)
    "pad_in_pos"       pos ignores the alignment padding       (sort)
    "dw_from_w"        dw is taken from w instead of dout . y  (combine backward)

Bounds.  u = 2^-24 is the unit roundoff of fp32; the hardware exp2 (v_exp_f32) and reciprocal (v_rcp_f32) are taken as 1 ulp =
2 u relative (the ISA's stated accuracy); IEEE divisions, products, sums and fma round once, u.  Counting first-order terms:
    e(t) = exp2(t * log2e), t = c - m      (t: u, log2e: u, product: u) scaled by |t|, then the hardware: (2 + 3 |t|) u
    sig(l) = rcp(1 + exp2(-l * log2e))     exp2: (2 + 2 |l|) u, times e / (1 + e) <= 1; the sum u; the reciprocal 2 u: (5 + 2 |l|) u
    a sum of n positive terms              the terms' own error + (n - 1) u      (any order)
    softmax, renormalised                  w = e / S * scale:   2 (2 + 3 tmax) + (K - 1) + 2           = (K + 5 + 6 tmax) u
    softmax over all E                     Z: at most 7 + 6 additions deep: (2 + 3 tmax) + 13;  w: (2 (2 + 3 tmax) + 15) u
    sigmoid                                w = s * scale: (6 + 2 lmax) u;   renormalised: 2 (5 + 2 lmax) + (K - 1) + 2 = (K + 11 + 4 lmax) u
each times |w_ref|, widened by 2^-10 for the second-order terms, plus 2^-126 (results below the normal range may be flushed).
tmax / lmax are the row's own (over the columns that enter)."""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
TINY = 2.0 ** -126


def widen(t):
    """a torch tensor's values as float64 numpy"""
    return t.detach().double().cpu().numpy()


def _sigmoid(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def route_scores(logits, scoring, bias):
    """(z, s, c): sanitised logits (softmax), sigmoid values, selection scores with NaN -> -inf"""
    logits = np.asarray(logits, dtype=np.float64)
    if scoring == "softmax":
        z = np.where(np.isnan(logits), -np.inf, logits)
        return z, None, z
    s = _sigmoid(logits)
    c = s if bias is None else s + np.asarray(bias, dtype=np.float64)[None, :]
    return None, s, np.where(np.isnan(c), -np.inf, c)


def route_ref(logits, k, *, scoring="softmax", renormalize=True, bias=None, scale=1.0, variant=None):
    """(weights f64 [T, K], ids int32 [T, K], gap f64 [T]).  gap: the smallest difference between consecutive scores among the
    row's first K + 1 - the K-th against the (K+1)-th, and the winners among themselves, whose order the slots record: the
    margin by which the selection is decisive."""
    z, s, c = route_scores(logits, scoring, bias)
    T, E = c.shape
    if variant == "tie_high":
        order = (E - 1 - np.argsort(-c[:, ::-1], axis=1, kind="stable"))
    else:
        order = np.argsort(-c, axis=1, kind="stable")           # stable: the lowest index among equals (-0 == +0)
    ids = order[:, :k].astype(np.int32)
    rows = np.arange(T)[:, None]
    csel = c[rows, ids]
    with np.errstate(invalid="ignore"):
        top = c[rows, order[:, :min(k + 1, E)]]
        gap = (top[:, :-1] - top[:, 1:]).min(1) if top.shape[1] > 1 else np.full(T, np.inf)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if scoring == "softmax":
            m = csel[:, :1]
            e = np.exp(csel - m)
            den = e.sum(1, keepdims=True) if renormalize else np.exp(z - m).sum(1, keepdims=True)
            w = e / den
        else:
            w = (c if variant == "bias_in_weight" else s)[rows, ids]
            if renormalize:
                w = w / w.sum(1, keepdims=True)
        w = w * scale
    return w, ids, gap


def route_weight_bound(logits, w_ref, ids, *, scoring, renormalize, bias=None):
    """the bound of the module docstring on |w - w_ref|, [T, K]"""
    z, s, c = route_scores(logits, scoring, bias)
    T, K = ids.shape
    rows = np.arange(T)[:, None]
    fin = lambda t: np.where(np.isfinite(t), np.abs(t), 0.0)      # noqa: E731  (an infinite argument gives an exact 0 / 1 / inf)
    with np.errstate(invalid="ignore"):
        if scoring == "softmax":
            m = c[rows, ids[:, :1]]
            if renormalize:
                steps = K + 5 + 6 * fin(c[rows, ids] - m).max(1, keepdims=True)
            else:
                steps = 2 * (2 + 3 * fin(z - m).max(1, keepdims=True)) + 15
        else:
            lmax = fin(np.asarray(logits, dtype=np.float64)[rows, ids]).max(1, keepdims=True)
            steps = (K + 11 + 4 * lmax) if renormalize else (6 + 2 * lmax)
    return steps * U * np.abs(w_ref) * SLACK + TINY


def route_bwd_ref(dw, logits, ids, *, scoring="softmax", renormalize=True, bias=None, scale=1.0, with_bound=False, io="float32"):
    """dlogits f64 [T, E] by the formulas of flash_attn_mi355.moe.  with_bound: (dlogits, bound) - the first-order error of the
    kernel's fp32 evaluation (the weights' bound above, one u per further operation, K + 1 per fma chain) plus the rounding to
    the io type `io` ("bfloat16", "float16", "float32"): half an ulp at the value - absolute below the normal range, where
    fp16's small gradients live."""
    logits = np.asarray(logits, dtype=np.float64)
    dw = np.asarray(dw, dtype=np.float64)
    z, s, c = route_scores(logits, scoring, bias)
    T, E = logits.shape
    K = ids.shape[1]
    rows = np.arange(T)[:, None]
    w, _, _ = route_ref(logits, K, scoring=scoring, renormalize=renormalize, bias=bias, scale=1.0)
    relw = route_weight_bound(logits, w, ids, scoring=scoring, renormalize=renormalize, bias=bias) / np.maximum(np.abs(w), TINY)
    out = np.zeros((T, E))
    err = np.zeros((T, E))
    if scoring == "softmax":
        g = dw * scale
        D = (g * w).sum(1, keepdims=True)
        A = np.abs(g * w).sum(1, keepdims=True)
        errD = A * (relw.max(1, keepdims=True) + (K + 1) * U)
        if renormalize:
            val = w * (g - D)
            e = np.abs(w) * (np.abs(g) * U + errD + U * np.abs(g - D)) + np.abs(val) * (relw + U)
            out[rows, ids] = val
            err[rows, ids] = e
        else:
            m = c[rows, ids[:, :1]]
            with np.errstate(over="ignore", invalid="ignore"):
                p = np.exp(z - m)
                p = p / p.sum(1, keepdims=True)
            gj = np.zeros((T, E))
            gj[rows, ids] = g
            out = p * (gj - D)
            rp = relw.max(1, keepdims=True)
            err = np.abs(p) * (np.abs(gj) * U + errD + U * np.abs(gj - D)) + np.abs(out) * (rp + U)
    else:
        ssel = s[rows, ids]
        lmax = np.abs(logits[rows, ids])
        rels = (5 + 2 * lmax) * U
        if renormalize:
            S = ssel.sum(1, keepdims=True)
            D = (dw * w).sum(1, keepdims=True)
            A = np.abs(dw * w).sum(1, keepdims=True)
            errD = A * (relw.max(1, keepdims=True) + (K + 1) * U)
            ds = (dw - D) * scale / S
            relS = rels.max(1, keepdims=True) + (K - 1) * U
            eds = (errD + U * np.abs(dw - D)) * np.abs(scale / S) + np.abs(ds) * (3 * U + relS)
        else:
            ds = dw * scale
            eds = np.abs(ds) * U
        val = ds * ssel * (1 - ssel)
        e1s = np.abs(ssel) * rels + U * np.abs(1 - ssel)
        e = eds * np.abs(ssel * (1 - ssel)) + np.abs(val) * (rels + 2 * U) + np.abs(ds * ssel) * e1s
        out[rows, ids] = val
        err[rows, ids] = e
    if not with_bound:
        return out
    err = err * SLACK
    return out, err + half_ulp(np.abs(out) + err, io) + TINY


def sort_ref(ids, num_experts, *, align=1, variant=None):
    """(sorted_slot int32 [M_max], pos int32 [T, K], expert_offsets int32 [E + 1]): exact integers"""
    ids = np.asarray(ids)
    T, K = ids.shape
    E = num_experts
    flat = ids.reshape(-1).astype(np.int64)
    M = T * K + E * (align - 1)
    sorted_slot = np.full(M, -1, dtype=np.int32)
    pos = np.full(T * K, -1, dtype=np.int32)
    offsets = np.zeros(E + 1, dtype=np.int32)
    at = unpadded = 0
    for e in range(E):
        offsets[e] = at
        slots = np.nonzero(flat == e)[0]
        if variant == "unstable":
            slots = slots[::-1]
        sorted_slot[at:at + len(slots)] = slots
        pos[slots] = (unpadded if variant == "pad_in_pos" else at) + np.arange(len(slots))
        unpadded += len(slots)
        at += (len(slots) + align - 1) // align * align
    offsets[E] = at
    return sorted_slot, pos.reshape(T, K), offsets


def permute_ref(x, sorted_slot, k, scale=None):
    """xp f64 [M_max, N]: the copy, or the exact product scale[slot] * x[slot // k] (the kernel rounds it once); padding rows 0"""
    x = np.asarray(x, dtype=np.float64)
    sorted_slot = np.asarray(sorted_slot)
    out = np.zeros((len(sorted_slot), x.shape[1]))
    live = sorted_slot >= 0
    s = sorted_slot[live].astype(np.int64)
    rows = x[s // k]
    if scale is not None:
        rows = rows * np.asarray(scale, dtype=np.float64).reshape(-1)[s][:, None]
    out[live] = rows
    return out


def combine_ref(y, weights, pos):
    """(out f64 [T, N], mag f64 [T, N]): sum_k w y over the live slots and sum_k |w y| (what enters the sum); the kernel's
    error is at most 0.5 ulp16 of the result + K 2^-24 mag (K fma, one u each on a partial sum bounded by mag)"""
    y = np.asarray(y, dtype=np.float64)
    pos = np.asarray(pos)
    T, K = pos.shape
    w = np.ones((T, K)) if weights is None else np.asarray(weights, dtype=np.float64)
    out = np.zeros((T, y.shape[1]))
    mag = np.zeros((T, y.shape[1]))
    for k in range(K):
        live = pos[:, k] >= 0
        term = w[live, k][:, None] * y[pos[live, k]]
        out[live] += term
        mag[live] += np.abs(term)
    return out, mag


def combine_bwd_ref(dout, y, weights, pos, *, variant=None):
    """(dy f64 [M, N] - the exact products w dout, padding rows 0 -, dw f64 [T, K], mag f64 [T, K] = sum_n |dout y|).  The
    kernel's dw is a sum of n products in fa_rowsum.h's order - at most 8 fma in a lane, 7 additions of a lane's pieces, 6
    butterfly stages, 3 additions over the waves: 24 roundings deep - so |dw - dw_ref| <= 24 2^-24 mag (+ the 2^-10 widening)."""
    dout = np.asarray(dout, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    pos = np.asarray(pos)
    T, K = pos.shape
    dy = np.zeros_like(y)
    dw = np.zeros((T, K))
    mag = np.zeros((T, K))
    for k in range(K):
        live = pos[:, k] >= 0
        p = pos[live, k]
        dy[p] = w[live, k][:, None] * dout[live]
        prod = dout[live] * y[p]
        dw[live, k] = w[live, k] if variant == "dw_from_w" else prod.sum(1)
        mag[live, k] = np.abs(prod).sum(1)
    return dy, dw, mag


DW_DEPTH = 24


def half_ulp(x, dtype_name):
    """half an ulp of the io type at |x|: fp32 relative (2^-24 of the value at the most), the 16-bit types by half_ulp16"""
    return np.abs(x) * U if dtype_name == "float32" else half_ulp16(x, dtype_name)


def half_ulp16(x, dtype_name):
    """half an ulp of the 16-bit type at |x| (normal range), elementwise: bf16 has 8 significand bits, fp16 11"""
    bits = 8 if dtype_name == "bfloat16" else 11
    ax = np.maximum(np.abs(x), 2.0 ** (-126 if dtype_name == "bfloat16" else -14))
    return 2.0 ** (np.floor(np.log2(ax)) - bits)


LADDER = (np.arange(512) - 256) / 128.0                      # 512 logits in [-2, 2): exact in bf16, fp16 and fp32
DECISIVE_GAP = 1e-4


def decisive_logits(T, E, k, seed):
    """(logits f32 [T, E], bias f32 [E]) for sigmoid scoring with a bias, where a hardware exp2 / rcp could otherwise turn a
    near-tie: seeded and decisive by construction.  A row's logits are E distinct rungs of LADDER - exact in every io dtype,
    their sigmoids at least 8e-4 apart -, the bias is -0.25, 0 or 0.25 per expert (large enough to change who wins), and a
    row whose first k + 1 scores come closer than 2e-4 to each other is drawn again.  test_moe_cpu.py asserts the gap of every
    row for every (seed, shape) the GPU tests use."""
    rng = np.random.default_rng(seed)
    bias = (rng.integers(-1, 2, size=E) * 0.25).astype(np.float32)
    logits = np.empty((T, E), dtype=np.float32)
    for t in range(T):
        for _ in range(1000):
            row = LADDER[rng.permutation(512)[:E]]
            c = np.sort(_sigmoid(row) + bias)[::-1][:k + 1]
            if len(c) < 2 or (c[:-1] - c[1:]).min() > 2 * DECISIVE_GAP:
                break
        else:
            raise AssertionError("no decisive row found")
        logits[t] = row
    return logits, bias


# the router shapes of the GPU tests, (T, E, K): every G = 1, 2, .. 64 lanes per row (E = 8, 16, 32, 60 / 64, 128, 256, 384 / 512),
# a ragged last lane (60) and a ragged last lane group (384), K = 1 and K = E, one row, and more rows than a workgroup holds
ROUTE_SHAPES = [(1, 8, 1), (3, 8, 2), (67, 8, 8), (67, 16, 16), (67, 32, 2), (67, 60, 6), (67, 64, 8), (300, 128, 8), (67, 256, 8),
                (67, 384, 8), (67, 512, 16), (3, 512, 1)]


def route_seed(T, E, K):
    return 1000 + ROUTE_SHAPES.index((T, E, K))
