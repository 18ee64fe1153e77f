"""The fp64 restatement of fa_moe_gemm_wgrad (flash_attn_mi355.moe.moe_gemm_wgrad, csrc/fa_moe_gemm_wgrad.hip), the witness data
its GPU tests compare bit for bit, and the bounds they hold random data to.  A plain helper module, like moe_gemm_ref.py, whose
`witness`, `offsets_of`, `round16` and `gather_ref` it reuses: no fixtures, numpy only.

    dW_e[n, k]  = sum_r dy[r, n] a_r[k]   (+ the old dw with accumulate)     r in [expert_offsets[e], expert_offsets[e + 1])
    dbias[e, n] = sum_r dy[r, n]
    an empty expert: 0 (with accumulate: the old dw)
    offsets clamped to [0, rows]; a_r = x[r], or with sorted_slot: moe_gemm_ref.gather_ref's row (a slot of -1: zeros)
    "nk": dw [E, N, K];  "kn": dw [E, K, N]

`variant` builds a deliberately WRONG reference - tests/test_moe_gemm_wgrad_cpu.py shows that the witness data tell each from
the right one in elements the right one owns:
    "read_past_end"       the last MFMA step of 16 rows is read whole: rows behind the segment's end, the next segment's, enter
    "drop_row_tail"       rows behind the segment's last multiple of 64 are dropped
    "start_rounded_down"  the segment's start is rounded down to a multiple of 16
    "kn_as_nk"            a "kn" gradient written in "nk" order (N = K: the shapes agree)
    "no_accumulate"       `old` ignored
    (a padding slot read as token 0: moe_gemm_ref.gather_ref(variant="pad_as_token0"))

Witness data (`witness`): dy and x hold integers in [-3, 3], exact in fp16 and bf16.  Every product is an integer of magnitude
<= 9 and every partial sum of any subset in any order an integer of magnitude <= 9 L < 2^24 for a segment of L rows - exact in
fp32 whatever order the hardware adds in - and below both 16-bit types' largest finite number (65504) for L <= 2880.  So dw must
be round_out(exact sum): no tolerance (`witness_is_exact` checks the inequalities on the data).  The first four columns of dy and
of x are positive, so those sums grow like 4 L, past the integers the 16-bit types hold exactly (256 in bf16 from L = 129, 2048
in fp16 at L = 2880): the ONE rounding shows.  dbias' sums grow like 2 L and pass both at L = 2880.

Random data (`bound`): |got - ref| <= 0.5 ulp_out + (L + 2) 2^-23 sum_r |dy a|, the forward's form with the segment length L in
the place of K.  It rests on the same assumption, which could not be sourced: every addition inside the MFMA and along the
accumulator chain errs by at most one fp32 ulp.  The GPU tests print the share they measure.  dbias (`dbias_bound`): 0.5 ulp_out
+ L 2^-24 sum_r |dy| - at most L fp32 additions on the way to an element, each within 2^-24 of a partial sum that sum |dy| bounds."""
import numpy as np

import moe_gemm_ref as G
import moe_ref as R

offsets_of, round16, gather_ref = G.offsets_of, G.round16, G.gather_ref

# segment lengths: empty, one row, one under / at / over the MFMA step (16) and the staging step (64), two steps and a row
PATTERN = [0, 1, 15, 16, 17, 63, 64, 65, 129]
VARIANTS = ("read_past_end", "drop_row_tail", "start_rounded_down", "kn_as_nk", "no_accumulate")


def segments(offsets, rows, variant=None):
    """[(lo, hi)] per expert, clamped to [0, rows] as the kernel clamps"""
    off = np.clip(np.asarray(offsets, dtype=np.int64), 0, rows)
    segs = []
    for e in range(len(off) - 1):
        lo, hi = int(off[e]), int(off[e + 1])
        if hi > lo:
            if variant == "read_past_end":
                hi = min(rows, lo + (hi - lo + 15) // 16 * 16)
            elif variant == "drop_row_tail":
                hi = lo + (hi - lo) // 64 * 64
            elif variant == "start_rounded_down":
                lo = lo // 16 * 16
        segs.append((lo, max(lo, hi)))
    return segs


def wgrad_ref(dy, a, offsets, *, layout="nk", old=None, variant=None, with_mag=False):
    """(dw f64 [E, N, K] / [E, K, N], dbias f64 [E, N]) from dy f64 [M, N] and a f64 [M, K] (the rows as the GEMM sees them);
    old: the dw that is accumulated onto (an empty expert keeps it).  with_mag: also (sum_r |dy a| in dw's layout, sum_r |dy|)"""
    dy, a = np.asarray(dy, dtype=np.float64), np.asarray(a, dtype=np.float64)
    M, N = dy.shape
    K = a.shape[1]
    segs = segments(offsets, M, variant)
    E = len(segs)
    nk = layout == "nk" or variant == "kn_as_nk"
    if variant == "kn_as_nk":
        assert layout == "kn" and N == K
    dw = np.zeros((E, N, K) if nk else (E, K, N))
    mag, db, dbmag = np.zeros_like(dw), np.zeros((E, N)), np.zeros((E, N))
    for e, (lo, hi) in enumerate(segs):
        g = dy[lo:hi].T @ a[lo:hi]
        m = np.abs(dy[lo:hi]).T @ np.abs(a[lo:hi])
        dw[e], mag[e] = (g, m) if nk else (g.T, m.T)
        db[e], dbmag[e] = dy[lo:hi].sum(0), np.abs(dy[lo:hi]).sum(0)
    if old is not None and variant != "no_accumulate":
        dw = dw + np.asarray(old, dtype=np.float64)
    return (dw, db, mag, dbmag) if with_mag else (dw, db)


def round_out(v, dtype_name):
    """float64 values rounded to fp32 and, for a 16-bit output, on to that type; as float64"""
    v = np.asarray(v, dtype=np.float64)
    return v.astype(np.float32).astype(np.float64) if dtype_name == "float32" else round16(v, dtype_name)


def expected(dy, a, offsets, out_name, *, layout="nk", old=None, variant=None, dbias_name=None):
    """what the kernel must write for witness data, as float64: (round_out(exact dw), round_out(exact dbias))"""
    dw, db = wgrad_ref(dy, a, offsets, layout=layout, old=old, variant=variant)
    return round_out(dw, out_name), round_out(db, dbias_name or out_name)


def witness(rows, N, K, seed):
    """(dy f64 [rows, N], x f64 [rows, K]): integers in [-3, 3], the first four columns of each positive"""
    dy = G.witness(rows, N, 8, 2, "nk", seed)[0]
    x = G.witness(rows, K, 8, 2, "nk", seed + 7919)[0]
    dy[:, :4] = np.maximum(np.abs(dy[:, :4]), 1)
    x[:, :4] = np.maximum(np.abs(x[:, :4]), 1)
    return dy, x


def witness_is_exact(dy, x, offsets, out_name, old=None):
    """the inequalities of the module docstring, on the data: integers, every partial sum below 2^24, 16-bit results finite"""
    segs = segments(offsets, len(dy))
    L = max([hi - lo for lo, hi in segs] + [0])
    ints = all((np.asarray(t) == np.round(t)).all() for t in (dy, x) + (() if old is None else (old,)))
    worst = L * np.abs(dy).max() * np.abs(x).max() + (0 if old is None else np.abs(old).max())
    return bool(ints and worst < 2 ** 24 and (out_name == "float32" or worst < 65504))


def seg_lengths(offsets, rows):
    return np.array([hi - lo for lo, hi in segments(offsets, rows)])


def bound(ref, mag, lengths, out_name):
    """|dw - ref| allowed, and its fp32 term alone; `lengths` [E] broadcasts over an expert's slab"""
    L = np.asarray(lengths, dtype=np.float64).reshape(-1, 1, 1)
    e32 = (L + 2) * 2.0 ** -23 * mag
    return e32 + R.half_ulp(np.abs(ref) + e32, out_name), e32


def dbias_bound(ref, mag, lengths, out_name):
    L = np.asarray(lengths, dtype=np.float64).reshape(-1, 1)
    e32 = L * 2.0 ** -24 * mag
    return e32 + R.half_ulp(np.abs(ref) + e32, out_name), e32
