"""The fp64 restatement of fa_moe_gemm (flash_attn_mi355.moe.moe_gemm, csrc/fa_moe_gemm.hip), the witness data its GPU tests
compare bit for bit, and the bound they hold random data to.  A plain helper module, like moe_ref.py: no fixtures, numpy only.

    out[r] = sum_k a_r[k] W_e[k, :] (+ bias[e])    expert_offsets[e] <= r < expert_offsets[e + 1]
    out[r] = 0                                     every other row
    a_r = x[r], or with sorted_slot: moe_ref.permute_ref's row (a slot of -1: zeros)

`variant` builds a deliberately WRONG reference - tests/test_moe_gemm_cpu.py shows that the witness data tell each from the
right one:
    "leak_row"       a tile leaks: the first row of the next non-empty segment is computed with the previous expert
    "drop_k_tail"    the contraction stops at the last multiple of 64
    "bias_late"      the bias is added after the rounding to 16 bits (two roundings)
    "kn_as_nk"       a "kn" weight's memory read as "nk"
    "pad_as_token0"  a padding slot (-1) reads token 0

Witness data (`witness`): x, w and bias hold integers in [-3, 3] (bias: [-8, 8]), exact in fp16 and bf16.  Every product is an
integer of magnitude <= 9, every partial sum of any subset in any order an integer of magnitude <= 9 K + 8 <= 25928 < 2^24 for
K <= 2880 - exact in fp32 whatever order the hardware adds in - and the result is below both types' largest finite number
(65504).  So out must be round16(exact sum): no tolerance (`witness_is_exact` checks the three inequalities on the data).

Random data (`bound`): |got - ref| <= 0.5 ulp16 + (K + 2) 2^-23 sum_k |a_k w_k| (+ 2^-24 |ref| with a bias).  This assumes that
every addition inside the MFMA and along the accumulator chain errs by at most one fp32 ulp (2^-23 relative), in whatever order:
K products and additions in all, 2 spare.  That property of v_mfma_f32_32x32x16 could not be sourced; the GPU tests print the
share of the bound they measure.  The 0.5 ulp16 is taken at |ref| + the fp32 term."""
import numpy as np

import moe_ref as R

PATTERN = [0, 1, 31, 32, 33, 0, 129]                        # segment lengths: empty, one row, one under / at / one over 32, 129


def offsets_of(lengths, align=1):
    """expert_offsets int32 [E + 1] of segment lengths, each padded to `align` as moe_sort pads"""
    off = np.zeros(len(lengths) + 1, dtype=np.int32)
    for e, n in enumerate(lengths):
        off[e + 1] = off[e] + (n + align - 1) // align * align
    return off


def w_of(w, e, layout):
    """W_e as [K, N] float64"""
    return np.asarray(w[e], dtype=np.float64).T if layout == "nk" else np.asarray(w[e], dtype=np.float64)


def gemm_ref(a, w, offsets, *, layout="nk", bias=None, variant=None, with_mag=False):
    """out f64 [M, N] from a f64 [M, K] (the rows as the GEMM sees them), w [E, N, K] / [E, K, N], offsets [E + 1]; with_mag: also
    sum_k |a_k w_k| (the products alone: no bias)"""
    a = np.asarray(a, dtype=np.float64)
    M, K = a.shape
    E = len(offsets) - 1
    if variant == "kn_as_nk":
        assert layout == "kn"
        w = np.ascontiguousarray(np.asarray(w)).reshape(E, w.shape[2], w.shape[1])
        layout = "nk"
    N = w.shape[1] if layout == "nk" else w.shape[2]
    out, mag = np.zeros((M, N)), np.zeros((M, N))
    off = np.clip(np.asarray(offsets, dtype=np.int64), 0, M)
    owner = np.full(M, -1)
    for e in range(E):
        owner[off[e]:off[e + 1]] = e
    if variant == "leak_row":
        for e in range(E):
            nxt = [f for f in range(e + 1, E) if off[f + 1] > off[f]]
            if off[e + 1] > off[e] and (off[e + 1] - off[e]) % 32 and nxt:
                owner[off[nxt[0]]] = e                      # (a segment that ends inside a tile spills into what follows)
    kk = K // 64 * 64 if variant == "drop_k_tail" else K
    for e in range(E):
        rows = np.nonzero(owner == e)[0]
        if len(rows) == 0:
            continue
        We = w_of(w, e, layout)
        out[rows] = a[rows, :kk] @ We[:kk]
        if with_mag:
            mag[rows] = np.abs(a[rows, :kk]) @ np.abs(We[:kk])
        if bias is not None and variant != "bias_late":
            out[rows] += np.asarray(bias[e], dtype=np.float64)     # (the bias enters the bound through 2^-24 |ref| alone, not mag)
    return (out, mag) if with_mag else out


def gather_ref(x, sorted_slot, top_k, variant=None):
    """the rows the fused gather feeds the GEMM: moe_ref.permute_ref (padding rows zeros)"""
    if variant == "pad_as_token0":
        sorted_slot = np.where(np.asarray(sorted_slot) < 0, 0, sorted_slot)
    return R.permute_ref(x, sorted_slot, top_k)


def round16(v, dtype_name):
    """float64 values rounded to fp32 and then to the 16-bit type (round to nearest even twice; for integers below 2^24 the first
    is exact), as float64"""
    import torch
    dt = {"bfloat16": torch.bfloat16, "float16": torch.float16}[dtype_name]
    return torch.from_numpy(np.asarray(v, dtype=np.float64)).to(torch.float32).to(dt).double().numpy()


def expected(a, w, offsets, dtype_name, *, layout="nk", bias=None, variant=None):
    """what the kernel must write for witness data, as float64: round16(exact); "bias_late": round16(round16(sum) + bias)"""
    out = round16(gemm_ref(a, w, offsets, layout=layout, bias=bias, variant=variant), dtype_name)
    if variant == "bias_late" and bias is not None:
        off = np.clip(np.asarray(offsets, dtype=np.int64), 0, len(out))
        for e in range(len(offsets) - 1):
            out[off[e]:off[e + 1]] = round16(out[off[e]:off[e + 1]] + np.asarray(bias[e], dtype=np.float64), dtype_name)
    return out


def witness(rows, K, N, E, layout, seed, with_bias=False):
    """(x f64 [rows, K], w f64 [E, N, K] or [E, K, N], bias f64 [E, N] or None): integers in [-3, 3] (bias [-8, 8]); every
    expert's weights and every row differ"""
    g = np.random.default_rng(seed)
    x = g.integers(-3, 4, size=(rows, K)).astype(np.float64)
    w = g.integers(-3, 4, size=(E, N, K) if layout == "nk" else (E, K, N)).astype(np.float64)
    bias = g.integers(-8, 9, size=(E, N)).astype(np.float64) if with_bias else None
    # every fourth row and the first four output columns are positive: their sums grow like 4 K, past the integers the 16-bit types
    # hold exactly (256 in bf16 from K = 264, 2048 in fp16 at K = 2880), so the ONE rounding - and a bias added after it - shows
    x[::4] = np.maximum(np.abs(x[::4]), 1)
    if layout == "nk":
        w[:, :4, :] = np.maximum(np.abs(w[:, :4, :]), 1)
    else:
        w[:, :, :4] = np.maximum(np.abs(w[:, :, :4]), 1)
    return x, w, bias


def witness_is_exact(x, w, bias, layout):
    """the three inequalities of the module docstring, on the data: integers, every partial sum below 2^24, results below 65504"""
    K = x.shape[1]
    ints = all((np.asarray(t) == np.round(t)).all() for t in (x, w) + (() if bias is None else (bias,)))
    worst = K * np.abs(x).max() * np.abs(w).max() + (0 if bias is None else np.abs(bias).max())
    return bool(ints and worst < 2 ** 24 and worst < 65504)


def bound(ref, mag, K, dtype_name, with_bias):
    e32 = (K + 2) * 2.0 ** -23 * mag + (2.0 ** -24 * np.abs(ref) if with_bias else 0.0)
    return e32 + R.half_ulp16(np.abs(ref) + e32, dtype_name), e32
