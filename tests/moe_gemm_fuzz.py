"""Seeded differential fuzz of the grouped expert GEMM family - moe_gemm, moe_gemm_glu, moe_gemm_wgrad, moe_gemm_mxfp4,
moe_gemm_mxfp4_glu - bit for bit against the fp64 restatements of moe_gemm_ref.py and moe_gemm_wgrad_ref.py.  A plain module like
fuzz_cases.py: no fixtures, no oracle, nothing read outside the repository.

A case is a function of (kind, seed, i) alone.  `draw` needs no GPU: it returns numpy data and the properties the CPU test counts
(tests/test_moe_gemm_fuzz_cpu.py); `expected` is the fp64 answer rounded once; `compare` holds outputs to it on bits; `check` runs
the case on the device.  Every assertion message ends with the case's one-line description, which begins with kind, seed and i:
`run_one(kind, seed, i)` replays it.  No comparison has a tolerance.

What is drawn: E from 2 ... 512 (from 64 on most experts are empty); segment lengths around the tile and step edges at unaligned
starts (wgrad: behind 0 ... 5 unowned head rows), a +0 tail, in a share of the forward cases with rows exactly 32 E or 32 E + 1
(the plan boundary: block_m 32 up to 32 E rows, 128 above); K, N and I around the staging step and the column tile; "nk" / "kn",
fp16 / bf16, bias none / 16-bit / fp32, interleaved / packed gate-up; x plain or gathered - through moe_sort's own tables (top_k
1 ... 8, align 1 ... 256, dropped ids -1 and E) or a hand-built sorted_slot with -1 and out-of-range slots; out as a strided slab
between guard bands, x as a row-strided view, the weights / code blocks / scale blocks as expert-strided views with 0xFF between
the experts, dw as an expert-strided view between NaN bands.

Data are the family's witness data: integers in [-3, 3] (bias [-8, 8]; MXFP4: every code, scale bytes 126 ... 128), for which every
fp32 partial sum is exact in any order, so out is round16(exact).  Two draws narrow them and stay exact: a GLU case whose
relu(g) * u would overflow its dtype gets smaller x, then w, then a sparser x spread over all of K (`_narrow`), until every
expected element is finite; an fp16 wgrad case sets the first column of dy and of x to 3, so that a segment of 228 rows or more
(the drawn lengths end at 300) carries the sum 9 L past 2048 and the one rounding shows.  On a share of the cases the same shape is drawn again with N(0, 1) data (MXFP4: scale bytes
117 ... 137) and the documented bit identities between the kernels are asserted.

wgrad has no plan boundary: its tile is 128 x 128 over steps of 64 rows of the segment, so its "step" is 64 rows and its step
count is per segment.

  pytest runs a fixed sample (tests/test_moe_gemm_fuzz_gpu.py);  more:   python tests/moe_gemm_fuzz.py --kind gemm --seed 7 --n 400
"""
import argparse
import os
import sys
import time
from collections import Counter

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flash-attention-v100_amd"))

import guard                                                      # noqa: E402
import moe_gemm_ref as G                                          # noqa: E402
import moe_gemm_wgrad_ref as W                                    # noqa: E402
import moe_ref as R                                               # noqa: E402
from act_mul_ref import ACTIVATIONS                               # noqa: E402
from test_moe_gemm_mxfp4_gpu import dequant                       # noqa: E402

# (appended only: a kind's id seeds its random stream, and pinned cases replay by (kind, seed, i))
KIND_ID = {"gemm": 0, "glu": 1, "wgrad": 2, "mxfp4": 3, "mxfp4_glu": 4}
KINDS = tuple(KIND_ID)
FORWARD = ("gemm", "glu", "mxfp4", "mxfp4_glu")
MX = ("mxfp4", "mxfp4_glu")
GLU = ("glu", "mxfp4_glu")

EXPERTS, EXPERTS_P = (2, 3, 7, 8, 9, 64, 512), (0.18, 0.18, 0.2, 0.13, 0.13, 0.1, 0.08)
LEN_EDGES = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
K16_EDGES = (8, 16, 24, 56, 64, 72, 120, 128, 136, 184, 192, 200, 248, 256, 264, 320, 384, 448, 512, 1024)
KMX_EDGES = (32, 64, 96, 128, 160, 224, 256, 288, 384, 480, 512, 544, 768, 1024)
N_EDGES = (8, 16, 24, 32, 40, 64, 120, 128, 136, 248, 256, 264, 384, 392)
I_EDGES = (8, 24, 32, 40, 56, 64, 72, 120, 128, 136, 192, 200)
ALIGNS = (1, 1, 2, 4, 8, 16, 16, 32, 128, 256)
MAX_ROWS, MAX_WEIGHTS = 1500, 2 ** 22
# the fixed sample of tests/test_moe_gemm_fuzz_gpu.py, whose coverage tests/test_moe_gemm_fuzz_cpu.py asserts: seed, cases per kind
SAMPLE_SEED, SAMPLE_N = 20261126, {"gemm": 40, "glu": 24, "wgrad": 24, "mxfp4": 24, "mxfp4_glu": 24}
DT = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32}
DEV = "cuda"


# ------------------------------------------------------------------------------------------------------------------ the draw
def _lengths(rng, E, cap, focus=None):
    """segment lengths [E]: an edge with probability 0.7, else uniform in [0, 300]; from 64 experts on 3 ... 8 hold rows.  `focus`
    (a tile height, or "long") then places 0, 1, focus - 1, focus, focus + 1 - or one segment of 255 / 257 rows - on random
    experts; focus 32 keeps the sum at 32 E or below (the decode plan).  The largest other lengths are drawn again from the short
    edges until the sum fits `cap`"""
    L = np.zeros(E, dtype=np.int64)
    live = np.arange(E) if E < 64 else rng.choice(E, size=int(rng.integers(3, 9)), replace=False)
    if E >= 64 and rng.random() < 0.5:
        live[0] = E - 1                                           # (the last expert: the tile search's far end)
    for e in live:
        L[e] = int(rng.choice(LEN_EDGES)) if rng.random() < 0.7 else int(rng.integers(0, 301))
    fixed = np.zeros(E, dtype=bool)
    if focus == "long":
        e = int(rng.choice(live))
        L[e], fixed[e] = int(rng.choice([255, 257])), True
    elif focus:
        at = rng.choice(E, size=min(E, 5), replace=False)
        L[at] = rng.permutation([0, 1, focus - 1, focus, focus + 1])[:len(at)]
        fixed[at] = True
        if focus == 32:
            cap = min(cap, 32 * E)
    while L.sum() > cap:
        e = int(np.argmax(np.where(fixed, -1, L))) if (L[~fixed] > 0).any() else int(np.argmax(L))
        L[e] = int(rng.choice([n for n in LEN_EDGES[:9] if n < L[e]]))
    return L


def _gather_rows(x, ss, topk, variant=None):
    """the rows the fused gather feeds the GEMM, f64 [len(ss), K]: x[slot // top_k], a slot outside [0, T top_k) a row of zeros"""
    ss = np.asarray(ss, dtype=np.int64)
    if variant == "pad_as_token0":
        ss = np.where(ss < 0, 0, ss)
    ok = (ss >= 0) & (ss < len(x) * topk)
    return np.where(ok[:, None], np.asarray(x, dtype=np.float64)[np.where(ok, ss, 0) // topk], 0.0)


def _narrow(x, w, level, rng_seed):
    """GLU data whose relu(g) * u must stay finite: level 1 clips x to [-1, 1], 2 also w, 3 gives x random signs (no all-positive
    rows), from 4 on x keeps every 2^(level - 3)-th k and the last 8 - integers throughout, and the last staging step stays live"""
    if level >= 1:
        x = np.clip(x, -1, 1)
    if level >= 2:
        w = np.clip(w, -1, 1)
    if level >= 3:
        x = x * np.random.default_rng(rng_seed).choice([-1.0, 1.0], size=x.shape)
    if level >= 4:
        keep = np.arange(x.shape[1]) % 2 ** (level - 3) == 0
        keep[-8:] = True
        x = x * keep[None, :]
    return x, w


def draw(kind, rng, i):
    """case `i` of a stream: a dict of numpy data, python scalars and the properties c["props"]; no GPU, no torch device"""
    fwd, mx, glu = kind in FORWARD, kind in MX, kind in GLU
    c = dict(kind=kind, i=i)
    # the forms that the sample must hold rotate with the index inside a layout; everything else is drawn
    j = i // 2 if kind in ("gemm", "glu", "wgrad") else i
    c["layout"] = "nk" if mx else ("nk", "kn")[i % 2]
    focus = (32, 128, "boundary", None)[j % 4] if fwd else (64, "long", None)[j % 3]
    src = c["src"] = ("plain", "sort", "hand", "plain", ("plain", "sort", "hand")[int(rng.integers(3))])[j % 5]
    if focus == "boundary" and src == "sort":
        src = c["src"] = "hand"                                   # (moe_sort fixes M_max: the tail cannot be chosen)
    es = [e for e in EXPERTS if e <= 9] if focus == "boundary" else EXPERTS
    E = c["E"] = int(rng.choice(es, p=np.asarray(EXPERTS_P[:len(es)]) / sum(EXPERTS_P[:len(es)])))
    c["dtype"] = "bfloat16" if mx else ("bfloat16", "float16")[(j // (4 if fwd else 3)) % 2]
    c["bias"] = (None, "io", "fp32")[(j + j // 3) % 3]
    c["gate_up"] = ("interleaved", "packed")[int(rng.integers(2))] if kind == "mxfp4_glu" else "packed"
    # N (GLU: I) and K inside the weight cap; every third N in turn a multiple of the column tile, one 8 over, any
    kmin, tile = 32 if mx else 8, 64 if glu else 128
    ns = [n for n in (I_EDGES if glu else N_EDGES) if E * n * (2 if glu else 1) * kmin <= MAX_WEIGHTS]
    cls = [n for n in ns if n % tile == (0, 8)[(j // 3) % 3]] if (j // 3) % 3 < 2 else ns
    n = int(rng.choice(cls or ns))
    N = c["N"] = 2 * n if glu else n
    c["I"] = n if glu else None
    kcap = min(1024, MAX_WEIGHTS // (E * N))
    kstep = 32 if mx else 8
    if rng.random() < 0.7:
        K = int(rng.choice([k for k in (KMX_EDGES if mx else K16_EDGES) if k <= kcap]))
    else:
        K = int(rng.integers(1, kcap // kstep + 1)) * kstep
    c["K"] = K
    # segmentation, tail, tables
    head = c["head"] = int(rng.integers(0, 6)) if kind == "wgrad" and src != "sort" else 0
    c["align"] = c["ids"] = c["ss"] = c["topk"] = None
    lf = focus if focus != "boundary" else None
    if src == "sort":
        topk = c["topk"] = int(rng.integers(1, min(8, E) + 1))    # (moe_sort takes top_k <= E)
        aligns = [a for a in ALIGNS if E * (a - 1) <= MAX_ROWS - 500] if lf != 32 else [1]
        align = c["align"] = int(rng.choice(aligns))
        L = _lengths(rng, E, MAX_ROWS - E * (align - 1) - 24, lf)
        ids = np.repeat(np.arange(E), L).tolist() + [(-1, E)[d % 2] for d in range(int(rng.integers(2, 7)))]
        ids += [-1] * (-len(ids) % topk)
        ids = c["ids"] = rng.permutation(np.asarray(ids, dtype=np.int32)).reshape(-1, topk)
        c["ss"], c["pos"], off = R.sort_ref(ids, E, align=align)
        T, rows = len(ids), len(c["ss"])
    else:
        L = _lengths(rng, E, MAX_ROWS - 45, lf)
        tail = 0 if rng.random() < 0.3 else int(rng.integers(1, 41))
        if lf == 32:
            tail = min(tail, 32 * E - int(L.sum()))               # (the decode plan: rows <= 32 E)
        if focus == "boundary":                                   # the plan boundary: rows == 32 E or 32 E + 1
            target = 32 * E + (j // 4) % 2
            while L.sum() > target:
                L[int(np.argmax(L))] = int(rng.choice([m for m in LEN_EDGES[:9] if m < L.max()]))
            tail = target - int(L.sum())
        off = (G.offsets_of(L) + head).astype(np.int32)
        rows = int(off[E]) + tail
        if rows == 0:
            rows = 1                                              # (no rows launches nothing: the wrappers' own tests cover it)
        T = rows
        if src == "hand":
            topk, T = int(rng.integers(1, 9)), int(rng.integers(1, 61))
            c["topk"] = topk
            ss = rng.integers(0, T * topk, rows).astype(np.int32)
            if rows >= 2:
                ss[0] = -1
                ss[rows // 2] = int(rng.choice([T * topk, T * topk + 7, 2 ** 31 - 1, -7]))
            c["ss"] = ss
    c["off"], c["rows"], c["T"] = off, rows, T
    c["lengths"] = np.diff(off)
    seed = c["seed"] = int(rng.integers(2 ** 31))
    c["out_slab"], c["x_strided"], c["w_strided"] = (bool(rng.random() < p) for p in (0.5, 0.3, 0.3))
    c["ident"] = bool(rng.random() < 0.35)
    c["ident_act"] = str(rng.choice(ACTIVATIONS))
    # data
    g = np.random.default_rng(seed)
    if kind == "wgrad":
        c["dy"], _ = W.witness(rows, N, 8, seed)
        c["x"] = W.witness(T, 8, K, seed + 1)[1]
        if c["dtype"] == "float16":
            c["dy"][:, 0] = c["x"][:, 0] = 3                      # (dw[e, 0, 0] = 9 L passes 2048 at 228 rows: fp16's one rounding shows)
        c["dw_dtype"] = ("io", "float32")[(j // 6) % 2]
        c["accumulate"] = bool(c["dw_dtype"] == "float32" and rng.random() < 0.5)
        c["old"] = g.integers(-50, 51, size=(E, N, K) if c["layout"] == "nk" else (E, K, N)).astype(np.float64) if c["accumulate"] else None
        c["dbias"], c["bias"] = c["bias"], None
    elif mx:
        c["blocks"] = g.integers(0, 256, (E, N, K // 2), dtype=np.uint8)
        c["scales"] = g.integers(126, 129, (E, N, K // 32)).astype(np.uint8)
        c["x"] = g.integers(-3, 4, (T, K)).astype(np.float64)
        c["bias_data"] = g.integers(-8, 9, (E, N)).astype(np.float64) if c["bias"] else None
    else:
        c["x"], c["w"], c["bias_data"] = G.witness(T, K, N, E, c["layout"], seed, c["bias"] is not None)
    c["narrow"] = 0
    if kind == "glu":                                             # (bf16 never overflows: (9 K + 8)^2 < 2^127)
        x0, w0 = c["x"], c["w"]
        while not np.isfinite(G.round16(_exact(kind, c)["out"][0], c["dtype"])).all():
            c["narrow"] += 1
            c["x"], c["w"] = _narrow(x0, w0, c["narrow"], seed)
    c["props"] = _props(c)
    c["desc"] = _describe(c)
    return c


def _props(c):
    kind, E, rows, K = c["kind"], c["E"], c["rows"], c["K"]
    p = dict(E=E, layout=c["layout"], dtype=c["dtype"], bias=c["bias"], src=c["src"], K=K, N=c["N"])
    if kind in FORWARD:
        bm = p["block_m"] = 32 if rows <= 32 * E else 128
        p["bk"] = 64 if kind not in MX else (256 if bm == 32 else 128)
        p["steps"] = [-(-K // p["bk"])]
        p["k_exact"] = K % p["bk"] == 0
        p["boundary"] = rows - 32 * E if rows - 32 * E in (0, 1) else None
    else:
        bm, p["block_m"], p["bk"], p["boundary"] = 64, 64, 64, None
        p["steps"] = sorted({-(-int(n) // 64) for n in c["lengths"] if n > 0})
        p["k_exact"] = any(n > 0 and n % 64 == 0 for n in c["lengths"])
        p["bias"] = c["dbias"]
    p["n_over"] = c["I"] % 64 if kind in GLU else c["N"] % 128    # columns past a whole column tile (GLU: of 64 outputs = 128 weight columns)
    p["len_edges"] = sorted({int(n) for n in c["lengths"]} & {0, 1, bm - 1, bm, bm + 1})
    ss = c["ss"]
    p["bad_slots"] = bool(ss is not None and (ss == -1).any() and ((ss < -1) | (ss >= c["T"] * c["topk"])).any())
    return p


def _describe(c):
    L = c["lengths"]
    seg = str(L.tolist()) if c["E"] <= 9 else "{" + ", ".join(f"{e}: {int(L[e])}" for e in np.nonzero(L)[0]) + "}"
    s = f"E{c['E']} rows{c['rows']} K{c['K']} N{c['N']} {c['layout']} {c['dtype']} x={c['src']}"
    if c["src"] != "plain":
        s += f"(T{c['T']} top_k{c['topk']}" + (f" align{c['align']})" if c["src"] == "sort" else ")")
    s += f" lengths={seg} head={c['head']} block_m={c['props']['block_m']} steps={c['props']['steps']}"
    if c["kind"] == "wgrad":
        s += f" dw={c['dw_dtype']} accumulate={c['accumulate']} dbias={c['dbias']}"
    else:
        s += f" bias={c['bias']}" + (f" gate_up={c['gate_up']}" if c["kind"] == "mxfp4_glu" else "") + (f" narrow={c['narrow']}" if c["narrow"] else "")
    return s + f" slab={c['out_slab']} x_strided={c['x_strided']} w_strided={c['w_strided']} ident={c['ident']}"


def case_of(kind, seed, i):
    """the case (kind, seed, i) names; its description begins with the three"""
    c = draw(kind, np.random.default_rng([seed, KIND_ID[kind], i]), i)
    c["desc"] = f"{kind} seed {seed} #{i}: " + c["desc"]
    return c


def sample(kind, seed, n):
    return [case_of(kind, seed, i) for i in range(n)]


# ------------------------------------------------------------------------------------------------------------ the reference
def mxfp4_witness_is_exact(x, blocks, scales, bias):
    """the MXFP4 kinds' exactness on the data: x integers and every weight a multiple of 1/4, so every product is one; every
    partial sum - K x the largest product + the bias, in quarter units - below 2^24; the results finite in bf16"""
    w = dequant(blocks, scales)
    K = x.shape[1]
    quarters = (np.asarray(x) == np.round(x)).all() and (4 * w == np.round(4 * w)).all() and (bias is None or (bias == np.round(bias)).all())
    worst = K * np.abs(x).max(initial=0) * np.abs(w).max() + (0 if bias is None else np.abs(bias).max())
    return bool(quarters and worst * 4 < 2 ** 24 and worst < 3.3e38)


def is_exact(c):
    """the precondition of the bit-for-bit comparison, on the case's data"""
    if c["kind"] == "wgrad":
        a = c["x"] if c["ss"] is None else _gather_rows(c["x"], c["ss"], c["topk"])
        return W.witness_is_exact(c["dy"], a, c["off"], _dw_name(c), old=c["old"])
    if c["kind"] in MX:
        return mxfp4_witness_is_exact(c["x"], c["blocks"], c["scales"], c["bias_data"])
    return G.witness_is_exact(c["x"], c["w"], c["bias_data"], c["layout"])


def _dw_name(c):
    return c["dtype"] if c["dw_dtype"] == "io" else "float32"


def _halves(h, gate_up):
    return (h[..., 0::2], h[..., 1::2]) if gate_up == "interleaved" else (h[..., :h.shape[-1] // 2], h[..., h.shape[-1] // 2:])


def _exact(kind, c, variant=None):
    """{name: (f64 values before the ONE final rounding, the dtype it rounds to)}: out, or dw and dbias.  GLU: relu(g16) * u16 of
    the 16-bit h, a product of two 16-bit values.  `variant`: a deliberately wrong reference (moe_gemm_ref / moe_gemm_wgrad_ref)"""
    gv = variant if variant == "pad_as_token0" else None
    a = c["x"] if c["ss"] is None else _gather_rows(c["x"], c["ss"], c["topk"], gv)
    if kind == "wgrad":
        v = None if gv else variant
        if v == "kn_as_nk":                                       # a "kn" gradient written in "nk" order, any N and K
            dw, db = W.wgrad_ref(c["dy"], a, c["off"], layout="nk", old=None if c["old"] is None else c["old"].reshape(c["E"], c["N"], c["K"]))
            dw = dw.reshape(c["E"], c["K"], c["N"])
        else:
            dw, db = W.wgrad_ref(c["dy"], a, c["off"], layout=c["layout"], old=c["old"], variant=v)
        res = {"dw": (dw, _dw_name(c))}
        if c["dbias"]:
            res["dbias"] = (db, c["dtype"] if c["dbias"] == "io" else "float32")
        return res
    v = None if gv else variant
    w = dequant(c["blocks"], c["scales"]) if kind in MX else c["w"]
    pre = G.gemm_ref(a, w, c["off"], layout=c["layout"], bias=c["bias_data"], variant=v)
    if kind not in GLU and v != "bias_late":
        return {"out": (pre, c["dtype"])}
    h = G.round16(pre, c["dtype"])
    if v == "bias_late" and c["bias_data"] is not None:           # (two roundings: the wrong order)
        for e in range(c["E"]):
            lo, hi = int(c["off"][e]), int(c["off"][e + 1])
            h[lo:hi] = G.round16(h[lo:hi] + c["bias_data"][e], c["dtype"])
    if kind not in GLU:
        return {"out": (h, c["dtype"])}
    g16, u16 = _halves(h, c["gate_up"])
    return {"out": (np.where(g16 <= 0, 0.0, g16) * u16, c["dtype"])}


def expected(kind, c, variant=None):
    """{name: torch CPU tensor of the output's dtype}: what the kernel must write, round(exact) (+0 where nothing is owned)"""
    return {k: torch.from_numpy(W.round_out(v, name)).to(DT[name]) for k, (v, name) in _exact(kind, c, variant).items()}


def _int(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def compare(kind, c, got):
    """`got` {name: CPU tensor} against `expected` on bits; forward: the rows behind expert_offsets[E] are +0"""
    want = expected(kind, c)
    assert set(got) == set(want), f"outputs {sorted(got)} against {sorted(want)}  [{c['desc']}]"
    for name, w in want.items():
        t = got[name]
        assert t.shape == w.shape and t.dtype == w.dtype, f"{name}: {t.dtype} {tuple(t.shape)} against {w.dtype} {tuple(w.shape)}  [{c['desc']}]"
        bad = torch.nonzero(_int(t) != _int(w))
        assert len(bad) == 0, f"{name}: {len(bad)} of {w.numel()} elements differ from round(fp64), first at {bad[0].tolist()}: " \
                              f"got {float(t[tuple(bad[0])])} want {float(w[tuple(bad[0])])}  [{c['desc']}]"
    if kind in FORWARD:
        assert (_int(got["out"][int(c["off"][-1]):]) == 0).all(), f"out: rows behind expert_offsets[E] are not +0  [{c['desc']}]"


# ------------------------------------------------------------------------------------------------------------ on the device
def _M():
    from flash_attn_mi355 import moe
    import flash_attn_mi355.torch_ops  # noqa: F401
    return moe


def _same(a, b, name, c):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{name}  [{c['desc']}]"
    n = int((_int(a) != _int(b)).sum())
    assert n == 0, f"{name}: {n} elements differ  [{c['desc']}]"


def _strided_experts(t):
    """(buf, view): `t` [E, ...] as a view whose experts lie 48 bytes further apart than they need, between bands of 0xFF"""
    E, n, item = t.shape[0], t[0].numel(), t.element_size()
    buf = torch.full(((64 + E * (n * item + 48)),), 0xFF, dtype=torch.uint8, device=t.device).view(t.dtype)
    view = buf[64 // item:].as_strided(t.shape, (n + 48 // item,) + tuple(t[0].stride()))
    view.copy_(t)
    return buf, view


def _dw_slab(shape, dtype):
    """(buf, flat view [E, N K], dw view of `shape`): experts contiguous, a gap between experts, NaN-filled guard bands around"""
    buf, flat = guard.slab((shape[0], shape[1] * shape[2]), dtype, gaps=True, device=DEV, check_prep=False)
    return buf, flat, buf.as_strided(shape, (flat.stride(0), shape[2], 1), flat.storage_offset())


class _Inputs:
    """the device tensors of a case's inputs and the bits of their whole allocations (the bands between experts included)"""

    def __init__(self):
        self.held = []

    def add(self, name, t, strided=None):
        t = t.to(DEV)
        if strided == "rows":
            buf, view, _ = guard.guarded(t, gaps=True)
        elif strided == "experts":
            buf, view = _strided_experts(t)
        else:
            buf = view = t
        self.held.append((name, buf, buf.clone()))
        return view

    def assert_unchanged(self, c):
        for name, buf, snap in self.held:
            flat = (lambda t: t.view(torch.uint8) if t.dtype != torch.int32 else t)
            assert torch.equal(flat(buf), flat(snap)), f"{name} was written  [{c['desc']}]"


def _tables(M, c, ins):
    """(expert_offsets, gather kwargs) on the device; a sort case runs moe_sort itself and holds it to the drawn tables"""
    off = ins.add("expert_offsets", torch.from_numpy(c["off"]))
    if c["src"] == "plain":
        return off, {}
    if c["src"] == "sort":
        ss, pos, soff = M.moe_sort(torch.from_numpy(c["ids"]).to(DEV), c["E"], align=c["align"])
        for name, t, want in (("sorted_slot", ss, c["ss"]), ("pos", pos, c["pos"]), ("expert_offsets", soff, c["off"])):
            assert torch.equal(t.cpu(), torch.from_numpy(want)), f"moe_sort's {name} differs from sort_ref  [{c['desc']}]"
        ins.held.append(("sorted_slot", ss, ss.clone()))
        return off, dict(sorted_slot=ss, top_k=c["topk"])
    return off, dict(sorted_slot=ins.add("sorted_slot", torch.from_numpy(c["ss"])), top_k=c["topk"])


def _bias(c, data):
    return None if c["bias"] is None else torch.from_numpy(data).to(DT[c["dtype"]] if c["bias"] == "io" else torch.float32)


def _forward_call(M, c):
    kind, dt = c["kind"], DT[c["dtype"]]
    plan = dict(gemm=lambda: M.moe_gemm_plan(c["rows"], c["N"], c["K"], c["E"], w_layout=c["layout"], dtype=dt),
                glu=lambda: M.moe_gemm_glu_plan(c["rows"], c["I"], c["K"], c["E"], w_layout=c["layout"], dtype=dt),
                mxfp4=lambda: M.moe_gemm_mxfp4_plan(c["rows"], c["N"], c["K"], c["E"]),
                mxfp4_glu=lambda: M.moe_gemm_mxfp4_glu_plan(c["rows"], c["I"], c["K"], c["E"]))[kind]()
    p = c["props"]
    assert (plan[0], plan[2]) == (p["block_m"], p["bk"]), f"plan {plan} against block_m {p['block_m']} block_k {p['bk']}  [{c['desc']}]"
    if kind == "gemm":
        return lambda x, w, off, bias, kw: M.moe_gemm(x, *w, off, w_layout=c["layout"], bias=bias, **kw)
    if kind == "glu":
        return lambda x, w, off, bias, kw, act="relu": M.moe_gemm_glu(x, *w, off, activation=act, w_layout=c["layout"], bias=bias, **kw)
    if kind == "mxfp4":
        return lambda x, w, off, bias, kw: M.moe_gemm_mxfp4(x, *w, off, bias=bias, **kw)
    return lambda x, w, off, bias, kw, act="relu": M.moe_gemm_mxfp4_glu(x, *w, off, activation=act, gate_up=c["gate_up"], bias=bias, **kw)


def check(kind, c):
    """run the case on the device: the plan, the output's bits against fp64, the +0 tail, the guard bands, the inputs' bits, and -
    where the case draws them - the bit identities on random data"""
    assert is_exact(c), f"the witness data are not exact  [{c['desc']}]"
    M, dt, ins = _M(), DT[c["dtype"]], _Inputs()
    x = ins.add("x", torch.from_numpy(c["x"]).to(dt), "rows" if c["x_strided"] else None)
    off, kw = _tables(M, c, ins)
    ws = "experts" if c["w_strided"] else None
    if kind == "wgrad":
        dy = ins.add("dy", torch.from_numpy(c["dy"]).to(dt), "rows" if c["w_strided"] else None)
        shape, dwt = ((c["E"], c["N"], c["K"]) if c["layout"] == "nk" else (c["E"], c["K"], c["N"])), DT[_dw_name(c)]
        if c["out_slab"]:
            buf, flat, view = _dw_slab(shape, dwt)
        else:
            buf = flat = view = torch.empty(shape, dtype=dwt, device=DEV)
            guard.fill_nan(view)
        if c["accumulate"]:
            view.copy_(torch.from_numpy(c["old"]).to(dwt))
        snap = guard.snapshot(buf)
        call = lambda dy, x, k, out=None, acc=False: M.moe_gemm_wgrad(                      # noqa: E731
            dy, x, off, w_layout=c["layout"], dw_dtype=dwt, out=out, accumulate=acc, need_dbias=c["dbias"] is not None,
            dbias_dtype=None if c["dbias"] is None else (dt if c["dbias"] == "io" else torch.float32), **k)
        res = call(dy, x, kw, view, c["accumulate"])
        torch.cuda.synchronize()
        dw, db = res if c["dbias"] else (res, None)
        assert dw is view, f"dw is not out  [{c['desc']}]"
        if c["out_slab"]:
            guard.assert_untouched(buf, flat, snap, f"dw [{c['desc']}]")
        ins.assert_unchanged(c)
        compare(kind, c, {"dw": view.cpu()} | ({"dbias": db.cpu()} if c["dbias"] else {}))
        if c["ident"]:
            g = torch.Generator().manual_seed(c["seed"] + 1)
            dy2 = torch.randn(c["rows"], c["N"], generator=g).to(dt).to(DEV)
            x2 = torch.randn(c["T"], c["K"], generator=g).to(dt).to(DEV)
            one, two = call(dy2, x2, kw), call(dy2, x2, kw)
            pair = (lambda r: r if c["dbias"] else (r,))
            for name, a, b in zip(("dw", "dbias"), pair(one), pair(two)):
                _same(a, b, f"{name}: two runs", c)
            if kw:
                xp = M.moe_permute_forward(x2, kw["sorted_slot"], c["topk"])
                for name, a, b in zip(("dw", "dbias"), pair(one), pair(call(dy2, xp, {}))):
                    _same(a, b, f"{name}: fused gather against moe_permute_forward + the plain form", c)
        return c["desc"]
    # the forward kinds
    if kind in MX:
        w = (ins.add("w_blocks", torch.from_numpy(c["blocks"]), ws), ins.add("w_scales", torch.from_numpy(c["scales"]), ws))
    else:
        w = (ins.add("w", torch.from_numpy(c["w"]).to(dt), ws),)
    bias = None if c["bias"] is None else ins.add("bias", _bias(c, c["bias_data"]))
    run = _forward_call(M, c)
    NO = c["I"] if kind in GLU else c["N"]
    if c["out_slab"]:
        buf, view = guard.slab((c["rows"], NO), dt, gaps=True, device=DEV, check_prep=False)
    else:
        buf = view = guard.fill_nan(torch.empty((c["rows"], NO), dtype=dt, device=DEV))
    snap = guard.snapshot(buf)
    got = run(x, w, off, bias, dict(kw, out=view))
    torch.cuda.synchronize()
    assert got is view, f"the result is not out  [{c['desc']}]"
    if c["out_slab"]:
        guard.assert_untouched(buf, view, snap, f"out [{c['desc']}]")
    ins.assert_unchanged(c)
    compare(kind, c, {"out": view.cpu()})
    if c["ident"]:
        _identities(M, c, run, off, kw)
    return c["desc"]


def _identities(M, c, run, off, kw):
    """the same shape with N(0, 1) data: the documented bit identities, no tolerance"""
    from flash_attn_mi355 import act_mul
    kind, dt, E, N, K, I = c["kind"], DT[c["dtype"]], c["E"], c["N"], c["K"], c["I"]
    g = torch.Generator().manual_seed(c["seed"] + 1)
    x = torch.randn(c["T"], K, generator=g).to(dt).to(DEV)
    bias = None if c["bias"] is None else torch.randn(E, N, generator=g).to(dt if c["bias"] == "io" else torch.float32).to(DEV)
    if kind in MX:
        rng = np.random.default_rng(c["seed"] + 2)
        blocks, scales = rng.integers(0, 256, (E, N, K // 2), dtype=np.uint8), rng.integers(117, 138, (E, N, K // 32)).astype(np.uint8)
        w = (torch.from_numpy(blocks).to(DEV), torch.from_numpy(scales).to(DEV))
        wq = torch.from_numpy(dequant(blocks, scales)).to(dt).to(DEV)                      # exact in bf16
    else:
        w = ((torch.randn((E, N, K) if c["layout"] == "nk" else (E, K, N), generator=g) / K ** 0.5).to(dt).to(DEV),)
    act = dict(gemm=None, mxfp4=None, glu=c["ident_act"], mxfp4_glu="silu")[kind]
    call = (lambda xa, k: run(xa, w, off, bias, k)) if act is None else (lambda xa, k: run(xa, w, off, bias, k, act))
    got = call(x, kw)
    _same(got, call(x, kw), "two runs", c)
    if kw:
        xp = M.moe_permute_forward(x, kw["sorted_slot"], c["topk"])
        _same(got, call(xp, {}), "fused gather against moe_permute_forward + the plain form", c)
    if kind == "glu":
        h = M.moe_gemm(x, *w, off, w_layout=c["layout"], bias=bias, **kw)
        _same(got, act_mul.act_mul_forward(h[:, :I], h[:, I:], activation=act), f"moe_gemm_glu against act_mul_forward(moe_gemm), {act}", c)
    elif kind == "mxfp4":
        _same(got, M.moe_gemm(x, wq, off, bias=bias, **kw), "moe_gemm_mxfp4 against moe_gemm on the dequantised weights", c)
    elif kind == "mxfp4_glu":                                     # rows and bias columns in packed order, as test_bit_for_bit
        wp = torch.cat(_halves(wq.transpose(1, 2), c["gate_up"]), dim=2).transpose(1, 2).contiguous()
        bp = None if bias is None else torch.cat(_halves(bias, c["gate_up"]), dim=1).contiguous()
        _same(got, M.moe_gemm_glu(x, wp, off, activation="silu", bias=bp, **kw),
              "moe_gemm_mxfp4_glu(silu) against moe_gemm_glu on the dequantised weights", c)


# ------------------------------------------------------------------------------------------------------------------- running
def histogram(cases):
    """the coverage of a list of cases, as lines: plans, step parities, the K and N classes, forms"""
    h = {k: Counter() for k in ("block_m", "boundary", "steps", "K", "N", "layout", "dtype", "bias", "x", "E")}
    for c in cases:
        p = c["props"]
        h["block_m"][p["block_m"]] += 1
        h["boundary"][{None: "off", 0: "32E", 1: "32E+1"}[p["boundary"]]] += 1
        for s in p["steps"]:
            h["steps"]["one" if s == 1 else ("even", "odd")[s % 2]] += 1
        h["K"]["multiple of the step" if p["k_exact"] else "tail"] += 1
        h["N"][{0: "whole tiles", 8: "tiles + 8"}.get(p["n_over"], "other")] += 1
        for k, v in (("layout", p["layout"]), ("dtype", p["dtype"]), ("bias", str(p["bias"])), ("x", p["src"] + ("+bad" if p["bad_slots"] else "")), ("E", p["E"])):
            h[k][v] += 1
    return [f"  {k:9s} " + "  ".join(f"{a}: {b}" for a, b in sorted(v.items(), key=lambda t: str(t[0]))) for k, v in h.items()]


def run_one(kind, seed, i):
    """Re-run case `i` of the (kind, seed) stream alone (how a logged failure is pinned as a test)."""
    return check(kind, case_of(kind, seed, i))


def run(kind, seed, n, verbose=False, keep_going=False):
    """cases 0 ... n - 1; stops at the first failure.  keep_going: past an AssertionError (a comparison) only - a HIP error or any
    other exception ends the run.  Returns (failures, cases)."""
    failures, cases = [], []
    for i in range(n):
        c = case_of(kind, seed, i)
        cases.append(c)
        try:
            check(kind, c)
            if verbose:
                print("ok  ", c["desc"], flush=True)
        except AssertionError as e:
            if not keep_going:
                raise
            failures.append(str(e))
            print("FAIL", failures[-1], flush=True)
    return failures, cases


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=KINDS, required=True)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--keep-going", action="store_true", help="continue past a failed comparison (never past any other error)")
    ap.add_argument("-v", action="store_true")
    a = ap.parse_args()
    t0 = time.time()
    f, cases = run(a.kind, a.seed, a.n, verbose=a.v, keep_going=a.keep_going)
    print(f"{a.kind}: seed {a.seed}, {a.n - len(f)} / {a.n} cases agree bit for bit ({time.time() - t0:.1f} s)", flush=True)
    print("\n".join(histogram(cases)), flush=True)
    sys.exit(1 if f else 0)
