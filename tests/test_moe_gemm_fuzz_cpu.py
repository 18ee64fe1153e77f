"""CPU: the fuzz of the grouped expert GEMM family (tests/moe_gemm_fuzz.py) proved on the very cases the GPU runs - the fixed
sample of tests/test_moe_gemm_fuzz_gpu.py (moe_gemm_fuzz.SAMPLE_SEED / SAMPLE_N).  Exactness of the drawn data is a precondition
checked on the data; the sample's coverage of plans, step parities, tile edges and forms is asserted; and the comparison step
rejects every wrong variant of moe_gemm_ref.py and moe_gemm_wgrad_ref.py.  Nothing here needs a GPU."""
import functools

import numpy as np
import pytest
import torch

import moe_gemm_fuzz as F
import moe_gemm_ref as G
import moe_gemm_wgrad_ref as W

SIXTEEN = ("gemm", "glu", "wgrad")


@functools.lru_cache(maxsize=None)
def _sample(kind):
    return F.sample(kind, F.SAMPLE_SEED, F.SAMPLE_N[kind])


@functools.lru_cache(maxsize=None)
def _expected(kind):
    return [F.expected(kind, c) for c in _sample(kind)]


def _groups(kind):
    """the cases the coverage is asked of: per kind, and for the 16-bit kinds per layout"""
    cases = _sample(kind)
    return {(kind, lay): [c for c in cases if c["layout"] == lay] for lay in (("nk", "kn") if kind in SIXTEEN else ("nk",))}


@pytest.mark.parametrize("kind", F.KINDS)
def test_a_case_is_a_function_of_kind_seed_and_index(kind):
    a, b = F.case_of(kind, F.SAMPLE_SEED, 3), F.case_of(kind, F.SAMPLE_SEED, 3)
    assert a["desc"] == b["desc"] == _sample(kind)[3]["desc"] and a["desc"].startswith(f"{kind} seed {F.SAMPLE_SEED} #3: ")
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, b[k]), k
    assert F.case_of(kind, F.SAMPLE_SEED + 1, 3)["desc"] != a["desc"]
    assert sorted(F.SAMPLE_N) == sorted(F.KINDS) == sorted(F.KIND_ID)


@pytest.mark.parametrize("kind", F.KINDS)
def test_every_drawn_case_is_exact_well_formed_and_inside_the_caps(kind):
    """the precondition of a comparison without tolerance, on the data: integers (MXFP4: quarters), every partial sum below 2^24,
    every expected element finite in the case's dtype - GLU included, whose draw narrows the data rather than drop the case"""
    for c, want in zip(_sample(kind), _expected(kind)):
        assert F.is_exact(c), c["desc"]
        for name, t in want.items():
            assert torch.isfinite(t.float()).all(), (name, c["desc"])
        off = c["off"].astype(np.int64)
        assert len(off) == c["E"] + 1 and (np.diff(off) >= 0).all() and 0 <= off[0] <= 5 and off[-1] <= c["rows"] <= F.MAX_ROWS, c["desc"]
        assert (kind == "wgrad" or off[0] == 0) and 1 <= c["rows"]
        assert c["E"] * c["N"] * c["K"] <= F.MAX_WEIGHTS and c["K"] % (32 if kind in F.MX else 8) == 0 and c["N"] % 8 == 0
        for t in (c["x"], c.get("w"), c.get("dy"), c.get("bias_data")):
            if t is not None:                                     # exact in the io dtype
                assert (torch.from_numpy(t).to(F.DT[c["dtype"]]).double().numpy() == t).all(), c["desc"]
    assert not F.mxfp4_witness_is_exact(np.full((1, 32), 0.5), np.full((2, 8, 16), 0x11, np.uint8), np.full((2, 8, 1), 126, np.uint8), None)
    assert not F.mxfp4_witness_is_exact(np.ones((1, 32)), np.full((2, 8, 16), 0x11, np.uint8), np.full((2, 8, 1), 124, np.uint8), None)
    assert not F.mxfp4_witness_is_exact(np.full((1, 32), 3.0), np.full((2, 8, 16), 0x77, np.uint8), np.full((2, 8, 1), 145, np.uint8), None)
    assert F.mxfp4_witness_is_exact(np.full((1, 32), 3.0), np.full((2, 8, 16), 0x77, np.uint8), np.full((2, 8, 1), 128, np.uint8), np.ones((2, 8)))


@pytest.mark.parametrize("kind", F.KINDS)
def test_the_one_rounding_is_decisive_for_every_dtype(kind):
    """per kind and 16-bit dtype, some case holds an exact value that the dtype cannot represent: the ONE rounding shows"""
    for dtype in (("bfloat16",) if kind in F.MX else ("bfloat16", "float16")):
        hit = False
        for c in _sample(kind):
            for v, name in F._exact(kind, c).values():
                hit = hit or (c["dtype"] == dtype and name == dtype and bool((W.round_out(v, name) != v).any()))
        assert hit, (kind, dtype)


@pytest.mark.parametrize("kind", F.KINDS)
def test_the_sample_covers_what_the_fuzz_is_for(kind):
    for key, cases in _groups(kind).items():
        P = [c["props"] for c in cases]
        msg = lambda what: f"{key}: the sample misses {what}"   # noqa: E731
        if kind in F.FORWARD:
            assert {p["block_m"] for p in P} == {32, 128}, msg("a plan")
            assert {0, 1} <= {p["boundary"] for p in P}, msg("rows == 32 E or 32 E + 1")
        bms = (32, 128) if kind in F.FORWARD else (64,)
        for bm in bms:
            have = set().union(*[p["len_edges"] for p in P if p["block_m"] == bm])
            assert have >= {0, 1, bm - 1, bm, bm + 1}, msg(f"segment lengths {sorted({0, 1, bm - 1, bm, bm + 1} - have)} under block_m {bm}")
        for parity, name in ((0, "even"), (1, "odd")):
            n = sum(any(s > 1 and s % 2 == parity for s in p["steps"]) for p in P)
            assert n >= 2, msg(f"two cases with an {name} count (> 1) of staging steps: {n}")
        assert any(p["k_exact"] for p in P), msg("a contraction that is an exact multiple of the step")
        assert {0, 8} <= {p["n_over"] for p in P}, msg("an N (2 I) that is a multiple of the 128-column weight tile, or one 8 over")
        assert any(p["bad_slots"] for p in P), msg("a gather with a -1 and an out-of-range slot")
        assert any(p["src"] == "sort" for p in P) and any(p["src"] == "plain" for p in P), msg("an x source")
        assert {p["bias"] for p in P} == {None, "io", "fp32"}, msg("a bias kind")
        assert {p["dtype"] for p in P} == ({"bfloat16"} if kind in F.MX else {"bfloat16", "float16"}), msg("a dtype")
    cases = _sample(kind)
    assert {c["out_slab"] for c in cases} == {c["x_strided"] for c in cases} == {c["w_strided"] for c in cases} == {False, True}
    assert any(c["ident"] for c in cases) and max(c["E"] for c in cases) >= 64
    if kind == "mxfp4_glu":
        assert {c["gate_up"] for c in cases} == {"interleaved", "packed"}
    if kind == "wgrad":
        assert {c["dw_dtype"] for c in cases} == {"io", "float32"} and any(c["accumulate"] for c in cases) and any(c["head"] for c in cases)
    if kind == "glu":                                             # the narrowing is exercised, and only where fp16 needs it
        assert any(c["narrow"] for c in cases) and all(c["dtype"] == "float16" for c in cases if c["narrow"])


GEMM_VARIANTS = ("leak_row", "drop_k_tail", "bias_late", "kn_as_nk", "pad_as_token0", "stale_last_step")


def _rejected(kind, c, variant):
    try:
        F.compare(kind, c, F.expected(kind, c, variant))
    except AssertionError as e:
        assert str(e).endswith(f"[{c['desc']}]")                 # the message alone replays the case
        return True
    return False


@pytest.mark.parametrize("kind", F.KINDS)
def test_the_comparison_rejects_every_wrong_variant(kind):
    """"outputs" built from each deliberately wrong reference, over the fixed sample: every variant fails the comparison in at
    least one case (a "kn" variant: among the "kn" cases), and the right reference passes in all"""
    cases = _sample(kind)
    for c, want in zip(cases, _expected(kind)):
        F.compare(kind, c, want)
    if kind == "wgrad":
        variants = W.VARIANTS + ("pad_as_token0",)
    else:
        variants = tuple(v for v in GEMM_VARIANTS if v != "kn_as_nk" or kind in SIXTEEN)
    for variant in variants:
        use = [c for c in cases if (variant != "kn_as_nk" or c["layout"] == "kn") and (variant != "no_accumulate" or c["accumulate"])]
        n = sum(_rejected(kind, c, variant) for c in use)
        print(f"{kind}: {variant} rejected in {n} of {len(use)} cases")
        assert n >= 1, (kind, variant)


def test_stale_last_step_passes_the_hand_picked_k_list_and_fails_the_sample():
    """the record of why this file exists: with the K of test_witness_every_k_and_n (and 136, the end-to-end block's) the count of
    64-element staging steps is never even, so a kernel whose loop mishandles its last step in LDS stage 1 would give the right
    bits there; the fuzz's sample tells it apart"""
    off = G.offsets_of(G.PATTERN)
    for K in (8, 16, 24, 48, 264, 2880, 136):
        assert -(-K // 64) % 2 == 1
        for layout in ("nk", "kn"):
            x, w, bias = G.witness(int(off[-1]), K, 8, len(G.PATTERN), layout, K, True)
            for dt in ("bfloat16", "float16"):
                good = G.expected(x, w, off, dt, layout=layout, bias=bias)
                assert (G.expected(x, w, off, dt, layout=layout, bias=bias, variant="stale_last_step") == good).all(), (K, layout)
    x, w, bias = G.witness(int(off[-1]), 96, 8, len(G.PATTERN), "nk", 1, True)       # K = 96: two steps, and it differs
    assert (G.expected(x, w, off, "bfloat16", bias=bias, variant="stale_last_step") != G.expected(x, w, off, "bfloat16", bias=bias)).any()
    for kind in ("gemm", "glu"):
        for layout in ("nk", "kn"):
            for dtype in ("bfloat16", "float16"):
                hit = [c for c in _sample(kind) if (c["layout"], c["dtype"]) == (layout, dtype) and _rejected(kind, c, "stale_last_step")]
                assert hit, (kind, layout, dtype)
                assert all(c["props"]["steps"][0] % 2 == 0 for c in hit)
