"""The read-out data of tests/dropout_readout.py, proved on the oracle (no GPU).

  * design: for every case of the GPU list the oracle's own outputs - the backward fed the SAVED O rounded to the io type,
    every output rounded to the io type - decode to exactly keep AND visible in all four channels, and that rounding
    uses at most 1 / 8 of any element's gate (measured, bf16: 0.016 for O and dV, 0.025 for dQ and dK; fp16 0.003).
    The restated P is the oracle's return_p.
  * sensitivity: ONE bit of the mask flipped for the forward only, or for the backward only (a ragged last column, a
    column with j % 4 == 3, an inner element, a row of the second query block): the decoder names exactly that element in
    exactly the channels the mistaken kernel writes - O for the forward, dQ / dK / dV for the backward.  A decoder that
    leaves any one channel out fails that comparison (test_sensitivity_needs_every_channel).
  * the gap: the same flips on N(0, 1) data, as max |change| / max |ref| - the quantity util.assert_close gates.  Printed;
    measured here on this file's draws (out dq dk dv):
        D 64  200 x 200 causal p .1  (199, 199)   1.7e-3  1.4e-3  1.2e-3  1.2e-3
        D 64  200 x 200 causal p .1  (199, 100)   8.8e-4  1.8e-3  1.5e-3  5.9e-4
        D 128 96 x 130  causal p .5  (95, 129)    1.5e-3  4.6e-4  5.3e-4  1.4e-3
        D 128 760 x 760 full   p .1  (300, 511)   2.9e-2  2.8e-3  2.1e-3  2.4e-2
    The first three stay at 0.08 - 0.16 of their bf16 dropout gates (out 1.05e-2, gradients 2.1e-2) and at 0.6 - 1.2 of
    the fp16 ones; in the fourth draw the flipped key happens to carry a large probability and the gates see it.  How much
    one bit moves depends on the draw (another draw of the same shapes gave 3e-3 .. 1.6e-2, all hidden); the read-out data
    puts every bit at 4.0 of its gate.  The test asserts only that most of the flips hide.
"""
import functools

import numpy as np
import pytest

import oracle
import dropout_readout as dr
from util import TOL_MAXREL, rand16

SEED = dr.SEED


@functools.lru_cache(maxsize=None)
def _ref(name, call):
    c = dr.BY_NAME[name]
    off = dr.offsets(c)["AB".index(call)]
    return c.reference(call, SEED, off), c.expected(SEED, off), off


def _named(c, call, ref, got, keep, ignore=()):
    """{channel: set of (sequence, i, j) the decoder names as wrong}; every reading of an element must agree"""
    out = {}
    for ch, (implied, _, _) in c.decode(call, ref, got, keep, ignore=ignore).items():
        wrong = dr.wrong_bits(implied, keep)
        readings = implied[0].shape[0]
        elems = {(b, i, j) for b, _, i, j in wrong}
        assert len(wrong) == readings * len(elems), f"{ch}: the readings of one element disagree: {wrong[:8]}"
        out[ch] = elems
    return out


# ------------------------------------------------------------------------------------------------ design
@pytest.mark.parametrize("name", [c.name for c in dr.CASES])
def test_oracle_outputs_decode_to_the_mask(name):
    c = dr.BY_NAME[name]
    for call in "AB":
        ref, keep, off = _ref(name, call)
        vis = c.visible()
        assert all(np.array_equal(k & v, k) for k, v in zip(keep, vis))
        assert sum(int(k.sum()) for k in keep) > 0
        for dt in ("fp16", "bf16"):
            sim = c.reference(call, SEED, off, o_dtype=dt)       # the backward sees the saved 16-bit O ...
            got = {k: oracle.round_to(v, dt) for k, v in sim.items() if k != "lse"}        # ... and rounds what it writes
            for ch, (implied, worst, at) in c.decode(call, ref, got, keep).items():
                assert not dr.wrong_bits(implied, keep), f"{name} {call} {dt} {ch}: {dr.wrong_bits(implied, keep)[:4]}"
                assert worst <= 0.125, f"{name} {call} {dt} {ch}: rounding alone uses {worst:.3f} of the gate at {at}"


def test_inputs_are_exact_in_both_io_types_and_scores_are_zero():
    for c in dr.CASES:
        for call in "AB":
            x = c.build(call)
            for a in x.values():
                assert set(np.unique(a)).issubset({0.0, 1.0})
            B, Hq, Hk = c.dims(call)
            assert x["q"].shape[-2] == Hq and x["k"].shape[-2] == Hk
            # Q lives in dims [0, h), K in [h, 2 h): no score can be anything but 0
            assert not x["q"][..., c.h:].any() and not x["k"][..., :c.h].any()
            if c.alibi is not None:
                assert c.slopes(call).max() <= 2.0 ** -7


@pytest.mark.parametrize("name", ["d32_70x50_causal", "d96_130x131_win40_7", "alibi_d64_130x131_full",
                                  "alibi_bh_d128_130x131_causal", "gqa4_d128_129x66_win20_0"])
def test_restated_p_is_the_oracles(name):
    c = dr.BY_NAME[name]
    for call in "AB":
        x = c.build(call)
        t = lambda a: a.transpose(0, 2, 1, 3)
        ps = oracle.attn_fwd(t(x["q"]), t(x["k"]), t(x["v"]), c.scale, return_p=True, **c.oracle_kw(call, SEED, 0))[3]
        B, Hq, _ = c.dims(call)
        P = c.probs(call)[0]
        for b in range(B):
            for hq in range(Hq):
                assert np.abs(ps[b * Hq + hq] - P[b, hq]).max() <= 1e-15


def test_the_varlen_reading_covers_every_element_once():
    """every (i, j) of every sequence is read from a different element of the tensor (no two share one)"""
    c = dr.BY_NAME["varlen_gqa2_d64_causal"]
    for call, chs in dr.CHANNELS.items():
        B, Hq, Hk = c.dims(call)
        for ch in chs:
            H, T = (Hq, int(c.cu_q[-1])) if ch in ("o", "dq") else (Hk, int(c.cu_k[-1]))
            ids = np.arange(T * H * c.D, dtype=np.float64).reshape(T, H, c.D)
            flat = np.concatenate([g.reshape(-1) for g in c.gather(ch, ids)])
            assert flat.size == np.unique(flat).size


# ------------------------------------------------------------------------------------------------ sensitivity
# (sequence, i, j) per case: a ragged last column, a column with j % 4 == 3, an inner element, a row of the second 128-row
# query block.  Every row named here sees eight keys or more, so a forward-only flip - which also moves D_i of its row,
# by rp P_ij - leaves the row's other dS elements on their level (4 P_ij <= 1 / 2 of the gate).
FLIPS = [
    ("d64_130x203_full", [(0, 5, 202), (0, 77, 199), (0, 64, 100), (0, 129, 31)]),
    ("d128_257x259_causal", [(0, 256, 258), (0, 200, 3), (0, 130, 64), (0, 128, 129)]),
    ("d96_130x131_win40_7", [(0, 129, 130), (0, 60, 63), (0, 40, 20)]),
    ("gqa4_d64_130x203_full", [(0, 129, 202), (0, 1, 7)]),
    ("alibi_d128_130x131_full", [(0, 0, 130), (0, 129, 67)]),
    ("varlen_gqa2_d64_causal", [(2, 4, 130), (3, 129, 63), (0, 69, 32), (3, 128, 11)]),
    ("varlen_maxk_d64_causal", [(2, 0, 126), (3, 100, 7)]),
]
FLIP_IDS = [f"{n}-{s}_{i}_{j}" for n, els in FLIPS for s, i, j in els]
FLIP_ARGS = [(n, e) for n, els in FLIPS for e in els]


def _flip_named(name, elem, side, ignore=()):
    c = dr.BY_NAME[name]
    assert c.visible()[elem[0]][elem[1], elem[2]], "the flipped element must be visible"
    named = {}
    for call in "AB":
        ref, keep, off = _ref(name, call)
        got = c.reference(call, SEED, off, **{f"flip_{side}": elem})
        named.update(_named(c, call, ref, got, keep, ignore=ignore))
    return named


@pytest.mark.parametrize("name,elem", FLIP_ARGS, ids=FLIP_IDS)
def test_one_flipped_bit_is_named_in_exactly_the_affected_channels(name, elem):
    assert _flip_named(name, elem, "fwd") == {"o": {elem}, "dq": set(), "dk": set(), "dv": set()}
    assert _flip_named(name, elem, "bwd") == {"o": set(), "dq": {elem}, "dk": {elem}, "dv": {elem}}


@pytest.mark.parametrize("ch", ["o", "dq", "dk", "dv"])
def test_sensitivity_needs_every_channel(ch):
    """the control: with one channel left out of the decoder the comparison above does not hold"""
    name, elem = FLIP_ARGS[0]
    want = {"fwd": {"o": {elem}, "dq": set(), "dk": set(), "dv": set()},
            "bwd": {"o": set(), "dq": {elem}, "dk": {elem}, "dv": {elem}}}
    for side in ("fwd", "bwd"):
        assert _flip_named(name, elem, side, ignore=(ch,)) != want[side]


def test_a_flip_exceeds_the_gate_fourfold():
    """the gate is a quarter of what the element's own bit does to it: a flipped element sits at 4.0 of its gate (to the
    fp32 rounding of the LSE the oracle's backward takes its P from)"""
    name, elem = FLIP_ARGS[0]
    c = dr.BY_NAME[name]
    for call, side in (("A", "bwd"), ("B", "bwd"), ("B", "fwd")):
        ref, keep, off = _ref(name, call)
        got = c.reference(call, SEED, off, **{f"flip_{side}": elem})
        for ch, (_, worst, at) in c.decode(call, ref, got, keep).items():
            if (ch == "o") == (side == "fwd"):
                assert abs(worst - 4.0) < 1e-5 and at[0] == elem[0] and at[2:] == elem[1:], (ch, side, worst, at)


# ------------------------------------------------------------------------------------------------ the gap
GAP = [(64, 200, 200, True, 0.1, (199, 199)), (64, 200, 200, True, 0.1, (199, 100)),
       (128, 96, 130, True, 0.5, (95, 129)), (128, 760, 760, False, 0.1, (300, 511))]


def test_random_inputs_hide_one_flipped_bit_from_the_bf16_gates(capsys):
    """One keep bit flipped (forward and backward alike) on N(0, 1) data, one head: the change of each tensor as
    max-abs / max |ref|, next to the gates of the dropout tests (TOL_MAXREL x 1.5 for out, x 3 for the gradients)."""
    lines, hidden = [], 0
    for D, Sq, Sk, causal, p, (i, j) in GAP:
        q, k, v, do = (rand16(s, "bf16", 10 + n, device="cpu").double().numpy()
                       for n, s in enumerate([(1, 1, Sq, D), (1, 1, Sk, D), (1, 1, Sk, D), (1, 1, Sq, D)]))
        kw = dict(causal=causal, dropout_p=p, seed=SEED, offset=0)

        def run():
            o, lse, _ = oracle.attn_fwd(q, k, v, D ** -0.5, **kw)
            return (o,) + oracle.attn_bwd(do, q, k, v, oracle.round_to(o, "bf16"), lse.astype(np.float64), D ** -0.5, **kw)[:3]
        good = run()
        with dr.flipped((0, i, j)):
            bad = run()
        e = [float(np.abs(b - g).max() / np.abs(g).max()) for b, g in zip(bad, good)]
        gates = {dt: [TOL_MAXREL[dt] * m for m in (1.5, 3.0, 3.0, 3.0)] for dt in ("fp16", "bf16")}
        under = all(x <= g for x, g in zip(e, gates["bf16"]))
        hidden += under
        lines.append(f"D {D} {Sq} x {Sk} causal={causal} p {p} flip ({i}, {j}): out {e[0]:.1e} dq {e[1]:.1e} dk {e[2]:.1e} "
                     f"dv {e[3]:.1e}  worst {max(x / g for x, g in zip(e, gates['bf16'])):.2f} x its bf16 gate, "
                     f"{max(x / g for x, g in zip(e, gates['fp16'])):.1f} x its fp16 gate"
                     f"{'' if under else '  (seen by the bf16 gates)'}")
        assert min(e) > 0.0
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert hidden > len(GAP) // 2, f"the bf16 gates caught the flip in {len(GAP) - hidden} of {len(GAP)} cases: no gap"
