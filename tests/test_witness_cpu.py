"""The witness data of tests/witness.py does what it claims - shown on the CPU oracle, for every case of the GPU list.

  * design: from the integer score matrix every row with two visible keys or more has two targets that tie exactly, any
    third key a unit (U scale: 16 nats at D 256, 32 at D 64) or more behind; the keys fit the code capacity; every
    reference gradient stays below 1/8 of the fp16 range (8188; largest: |dK| 6073 in the varlen D 128 `edges` case, where
    dK of the poisoned dim sums 8 U dS; dense 4235 at 1300 x 1300 with four heads on one key head);
  * sensitivity: the oracle itself computes what a kernel with one localised mask mistake would (witness.mistakes: one
    32-row band or one single row loses a target or gains the first invisible key; witness.leak_forward: rows see one
    poisoned row).  Each mistake must move out, LSE, dq, dk or dv by 10 x the gate tests/test_witness_gpu.py uses, with
    the wider (bf16) gates - which covers fp16's.  Pair mistakes go into the backward's P (the forward has its LSE),
    decoy and poison mistakes into the forward;
  * the gap: the same kind of mistake on N(0, 1) inputs at S 1300, D 128 stays below the bf16 gates in the backward;
  * oracle timing: measured here per call, forward / backward: dense 1300 x 1300 with 4 heads 0.20 / 0.28 s, the very
    first call of the run 0.48 / 0.60 s (the largest), varlen 0.05 / 0.06 s, kv-cache 0.08 s (64 heads).  The bound is 60
    unit calls (one 650 x 650 head forward, 0.09 s here, timed in the same run) per oracle call.
"""
import time

import numpy as np
import pytest

import oracle
import witness as w
from util import LSE_ATOL, TOL_MAXREL, rand16

FACTOR = 10.0                                                 # a mistake must exceed the GPU test's gate this many times
GATE = {"out": TOL_MAXREL["bf16"] * 1.0, "grad": TOL_MAXREL["bf16"] * 2.0}     # the wider of the two dtypes' gates
assert TOL_MAXREL["bf16"] >= TOL_MAXREL["fp16"]


@pytest.fixture(scope="module")
def unit():
    """seconds of one unit oracle call on this machine (best of three)"""
    x = np.ones((1, 1, 650, 128))
    best = 1e9
    for _ in range(3):
        t = time.perf_counter()
        oracle.attn_fwd(x, x, x, 0.1, causal=True)
        best = min(best, time.perf_counter() - t)
    return best


def _timed(fn, unit, what, budget=60):
    t = time.perf_counter()
    r = fn()
    dt = time.perf_counter() - t
    assert dt <= max(budget * unit, 0.05), f"{what}: the oracle took {dt:.2f} s, {dt / unit:.0f} unit calls"
    return r


def _rel(x, y, top):
    return float(np.abs(np.asarray(x) - np.asarray(y)).max(initial=0.0) / top)


def _fwd_factor(o, lse, o0, lse0, otop, atol):
    """how many times its gate the largest of the out and LSE changes is"""
    return max(_rel(o, o0, otop) / GATE["out"], w.lse_ratio(lse, lse0, atol))


# ------------------------------------------------------------------------------------------------ dense
@pytest.mark.parametrize("cid", [c[0] for c in w.DENSE_CASES])
def test_dense_case_is_decisive(cid, unit):
    kw = next(c[2] for c in w.DENSE_CASES if c[0] == cid)
    c = w.Dense(**kw)
    assert c.sk <= w.capacity(c.D)
    pairs, bad = c.design()
    assert bad == 0, f"{bad} of {pairs} pair rows miss the tie or the one-unit margin"
    if c.variant != "decoy":
        assert pairs == c.B * c.hq * int((c.vis.sum(axis=1) >= 2).sum())
    o, lse = _timed(c.forward, unit, "forward")
    g = _timed(lambda: c.backward(o, lse, "bf16"), unit, "backward")          # (asserts the gradient cap)
    if c.variant != "decoy":
        assert np.abs(o - c.pair_out()).max() < 2e-6
    # one head alone, clean and with each mistake; errors relative to the whole reference, as the GPU gate takes them
    grp = c.hq // c.hk
    one = lambda x, h: x[:1, h:h + 1]
    h = c.hq - 1
    q, k, v, do = one(c.q, h), one(c.k, h // grp), one(c.v, h // grp), one(c.do, h)
    al = None if c.alibi is None else c.alibi[h:h + 1]
    a, b = c.a[0, h], c.b[0, h]
    todo = w.mistakes(c.vis, c.variant, a, b)
    assert len(todo) >= 2, "no mistake bites on this case"
    normal = dict(causal=c.causal, window=c.window, alibi_slopes=al)
    if c.variant == "decoy":
        o0, l0, _ = oracle.attn_fwd(q, k, v, c.scale, **normal)
        for name, vis in todo:
            assert not np.array_equal(vis, c.vis), name
            with w.patched_mask(vis):
                o1, l1, _ = oracle.attn_fwd(q, k, v, c.scale, **normal)
            f = _fwd_factor(o1, l1, o0, l0, np.abs(o).max(), w.lse_atol(lse))
            assert f >= FACTOR, f"{name}: only {f:.1f} x the forward gates"
        return
    lse1 = one(lse, h).astype(np.float64)
    o16 = oracle.round_to(one(o, h), "bf16")
    g0 = oracle.attn_bwd(do, q, k, v, o16, lse1, c.scale, **normal)[:3]
    for name, vis in todo:
        assert not np.array_equal(vis, c.vis), name
        with w.patched_mask(vis):
            g1 = oracle.attn_bwd(do, q, k, v, o16, lse1, c.scale, **normal)[:3]
        f = max(_rel(x1, x0, np.abs(ref).max()) for x1, x0, ref in zip(g1, g0, g)) / GATE["grad"]
        assert f >= FACTOR, f"{name}: only {f:.1f} x the gradient gates"


# ------------------------------------------------------------------------------------------------ varlen
def _poison(D):
    k = np.zeros(D)
    k[D - 2:] = 1.0
    return k, np.full(D, w.POISON_V)


@pytest.mark.parametrize("cid,fam,kw,force", w.VARLEN_CASES, ids=[c[0] for c in w.VARLEN_CASES])
def test_varlen_case_is_decisive(cid, fam, kw, force, unit):
    c = w.Varlen(**kw)
    assert max(c.lens_k) <= w.capacity(c.D)
    pairs, bad = c.design()
    assert bad == 0, f"{bad} of {pairs} pair rows miss the tie or the one-unit margin"
    o, lse = _timed(c.forward, unit, "forward")
    assert np.abs(o).max() < 8.0, "a poisoned row reached the reference"
    bwd = c.used is None and not c.page
    atol = w.lse_atol(lse)
    s = int(np.argmax(c.lens_q))                              # the longest sequence, its last head
    h, grp = c.hq - 1, c.hq // c.hk
    q0, k0, vis = int(c.cu_q[s]), int(c.cu_k[s]), c.vis[s]
    sq, sk = vis.shape
    if bwd:
        g = _timed(lambda: c.backward(o, lse, "bf16"), unit, "backward")
        # the backward's P loses a target / gains a decoy in one band or row of that sequence (all heads)
        assert sum(v_.shape == vis.shape for v_ in c.vis) == 1
        for name, bad_vis in w.mistakes(vis, c.variant, c.a[s][h], c.b[s][h]):
            with w.patched_mask(bad_vis):
                g1 = c.backward(o, lse, "bf16") if c.variant != "decoy" else None
                o1, l1 = c.forward() if c.variant == "decoy" else (None, None)
            if c.variant == "decoy":
                f = _fwd_factor(o1, l1.astype(np.float64), o, lse, np.abs(o).max(), atol)
            else:
                f = max(_rel(x1, x0, np.abs(x0).max()) for x1, x0 in zip(g1, g)) / GATE["grad"]
            assert f >= FACTOR, f"{name}: only {f:.1f} x the gates"
    # poison: one row, then a band, of that sequence sees one row it must not
    if c.page:
        kk = c.k[c.block_table[s, np.arange(sk) // c.page], np.arange(sk) % c.page, h // grp]
        vv = c.v[c.block_table[s, np.arange(sk) // c.page], np.arange(sk) % c.page, h // grp]
        leaks = [("page tail", c.k[c.block_table[s, (c.lens_k[s] - 1) // c.page], -1, 0],
                  c.v[c.block_table[s, (c.lens_k[s] - 1) // c.page], -1, 0]),
                 ("unreferenced page", c.k[c.spare[0], 0, 0], c.v[c.spare[0], 0, 0])]
        if c.lens_k[s] % c.page == 0:
            leaks = leaks[1:]
    else:
        kk, vv = c.k[k0:k0 + sk, h // grp], c.v[k0:k0 + sk, h // grp]
        if c.used is not None:
            leaks = [("key past seqused_k", c.k[k0 + sk, 0], c.v[k0 + sk, 0])]
        else:
            leaks = [("previous sequence", c.k[k0 - 1, 0], c.v[k0 - 1, 0])]
            if k0 + c.lens_k[s] < c.k.shape[0]:
                leaks.append(("next sequence", c.k[k0 + c.lens_k[s], 0], c.v[k0 + c.lens_k[s], 0]))
    qq = c.q[q0:q0 + sq, h]
    o0, l0 = w.leak_forward(qq, kk, vv, vis, c.scale)
    assert np.abs(o0 - o[q0:q0 + sq, h]).max() < 1e-9
    for name, kl, vl in leaks:
        for rows in (np.arange(sq - 40, sq - 8), np.array([sq - 1])):
            o1, l1 = w.leak_forward(qq, kk, vv, vis, c.scale, rows, kl, vl)
            f = _fwd_factor(o1, l1, o0, l0, np.abs(o).max(), atol)
            assert f >= FACTOR, f"{name} seen by rows {rows[0]}..{rows[-1]}: only {f:.1f} x the forward gates"


# ------------------------------------------------------------------------------------------------ kv-cache decode
@pytest.mark.parametrize("cid,kw", w.KVCACHE_CASES, ids=[c[0] for c in w.KVCACHE_CASES])
def test_kvcache_case_is_decisive(cid, kw, unit):
    c = w.KVCache(**kw)
    pairs, bad = c.design()
    assert bad == 0 and pairs > 0, f"{bad} of {pairs} pair rows miss the tie or the one-unit margin"
    o, lse, kc, vc = _timed(c.forward, unit, "forward")
    assert np.abs(o).max() < 8.0, "a poisoned row reached the reference"
    atol = w.lse_atol(lse)
    kd, vd = c.kd or 1.0, c.vd or 1.0
    kp, vp = _poison(c.D)
    h, grp = c.hq - 1, c.hq // c.hk
    for s in range(c.B):
        vis = c.vis[s]
        sk = vis.shape[1]
        lp = 0 if c.leftpad is None else int(c.leftpad[s])
        pos = lp + np.arange(sk)
        if c.page:
            kk, vv = (x[c.block_table[s, pos // c.page], pos % c.page, h // grp] for x in (kc, vc))
        else:
            kk, vv = kc[s, pos, h // grp], vc[s, pos, h // grp]
            # the memory around the visible keys is poison: the first stale row, the row below the left pad
            assert np.array_equal(kc[s, lp + sk, 0] * kd, kp) and np.array_equal(vc[s, lp + sk, 0] * vd, vp)
            if lp:
                assert np.array_equal(kc[s, lp - 1, 0] * kd, kp) and np.array_equal(vc[s, lp - 1, 0] * vd, vp)
        kk, vv, qq = kk * kd, vv * vd, c.q[s, :, h]
        o0, l0 = w.leak_forward(qq, kk, vv, vis, c.scale)
        assert np.abs(o0 - o[s, :, h]).max() < 1e-9
        # wrongful exclusion: a row loses its first cached / last appended target (the forward's LSE and out see it)
        for name, bad_vis in w.mistakes(vis, "edges"):
            with w.patched_mask(bad_vis):
                o1, l1, _ = oracle.attn_fwd(qq[None, None], kk[None, None], vv[None, None], c.scale, normalize=False)
            f = _fwd_factor(o1[0, 0], l1[0, 0], o0, l0, np.abs(o).max(), atol)
            assert f >= FACTOR, f"batch {s} {name}: only {f:.1f} x the forward gates"
        # stale rows, rows below the left pad and unreferenced pages all hold the same poison: one row sees one
        o1, l1 = w.leak_forward(qq, kk, vv, vis, c.scale, np.array([c.tq - 1]), kp, vp)
        f = _fwd_factor(o1, l1, o0, l0, np.abs(o).max(), atol)
        assert f >= FACTOR, f"batch {s}, a poisoned row seen: only {f:.1f} x the forward gates"
    if c.page:
        used = set(c.block_table.reshape(-1).tolist())
        assert c.spare and not used & set(c.spare)
        for blk in c.spare:
            assert np.array_equal(kc[blk, :, 0] * kd, np.tile(kp, (c.page, 1)))


# ------------------------------------------------------------------------------------------------ the gap
def test_random_inputs_hide_the_same_mistake_from_the_bf16_gates(capsys):
    """N(0, 1) bf16 inputs, S 1300, D 128, causal, one head: the backward's P drops the diagonal key for rows 1024..1055.
    Measured here over 6 draws (max error / max |ref|): dq 2.6e-3 .. 2.9e-2, dk 1.6e-3 .. 2.1e-2, dv 1.3e-3 .. 7.5e-3 - under
    the bf16 gradient gate (1.4e-2) in 5 draws of 6, over the fp16 one (2e-3) in all 6.  The witness `edges` case of the
    same shape answers the same mistake, even in a single row, with 10 x the bf16 gate or more
    (test_dense_case_is_decisive)."""
    S, D, draws = 1300, 128, 6
    vis = w.visible(S, S, True, (-1, -1))
    bad = w.mutate_mask(vis, "lose_last", np.arange(1024, 1056))
    hidden = seen16 = 0
    lines = []
    for d in range(draws):
        q, k, v, do = (rand16((1, 1, S, D), "bf16", 100 * d + i, device="cpu").double().numpy() for i in range(4))
        o, lse, _ = oracle.attn_fwd(q, k, v, D ** -0.5, causal=True)
        args = (do, q, k, v, oracle.round_to(o, "bf16"), lse.astype(np.float64), D ** -0.5)
        g0 = oracle.attn_bwd(*args, causal=True)[:3]
        with w.patched_mask(bad):
            g1 = oracle.attn_bwd(*args, causal=True)[:3]
        e = [_rel(x1, x0, np.abs(x0).max()) for x1, x0 in zip(g1, g0)]
        hidden += max(e) <= 2 * TOL_MAXREL["bf16"]
        seen16 += max(e) > 2 * TOL_MAXREL["fp16"]
        lines.append(f"draw {d}: dq {e[0]:.1e} dk {e[1]:.1e} dv {e[2]:.1e}  ({max(e) / (2 * TOL_MAXREL['bf16']):.2f} x the bf16 gate, "
                     f"{max(e) / (2 * TOL_MAXREL['fp16']):.1f} x the fp16 gate)")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert hidden > draws // 2, f"the bf16 gates caught the mistake in {draws - hidden} of {draws} draws: no gap"
    assert seen16 > draws // 2


def test_lse_gate_follows_the_fp32_ulp():
    assert w.lse_atol(np.array([5.0, -np.inf])) == LSE_ATOL
    assert w.lse_atol(np.array([91.2])) == 2 * LSE_ATOL
    assert w.lse_atol(np.array([128.7])) == 4 * LSE_ATOL
