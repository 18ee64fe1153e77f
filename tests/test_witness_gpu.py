"""Witness data (tests/witness.py) through every attention kernel family, against the fp64 oracle.

Random N(0, 1) inputs let a mask mistake confined to a few rows hide below the bf16 gates (tests/test_witness_cpu.py
measures it); on witness data each row's probability sits on two keys at the mask's edges (pair rows), or would jump to
the first key outside it (decoy rows), or to a poisoned row no query may see, and the SAME gates - util.assert_close with
mult 1 for out and 2 for the gradients, assert_lse_close at LSE_ATOL times the fp32 ulp growth of witness.lse_atol -
catch a single wrong row.  The pair forward is also held to (V_a + V_b) / 2 within one ulp of the io type.  No kernel
output enters a reference; the oracle backward takes its own forward output rounded to the io type.

Worst error / gate per family (printed when the module finishes; 1.0 is the gate), MI355X, all 386 cases passing.  The
families name the forward and dQ kernels a case reaches (witness._dense_cases, _varlen_cases): at D 128 the dK/dV pass
is the hand-scheduled kernel in every family, and the D 64 cases at 400 - 520 rows are `hip` (the library has no D 64
hand-scheduled forward).

  family                                             out    lse    dq     dk     dv
  hip         (compiler-scheduled fwd / dQ)          0.515  0.076  0.421  0.347  0.307
  asm         (hand-scheduled, 256-row blocks)       0.497  0.114  0.488  0.351  0.296
  d256        (head dims 160 and 256)                0.425  0.076  0.421  0.259  0.246
  varlen      (823 rows in 5 sequences: hip)         0.378  0.076  0.394  0.240  0.211
  varlen_asm  (300, 520, 257: flat 256-row blocks)   0.354  0.076  0.370  0.202  0.218
  kvcache                                            0.534  0.076  -      -      -

The worst cases are bf16 roundings of `out` and of the gradients on decoy and `random` rows (several keys share a row);
the LSE stays within 1.5e-5 of the oracle at |LSE| up to 129.  The pair forward met (V_a + V_b) / 2 in every case.

tests/test_witness_features_gpu.py feeds the families added since (sinks, tree masks, shared prefix, further kv-cache
routes; 94 cases) through the helpers of this module.  Same run, all 94 passing; fp8-cache cases of these lists at the
fp8-cache gates (out 1.5 x, LSE_ATOL_FP8 grown with the fp32 ulp):

  family                                             out    lse    dq     dk     dv     dsinks
  sinks dense    (D 64 / 128 / 256, GQA and MQA)     0.364  0.050  0.424  0.229  0.294  0.274
  sinks varlen   (0, 1, 2, 300, 520; one paged)      0.331  0.076  0.404  0.226  0.238  0.005
  sinks kvcache  (16-bit and fp8, splits 0 1 3 5)    0.400  0.014  -      -      -      -
  kvcache routes (batch idx, D 256 / 96, fp8 T_q 5,  0.504  0.076  -      -      -      -
                  k=None, the general kernel)
  tree           (T 2 .. 64, own / root / decoy)     0.552  0.095  -      -      -      -
  shared prefix  (S_p 1 / 200 / 257, T 1 and 3)      0.538  0.076  -      -      -      -

No case of either file failed on the GPU, so no kernel changed.  Every tie row met (V_a + V_b) / 3 (V_a / 2 with one
target) within an ulp, every pair row of the tree and shared-prefix cases on 16-bit caches (V_a + V_b) / 2.

Cases and wall time of the witness GPU files on the MI355X (pytest's own total, references included):
  before   386 cases  33.1 s   (this file)
  now      480 cases  40.5 s   (this file 33.1 s + test_witness_features_gpu.py 94 cases in 7.4 s)
"""
import functools

import numpy as np
import pytest
import torch

import witness as w
from util import LSE_ATOL, LSE_ATOL_FP8, assert_close, assert_lse_close, f64

pytestmark = pytest.mark.gpu

WORST = {}                                                    # family -> {quantity: (ratio, case)}


def _fa():
    import flash_attn
    return flash_attn


def _record(fam, what, r, cid, worst=WORST):
    d = worst.setdefault(fam, {})
    if r > d.get(what, (-1.0, ""))[0]:
        d[what] = (r, cid)


def report(worst):
    for fam, d in worst.items():
        print(f"\nwitness {fam}: worst error / gate  " + "  ".join(f"{k} {r:.3f} [{c}]" for k, (r, c) in sorted(d.items())))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    report(WORST)


def _close(fam, cid, got, ref, dt, name, mult, worst=WORST):
    print(f"{cid} {dt} {name}: {w.ratio(got, ref, dt, mult):.3f} of the gate")
    _record(fam, name, w.ratio(got, ref, dt, mult), f"{cid} {dt}", worst)
    assert_close(got, ref, dt, f"{name} [{cid} {dt}]", mult=mult)


def _lse(fam, cid, got, ref, dt, worst=WORST, base=LSE_ATOL):
    atol = w.lse_atol(ref, base)
    _record(fam, "lse", w.lse_ratio(got, ref, atol), f"{cid} {dt}", worst)
    assert_lse_close(got, ref, f"lse [{cid} {dt}]", atol=atol)


def _pair_identity(got, pair, mag, o_ref, dt, tag):
    """out is the pair rows' closed form within one ulp of the io type, plus what is no rounding of the result: the keys a
    unit or more behind (the oracle's own o_ref - pair, <= 1e-6; with a tie sink the fp32 rounding of the sink value too)
    and, where V_a = -V_b cancel, the fp32 roundings of the two probabilities (exp2, rescale, normalise: 4 x 2^-24 of the
    operands' size `mag`)"""
    resid = np.abs(o_ref - pair).max() + 2.0 ** -22 * mag
    bad = np.abs(got - pair) > _ulp(pair, dt) + resid
    at = tuple(np.argwhere(bad)[0]) if bad.any() else None
    assert at is None, f"out is not the closed form of its targets within an ulp at {np.argwhere(bad)[:4].tolist()}: got " \
                       f"{got[at]!r}, want {pair[at]!r} [{tag} {dt}]"


def _ulp(x, dt):
    """spacing of the io type at |x| (fp16 subnormal spacing 2^-24 at the bottom)"""
    mant, emin = (10, -14) if dt == "fp16" else (7, -126)
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** emin)))
    return 2.0 ** (e - mant)


# ------------------------------------------------------------------------------------------------ dense
@functools.lru_cache(maxsize=2)
def _dense_ref(cid):
    kw = next(c[2] for c in w.DENSE_CASES if c[0] == cid)
    c = w.Dense(**kw)
    o, lse = c.forward()
    return c, o, lse


@pytest.mark.parametrize("cid,fam,force", [(c[0], c[1], c[3]) for c in w.DENSE_CASES], ids=[c[0] for c in w.DENSE_CASES])
def test_dense(cid, fam, force, monkeypatch):
    """forward and backward of one dense case in fp16 and bf16"""
    if force:
        monkeypatch.setenv("FA_ASM_FORCE", "1")
    c, o_ref, lse_ref = _dense_ref(cid)
    t = lambda x: f64(x).transpose(0, 2, 1, 3)
    for dt in ("fp16", "bf16"):
        q, k, v = (w.to_dev(x.transpose(0, 2, 1, 3), dt).requires_grad_(True) for x in (c.q, c.k, c.v))
        do = w.to_dev(c.do.transpose(0, 2, 1, 3), dt)
        slopes = None if c.alibi is None else torch.tensor(c.alibi, dtype=torch.float32, device="cuda")
        out, lse, _ = _fa().flash_attn_func(q, k, v, causal=c.causal, window_size=c.window, alibi_slopes=slopes,
                                            return_attn_probs=True)
        dq, dk, dv = torch.autograd.grad(out, (q, k, v), do)
        _close(fam, cid, t(out), o_ref, dt, "out", 1.0)
        _lse(fam, cid, f64(lse), lse_ref, dt)
        if c.variant != "decoy":
            _pair_identity(t(out), c.pair_out(), c.pair_out(magnitude=True), o_ref, dt, cid)
        g = c.backward(o_ref, lse_ref, dt)
        for name, got, ref in zip(("dq", "dk", "dv"), (dq, dk, dv), g):
            _close(fam, cid, t(got), ref, dt, name, 2.0)


# ------------------------------------------------------------------------------------------------ varlen
@pytest.mark.parametrize("cid,fam,kw,force", w.VARLEN_CASES, ids=[c[0] for c in w.VARLEN_CASES])
def test_varlen(cid, fam, kw, force, monkeypatch):
    """packed sequences that are poison to each other; seqused_k and paged K/V forward only, with poisoned tails"""
    if force:
        monkeypatch.setenv("FA_ASM_FORCE", "1")
    c = w.Varlen(**kw)
    o_ref, lse_ref = c.forward()
    bwd = c.used is None and not c.page
    ti = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")
    for dt in ("fp16", "bf16"):
        q, k, v = (w.to_dev(x, dt).requires_grad_(bwd) for x in (c.q, c.k, c.v))
        extra = {}
        if c.used is not None:
            extra["seqused_k"] = ti(c.used)
        if c.page:
            extra["block_table"] = ti(c.block_table)
        out, lse, _ = _fa().flash_attn_varlen_func(q, k, v, ti(c.cu_q), ti(c.cu_k), c.mq, c.mk, causal=c.causal,
                                                   return_attn_probs=True, **extra)
        if bwd:
            dq, dk, dv = torch.autograd.grad(out, (q, k, v), w.to_dev(c.do, dt))
        _close(fam, cid, f64(out), o_ref, dt, "out", 1.0)
        _lse(fam, cid, f64(lse), lse_ref, dt)
        if bwd:
            g = c.backward(o_ref, lse_ref, dt)
            for name, got, ref in zip(("dq", "dk", "dv"), (dq, dk, dv), g):
                _close(fam, cid, f64(got), ref, dt, name, 2.0)


# ------------------------------------------------------------------------------------------------ kv-cache decode
@functools.lru_cache(maxsize=2)
def _kv_ref(cid):
    kw = next(c[1] for c in w.KVCACHE_CASES if c[0] == cid)
    c = w.KVCache(**kw)
    return (c,) + c.forward()


def ti(x):
    return None if x is None else torch.tensor(np.asarray(x), dtype=torch.int32, device="cuda")


def dev_caches(c, dt):
    if c.fp8:
        return tuple(torch.from_numpy(x).float().to(torch.float8_e4m3fn).cuda() for x in (c.kc, c.vc))
    return w.to_dev(c.kc, dt), w.to_dev(c.vc, dt)


def check_caches(kc, vc, kc_ref, vc_ref, dt, tag):
    kg, vg = kc.float().double().cpu().numpy(), vc.float().double().cpu().numpy()
    tol = 2.0 ** (-7 if dt == "bf16" else -10)
    assert np.abs(kg - kc_ref).max() <= tol * max(1.0, np.abs(kc_ref).max()), f"k cache differs [{tag} {dt}]"
    assert np.array_equal(vg, vc_ref), f"v cache differs [{tag} {dt}]"


def run_kvcache(c, refs, splits, fam, tag, worst=WORST, fp8_gates=False):
    """one witness.KVCache case through flash_attn_with_kvcache in fp16 and bf16.  fp8_gates: out at 1.5 x and the LSE at
    LSE_ATOL_FP8 (grown with the fp32 ulp), the gates of the fp8-cache tests, for an fp8 case"""
    o_ref, lse_ref, kc_ref, vc_ref = refs
    wide = fp8_gates and c.fp8
    for dt in ("fp16", "bf16"):
        kc, vc = dev_caches(c, dt)
        new = dict(k=w.to_dev(c.knew, dt), v=w.to_dev(c.vnew, dt), cache_seqlens=ti(c.seqlens)) if c.append else \
            dict(cache_seqlens=ti(c.seqlens + c.tq))
        extra = {} if c.sinks is None else dict(sinks=torch.tensor(c.sinks, dtype=torch.float32, device="cuda"))
        out, lse = _fa().flash_attn_with_kvcache(
            w.to_dev(c.q, dt), kc, vc, cache_batch_idx=ti(c.bidx), cache_leftpad=ti(c.leftpad), block_table=ti(c.block_table),
            causal=c.causal, window_size=c.window, num_splits=splits, return_softmax_lse=True, k_descale=c.kd,
            v_descale=c.vd, **new, **extra)
        check_caches(kc, vc, kc_ref, vc_ref, dt, tag)
        _close(fam, tag, f64(out), o_ref, dt, "out", 1.5 if wide else 1.0, worst)
        _lse(fam, tag, f64(lse), lse_ref, dt, worst, LSE_ATOL_FP8 if wide else LSE_ATOL)


@pytest.mark.parametrize("splits", w.SPLITS)
@pytest.mark.parametrize("cid", [c[0] for c in w.KVCACHE_CASES])
def test_kvcache(cid, splits):
    """decode with an append: the first cached and the last appended key carry each row, every stale row, every row
    below the left pad and every unreferenced page is poison; the caches after the call hold the appended rows"""
    c, *refs = _kv_ref(cid)
    run_kvcache(c, refs, splits, "kvcache", f"{cid}-splits{splits}")
