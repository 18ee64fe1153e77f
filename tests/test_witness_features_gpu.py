"""Witness data (tests/witness.py) through what the attention core gained after the plain paths: attention sinks (dense
forward and backward with dsinks, varlen, kv-cache with split-KV), tree masks, shared-prefix decode, and the kv-cache
routes the first witness list never reached.  Same conventions and gates as tests/test_witness_gpu.py, whose helpers run
here: one fp64 reference for fp16 and bf16, no kernel output in a reference, util.assert_close with mult 1 for out and 2
for the gradients (dsinks among them), assert_lse_close at witness.lse_atol; the fp8-cache cases of THESE lists take the
gates of the fp8-cache tests, out 1.5 x and LSE_ATOL_FP8 grown like the 16-bit one.  tests/test_witness_cpu.py shows on
the oracle that each case answers a dropped or doubled sink, one tree bit at a word boundary, a V row from the
neighbouring slot, a neighbour's merge weights and a poisoned row with 10 x these gates or more.

Out of scope here, with the reasons in witness.py: softcap, rotary, ALiBi with sinks, the fp8 q / k / v forward.

Identities held besides the gates: a tie row's out is (V_a + V_b) / 3 (V_a / 2 with one target), a pair row's
(V_a + V_b) / 2, within one ulp of the io type (16-bit caches; the fp8 row-block kernels carry each probability as two
e4m3 terms, about 2^-8 relative, so only the gates hold there); a row without keys gives out 0 and LSE = s_h; the
caches after a call hold the appended rows and nothing else changed.

Which kernel a case reaches is said next to it in witness._sink_dense_cases, _route_cases and _tree_cases.  The worst
error / gate per family of this file, from the MI355X run, stands in the table of tests/test_witness_gpu.py.
"""
import functools

import pytest
import torch

import witness as w
from test_witness_gpu import _close, _lse, _pair_identity, check_caches, dev_caches, report, run_kvcache, ti
from util import LSE_ATOL, LSE_ATOL_FP8, f64

pytestmark = pytest.mark.gpu

WORST = {}                                                    # family -> {quantity: (ratio, case)}


def _fa():
    import flash_attn
    return flash_attn


def _mi():
    import flash_attn_mi355
    return flash_attn_mi355


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    report(WORST)


def _sinks(c):
    return None if c.sinks is None else torch.tensor(c.sinks, dtype=torch.float32, device="cuda")


def _forward_gates(c, fam, tag, out, lse, o_ref, lse_ref, dt):
    _close(fam, tag, f64(out), o_ref, dt, "out", 1.5 if c.fp8 else 1.0, WORST)
    _lse(fam, tag, f64(lse), lse_ref, dt, WORST, LSE_ATOL_FP8 if c.fp8 else LSE_ATOL)


# ------------------------------------------------------------------------------------------------ sinks, dense
@functools.lru_cache(maxsize=2)
def _sink_dense_ref(cid):
    c = w.SinkDense(**next(x[2] for x in w.SINK_DENSE_CASES if x[0] == cid))
    return (c,) + c.forward()


@pytest.mark.parametrize("cid,fam,force", [(c[0], c[1], c[3]) for c in w.SINK_DENSE_CASES], ids=[c[0] for c in w.SINK_DENSE_CASES])
def test_sink_dense(cid, fam, force, monkeypatch):
    """flash_attn_sinks_func forward and backward: every row ties with its head's sink (1/3 or 1/2 of the row), next to
    heads whose sink is -inf or 16 nats behind; dq, dk, dv and dsinks against the oracle's backward on the sink-inclusive
    LSE and its own rounded out"""
    if force:
        monkeypatch.setenv("FA_ASM_FORCE", "1")
    c, o_ref, lse_ref = _sink_dense_ref(cid)
    t = lambda x: f64(x).transpose(0, 2, 1, 3)
    nokey = c.vis.sum(axis=1) == 0
    for dt in ("fp16", "bf16"):
        q, k, v = (w.to_dev(x.transpose(0, 2, 1, 3), dt).requires_grad_(True) for x in (c.q, c.k, c.v))
        sinks = _sinks(c).requires_grad_(True)
        out, lse, _ = _mi().flash_attn_sinks_func(q, k, v, sinks, causal=c.causal, window_size=c.window, return_attn_probs=True)
        dq, dk, dv, ds = torch.autograd.grad(out, (q, k, v, sinks), w.to_dev(c.do.transpose(0, 2, 1, 3), dt))
        _close("sinks dense", cid, t(out), o_ref, dt, "out", 1.0, WORST)
        _lse("sinks dense", cid, f64(lse), lse_ref, dt, WORST)
        _pair_identity(t(out), c.pair_out(), c.pair_out(magnitude=True), o_ref, dt, cid)
        assert not t(out)[:, :, nokey].any(), "a row without keys has out != 0"
        g = c.backward(o_ref, lse_ref, dt)
        for name, got, ref in zip(("dq", "dk", "dv"), (dq, dk, dv), g):
            _close("sinks dense", cid, t(got), ref, dt, name, 2.0, WORST)
        _close("sinks dense", cid, f64(ds), g[3], dt, "dsinks", 2.0, WORST)


# ------------------------------------------------------------------------------------------------ sinks, varlen
@pytest.mark.parametrize("cid,kw", w.SINK_VARLEN_CASES, ids=[c[0] for c in w.SINK_VARLEN_CASES])
def test_sink_varlen(cid, kw):
    """flash_attn_varlen_func(sinks=) on lengths 0, 1, 2, 300, 520 that are poison to each other; the paged case forward
    only, with poisoned page tails and spare pages"""
    c = w.SinkVarlen(**kw)
    o_ref, lse_ref = c.forward()
    bwd = not c.page
    for dt in ("fp16", "bf16"):
        q, k, v = (w.to_dev(x, dt).requires_grad_(bwd) for x in (c.q, c.k, c.v))
        sinks = _sinks(c).requires_grad_(bwd)
        extra = dict(block_table=ti(c.block_table)) if c.page else {}
        out, lse, _ = _fa().flash_attn_varlen_func(q, k, v, ti(c.cu_q), ti(c.cu_k), c.mq, c.mk, causal=c.causal,
                                                   return_attn_probs=True, sinks=sinks, **extra)
        if bwd:
            dq, dk, dv, ds = torch.autograd.grad(out, (q, k, v, sinks), w.to_dev(c.do, dt))
        _close("sinks varlen", cid, f64(out), o_ref, dt, "out", 1.0, WORST)
        _lse("sinks varlen", cid, f64(lse), lse_ref, dt, WORST)
        if bwd:
            _pair_identity(f64(out), c.pair_out(), c.pair_out(magnitude=True), o_ref, dt, cid)
            g = c.backward(o_ref, lse_ref, dt)
            for name, got, ref in zip(("dq", "dk", "dv", "dsinks"), (dq, dk, dv, ds), g):
                _close("sinks varlen", cid, f64(got), ref, dt, name, 2.0, WORST)


# ------------------------------------------------------------------------------------------------ kv-cache: sinks, routes
@functools.lru_cache(maxsize=2)
def _kv_ref(cid):
    c = w.KVCache(**next(x[1] for x in w.SINK_KVCACHE_CASES + w.ROUTE_CASES if x[0] == cid))
    return (c,) + c.forward()


@pytest.mark.parametrize("splits", w.SPLITS)
@pytest.mark.parametrize("cid", [c[0] for c in w.SINK_KVCACHE_CASES])
def test_sink_kvcache(cid, splits):
    """flash_attn_with_kvcache(sinks=) with an append: the sink must enter once however many key splits there are (n times
    would give it n / (n + 2) of a row instead of 1/3)"""
    c, *refs = _kv_ref(cid)
    run_kvcache(c, refs, splits, "sinks kvcache", f"{cid}-splits{splits}", WORST, fp8_gates=True)


@pytest.mark.parametrize("cid,splits", [(c[0], s) for c in w.ROUTE_CASES for s in c[2]])
def test_kvcache_route(cid, splits):
    """cache_batch_idx with poisoned unreferenced rows, D 256 and a narrow width, fp8 caches with T_q 5 on the
    head-per-wave and row-block routes, k=None, and a call the decode kernels decline (the general kernel on the cache)"""
    c, *refs = _kv_ref(cid)
    run_kvcache(c, refs, splits, "kvcache routes", f"{cid}-splits{splits}", WORST, fp8_gates=True)


# ------------------------------------------------------------------------------------------------ tree masks
@pytest.mark.parametrize("cid,kw,splits", w.TREE_CASES, ids=[c[0] for c in w.TREE_CASES])
def test_tree(cid, kw, splits):
    """flash_attn_with_kvcache(tree_mask=): pair rows on a committed key and a visible tree column, decoy rows on two
    invisible ones; the mask as a bool matrix or packed words, per batch entry or shared"""
    c = w.Tree(**kw)
    o_ref, lse_ref, kc_ref, vc_ref = c.forward()
    mask = torch.from_numpy(c.call_mask()).cuda()
    for dt in ("fp16", "bf16"):
        kc, vc = dev_caches(c, dt)
        new = dict(k=w.to_dev(c.knew, dt), v=w.to_dev(c.vnew, dt), cache_seqlens=ti(c.seqlens)) if c.append else \
            dict(cache_seqlens=ti(c.seqlens + c.T))
        out, lse = _fa().flash_attn_with_kvcache(
            w.to_dev(c.q, dt), kc, vc, cache_leftpad=ti(c.leftpad), block_table=ti(c.block_table), causal=True,
            num_splits=splits, return_softmax_lse=True, k_descale=c.kd, v_descale=c.vd, sinks=_sinks(c), tree_mask=mask,
            **new)
        check_caches(kc, vc, kc_ref, vc_ref, dt, cid)
        _forward_gates(c, "tree", cid, out, lse, o_ref, lse_ref, dt)
        if c.variant != "decoy" and not c.fp8:
            _pair_identity(f64(out), c.pair_out(), c.pair_out(magnitude=True), o_ref, dt, cid)


# ------------------------------------------------------------------------------------------------ shared prefix
@pytest.mark.parametrize("cid,kw", w.PREFIX_CASES, ids=[c[0] for c in w.PREFIX_CASES])
def test_shared_prefix(cid, kw):
    """flash_attn_with_shared_prefix: targets on both sides of the merge (weights 1/2, 1/2), on one side only (1, 0 and
    0, 1 in neighbouring sequences), the next appended token and the poison as decoys"""
    from flash_attn_mi355 import cascade
    c = w.SharedPrefix(**kw)
    o_ref, lse_ref = c.forward()
    kc_ref, vc_ref = c.after()
    for dt in ("fp16", "bf16"):
        kc, vc = dev_caches(c, dt)
        new = dict(k=w.to_dev(c.knew, dt), v=w.to_dev(c.vnew, dt)) if c.append else {}
        out, lse = cascade.flash_attn_with_shared_prefix(
            w.to_dev(c.q, dt), w.to_dev(c.pk, dt), w.to_dev(c.pv, dt), kc, vc, cache_seqlens=ti(c.seqlens),
            cache_batch_idx=ti(c.bidx), block_table=ti(c.block_table), k_descale=c.kd, v_descale=c.vd, sinks=_sinks(c),
            return_softmax_lse=True, **new)
        check_caches(kc, vc, kc_ref, vc_ref, dt, cid)
        _forward_gates(c, "shared prefix", cid, out, lse, o_ref, lse_ref, dt)
        if c.variant != "decoy" and not c.fp8:
            _pair_identity(f64(out), c.pair_out(), c.pair_out(magnitude=True), o_ref, dt, cid)
