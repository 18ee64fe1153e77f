"""GPU: flash_attn_with_shared_prefix (flash_attn_mi355/cascade.py) against the oracle's attention over the CONCATENATED keys of
every sequence - [prefix ; its own cache ; the appended tokens] - a CPU computation that shares nothing with the three launches
under test.

Tolerance: util.assert_close(mult=2.0) and assert_lse_close.  Why 2: each 16-bit partial (prefix pass, suffix pass) carries at
most the calibrated gate error and enters with a weight w_s, sum w_s = 1; the rounding of the merged result adds at most another
half ulp (tests/test_kvcache_gpu.py uses the same factor for its rotary cases).  The fp8 suffix cache keeps the gates of the
kv-cache fp8 tests (out 1.5 x, LSE_ATOL_FP8): the oracle reads the same codes."""
import numpy as np
import pytest
import torch

import guard
import oracle
from sink_ref import sink_identity_bshd
from util import DT, LSE_ATOL_FP8, assert_close, assert_lse_close, errs, f64, rand16

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
SUFFIX = [0, 5, 130]                                   # tokens each sequence holds after the prefix
KD, VD = 0.05, 0.04


def _fa():
    import flash_attn
    return flash_attn


def _cascade():
    from flash_attn_mi355 import cascade
    return cascade


class Case:
    """One problem: the logical data, the suffix cache in the physical layout the case asks for, and the fp64 reference cache that
    holds [prefix ; suffix] per sequence."""

    def __init__(self, T, dt="bf16", H=8, Hk=2, D=128, S_p=200, layout="contig", fp8=False, append=True, seed=0):
        B = len(SUFFIX)
        self.B, self.T, self.dt, self.H, self.Hk, self.D, self.S_p, self.fp8 = B, T, dt, H, Hk, D, S_p, fp8
        self.lens = torch.tensor(SUFFIX, dtype=torch.int32)
        Tn = T if append else 0
        cap = max(SUFFIX) + Tn + 6
        self.q = rand16((B, T, H, D), dt, seed + 1)
        self.pk, self.pv = rand16((S_p, Hk, D), dt, seed + 2), rand16((S_p, Hk, D), dt, seed + 3)
        if fp8:
            # (the plain kv-cache op this is compared with keeps the prefix in the fp8 cache: give the 16-bit prefix values that
            #  survive that trip - code x descale, rounded to 16 bits - so that both see the same prefix up to that rounding)
            self.pk = ((self.pk.float() / KD).to(FP8).float() * KD).to(DT[dt])
            self.pv = ((self.pv.float() / VD).to(FP8).float() * VD).to(DT[dt])
        sc = 1.5 if fp8 else 1.0
        sk, sv = rand16((B, cap, Hk, D), dt, seed + 4, scale=sc), rand16((B, cap, Hk, D), dt, seed + 5, scale=sc)
        if fp8:
            sk, sv = (sk.float() / KD).to(FP8), (sv.float() / VD).to(FP8)
        self.knew = rand16((B, Tn, Hk, D), dt, seed + 6) if append else None
        self.vnew = rand16((B, Tn, Hk, D), dt, seed + 7) if append else None
        self.bidx = self.bt = None
        if layout == "contig":
            self.kc, self.vc = sk.clone(), sv.clone()
        elif layout == "batch_idx":
            self.bidx = torch.tensor([B + 1 - i for i in range(B)], dtype=torch.int32)
            self.kc = torch.zeros((B + 2,) + tuple(sk.shape[1:]), dtype=sk.dtype, device="cuda")
            self.vc = self.kc.clone()
            self.kc[self.bidx.long().cuda()] = sk
            self.vc[self.bidx.long().cuda()] = sv
        else:                                          # paged: 16-token pages in a shuffled table, stale entries on a NaN page
            page = 16
            bt, nblk, nan_page = guard.paged_table([l + Tn for l in SUFFIX], page, seed=seed + 8)
            self.kc = guard.fill_nan(torch.empty((nblk, page, Hk, D), dtype=sk.dtype, device="cuda"))
            self.vc = guard.fill_nan(torch.empty((nblk, page, Hk, D), dtype=sk.dtype, device="cuda"))
            for b in range(B):
                for j in range(-(-(SUFFIX[b] + Tn) // page)):
                    n = min(page, cap - j * page)
                    blk, rows = int(bt[b, j]), slice(j * page, j * page + n)
                    self.kc.view(torch.uint8)[blk, :n] = sk.view(torch.uint8)[b, rows]
                    self.vc.view(torch.uint8)[blk, :n] = sv.view(torch.uint8)[b, rows]
            self.bt = bt
        # the reference cache: values as the oracle stores them (fp8: code values, the prefix divided by the descale so that
        # code x descale gives the 16-bit prefix back)
        val = lambda t: t.float().double().cpu().numpy()
        kd, vd = (KD, VD) if fp8 else (1.0, 1.0)
        self.ref_k = np.concatenate([np.broadcast_to(val(self.pk) / kd, (B, S_p, Hk, D)), val(sk)], axis=1).copy()
        self.ref_v = np.concatenate([np.broadcast_to(val(self.pv) / vd, (B, S_p, Hk, D)), val(sv)], axis=1).copy()

    def kwargs(self):
        kw = dict(k=self.knew, v=self.vnew, cache_seqlens=self.lens.cuda())
        if self.bidx is not None:
            kw["cache_batch_idx"] = self.bidx.cuda()
        if self.bt is not None:
            kw["block_table"] = self.bt.cuda()
        if self.fp8:
            kw.update(k_descale=KD, v_descale=VD)
        return kw

    def reference(self, softcap=0.0, sinks=None):
        kd = dict(k_descale=KD, v_descale=VD) if self.fp8 else {}
        o, lse = oracle.kvcache_fwd(f64(self.q), self.ref_k.copy(), self.ref_v.copy(),
                                    k=None if self.knew is None else f64(self.knew), v=None if self.vnew is None else f64(self.vnew),
                                    cache_seqlens=(self.lens + self.S_p).numpy(), causal=True, softcap=softcap, io_dtype=self.dt, **kd)
        if sinks is not None:
            o, lse = sink_identity_bshd(o, lse.astype(np.float64), f64(sinks))
        return o, lse

    def concatenated_cache(self):
        """[prefix ; suffix] physically, per sequence, in the suffix cache's dtype: what a caller without this operator holds"""
        if self.fp8:
            k = torch.from_numpy(self.ref_k).float().to(FP8).cuda()            # (code values: exact in fp8)
            v = torch.from_numpy(self.ref_v).float().to(FP8).cuda()
            return k, v
        return torch.from_numpy(self.ref_k).to(DT[self.dt]).cuda(), torch.from_numpy(self.ref_v).to(DT[self.dt]).cuda()


CASES = {
    # name: (Case arguments, call options)
    "T1": (dict(T=1), {}),
    "T3": (dict(T=3), {}),
    "T1-fp16": (dict(T=1, dt="fp16"), {}),
    "T3-paged": (dict(T=3, layout="paged"), {}),
    "T1-paged": (dict(T=1, layout="paged"), {}),
    "T1-fp8": (dict(T=1, fp8=True), {}),
    "T3-fp8-paged": (dict(T=3, fp8=True, layout="paged"), {}),
    "T1-softcap": (dict(T=1), dict(softcap=15.0)),        # (T > 1: the kv-cache op itself rejects softcap under its causal mask)
    "T1-softcap-fp16-paged": (dict(T=1, dt="fp16", layout="paged"), dict(softcap=15.0)),
    "T1-sinks": (dict(T=1), dict(sinks=True)),
    "T3-sinks-fp16": (dict(T=3, dt="fp16"), dict(sinks=True)),
    "T3-D64": (dict(T=3, D=64), {}),
    "T1-D80": (dict(T=1, D=80, dt="fp16"), {}),
    "T3-D80": (dict(T=3, D=80), {}),
    "T1-mqa": (dict(T=1, Hk=1), {}),
    "T3-batch-idx": (dict(T=3, layout="batch_idx"), {}),
    "T1-prefix-4d-splits": (dict(T=1), dict(num_splits=3, four_d=True)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_shared_prefix_vs_oracle_over_concatenated_keys(name):
    cargs, opts = CASES[name]
    c = Case(seed=sum(map(ord, name)), **cargs)
    sinks = None
    if opts.get("sinks"):
        sinks = torch.tensor([0.5 * (i % 5) - 1.0 for i in range(c.H)], dtype=torch.float32, device="cuda")
    softcap = opts.get("softcap", 0.0)
    pk, pv = (c.pk[None], c.pv[None]) if opts.get("four_d") else (c.pk, c.pv)
    out, lse = _cascade().flash_attn_with_shared_prefix(c.q, pk, pv, c.kc, c.vc, softcap=softcap, sinks=sinks,
                                                        num_splits=opts.get("num_splits", 0), return_softmax_lse=True, **c.kwargs())
    torch.cuda.synchronize()
    o_ref, lse_ref = c.reference(softcap, sinks)
    mult, lse_tol = (1.5, dict(atol=LSE_ATOL_FP8)) if c.fp8 else (2.0, {})
    mr, fro = assert_close(f64(out), o_ref, c.dt, name + " out", mult=mult)
    d = assert_lse_close(f64(lse), lse_ref, name + " lse", **lse_tol)
    print(f"{name}: vs oracle max-rel {mr:.3e} fro {fro:.3e} lse {d:.3e}")
    # and against this build's plain kv-cache op over a cache that physically holds prefix + suffix (reported, same gate)
    kf, vf = c.concatenated_cache()
    plain, plain_lse = _fa().flash_attn_with_kvcache(c.q, kf, vf, k=c.knew, v=c.vnew, cache_seqlens=(c.lens + c.S_p).cuda(), causal=True,
                                                     softcap=softcap, sinks=sinks, return_softmax_lse=True,
                                                     **(dict(k_descale=KD, v_descale=VD) if c.fp8 else {}))
    mr2, fro2, _ = errs(f64(out), f64(plain))
    print(f"{name}: vs plain flash_attn_with_kvcache over [prefix ; suffix] max-rel {mr2:.3e} fro {fro2:.3e}")
    assert_close(f64(out), f64(plain), c.dt, name + " vs plain kv-cache op", mult=mult)
    assert_lse_close(f64(lse), f64(plain_lse), name + " lse vs plain", **lse_tol)


@pytest.mark.parametrize("T", [1, 3])
def test_empty_suffix_is_the_prefix_pass_bit_for_bit(T):
    """sequence 0 holds no token after the prefix and nothing is appended: its suffix LSE is -inf, the merge passes the prefix part
    through.  The prefix-only dense call is the one the operator makes: all B x T rows as one sequence."""
    from flash_attn_mi355 import flash_attn_interface as fi
    c = Case(T=T, append=False, seed=40 + T)
    out, lse = _cascade().flash_attn_with_shared_prefix(c.q, c.pk, c.pv, c.kc, c.vc, return_softmax_lse=True, **c.kwargs())
    o_p, lse_p = fi._dense_forward(c.q.reshape(1, c.B * T, c.H, c.D), c.pk[None], c.pv[None], 0.0, None, False, (-1, -1), 0.0, None,
                                   False)[:2]
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int16), o_p[0, :T].view(torch.int16))
    assert torch.equal(lse[0].view(torch.int32), lse_p[0, :, :T].contiguous().view(torch.int32))
    assert not torch.equal(out[2], o_p[0, 2 * T:3 * T])                     # (a sequence WITH a suffix is not the prefix part)
    o_ref, lse_ref = c.reference()
    # (rows of sequence 0 at T = 3: the oracle's bottom-right causal mask over the prefix alone would hide prefix keys from the first
    #  rows; the operator shows every query the whole prefix, so sequence 0 is checked against the dense call above only)
    assert_close(f64(out)[1:], o_ref[1:], c.dt, "out", mult=2.0)
    assert_lse_close(f64(lse)[1:], lse_ref[1:], "lse")


def test_no_prefix_is_the_kvcache_call_bit_for_bit():
    c = Case(T=3, seed=50)
    kc0, vc0 = c.kc.clone(), c.vc.clone()
    empty = c.pk[:0]
    out, lse = _cascade().flash_attn_with_shared_prefix(c.q, empty, empty, c.kc, c.vc, return_softmax_lse=True, **c.kwargs())
    only = _cascade().flash_attn_with_shared_prefix(c.q, empty, empty, kc0.clone(), vc0.clone(), **c.kwargs())
    ref, ref_lse = _fa().flash_attn_with_kvcache(c.q, kc0, vc0, causal=True, return_softmax_lse=True, **c.kwargs())
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and torch.equal(lse, ref_lse) and torch.equal(only, ref)
    assert torch.equal(c.kc, kc0) and torch.equal(c.vc, vc0)                # (both appended the same rows)


def test_out_of_scope_arguments_raise_before_anything_is_launched():
    c = Case(T=3, seed=60)
    kc0, vc0 = c.kc.clone(), c.vc.clone()
    f = _cascade().flash_attn_with_shared_prefix
    cos = torch.zeros(512, 32, dtype=DT[c.dt], device="cuda")
    slopes = torch.ones(c.H, dtype=torch.float32, device="cuda")
    tree = torch.ones(3, 3, dtype=torch.bool, device="cuda")
    pk8 = c.pk.float().to(FP8)
    for kw, match in ((dict(rotary_cos=cos, rotary_sin=cos), "rotary"), (dict(window_size=(64, -1)), "window"),
                      (dict(window_size=(-1, 0)), "window"), (dict(alibi_slopes=slopes), "ALiBi"), (dict(tree_mask=tree), "tree")):
        with pytest.raises(RuntimeError, match=match):
            f(c.q, c.pk, c.pv, c.kc, c.vc, **c.kwargs(), **kw)
    with pytest.raises(RuntimeError, match="fp8"):
        f(c.q, pk8, pk8, c.kc, c.vc, **c.kwargs())
    with pytest.raises(RuntimeError, match="fp8"):
        f(c.q.float().to(FP8), c.pk, c.pv, c.kc, c.vc, **c.kwargs())
    with pytest.raises(RuntimeError, match="GPU"):
        f(c.q, c.pk.cpu(), c.pv, c.kc, c.vc, **c.kwargs())
    with pytest.raises(RuntimeError, match="GPU"):
        f(c.q.cpu(), c.pk, c.pv, c.kc, c.vc, **c.kwargs())
    with pytest.raises(RuntimeError, match="backward"):
        f(c.q.clone().requires_grad_(), c.pk, c.pv, c.kc, c.vc, **c.kwargs())
    with pytest.raises(RuntimeError, match="prefix_k"):
        f(c.q, c.pk[:, :1], c.pv[:, :1], c.kc, c.vc, **c.kwargs())
    # inherited from the kv-cache op, which runs first: softcap under its causal mask (T > 1) is rejected there, as it always was
    with pytest.raises(RuntimeError, match="Softcap"):
        f(c.q, c.pk, c.pv, c.kc, c.vc, softcap=15.0, **c.kwargs())
    torch.cuda.synchronize()
    assert torch.equal(c.kc, kc0) and torch.equal(c.vc, vc0)                # nothing was appended: no call got as far as a launch


def test_graph_replay_equals_eager():
    """the three launches captured on one stream (no parallel branches); the cache is restored between the runs because the call
    appends to it"""
    c = Case(T=3, seed=70)
    kc0, vc0 = c.kc.clone(), c.vc.clone()
    kw = c.kwargs()
    fn = lambda: _cascade().flash_attn_with_shared_prefix(c.q, c.pk, c.pv, c.kc, c.vc, return_softmax_lse=True, **kw)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    c.kc.copy_(kc0); c.vc.copy_(vc0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = fn()
    c.q.copy_(rand16(tuple(c.q.shape), c.dt, 71))                           # new contents, same buffers
    c.kc.copy_(kc0); c.vc.copy_(vc0)
    g.replay()
    torch.cuda.synchronize()
    kc_g = c.kc.clone()
    c.kc.copy_(kc0); c.vc.copy_(vc0)
    out_e, lse_e = fn()
    torch.cuda.synchronize()
    assert torch.equal(out_g, out_e) and torch.equal(lse_g, lse_e) and torch.equal(kc_g, c.kc)
