"""GPU: attention sinks through every path that takes them - flash_attn_sinks_func (dense forward + backward),
flash_attn_varlen_func(sinks=) (general kernel, paged, decode and mixed routes, backward) and
flash_attn_with_kvcache(sinks=) (decode kernels, split-KV combine, fp8 gemv kernels, chunked prefill), the C ABI's
*_ext entry points, the plan cache and graph capture.  References: tests/sink_ref.py - (a) direct fp64 with autograd, (b)
the identity on the oracle."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from sink_ref import ref_dense, ref_varlen, sink_identity_bshd, sink_identity_thd
from util import DT, LSE_ATOL, LSE_ATOL_FP8, assert_close, assert_lse_close, f64, rand16

pytestmark = pytest.mark.gpu

SINK_POOL = [float("-inf"), -30.0, None, 0.0, 30.0, 80.0]          # None: N(0, 1)


def _fa():
    import flash_attn_mi355
    return flash_attn_mi355


def _sinks(H, seed, pool=SINK_POOL, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    vals = [pool[(h + seed) % len(pool)] for h in range(H)]
    vals = [float(torch.randn(1, generator=g)) if x is None else x for x in vals]
    return torch.tensor(vals, dtype=dtype, device="cuda")


def _dense_ref(q, k, v, sinks, scale, **kw):
    """(a) on the GPU in fp64: out [B, S, H, D], LSE [B, H, S]"""
    return ref_dense(q.double(), k.double(), v.double(), sinks, scale, **kw)


DENSE = [
    # dtype, D, B, Sq, Sk, Hq, Hk, causal, window, softcap, alibi
    ("bf16", 64, 2, 256, 256, 8, 1, True, (-1, -1), 0.0, False),       # gpt-oss: D 64, causal, MQA here
    ("fp16", 64, 1, 384, 384, 16, 2, True, (128, 0), 0.0, False),      # gpt-oss sliding layer: window (128, 0), GQA 8
    ("bf16", 128, 2, 200, 333, 8, 2, False, (-1, -1), 0.0, False),     # D 128 (the compiler-scheduled kernel), Sq != Sk
    ("fp16", 128, 1, 256, 256, 8, 8, True, (-1, -1), 30.0, False),     # softcap
    ("bf16", 256, 1, 160, 160, 4, 2, True, (-1, -1), 0.0, True),       # D 256, ALiBi
    ("fp16", 80, 2, 130, 170, 6, 3, False, (32, 16), 0.0, True),       # padded D 80, window, ALiBi
    ("bf16", 64, 1, 192, 128, 64, 8, True, (-1, -1), 0.0, False),      # H 64/8, Sq > Sk: rows without keys
]


@pytest.mark.parametrize("case", DENSE, ids=lambda c: "-".join(map(str, c)))
def test_dense_forward_backward(case):
    dt, D, B, Sq, Sk, Hq, Hk, causal, window, softcap, alibi = case
    q = rand16((B, Sq, Hq, D), dt, 1).requires_grad_()
    k = rand16((B, Sk, Hk, D), dt, 2).requires_grad_()
    v = rand16((B, Sk, Hk, D), dt, 3).requires_grad_()
    sinks = _sinks(Hq, D + Sq).requires_grad_()
    slopes = (torch.rand(Hq, generator=torch.Generator().manual_seed(5)) * 0.3).cuda() if alibi else None
    scale = D ** -0.5
    out, lse, _ = _fa().flash_attn_sinks_func(q, k, v, sinks, causal=causal, window_size=window, softcap=softcap,
                                              alibi_slopes=slopes, return_attn_probs=True)
    do = rand16((B, Sq, Hq, D), dt, 4)
    dq, dk, dv, ds = torch.autograd.grad(out, (q, k, v, sinks), do)
    qr, kr, vr, sr = (t.detach().double().requires_grad_() for t in (q, k, v, sinks))
    o_ref, lse_ref = _dense_ref(qr, kr, vr, sr, scale, causal=causal, window=window, softcap=softcap, alibi_slopes=slopes)
    g_ref = torch.autograd.grad(o_ref, (qr, kr, vr, sr), do.double())
    assert_close(f64(out), f64(o_ref), dt, "out")
    assert_lse_close(f64(lse), f64(lse_ref), "lse")
    for name, got, ref in (("dq", dq, g_ref[0]), ("dk", dk, g_ref[1]), ("dv", dv, g_ref[2])):
        assert_close(f64(got), f64(ref), dt, name, mult=2.0)
    assert_close(f64(ds), f64(g_ref[3]), dt, "dsinks", mult=3.0)
    # the reduction itself, on the kernel's own O and LSE: -sum exp(s - LSE) rowsum(dO o O)
    Dr = (do.double() * out.detach().double()).sum(-1).permute(0, 2, 1)
    closed = -(torch.exp(sinks.detach().double().view(1, -1, 1) - lse.double()) * Dr).sum((0, 2))
    terms = (torch.exp(sinks.detach().double().view(1, -1, 1) - lse.double()) * Dr.abs()).sum((0, 2))
    live = ~torch.isneginf(sinks.detach())
    closed = torch.where(live, closed, torch.zeros_like(closed))
    terms = torch.where(live, terms, torch.zeros_like(terms))
    # (fp32 accumulation of terms of both signs: the bound scales with the sum of their magnitudes)
    assert torch.all((ds.double() - closed).abs() <= 1e-4 * closed.abs() + 1e-5 * terms + 1e-7), (ds, closed)


def test_rows_without_keys_forward_and_backward():
    """causal Sq > Sk (bottom-right aligned): the first Sq - Sk rows see no key.  They give out 0 and LSE s_h; their dq
    rows are 0 and dk / dv are what the other rows make them - on every backward form (D 64 / 128 / 256)."""
    for D, dt in ((64, "bf16"), (128, "fp16"), (256, "bf16")):
        B, Sq, Sk, Hq, Hk = 2, 300, 180, 4, 2
        q = rand16((B, Sq, Hq, D), dt, 11).requires_grad_()
        k = rand16((B, Sk, Hk, D), dt, 12).requires_grad_()
        v = rand16((B, Sk, Hk, D), dt, 13).requires_grad_()
        sinks = torch.tensor([0.5, -1.0, 3.0, 80.0], device="cuda", requires_grad=True)
        out, lse, _ = _fa().flash_attn_sinks_func(q, k, v, sinks, causal=True, return_attn_probs=True)
        do = rand16((B, Sq, Hq, D), dt, 14)
        dq, dk, dv, ds = torch.autograd.grad(out, (q, k, v, sinks), do)
        empty = Sq - Sk
        assert torch.all(out[:, :empty] == 0)
        np.testing.assert_allclose(f64(lse[:, :, :empty]), np.broadcast_to(f64(sinks)[None, :, None], (B, Hq, empty)),
                                   rtol=0, atol=3e-5)
        assert torch.all(dq[:, :empty] == 0)
        qr, kr, vr, sr = (t.detach().double().requires_grad_() for t in (q, k, v, sinks))
        o_ref, _ = _dense_ref(qr, kr, vr, sr, D ** -0.5, causal=True)
        g_ref = torch.autograd.grad(o_ref, (qr, kr, vr, sr), do.double())
        assert_close(f64(dk), f64(g_ref[1]), dt, f"dk D{D}", mult=2.0)
        assert_close(f64(dv), f64(g_ref[2]), dt, f"dv D{D}", mult=2.0)
        assert_close(f64(dq), f64(g_ref[0]), dt, f"dq D{D}", mult=2.0)
        assert_close(f64(ds), f64(g_ref[3]), dt, f"dsinks D{D}", mult=3.0)


def test_sink_minus_inf_is_bit_identical_to_no_sink():
    fa = _fa()
    q, k, v = rand16((2, 300, 8, 64), "bf16", 21), rand16((2, 300, 2, 64), "bf16", 22), rand16((2, 300, 2, 64), "bf16", 23)
    ninf = torch.full((8,), float("-inf"), device="cuda")
    for kw in (dict(causal=True), dict(window_size=(128, 0)), dict(softcap=20.0)):
        o0, l0, _ = fa.flash_attn_func(q, k, v, return_attn_probs=True, **kw)
        o1, l1, _ = fa.flash_attn_sinks_func(q, k, v, ninf, return_attn_probs=True, **kw)
        assert torch.equal(o0, o1) and torch.equal(l0, l1), kw
    # the decode kernels: 16-bit (GQA packing, split-KV with the combine kernels) and fp8 gemv (H_q = H_k)
    B, S, Hq, Hk, D = 4, 2048, 64, 8, 64
    kc, vc = rand16((B, S, Hk, D), "bf16", 24), rand16((B, S, Hk, D), "bf16", 25)
    qd = rand16((B, 1, Hq, D), "bf16", 26)
    lens = torch.tensor([2000, 1500, 700, 33], dtype=torch.int32, device="cuda")
    ninf64 = torch.full((Hq,), float("-inf"), device="cuda")
    for ns in (1, 4, 16):
        o0, l0 = fa.flash_attn_with_kvcache(qd, kc, vc, cache_seqlens=lens, num_splits=ns, return_softmax_lse=True)
        o1, l1 = fa.flash_attn_with_kvcache(qd, kc, vc, cache_seqlens=lens, num_splits=ns, return_softmax_lse=True,
                                            sinks=ninf64)
        assert torch.equal(o0, o1) and torch.equal(l0, l1), ns
    kc8, vc8 = (kc.float() * 4).to(torch.float8_e4m3fn), (vc.float() * 4).to(torch.float8_e4m3fn)
    q8 = rand16((B, 1, Hk, D), "bf16", 27)
    for ns in (1, 0):
        o0, l0 = fa.flash_attn_with_kvcache(q8, kc8, vc8, cache_seqlens=lens, num_splits=ns, return_softmax_lse=True,
                                            k_descale=0.25, v_descale=0.25)
        o1, l1 = fa.flash_attn_with_kvcache(q8, kc8, vc8, cache_seqlens=lens, num_splits=ns, return_softmax_lse=True,
                                            k_descale=0.25, v_descale=0.25, sinks=torch.full((Hk,), float("-inf"), device="cuda"))
        assert torch.equal(o0, o1) and torch.equal(l0, l1), ns


def test_only_sinks_require_grad_bf16_param_and_determinism():
    fa = _fa()
    B, S, Hq, Hk, D = 2, 512, 8, 2, 64
    q, k, v = rand16((B, S, Hq, D), "bf16", 31), rand16((B, S, Hk, D), "bf16", 32), rand16((B, S, Hk, D), "bf16", 33)
    p = torch.nn.Parameter(torch.randn(Hq, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda())
    do = rand16((B, S, Hq, D), "bf16", 34)
    out = fa.flash_attn_sinks_func(q, k, v, p, causal=True, window_size=(128, 0))
    out.backward(do)
    assert p.grad is not None and p.grad.dtype == torch.bfloat16
    sr = p.detach().double().requires_grad_()
    o_ref, _ = _dense_ref(q, k, v, sr, D ** -0.5, causal=True, window=(128, 0))
    (g,) = torch.autograd.grad(o_ref, sr, do.double())
    assert_close(f64(p.grad), f64(g), "bf16", "dsinks (bf16 param)", mult=3.0)
    reps = []
    for _ in range(3):
        s32 = p.detach().float().requires_grad_()
        o = fa.flash_attn_sinks_func(q, k, v, s32, causal=True, deterministic=True)
        (gs,) = torch.autograd.grad(o, s32, do)
        reps.append(gs)
    assert all(torch.equal(reps[0], r) for r in reps[1:])


def _packed(lens, H, D, dt, seed):
    T = sum(lens)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device="cuda")
    return rand16((T, H, D), dt, seed), cu


def test_varlen_forward_backward_with_empty_sequences():
    dt, Hq, Hk, D = "bf16", 8, 2, 64
    lq, lk = [37, 0, 200, 1, 90], [50, 20, 180, 0, 300]
    q, cu_q = _packed(lq, Hq, D, dt, 41)
    k, cu_k = _packed(lk, Hk, D, dt, 42)
    v, _ = _packed(lk, Hk, D, dt, 43)
    q.requires_grad_(); k.requires_grad_(); v.requires_grad_()
    sinks = _sinks(Hq, 44).requires_grad_()
    out, lse, _ = _fa().flash_attn_varlen_func(q, k, v, cu_q, cu_k, max(lq), max(lk), causal=True, return_attn_probs=True,
                                               sinks=sinks)
    do, _ = _packed(lq, Hq, D, dt, 45)
    g = torch.autograd.grad(out, (q, k, v, sinks), do)
    qr, kr, vr, sr = (t.detach().double().requires_grad_() for t in (q, k, v, sinks))
    o_ref, lse_ref = ref_varlen(qr, kr, vr, cu_q.tolist(), cu_k.tolist(), sr, D ** -0.5, causal=True)
    g_ref = torch.autograd.grad(o_ref, (qr, kr, vr, sr), do.double())
    assert_close(f64(out), f64(o_ref), dt, "out")
    assert_lse_close(f64(lse), f64(lse_ref), "lse")
    for name, a, b in zip(("dq", "dk", "dv"), g[:3], g_ref[:3]):
        assert_close(f64(a), f64(b), dt, name, mult=2.0)
    assert_close(f64(g[3]), f64(g_ref[3]), dt, "dsinks", mult=3.0)


@pytest.mark.parametrize("page,Tq,lens_q", [
    (16, None, [33, 0, 120, 7]),            # general kernel over pages of 16
    (64, None, [1, 1, 1, 1, 1, 200]),       # mixed batch: decode kernels for the short sequences + fa_fwd_kernel
    (256, 1, None),                         # uniform T_q = 1: the decode route
    (64, 4, None),                          # uniform T_q = 4
])
def test_varlen_paged_routes(page, Tq, lens_q):
    dt, Hq, Hk, D = "bf16", 64, 8, 64
    g = torch.Generator().manual_seed(page + (Tq or 0))
    B = len(lens_q) if lens_q else 6
    lens_q = lens_q or [Tq] * B
    lens_k = [int(x) for x in torch.randint(300, 1200, (B,), generator=g)]
    lens_k = [max(a, b) for a, b in zip(lens_k, lens_q)]
    pps = (max(lens_k) + page - 1) // page
    nblk = B * pps
    kc, vc = rand16((nblk, page, Hk, D), dt, 51), rand16((nblk, page, Hk, D), dt, 52)
    bt = torch.randperm(nblk, generator=g).reshape(B, pps).to(torch.int32).cuda()
    q, cu_q = _packed(lens_q, Hq, D, dt, 53)
    cu_k = torch.tensor([0] + list(np.cumsum(lens_k)), dtype=torch.int32, device="cuda")
    sinks = _sinks(Hq, 54)
    used = torch.tensor([x - 3 if x > 200 else x for x in lens_k], dtype=torch.int32, device="cuda")
    out, lse, _ = _fa().flash_attn_varlen_func(q, kc, vc, cu_q, cu_k, max(lens_q), max(lens_k), causal=True,
                                               return_attn_probs=True, block_table=bt, seqused_k=used, sinks=sinks)
    o, l = oracle.varlen_fwd(f64(q), f64(kc), f64(vc), cu_q.cpu().numpy(), cu_k.cpu().numpy(), max(lens_q), max(lens_k),
                             D ** -0.5, causal=True, seqused_k=used.cpu().numpy(), block_table=bt.cpu().numpy())
    o_ref, lse_ref = sink_identity_thd(o, l.astype(np.float64), f64(sinks))
    assert_close(f64(out), o_ref, dt, "out")
    assert_lse_close(f64(lse), lse_ref, "lse")


KV = [
    # B, Tq, Hq, Hk, D, paged, fp8, num_splits, append+rotary
    (8, 1, 64, 8, 64, False, False, 1, False),      # gpt-oss decode, one split: the kernel's own epilogue
    (8, 4, 64, 8, 64, True, False, 5, False),       # T_q 4, paged, forced splits: decode_combine_kernel
    (2, 1, 64, 8, 64, True, False, 32, False),      # many partials: decode_combine_wide_kernel
    (4, 1, 8, 8, 128, False, True, 1, False),       # fp8 cache, H_q = H_k: the gemv kernels
    (4, 1, 8, 8, 64, True, True, 0, False),         # fp8 cache, heuristic splits
    (2, 3, 16, 2, 128, True, True, 3, True),        # fp8 cache (eight-wave MFMA form), append + rotary
    (2, 1, 16, 4, 128, False, False, 0, True),      # 16-bit, append + rotary
    (2, 200, 8, 2, 64, True, False, 0, True),       # chunked prefill (T_q >= 192): fa_fwd_kernel on the cache
]


@pytest.mark.parametrize("case", KV, ids=lambda c: "-".join(map(str, c)))
def test_kvcache(case):
    B, Tq, Hq, Hk, D, paged, fp8, ns, rot = case
    dt, Smax, page = "bf16", 2048, 64
    g = torch.Generator().manual_seed(B * 100 + Tq)
    lens = torch.randint(300, Smax - Tq - 8, (B,), generator=g, dtype=torch.int32)
    q = rand16((B, Tq, Hq, D), dt, 61)
    if paged:
        pps = Smax // page
        kc, vc = rand16((B * pps, page, Hk, D), dt, 62), rand16((B * pps, page, Hk, D), dt, 63)
        bt = torch.randperm(B * pps, generator=g).reshape(B, pps).to(torch.int32)
    else:
        kc, vc = rand16((B, Smax, Hk, D), dt, 62), rand16((B, Smax, Hk, D), dt, 63)
        bt = None
    kw, okw = {}, {}
    if fp8:
        kd, vd = 0.0625, 0.03125
        kc = (kc.float() / kd).to(torch.float8_e4m3fn); vc = (vc.float() / vd).to(torch.float8_e4m3fn)
        kw = okw = dict(k_descale=kd, v_descale=vd)
        kc_ref, vc_ref = kc.float().double().cpu().numpy(), vc.float().double().cpu().numpy()
    else:
        kc_ref, vc_ref = f64(kc), f64(vc)
    knew = vnew = cos = sin = None
    if rot:
        knew, vnew = rand16((B, Tq, Hk, D), dt, 64), rand16((B, Tq, Hk, D), dt, 65)
        pos = torch.arange(Smax, dtype=torch.float32)[:, None]
        ang = pos / (10000 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))[None, :]
        cos, sin = torch.cos(ang).to(DT[dt]).cuda(), torch.sin(ang).to(DT[dt]).cuda()
    sinks = _sinks(Hq, 66)
    out, lse = _fa().flash_attn_with_kvcache(q, kc, vc, knew, vnew, rotary_cos=cos, rotary_sin=sin,
                                             cache_seqlens=lens.cuda(), block_table=None if bt is None else bt.cuda(),
                                             causal=True, num_splits=ns, return_softmax_lse=True, sinks=sinks, **kw)
    o, l = oracle.kvcache_fwd(f64(q), kc_ref, vc_ref, k=None if knew is None else f64(knew),
                              v=None if vnew is None else f64(vnew), rotary_cos=None if cos is None else f64(cos),
                              rotary_sin=None if sin is None else f64(sin), cache_seqlens=lens.numpy(),
                              block_table=None if bt is None else bt.numpy(), causal=True, io_dtype=dt, **okw)
    o_ref, lse_ref = sink_identity_bshd(o, l.astype(np.float64), f64(sinks))
    assert_close(f64(out), o_ref, dt, "out", mult=1.5 if fp8 else 1.0)
    assert_lse_close(f64(lse), lse_ref, "lse", **(dict(atol=LSE_ATOL_FP8) if fp8 else {}))


def test_kvcache_plan_cache_separates_sink_calls():
    fa = _fa()
    B, Hq, Hk, D, S = 4, 64, 8, 64, 1024
    kc, vc = rand16((B, S, Hk, D), "bf16", 71), rand16((B, S, Hk, D), "bf16", 72)
    q = rand16((B, 1, Hq, D), "bf16", 73)
    lens = torch.tensor([1000, 600, 300, 17], dtype=torch.int32, device="cuda")
    o, l = oracle.kvcache_fwd(f64(q), f64(kc), f64(vc), cache_seqlens=lens.cpu().numpy(), io_dtype="bf16")
    s1, s2 = _sinks(Hq, 74), _sinks(Hq, 75, pool=[1.0, -2.0, 5.0, None])
    for sinks in (None, s1, s2, None, s1):
        for _ in range(2):                                       # (the second call of each takes the cached plan)
            out, lse = fa.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, return_softmax_lse=True, sinks=sinks)
            o_ref, lse_ref = (o, l) if sinks is None else sink_identity_bshd(o, l.astype(np.float64), f64(sinks))
            assert_close(f64(out), o_ref, "bf16", "out")
            assert_lse_close(f64(lse), lse_ref, "lse")


def test_graph_capture_decode_and_training_step():
    fa = _fa()
    B, Hq, Hk, D, S = 8, 64, 8, 64, 2048
    kc, vc = rand16((B, S, Hk, D), "bf16", 81), rand16((B, S, Hk, D), "bf16", 82)
    q = rand16((B, 1, Hq, D), "bf16", 83)
    lens = torch.full((B,), 1500, dtype=torch.int32, device="cuda")
    sinks = _sinks(Hq, 84)
    eager = fa.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, sinks=sinks)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fa.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, sinks=sinks)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        static = fa.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, sinks=sinks)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)
    # forward + backward with sinks
    qt, kt, vt = rand16((2, 256, 8, 64), "bf16", 85), rand16((2, 256, 2, 64), "bf16", 86), rand16((2, 256, 2, 64), "bf16", 87)
    st = _sinks(8, 88)
    do = rand16((2, 256, 8, 64), "bf16", 89)

    def step():
        qq, kk, vv, ss = (t.detach().requires_grad_() for t in (qt, kt, vt, st))
        o = fa.flash_attn_sinks_func(qq, kk, vv, ss, causal=True)
        return (o,) + torch.autograd.grad(o, (qq, kk, vv, ss), do)

    ref = step()
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        static2 = step()
    g2.replay()
    torch.cuda.synchronize()
    for a, b in zip(static2, ref):
        assert torch.equal(a, b)


def test_c_abi_ext_null_equals_abi4():
    from flash_attn_mi355 import _lib
    from flash_attn_mi355 import flash_attn_interface as fi
    q, k, v = rand16((1, 200, 4, 64), "fp16", 91), rand16((1, 200, 4, 64), "fp16", 92), rand16((1, 200, 4, 64), "fp16", 93)
    res = []
    for ext in (False, True):
        out = torch.empty_like(q)
        lse = torch.empty((1, 4, 200), dtype=torch.float32, device="cuda")
        p = fi._base_params(q, q.dtype, 0.125, True, (-1, -1), 0.0)
        p.q, p.k, p.v, p.o, p.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr()
        for name, t in (("q", q), ("k", k), ("v", v), ("o", out)):
            fi._set3(p, name, t, "bshd")
        p.lse_batch_stride, p.lse_head_stride = lse.stride(0), lse.stride(1)
        p.batch, p.nheads_q, p.nheads_k, p.seqlen_q, p.seqlen_k, p.head_dim = 1, 4, 4, 200, 200, 64
        stream = torch.cuda.current_stream().cuda_stream
        rc = (_lib.lib.fa_fwd_ext(ctypes.byref(p), None, ctypes.c_void_p(stream)) if ext
              else _lib.lib.fa_fwd(ctypes.byref(p), ctypes.c_void_p(stream)))
        assert rc == 0, _lib.lib.fa_last_error()
        res.append((out, lse))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
