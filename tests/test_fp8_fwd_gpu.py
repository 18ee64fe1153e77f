"""GPU: the fp8-e4m3 q / k / v forward (csrc/fa_fwd_fp8.hip) - flash_attn_func / flash_attn_varlen_func with float8_e4m3fn
inputs, bf16 out.

Exact-data layout tests catch row / column / key-order permutations in both products (S^T = K Q^T and O^T = V^T P^T on the
block-scaled K = 64 MFMA); random data is held against the fp64 oracle on the dequantised inputs.

The out gate (derived, not fitted).  Both products are exact up to fp32 accumulation: an e4m3 x e4m3 product has 8
significant bits.  The one rounding the fp8 path adds is P -> e4m3 (v_cvt_pk_fp8_f32, round to nearest): P is at most
2^8 under the deferred rescale, so |q(P) - P| <= max(2^-4 P, 2^-10) - half an ulp of 3 mantissa bits for normal values,
half the subnormal spacing 2^-9 below 2^-6.  The row sum l is taken from the fp32 P, so with p = P / l (the exact
probabilities) the error of one output element is bounded by
    |out_i - ref_i| <= 2^-4 sum_j p_ij |v_jd| + 2^-10 sum_j |v_jd| / l_i  +  bf16 rounding of out (2^-9 |ref|),
and l_i >= 1 (the row's largest P is exp2(s_max - m_run) with m_run <= s_max), i.e. 1 / l_i <= max_j p_ij.  The gate is
that bound with the bf16 term doubled (2^-8 |ref|) and 1e-6 for fp32 accumulation; the tests assert every element inside
it and report the largest ratio error / bound.  It is never widened to make a case pass.  One MI355X run of this file: the
largest ratio over all random, varlen and bf16-consistency cases was 0.71 (the P roundings do not all line up as the bound
assumes), the smallest 0.16.
The LSE gate is tests/util.py's LSE_ATOL: the scores are exact e4m3 products summed in fp32 and P's rounding does not
enter l."""

import numpy as np
import pytest
import torch

import oracle
from oracle.attention import normalize_flags, score_matrix, visible_mask
from util import LSE_ATOL, assert_lse_close

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn


def _fa():
    import flash_attn
    return flash_attn


def _rand8(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(F8).cuda()


def _d(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _bhsd(t):
    return _d(t).transpose(0, 2, 1, 3)


def _vcodes(B, S, H, D, seed=0):
    """asymmetric, column-distinct multiples of 1/8 in [-1, 1] (exact in e4m3; sums of a few thousand exact in fp32)"""
    j = torch.arange(S).view(1, S, 1, 1)
    h = torch.arange(H).view(1, 1, H, 1)
    d = torch.arange(D).view(1, 1, 1, D)
    b = torch.arange(B).view(B, 1, 1, 1)
    x = ((j * 7 + d * 3 + h * 5 + b * 11 + seed) % 17 - 8).float() / 8.0
    return x.to(F8).cuda()


def _bound(qh, kh, vh, scale, causal, window):
    """per element (rows x D) gate of one head, see the module docstring"""
    sq, sk = qh.shape[0], kh.shape[0]
    if sk == 0:
        return np.zeros((sq, vh.shape[1]))
    c, wl, wr = normalize_flags(sq, sk, causal, window[0], window[1], False)
    s, vis = score_matrix(qh, kh, scale, c, wl, wr, 0.0, None)
    m = np.max(s, axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    e = np.where(vis, np.exp(s - m), 0.0)
    l = e.sum(axis=1, keepdims=True)
    p = e / np.where(l > 0, l, 1.0)
    av = np.abs(vh)
    return 2.0 ** -4 * (p @ av) + 2.0 ** -10 * p.max(axis=1, keepdims=True) * (vis @ av)


def _check_out(got, ref, bound, name):
    """got / ref [..., D]; bound of the same shape (without the output-rounding term)"""
    tol = bound + 2.0 ** -8 * np.abs(ref) + 1e-6
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    ratio = float((err / tol).max()) if err.size else 0.0
    print(f"{name}: max |err| {err.max() if err.size else 0:.3e}, max err / gate {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: error {ratio:.3f} x the P-rounding gate"
    return ratio


def _dense_bound(q8, k8, v8, scale, causal, window):
    q, k, v = _bhsd(q8), _bhsd(k8), _bhsd(v8)
    B, H, S, D = q.shape
    G = H // k.shape[1]
    out = np.zeros_like(q)
    for b in range(B):
        for h in range(H):
            out[b, h] = _bound(q[b, h], k[b, h // G], v[b, h // G], scale, causal, window)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# exact data
# ---------------------------------------------------------------------------------------------------------------------
ZERO_Q_CASES = [
    # (B, Sq, Sk, H, Hk, D, causal, window)
    (2, 1, 1, 4, 4, 128, False, (-1, -1)),
    (2, 63, 63, 4, 1, 128, True, (-1, -1)),       # MQA
    (1, 65, 65, 8, 2, 64, False, (-1, -1)),       # GQA 4:1
    (2, 200, 200, 4, 4, 128, True, (-1, -1)),
    (1, 1000, 1000, 2, 2, 128, False, (48, 7)),   # window
    (1, 1000, 1000, 4, 1, 64, True, (-1, -1)),
    (2, 63, 200, 4, 2, 128, True, (-1, -1)),      # Sq < Sk
    (1, 200, 65, 4, 4, 128, True, (-1, -1)),      # Sq > Sk: leading rows see no key
    (1, 1000, 200, 2, 1, 128, False, (-1, -1)),
]


@pytest.mark.parametrize("B,Sq,Sk,H,Hk,D,causal,window", ZERO_Q_CASES)
def test_zero_q_gives_the_mean_of_the_visible_v_rows(B, Sq, Sk, H, Hk, D, causal, window):
    """q = 0: every visible score is 0, every visible P exactly 1, so out_i is the plain mean of the visible v rows
    (sums of multiples of 1/8, exact in fp32) and LSE_i = ln(count)"""
    fa = _fa()
    q8 = torch.zeros(B, Sq, H, D, dtype=F8, device="cuda")
    k8 = _rand8((B, Sk, Hk, D), 1)
    v8 = _vcodes(B, Sk, Hk, D)
    out, lse, _ = fa.flash_attn_func(q8, k8, v8, causal=causal, window_size=window, return_attn_probs=True)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32
    c, wl, wr = normalize_flags(Sq, Sk, causal, window[0], window[1], False)
    vis = visible_mask(Sq, Sk, c, wl, wr).astype(np.float64)
    cnt = vis.sum(axis=1)
    v = _bhsd(v8)
    G = H // Hk
    got, gl = _bhsd(out), _d(lse)
    for b in range(B):
        for h in range(H):
            ref = (vis @ v[b, h // G]) / np.where(cnt > 0, cnt, 1.0)[:, None]
            np.testing.assert_allclose(got[b, h], ref, rtol=2.0 ** -8, atol=1e-7, err_msg=f"out b{b} h{h}")
            with np.errstate(divide="ignore"):
                lref = np.where(cnt > 0, np.log(np.where(cnt > 0, cnt, 1.0)), -np.inf)
            assert_lse_close(gl[b, h], lref, f"lse b{b} h{h}")


ONE_HOT_CASES = [
    # (B, Sq, Sk, H, Hk, D, causal, window)
    (2, 128, 128, 4, 4, 128, False, (-1, -1)),
    (1, 200, 200, 4, 1, 128, True, (-1, -1)),
    (2, 333, 1000, 8, 2, 128, True, (-1, -1)),
    (1, 256, 256, 4, 4, 64, False, (-1, -1)),
    (1, 500, 500, 4, 2, 64, False, (100, 20)),
    (1, 300, 100, 2, 2, 128, False, (-1, -1)),
]


@pytest.mark.parametrize("B,Sq,Sk,H,Hk,D,causal,window", ONE_HOT_CASES)
def test_one_hot_scores_pick_exactly_one_v_row(B, Sq, Sk, H, Hk, D, causal, window):
    """key j carries the code e_(j mod D/2) + 2 e_(D/2 + (j div D/2) mod D/2); query row i carries 384 x the code of one
    visible target key t(i).  The target scores 3 x 384 x scale, every other key at most 2 x 384 x scale: >= 33 nats
    behind, so out_i is v[t(i)] up to the other keys' weight e^-33 x sum |v| < 1e-11 - i.e. exactly the bf16 value of
    v[t(i)] (multiples of 1/8) where that is non-zero, and within 1e-11 of 0 where it is 0 (a key seen in an earlier tile
    keeps an e^-33 share through the rescale; bf16 holds such values).  Any row, column or key permutation moves an
    element by >= 1/8."""
    fa = _fa()
    half = D // 2
    assert Sk <= half * half
    scale = D ** -0.5
    c, wl, wr = normalize_flags(Sq, Sk, causal, window[0], window[1], False)
    vis = visible_mask(Sq, Sk, c, wl, wr)
    rng = np.random.default_rng(Sq * 7 + Sk)
    k = torch.zeros(B, Sk, Hk, D)
    j = torch.arange(Sk)
    k[:, j, :, j % half] = 1.0
    k[:, j, :, half + (j // half) % half] = 2.0
    q = torch.zeros(B, Sq, H, D)
    tgt = np.full((B, H, Sq), -1)
    for b in range(B):
        for h in range(H):
            for i in range(Sq):
                cand = np.nonzero(vis[i])[0]
                if cand.size:
                    t = int(rng.choice(cand))
                    tgt[b, h, i] = t
                    q[b, i, h, t % half] = 384.0
                    q[b, i, h, half + (t // half) % half] = 384.0
    q8, k8, v8 = q.to(F8).cuda(), k.to(F8).cuda(), _vcodes(B, Sk, Hk, D, seed=3)
    out, lse, _ = fa.flash_attn_func(q8, k8, v8, softmax_scale=scale, causal=causal, window_size=window,
                                     return_attn_probs=True)
    torch.cuda.synchronize()
    got, v, gl = _bhsd(out), _bhsd(v8), _d(lse)
    G = H // Hk
    for b in range(B):
        for h in range(H):
            has = tgt[b, h] >= 0
            ref = np.zeros((Sq, D))
            ref[has] = v[b, h // G][tgt[b, h][has]]
            bad = np.nonzero((np.abs(got[b, h] - ref) > 1e-11).any(axis=1))[0]
            assert bad.size == 0, f"b{b} h{h}: rows {bad[:8]} differ (row {bad[0]}: got {got[b, h][bad[0], :6]}, want {ref[bad[0], :6]})"
            lref = np.where(has, 3 * 384.0 * scale, -np.inf)
            assert_lse_close(gl[b, h], lref, f"lse b{b} h{h}", atol=LSE_ATOL * 4)   # (|LSE| ~ 100 here: 4 fp32 ulps)


# ---------------------------------------------------------------------------------------------------------------------
# random data against the oracle
# ---------------------------------------------------------------------------------------------------------------------
RANDOM_CASES = [
    # (B, Sq, Sk, H, Hk, D, causal, window)
    (2, 256, 256, 4, 4, 128, False, (-1, -1)),
    (2, 300, 300, 4, 2, 128, True, (-1, -1)),
    (1, 257, 513, 8, 1, 128, True, (-1, -1)),
    (2, 200, 200, 4, 4, 64, True, (-1, -1)),
    (1, 384, 384, 4, 2, 64, False, (64, 16)),
    (2, 190, 190, 4, 4, 80, True, (-1, -1)),       # narrow rows: kernel width 128, 80 valid columns
    (1, 260, 130, 4, 2, 112, False, (-1, -1)),
    (1, 130, 260, 2, 2, 48, False, (32, 0)),       # width 64, 48 valid columns
]


@pytest.mark.parametrize("B,Sq,Sk,H,Hk,D,causal,window", RANDOM_CASES)
def test_random_against_oracle(B, Sq, Sk, H, Hk, D, causal, window):
    fa = _fa()
    q8 = _rand8((B, Sq, H, D), 10 + D)
    k8 = _rand8((B, Sk, Hk, D), 20 + D)
    v8 = _rand8((B, Sk, Hk, D), 30 + D)
    scale = D ** -0.5
    out, lse, _ = fa.flash_attn_func(q8, k8, v8, causal=causal, window_size=window, return_attn_probs=True)
    torch.cuda.synchronize()
    assert out.shape == (B, Sq, H, D) and out.dtype == torch.bfloat16
    o_ref, lse_ref, _ = oracle.attn_fwd(_bhsd(q8), _bhsd(k8), _bhsd(v8), scale, causal=causal, window=window)
    assert_lse_close(_d(lse), lse_ref, "lse")
    _check_out(_bhsd(out), o_ref, _dense_bound(q8, k8, v8, scale, causal, window), "out")


@pytest.mark.parametrize("D,causal,window", [(128, True, (-1, -1)), (64, False, (-1, -1)), (96, False, (40, 8))])
def test_varlen_with_empty_sequences_and_descales(D, causal, window):
    """packed batch with empty query / key sequences; descales != 1 fold into the scale / normalisation"""
    fa = _fa()
    lq = [0, 77, 130, 1, 0, 300, 64]
    lk = [5, 77, 200, 0, 0, 300, 129]
    H, Hk = 4, 2
    cu_q = torch.tensor(np.concatenate([[0], np.cumsum(lq)]), dtype=torch.int32, device="cuda")
    cu_k = torch.tensor(np.concatenate([[0], np.cumsum(lk)]), dtype=torch.int32, device="cuda")
    q8 = _rand8((sum(lq), H, D), 41)
    k8 = _rand8((sum(lk), Hk, D), 42)
    v8 = _rand8((sum(lk), Hk, D), 43)
    qd, kd, vd = 0.5, 0.25, 2.0
    scale = 0.11
    out, lse, _ = fa.flash_attn_varlen_func(q8, k8, v8, cu_q, cu_k, max(lq), max(lk), softmax_scale=scale,
                                            causal=causal, window_size=window, return_attn_probs=True,
                                            q_descale=qd, k_descale=kd, v_descale=vd)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and out.shape == (sum(lq), H, D)
    q, k, v = _d(q8) * qd, _d(k8) * kd, _d(v8) * vd
    o_ref, lse_ref = oracle.varlen_fwd(q, k, v, cu_q.cpu().numpy(), cu_k.cpu().numpy(), max(lq), max(lk), scale,
                                       causal=causal, window=window)
    assert_lse_close(_d(lse), lse_ref, "lse")
    got = _d(out)
    bound = np.zeros_like(o_ref)
    cq, ck = cu_q.cpu().numpy(), cu_k.cpu().numpy()
    for b in range(len(lq)):
        if lq[b] == 0:
            continue
        for h in range(H):
            g = h // (H // Hk)
            bound[cq[b]:cq[b + 1], h] = _bound(q[cq[b]:cq[b + 1], h], k[ck[b]:ck[b + 1], g], v[ck[b]:ck[b + 1], g], scale,
                                               causal, window)
    _check_out(got, o_ref, bound, "varlen out")


# ---------------------------------------------------------------------------------------------------------------------
# consistency with the 16-bit path
# ---------------------------------------------------------------------------------------------------------------------
def _against_bf16(B, S, H, D, causal, rows=None):
    """flash_attn_func(q8, k8, v8) against flash_attn_func(q8.bfloat16(), ...): e4m3 values are exact in bf16, so both paths
    see the same inputs.  LSE at LSE_ATOL everywhere; out inside the P-rounding gate (the bf16 kernel's own P rounding,
    2^-9 relative, is covered by one more 2^-8 |out| term) on all rows or on the sampled (b, h, i) `rows`."""
    fa = _fa()
    q8, k8, v8 = _rand8((B, S, H, D), 51), _rand8((B, S, H, D), 52), _rand8((B, S, H, D), 53)
    out8, lse8, _ = fa.flash_attn_func(q8, k8, v8, causal=causal, return_attn_probs=True)
    out16, lse16, _ = fa.flash_attn_func(q8.bfloat16(), k8.bfloat16(), v8.bfloat16(), causal=causal, return_attn_probs=True)
    torch.cuda.synchronize()
    assert_lse_close(_d(lse8), _d(lse16), "lse fp8 vs bf16")
    scale = D ** -0.5
    if rows is None:
        bound = _dense_bound(q8, k8, v8, scale, causal, (-1, -1))
        a, b16 = _bhsd(out8), _bhsd(out16)
    else:
        bound, a, b16 = [], [], []
        for b, h, i in rows:
            n = i + 1 if causal else S                           # (Sq == Sk: row i sees keys 0 .. i under the causal mask)
            bound.append(_bound(_d(q8[b, i:i + 1, h]), _d(k8[b, :n, h]), _d(v8[b, :n, h]), scale, False, (-1, -1))[0])
            a.append(_d(out8[b, i, h]))
            b16.append(_d(out16[b, i, h]))
        bound, a, b16 = np.stack(bound), np.stack(a), np.stack(b16)
    _check_out(a, b16, bound + 2.0 ** -8 * np.abs(b16), "out fp8 vs bf16")


def test_consistent_with_the_bf16_path():
    _against_bf16(2, 1000, 4, 128, True)
    _against_bf16(2, 513, 4, 64, False)


def test_consistent_with_the_bf16_path_at_config_2():
    """B 8, H 16, S 4096, D 128, causal (the bench's forward shape): LSE everywhere, out on 256 sampled rows"""
    rng = np.random.default_rng(7)
    rows = [(int(rng.integers(8)), int(rng.integers(16)), int(i)) for i in rng.integers(0, 4096, 256)]
    _against_bf16(8, 4096, 16, 128, True, rows=rows)


# ---------------------------------------------------------------------------------------------------------------------
# behaviour
# ---------------------------------------------------------------------------------------------------------------------
def test_rejections_raise_before_launch():
    fa = _fa()
    q8, k8, v8 = _rand8((1, 64, 2, 64), 1), _rand8((1, 64, 2, 64), 2), _rand8((1, 64, 2, 64), 3)
    slopes = torch.ones(2, device="cuda")
    for kw, match in ((dict(alibi_slopes=slopes), "ALiBi"), (dict(softcap=10.0), "softcap"),
                      (dict(dropout_p=0.1), "dropout")):
        with pytest.raises(RuntimeError, match=match):
            fa.flash_attn_func(q8, k8, v8, **kw)
    big = _rand8((1, 64, 2, 192), 4)
    with pytest.raises(RuntimeError, match="head dimension"):
        fa.flash_attn_func(big, big, big)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        fa.flash_attn_func(q8, k8.bfloat16(), v8.bfloat16())
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        fa.flash_attn_func(q8.bfloat16(), k8, v8)
    # paged fp8 K/V with fp8 q
    kc = _rand8((4, 16, 2, 64), 5)
    cu = torch.tensor([0, 64], dtype=torch.int32, device="cuda")
    bt = torch.arange(4, dtype=torch.int32, device="cuda").view(1, 4)
    with pytest.raises(RuntimeError, match="paged"):
        fa.flash_attn_varlen_func(q8[0], kc, kc, cu, torch.tensor([0, 64], dtype=torch.int32, device="cuda"), 64, 64,
                                  block_table=bt)
    torch.cuda.synchronize()


def test_backward_through_fp8_raises():
    fa = _fa()
    q8, k8, v8 = (_rand8((1, 64, 2, 64), s).requires_grad_() for s in (1, 2, 3))
    with pytest.raises(RuntimeError, match="fp8"):
        out = fa.flash_attn_func(q8, k8, v8, causal=True)
        out.float().sum().backward()
    cu = torch.tensor([0, 64], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="fp8"):
        out = fa.flash_attn_varlen_func(q8[0], k8[0], v8[0], cu, cu, 64, 64)
        out.float().sum().backward()


def test_two_calls_are_bit_identical():
    fa = _fa()
    q8, k8, v8 = _rand8((2, 777, 8, 128), 1), _rand8((2, 777, 2, 128), 2), _rand8((2, 777, 2, 128), 3)
    a, la, _ = fa.flash_attn_func(q8, k8, v8, causal=True, return_attn_probs=True)
    b, lb, _ = fa.flash_attn_func(q8, k8, v8, causal=True, return_attn_probs=True)
    assert torch.equal(a, b) and torch.equal(la, lb)


def test_opcheck_on_the_fp8_op():
    import flash_attn_mi355.torch_ops  # noqa: F401
    q8, k8, v8 = _rand8((1, 128, 2, 64), 1), _rand8((1, 128, 2, 64), 2), _rand8((1, 128, 2, 64), 3)
    args = (q8, k8, v8, None, 0.0, 0.125, True, -1, -1, 0.0, False)
    # (opcheck's test_schema compares the inputs before and after the call with arithmetic torch has no float8 kernel for -
    #  "mul_cuda" not implemented for 'Float8_e4m3fn' - so the schema's no-mutation claim is checked directly below)
    torch.library.opcheck(torch.ops.flash_attn_mi355.fwd.default, args,
                          test_utils=("test_faketensor", "test_autograd_registration"))
    before = [t.view(torch.uint8).clone() for t in (q8, k8, v8)]
    out = torch.ops.flash_attn_mi355.fwd(*args)[0]
    assert all(torch.equal(t.view(torch.uint8), b) for t, b in zip((q8, k8, v8), before))
    assert out.dtype == torch.bfloat16
    ref = _fa().flash_attn_func(q8, k8, v8, softmax_scale=0.125, causal=True)
    assert torch.equal(out, ref)


def test_graph_replay_equals_eager():
    """one graph, one stream, no parallel branches"""
    fa = _fa()
    q8, k8, v8 = _rand8((2, 500, 4, 128), 1), _rand8((2, 500, 2, 128), 2), _rand8((2, 500, 2, 128), 3)
    fn = lambda: fa.flash_attn_func(q8, k8, v8, causal=True, return_attn_probs=True)[:2]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = fn()
    q8.view(torch.uint8).copy_(_rand8((2, 500, 4, 128), 11).view(torch.uint8))     # new contents, same buffers
    g.replay()
    torch.cuda.synchronize()
    out_e, lse_e = fn()
    torch.cuda.synchronize()
    assert torch.equal(out_g, out_e) and torch.equal(lse_g, lse_e)
