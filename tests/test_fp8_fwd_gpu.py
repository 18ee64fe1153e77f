"""GPU: the fp8-e4m3 q / k / v forward (csrc/fa_fwd_fp8.hip) - flash_attn_func / flash_attn_varlen_func with float8_e4m3fn
inputs, bf16 out.

Exact-data layout tests catch row / column / key-order permutations in both products (S^T = K Q^T and O^T = V^T P^T on the
block-scaled K = 64 MFMA); random data is held against the fp64 oracle on the dequantised inputs.

The out / LSE gate is tests/fp8_gate.py's (derived there, shared with the fp8 kinds of tests/fuzz_cases.py).  The fixed
unit-magnitude tests keep their LSE at LSE_ATOL alone."""

import numpy as np
import pytest
import torch

import fp8_gate
import oracle
from oracle.attention import normalize_flags, visible_mask
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
    """per element (rows x D) out bound of one head, see tests/fp8_gate.py"""
    return fp8_gate.bound(qh, kh, vh, scale, causal, window)[0]


_check_out = fp8_gate.check_out


def _dense_bound(q8, k8, v8, scale, causal, window):
    return fp8_gate.dense_bound(_bhsd(q8), _bhsd(k8), _bhsd(v8), scale, causal, window)[0]


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
    (1, 300, 300, 4, 2, 128, False, (-1, 40)),     # right-only window: q-block pairing
    (2, 260, 390, 4, 1, 64, True, (50, -1)),       # causal + left window
    (1, 200, 200, 2, 2, 16, True, (-1, -1)),       # width 64, 16 valid columns
    (1, 129, 200, 2, 1, 32, False, (-1, -1)),
    (1, 150, 150, 2, 2, 72, False, (-1, -1)),      # D 72: zero-padded to 80 in Python
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
    bound, _ = fp8_gate.varlen_bound(q, k, v, cu_q.cpu().numpy(), cu_k.cpu().numpy(), max(lq), max(lk), scale, causal,
                                     window)
    _check_out(_d(out), o_ref, bound, "varlen out")


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


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI: fp16 out (o_dtype = FA_FP16), descales, strided heads / batches
# ---------------------------------------------------------------------------------------------------------------------
def _abi_call(op, q8, k8, v8, o, lse, D, scale, causal, window, ds, o_dtype, cu=None):
    """fa_fwd ([B, S, H, D] views) or fa_varlen_fwd ([T, H, D] views, cu = (cu_q, cu_k, max_q, max_k)) straight through
    ctypes; o [.., H, D] 16-bit, lse [B, H, S] / [H, T]"""
    from flash_attn_mi355 import _lib
    p = _lib.FaParams()
    p.q, p.k, p.v, p.o, p.lse = q8.data_ptr(), k8.data_ptr(), v8.data_ptr(), o.data_ptr(), lse.data_ptr()
    p.dtype = p.kv_dtype = _lib.FA_FP8_E4M3
    p.o_dtype = o_dtype
    p.q_descale, p.k_descale, p.v_descale = ds
    p.softmax_scale = scale
    p.is_causal = int(causal)
    p.window_left, p.window_right = window
    p.head_dim = 64 if D <= 64 else 128
    p.head_dim_v = D if D != p.head_dim else 0
    p.nheads_q, p.nheads_k = q8.shape[-2], k8.shape[-2]
    for name, t in (("q", q8), ("k", k8), ("v", v8), ("o", o)):
        if cu is None:
            b, r, h = t.stride(0), t.stride(1), t.stride(2)
        else:
            b, r, h = 0, t.stride(0), t.stride(1)
        setattr(p, name + "_batch_stride", b)
        setattr(p, name + "_row_stride", r)
        setattr(p, name + "_head_stride", h)
    if cu is None:
        p.batch, p.seqlen_q, p.seqlen_k = q8.shape[0], q8.shape[1], k8.shape[1]
        p.lse_batch_stride, p.lse_head_stride = lse.stride(0), lse.stride(1)
    else:
        cu_q, cu_k, mq, mk = cu
        p.batch, p.seqlen_q, p.seqlen_k = cu_q.numel() - 1, mq, mk
        p.cu_seqlens_q, p.cu_seqlens_k = cu_q.data_ptr(), cu_k.data_ptr()
        p.total_q, p.total_k = q8.shape[0], k8.shape[0]
        p.lse_batch_stride, p.lse_head_stride = 0, lse.stride(0)
    _lib.call(op, p, torch.cuda.current_stream().cuda_stream)


def _strided8(shape, seed, mag=1.0):
    """every other head of a buffer twice as wide (non-contiguous head and batch strides, 16-byte multiples)"""
    *lead, H, D = shape
    return _rand8((*lead, 2 * H, D), seed, mag)[..., ::2, :]


def _both_roundings_agree(o16, obf, name):
    """fp16 and bf16 out are roundings of the same fp32 accumulator y: |fp16 - bf16| <= half an ulp of each at y, i.e.
    (2^-8 + 2^-11) |y| + 2^-25 (fp16's half subnormal spacing), with |y| <= (1 + 2^-8) max(|fp16|, |bf16|)"""
    a, b = o16.double(), obf.double()
    tol = (2.0 ** -8 + 2.0 ** -11) * (1 + 2.0 ** -8) * torch.maximum(a.abs(), b.abs()) + 2.0 ** -25
    bad = ((a - b).abs() > tol)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements of the fp16 out are not the bf16 out's rounding " \
                                f"(first at {tuple(torch.nonzero(bad)[0].tolist())})"


ABI_CASES = [
    # (D, causal, window, descales (q, k, v))
    (64, True, (-1, -1), (0.5, 0.25, 3.0)),
    (128, False, (-1, -1), (0.013, 2.0, 0.37)),
    (80, False, (33, 9), (2.0, 0.125, 0.013)),
]


@pytest.mark.parametrize("D,causal,window,ds", ABI_CASES)
def test_c_abi_fp16_and_bf16_out(D, causal, window, ds):
    from flash_attn_mi355 import _lib
    B, Sq, Sk, H, Hk = 2, 200, 263, 4, 2
    scale = 0.3
    q8, k8, v8 = _strided8((B, Sq, H, D), 61), _strided8((B, Sk, Hk, D), 62), _strided8((B, Sk, Hk, D), 63)
    outs = {}
    for name, odt, tdt in (("fp16", _lib.FA_FP16, torch.float16), ("bf16", _lib.FA_BF16, torch.bfloat16)):
        o = torch.full((B, Sq, 2 * H, D), float("nan"), dtype=tdt, device="cuda")[:, :, 1::2]
        lse = torch.empty(B, H, Sq, dtype=torch.float32, device="cuda")
        _abi_call("fa_fwd", q8, k8, v8, o, lse, D, scale, causal, window, ds, odt)
        outs[name] = (o, lse)
    torch.cuda.synchronize()
    _both_roundings_agree(outs["fp16"][0], outs["bf16"][0], "fa_fwd")
    assert torch.equal(outs["fp16"][1], outs["bf16"][1])
    q, k, v = (_bhsd(t) * d for t, d in zip((q8, k8, v8), ds))
    o_ref, lse_ref, _ = oracle.attn_fwd(q, k, v, scale, causal=causal, window=window)
    bnd, delta = fp8_gate.dense_bound(q, k, v, scale, causal, window)
    for name in ("fp16", "bf16"):
        _check_out(_bhsd(outs[name][0]), o_ref, bnd, f"fa_fwd {name} out", o_dtype=name)
    fp8_gate.check_lse(_d(outs["bf16"][1]), lse_ref, delta, "fa_fwd lse")


@pytest.mark.parametrize("D,causal,window,ds", ABI_CASES)
def test_c_abi_varlen_fp16_and_bf16_out(D, causal, window, ds):
    from flash_attn_mi355 import _lib
    lq, lk = [70, 0, 129, 1, 256], [70, 5, 300, 0, 64]
    H, Hk = 4, 1
    scale = 0.21
    cu_q = torch.tensor(np.concatenate([[0], np.cumsum(lq)]), dtype=torch.int32, device="cuda")
    cu_k = torch.tensor(np.concatenate([[0], np.cumsum(lk)]), dtype=torch.int32, device="cuda")
    q8, k8, v8 = _strided8((sum(lq), H, D), 71), _strided8((sum(lk), Hk, D), 72), _strided8((sum(lk), Hk, D), 73)
    outs = {}
    for name, odt, tdt in (("fp16", _lib.FA_FP16, torch.float16), ("bf16", _lib.FA_BF16, torch.bfloat16)):
        o = torch.full((sum(lq), 2 * H, D), float("nan"), dtype=tdt, device="cuda")[:, ::2]
        lse = torch.empty(H, sum(lq), dtype=torch.float32, device="cuda")
        _abi_call("fa_varlen_fwd", q8, k8, v8, o, lse, D, scale, causal, window, ds, odt, cu=(cu_q, cu_k, max(lq), max(lk)))
        outs[name] = (o, lse)
    torch.cuda.synchronize()
    _both_roundings_agree(outs["fp16"][0], outs["bf16"][0], "fa_varlen_fwd")
    assert torch.equal(outs["fp16"][1], outs["bf16"][1])
    q, k, v = (_d(t) * d for t, d in zip((q8, k8, v8), ds))
    cq, ck = cu_q.cpu().numpy(), cu_k.cpu().numpy()
    o_ref, lse_ref = oracle.varlen_fwd(q, k, v, cq, ck, max(lq), max(lk), scale, causal=causal, window=window)
    bnd, delta = fp8_gate.varlen_bound(q, k, v, cq, ck, max(lq), max(lk), scale, causal, window)
    for name in ("fp16", "bf16"):
        _check_out(_d(outs[name][0]), o_ref, bnd, f"fa_varlen_fwd {name} out", o_dtype=name)
    fp8_gate.check_lse(_d(outs["bf16"][1]), lse_ref, delta, "fa_varlen_fwd lse")


# ---------------------------------------------------------------------------------------------------------------------
# config 2 in full against an fp64 reference
# ---------------------------------------------------------------------------------------------------------------------
def test_config_2_every_row_against_fp64():
    """B 8, H 16, S 4096, D 128, causal (the bench's forward shape): every output row and LSE against an fp64 reference and
    the fp8 gate, both computed per (b, h) in torch.float64 on the device"""
    import time
    fa = _fa()
    B, S, H, D = 8, 4096, 16, 128
    q8, k8, v8 = _rand8((B, S, H, D), 51), _rand8((B, S, H, D), 52), _rand8((B, S, H, D), 53)
    out, lse, _ = fa.flash_attn_func(q8, k8, v8, causal=True, return_attn_probs=True)
    torch.cuda.synchronize()
    t0 = time.time()
    worst, worst_lse = 0.0, 0.0
    for b in range(B):
        for h in range(H):
            bnd, delta, ref, lref = fp8_gate.head_gate(q8[b, :, h].double(), k8[b, :, h].double(), v8[b, :, h].double(),
                                                       D ** -0.5, True, -1, -1, with_ref=True)
            got = out[b, :, h].double()
            assert bool(torch.isfinite(got).all()), f"b{b} h{h}: non-finite out"
            r = float(((got - ref).abs() / fp8_gate.gate(ref, bnd)).max())
            assert r <= 1.0, f"b{b} h{h}: out error {r:.3f} x the fp8 gate"
            gl = lse[b, h].double()
            rl = float(((gl - lref).abs() / (LSE_ATOL + delta)).max())
            assert rl <= 1.0, f"b{b} h{h}: LSE error {rl:.3f} x its gate"
            worst, worst_lse = max(worst, r), max(worst_lse, rl)
    torch.cuda.synchronize()
    print(f"config 2: worst out error / gate {worst:.3f}, LSE {worst_lse:.3f}; fp64 reference + gate {time.time() - t0:.1f} s")


# ---------------------------------------------------------------------------------------------------------------------
# the deferred rescale at its bound, exact data
# ---------------------------------------------------------------------------------------------------------------------
def _e4m3_terms(x, n):
    """x (a multiple of 1/4, 0 <= x < 128) as a sum of n e4m3 values (greedy; exact)"""
    grid = torch.arange(0, 256, dtype=torch.uint8).view(F8).float()
    grid = torch.unique(grid[torch.isfinite(grid) & (grid >= 0)]).double().numpy()
    out, r = [], float(x)
    for _ in range(n):
        t = float(grid[grid <= r + 1e-12].max())
        out.append(t)
        r -= t
    assert r == 0.0, (x, out)
    return out


def _rescale_plan(tmax, wave_of_b, ntiles):
    """host model of the kernel's deferred rescale for waves of 32 rows: per wave and tile, 'keep' or 'rescale' and
    whether some row alone would have kept (row maxima tmax[type][tile], log2 units)"""
    plan = {}
    for w, types in wave_of_b.items():
        m = np.full(len(types), -np.inf)
        for t in range(ntiles):
            mx = np.array([tmax[ty][t] for ty in types])
            with np.errstate(invalid="ignore"):
                keep = bool(np.all(mx - m <= 8.0))
                alone = bool(np.any(mx - m <= 8.0))
            plan[w, t] = ("keep", float((mx - m).max())) if keep else ("rescale", alone)
            if not keep:
                m = np.maximum(m, mx)
    return plan


def test_deferred_rescale_at_its_bound():
    """scaled log2 scores built from exact e4m3 sums (softmax_scale = ln 2: the kernel's c is 1): row type A raises its
    maximum by 7.75 every 64-key tile (just under the 2^8 threshold), type B by 8.25 (just over), type C by 8.25 / 7.75
    alternately.  A wave of A rows keeps the maximum on every other tile (P up to 2^7.75 = 215 of e4m3's 448), a wave of
    B rows rescales on every tile, a wave of A and C rows takes both paths with its rows disagreeing on the first
    rescale, and a wave of A rows with one B row rescales on every tile against 31 rows that would keep.  The remaining
    keys of a tile trail the tile's maximum by 1/4 .. 63/4 so that P covers e4m3's normal and subnormal ranges."""
    fa = _fa()
    D, ntiles, H = 64, 9, 2
    Sq, Sk = 128, 64 * ntiles
    tmax = {"A": [7.75 * t for t in range(ntiles)], "B": [8.25 * t for t in range(ntiles)], "C": [0.0]}
    for t in range(1, ntiles):
        tmax["C"].append(tmax["C"][-1] + (8.25 if t % 2 else 7.75))
    types = ["A"] * 32 + ["B"] * 32 + ["A", "C"] * 16 + ["A"] * 31 + ["B"]
    plan = _rescale_plan(tmax, {w: types[32 * w:32 * w + 32] for w in range(4)}, ntiles)
    for t in range(ntiles):
        print(f"tile {t}: " + "  ".join(f"wave {w} {plan[w, t]}" for w in range(4)))
    # (the construction: both paths and a disagreeing rescale in wave 2, the kept path near the bound)
    assert any(plan[2, t][0] == "keep" and plan[2, t][1] >= 7.5 for t in range(ntiles))
    assert any(plan[2, t] == ("rescale", True) for t in range(ntiles))
    assert any(plan[0, t][0] == "keep" for t in range(ntiles)) and all(plan[1, t][0] == "rescale" for t in range(ntiles))
    assert all(plan[3, t] == ("rescale", True) for t in range(1, ntiles))
    q = torch.zeros(1, Sq, H, D)
    k = torch.zeros(1, Sk, 1, D)
    dims = {"A": 0, "B": 8, "C": 16}
    for i, ty in enumerate(types):
        q[0, i, :, dims[ty]:dims[ty] + 8] = 1.0
    for j in range(Sk):
        t, pos = divmod(j, 64)
        peak = (5 * t + 3) % 64                                     # the tile's maximum moves around the tile
        trail = 0.25 * ((pos - peak) % 64)
        for ty, d0 in dims.items():                                 # (+16 keeps every sum >= 0; a row-wise shift)
            k[0, j, 0, d0:d0 + 4] = torch.tensor(_e4m3_terms(tmax[ty][t] - trail + 16.0, 4))
    q8, k8 = q.to(F8).cuda(), k.to(F8).cuda()
    assert torch.equal(q8.float().cpu(), q) and torch.equal(k8.float().cpu(), k)
    v8 = _rand8((1, Sk, 1, D), 81)
    scale = float(np.log(2.0))
    out, lse, _ = fa.flash_attn_func(q8, k8, v8, softmax_scale=scale, return_attn_probs=True)
    torch.cuda.synchronize()
    qd, kd, vd = _bhsd(q8), _bhsd(k8), _bhsd(v8)
    o_ref, lse_ref, _ = oracle.attn_fwd(qd, kd, vd, scale)
    bnd, delta = fp8_gate.dense_bound(qd, kd, vd, scale, False, (-1, -1))
    _check_out(_bhsd(out), o_ref, bnd, "rescale-bound out")
    fp8_gate.check_lse(_d(lse), lse_ref, delta, "rescale-bound lse")


# ---------------------------------------------------------------------------------------------------------------------
# edges and entry points
# ---------------------------------------------------------------------------------------------------------------------
def test_dense_without_keys_or_queries():
    fa = _fa()
    q8 = _rand8((2, 70, 4, 128), 1)
    e8 = torch.empty(2, 0, 2, 128, dtype=F8, device="cuda")
    for causal in (False, True):
        out, lse, _ = fa.flash_attn_func(q8, e8, e8, causal=causal, return_attn_probs=True)
        torch.cuda.synchronize()
        assert out.shape == (2, 70, 4, 128) and out.dtype == torch.bfloat16
        assert bool((out == 0).all()) and bool(torch.isneginf(lse).all()), "Sk = 0: out 0, LSE -inf"
    k8 = _rand8((2, 33, 2, 64), 2)
    out, lse, _ = fa.flash_attn_func(q8[:, :0, :, :64], k8, k8, causal=True, return_attn_probs=True)
    torch.cuda.synchronize()
    assert out.shape == (2, 0, 4, 64) and lse.shape == (2, 4, 0)


def test_packed_entry_points_match_the_unpacked_call():
    """fp8 through the four packed entry points (views into the packed buffer, passed to the kernel without a copy) gives
    bit for bit what flash_attn_func / flash_attn_varlen_func give on contiguous copies; with requires_grad they raise
    the forward-only error at forward time"""
    fa = _fa()
    B, S, H, D = 2, 300, 4, 128
    qkv = _rand8((B, S, 3, H, D), 91)
    c = lambda t: t.contiguous()
    got = fa.flash_attn_qkvpacked_func(qkv, causal=True, return_attn_probs=True)
    want = fa.flash_attn_func(c(qkv[:, :, 0]), c(qkv[:, :, 1]), c(qkv[:, :, 2]), causal=True, return_attn_probs=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "qkvpacked"
    q8, kv = _rand8((B, 200, 2 * H, D), 92), _rand8((B, S, 2, H, D), 93)
    got = fa.flash_attn_kvpacked_func(q8, kv, window_size=(40, 7), return_attn_probs=True)
    want = fa.flash_attn_func(q8, c(kv[:, :, 0]), c(kv[:, :, 1]), window_size=(40, 7), return_attn_probs=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "kvpacked"
    lens = [100, 0, 257, 64]
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")
    tqkv = _rand8((sum(lens), 3, H, D), 94)
    got = fa.flash_attn_varlen_qkvpacked_func(tqkv, cu, max(lens), causal=True, return_attn_probs=True)
    want = fa.flash_attn_varlen_func(c(tqkv[:, 0]), c(tqkv[:, 1]), c(tqkv[:, 2]), cu, cu, max(lens), max(lens),
                                     causal=True, return_attn_probs=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "varlen qkvpacked"
    tq, tkv = _rand8((sum(lens), 2 * H, D), 95), _rand8((sum(lens), 2, H, D), 96)
    got = fa.flash_attn_varlen_kvpacked_func(tq, tkv, cu, cu, max(lens), max(lens), return_attn_probs=True)
    want = fa.flash_attn_varlen_func(tq, c(tkv[:, 0]), c(tkv[:, 1]), cu, cu, max(lens), max(lens), return_attn_probs=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "varlen kvpacked"
    torch.cuda.synchronize()
    for call in (lambda: fa.flash_attn_qkvpacked_func(qkv.clone().requires_grad_()),
                 lambda: fa.flash_attn_kvpacked_func(q8, kv.clone().requires_grad_()),
                 lambda: fa.flash_attn_kvpacked_func(q8.clone().requires_grad_(), kv),
                 lambda: fa.flash_attn_varlen_qkvpacked_func(tqkv.clone().requires_grad_(), cu, max(lens)),
                 lambda: fa.flash_attn_varlen_kvpacked_func(tq, tkv.clone().requires_grad_(), cu, cu, max(lens), max(lens))):
        with pytest.raises(RuntimeError, match="forward-only"):
            call()
