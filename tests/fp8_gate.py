"""The error gate of the fp8-e4m3 q / k / v forward (csrc/fa_fwd_fp8.hip), shared by tests/test_fp8_fwd_gpu.py and the
differential fuzz (tests/fuzz_cases.py).  Derived, not fitted; never widened to make a case pass.

Inputs are the dequantised values (code x descale) in fp64; p = the exact softmax probabilities of one row, vis its
visible keys.

P rounding.  Both products are exact up to fp32 accumulation: an e4m3 x e4m3 product has 8 significant bits.  The one
rounding the fp8 path adds is P -> e4m3 (v_cvt_pk_fp8_f32, round to nearest): P is at most 2^8 under the deferred
rescale, so |q(P) - P| <= max(2^-4 P, 2^-10) - half an ulp of 3 mantissa bits for normal values, half the subnormal
spacing 2^-9 below 2^-6.  The row sum l is taken from the fp32 P, so the error of one output element is bounded by
    2^-4 sum_j p_ij |v_jd| + 2^-10 sum_j |v_jd| / l_i,
and l_i >= 1 (the row's largest P is exp2(s_max - m_run) with m_run <= s_max), i.e. 1 / l_i <= max_j p_ij.

Score accumulation.  The scores are exact e4m3 products summed in fp32 (D - 1 additions), so a scaled score is off by at
most  delta_ij = (D - 1) 2^-24 sum_d |q_id k_jd| x scale  (q, k dequantised: the descales are in it).  With
Delta_i = max over the row's visible keys, every ratio p'_ij / p_ij of the perturbed to the exact probabilities lies in
[e^-2Delta_i, e^2Delta_i], so the perturbation moves out by at most (e^2Delta_i - 1) sum_j p_ij |v_jd| and scales the
P-rounding term (taken on p') by at most e^2Delta_i; the LSE moves by at most Delta_i.  Delta_i >= (D - 1) 2^-24 |s_max|:
it also covers the few fp32 ulps of a large LSE's own value (|LSE| ~ s_max), where LSE_ATOL alone would not.  At unit
magnitudes e^2Delta - 1 is ~1e-4: the out gate is the P-rounding one (the fixed unit-magnitude tests keep LSE_ATOL alone).
Measured on an MI355X (one visible key per row, so LSE = the score): the block-scaled MFMA's sum of the exact products is
off by up to 6.6e-5 x sum_d |q_d k_d| at D 16 and 1.2e-5 x at D 128, 10 - 70 x this fp32 bound, at every input magnitude.
The LSE sees that in full, so the fuzz (tests/fuzz_cases.py) reports the LSE error instead of gating it; out, a ratio of
weights, stays inside the gate.

Output rounding.  bf16 out: 2^-8 |ref| (twice bf16's half-ulp 2^-9).  fp16 out: 2^-10 |ref| (twice fp16's half-ulp 2^-11)
plus 2^-24, fp16's subnormal spacing.  1e-6 on top for the fp32 accumulation of O.

The gate:  e^2Delta (P-rounding term) + (e^2Delta - 1) p|v| + output rounding + 1e-6;  LSE: LSE_ATOL + Delta.  Callers
report the largest ratio error / gate.  One MI355X run of the fixed fp8 tests before the shared gate: the largest ratio over
all random, varlen and bf16-consistency cases was 0.71 (the P roundings do not all line up as the bound assumes), the
smallest 0.16."""
import numpy as np
import torch

from oracle.attention import normalize_flags
from util import LSE_ATOL

# output rounding per out dtype: (relative, absolute)
OUT_ROUND = {"bf16": (2.0 ** -8, 0.0), "fp16": (2.0 ** -10, 2.0 ** -24)}
DTYPE_OF = {"bf16": torch.bfloat16, "fp16": torch.float16}
ACC_ATOL = 1e-6
U32 = 2.0 ** -24


def _t(x, device=None):
    if isinstance(x, torch.Tensor):
        return x.to(torch.float64)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(device or "cpu")


def head_gate(q, k, v, scale, causal, wl, wr, with_ref=False):
    """One head with flags ALREADY normalised (dense: normalize_flags(Sq, Sk, ...); varlen: with the max lengths, as the
    op does): q [Sq, D], k / v [Sk, D] dequantised.  numpy in -> numpy out; fp64 torch tensors stay on their device.
    Returns (bound [Sq, D] without the output-rounding term, delta [Sq]) and, with_ref, also (out_ref, lse_ref)."""
    as_np = not isinstance(q, torch.Tensor)
    dev = q.device if not as_np else "cpu"
    q, k, v = _t(q, dev), _t(k, dev), _t(v, dev)
    sq, sk, d = q.shape[0], k.shape[0], q.shape[1]
    if sk == 0:
        res = [torch.zeros(sq, v.shape[1], dtype=torch.float64, device=dev), torch.zeros(sq, dtype=torch.float64, device=dev)]
        if with_ref:
            res += [torch.zeros(sq, v.shape[1], dtype=torch.float64, device=dev),
                    torch.full((sq,), -np.inf, dtype=torch.float64, device=dev)]
    else:
        # the visible keys of a row are one contiguous range lo_i <= j <= hi_i (causal / window bands)
        i = torch.arange(sq, device=dev)
        lo = torch.clamp(i + (sk - sq) - wl, min=0) if wl >= 0 else torch.zeros_like(i)
        hi = torch.full_like(i, sk - 1)
        if causal:
            hi = torch.minimum(hi, i + (sk - sq))
        if wr >= 0:
            hi = torch.minimum(hi, i + (sk - sq) + wr)
        j = torch.arange(sk, device=dev)[None, :]
        vis = (j >= lo[:, None]) & (j <= hi[:, None])
        s = torch.where(vis, (q @ k.T) * scale, -torch.inf)
        m = s.max(dim=1, keepdim=True).values
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        s = torch.exp(s - m)                                   # (0 where masked)
        l = s.sum(dim=1, keepdim=True)
        p = s / torch.where(l > 0, l, torch.ones_like(l))
        del s
        dij = torch.where(vis, q.abs() @ k.abs().T, 0.0)
        delta = dij.max(dim=1).values * ((d - 1) * U32 * scale)
        del dij, vis
        av = v.abs()
        pv = p @ torch.cat([v, av], dim=1)
        ref, pav = pv[:, :v.shape[1]], pv[:, v.shape[1]:]
        csum = torch.cat([torch.zeros_like(av[:1]), av.cumsum(dim=0)])          # sum over the visible keys of |v|
        vsum = torch.where((hi >= lo)[:, None], csum[(hi + 1).clamp(min=0)] - csum[lo.clamp(max=sk)], 0.0)
        g = torch.exp(2.0 * delta)[:, None]
        pround = 2.0 ** -4 * pav + 2.0 ** -10 * p.max(dim=1, keepdim=True).values * vsum
        res = [g * pround + (g - 1.0) * pav, delta]
        if with_ref:
            has = l[:, 0] > 0
            lse = torch.where(has, m[:, 0] + torch.log(torch.where(has, l[:, 0], torch.ones_like(l[:, 0]))), -torch.inf)
            res += [ref, lse]
    return tuple(r.cpu().numpy() for r in res) if as_np else tuple(res)


def bound(qh, kh, vh, scale, causal, window, norm=None):
    """head_gate with the flags normalised on this head's own lengths (dense), or on `norm` = (max_seqlen_q,
    max_seqlen_k) (varlen, as the op does)"""
    sq, sk = norm if norm is not None else (qh.shape[0], kh.shape[0])
    c, wl, wr = normalize_flags(sq, sk, causal, window[0], window[1], False)
    return head_gate(qh, kh, vh, scale, c, wl, wr)


def dense_bound(q, k, v, scale, causal, window):
    """q [B, H, Sq, D], k / v [B, Hk, Sk, D] dequantised fp64 -> (bound [B, H, Sq, D], delta [B, H, Sq])"""
    B, H, Sq, D = q.shape
    G = H // k.shape[1]
    out = np.zeros((B, H, Sq, v.shape[3]))
    delta = np.zeros((B, H, Sq))
    for b in range(B):
        for h in range(H):
            out[b, h], delta[b, h] = bound(q[b, h], k[b, h // G], v[b, h // G], scale, causal, window)
    return out, delta


def varlen_bound(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, window, seqused_k=None):
    """q [Tq, H, D], k / v [Tk, Hk, D] dequantised fp64 -> (bound [Tq, H, D], delta [H, Tq])"""
    H, G = q.shape[1], q.shape[1] // k.shape[1]
    out = np.zeros((q.shape[0], H, v.shape[2]))
    delta = np.zeros((H, q.shape[0]))
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        if seqused_k is not None:
            k1 = k0 + min(max(int(seqused_k[b]), 0), k1 - k0)
        if q1 == q0:
            continue
        for h in range(H):
            out[q0:q1, h], delta[h, q0:q1] = bound(q[q0:q1, h], k[k0:k1, h // G], v[k0:k1, h // G], scale, causal,
                                                   window, norm=(max_q, max_k))
    return out, delta


def gate(ref, bnd, o_dtype="bf16"):
    """the whole out gate from the bound (numpy or torch)"""
    rel, ab = OUT_ROUND[o_dtype]
    return bnd + rel * abs(ref) + (ab + ACC_ATOL)


def check_out(got, ref, bnd, name, o_dtype="bf16"):
    """got / ref [..., D]; bnd of the same shape (without the output-rounding term).  Returns the largest err / gate."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = gate(ref, bnd, o_dtype)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    ratio = float((err / tol).max()) if err.size else 0.0
    print(f"{name}: max |err| {err.max() if err.size else 0:.3e}, max err / gate {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: error {ratio:.3f} x the fp8 gate"
    return ratio


def check_lse(got, ref, delta, name):
    """the -inf pattern of the reference, elsewhere |got - ref| <= LSE_ATOL + delta (per row)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    inf_ref = np.isneginf(ref)
    assert (np.isneginf(got) == inf_ref).all(), f"{name}: -inf pattern differs"
    d = np.abs(got[~inf_ref] - ref[~inf_ref])
    tol = LSE_ATOL + np.broadcast_to(np.asarray(delta, np.float64), ref.shape)[~inf_ref]
    assert np.isfinite(got[~inf_ref]).all(), f"{name}: non-finite LSE"
    ratio = float((d / tol).max()) if d.size else 0.0
    assert ratio <= 1.0, f"{name}: LSE max abs diff {d.max():.3e}, {ratio:.3f} x the gate"
    return ratio
