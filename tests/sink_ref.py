"""Two independent fp64 formulations of attention with sinks (one logit s_h per query head in the softmax denominator,
no value), used as the checker of the sink tests:

  (a) `ref_dense` / `ref_varlen`: direct.  The sink column is concatenated to the masked, scaled logits, softmax runs over
      keys + sink, the column is dropped and P multiplies V (the gpt-oss formulation).  Torch fp64 with autograd, so every
      gradient, dsinks included, comes from differentiating it.
  (b) `sink_identity`: on the existing oracle's out / LSE without sinks,
          out_s = out * sigmoid(LSE - s),   LSE_s = logaddexp(LSE, s)
      which reaches every feature the oracle knows (varlen, paged, kv-cache append + rotary, ALiBi, softcap, windows).
"""
import numpy as np
import torch

from oracle.attention import normalize_flags, visible_mask


def ref_dense(q, k, v, sinks, scale, causal=False, window=(-1, -1), softcap=0.0, alibi_slopes=None, normalize=True):
    """(a).  q [B, Sq, Hq, D], k / v [B, Sk, Hk, D], sinks [Hq] (None: no sink), alibi_slopes [Hq] or [B, Hq]; torch
    tensors, computed in fp64.  Returns out [B, Sq, Hq, D] and the sink-inclusive LSE [B, Hq, Sq].  A row without visible
    keys gives out 0 and LSE s_h; a sink of +inf gives out 0 and LSE +inf."""
    q, k, v = q.to(torch.float64), k.to(torch.float64), v.to(torch.float64)
    B, Sq, Hq, D = q.shape
    Sk, Hk = k.shape[1], k.shape[2]
    wl, wr = window
    if normalize:
        causal, wl, wr = normalize_flags(Sq, Sk, causal, wl, wr, alibi_slopes is not None)
    g = Hq // Hk
    kk = k.repeat_interleave(g, dim=2).permute(0, 2, 1, 3)          # [B, Hq, Sk, D]
    vv = v.repeat_interleave(g, dim=2).permute(0, 2, 1, 3)
    s = torch.matmul(q.permute(0, 2, 1, 3), kk.transpose(-1, -2)) * scale        # [B, Hq, Sq, Sk]
    if alibi_slopes is not None:
        sl = alibi_slopes.to(torch.float64).to(q.device)
        sl = sl.view(1, Hq, 1, 1) if sl.dim() == 1 else sl.view(B, Hq, 1, 1)
        i = torch.arange(Sq, device=q.device, dtype=torch.float64)[:, None]
        jp = torch.arange(Sk, device=q.device, dtype=torch.float64)[None, :] - (Sk - Sq)
        s = s - sl * (i - jp).abs()
    if softcap and softcap > 0.0:
        s = softcap * torch.tanh(s / softcap)
    vis = torch.from_numpy(visible_mask(Sq, Sk, causal, wl, wr)).to(q.device)
    s = s.masked_fill(~vis, float("-inf"))
    if sinks is None:
        col = torch.full((B, Hq, Sq, 1), float("-inf"), dtype=torch.float64, device=q.device)
    else:
        col = sinks.to(torch.float64).to(q.device).view(1, Hq, 1, 1).expand(B, Hq, Sq, 1)
    x = torch.cat([s, col], dim=-1)
    m = x.detach().amax(dim=-1, keepdim=True)
    pos_inf = torch.isposinf(m)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(torch.where(pos_inf, torch.full_like(x, float("-inf")), x) - m)
    l = e.sum(dim=-1, keepdim=True)
    p = torch.where(l > 0, e / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(e))
    out = torch.matmul(p[..., :Sk], vv).permute(0, 2, 1, 3)
    lse = torch.where(l > 0, m + torch.log(torch.where(l > 0, l, torch.ones_like(l))), torch.full_like(l, float("-inf")))
    lse = torch.where(pos_inf, torch.full_like(lse, float("inf")), lse)[..., 0]
    return out, lse


def ref_varlen(q, k, v, cu_q, cu_k, sinks, scale, causal=False, window=(-1, -1), softcap=0.0, alibi_slopes=None,
               max_seqlen_q=None, max_seqlen_k=None):
    """(a) on packed sequences: q [Tq, Hq, D], k / v [Tk, Hk, D], cu_q / cu_k int lists.  The mask flags are normalised
    with the batch maxima (as the varlen op does).  Returns out [Tq, Hq, D], LSE [Hq, Tq]."""
    B = len(cu_q) - 1
    msq = max_seqlen_q if max_seqlen_q is not None else max(cu_q[b + 1] - cu_q[b] for b in range(B))
    msk = max_seqlen_k if max_seqlen_k is not None else max(cu_k[b + 1] - cu_k[b] for b in range(B))
    causal, wl, wr = normalize_flags(msq, msk, causal, window[0], window[1], alibi_slopes is not None)
    outs, lses = [], []
    for b in range(B):
        q0, q1, k0, k1 = cu_q[b], cu_q[b + 1], cu_k[b], cu_k[b + 1]
        if q1 == q0:
            continue
        sl = None if alibi_slopes is None else (alibi_slopes if alibi_slopes.dim() == 1 else alibi_slopes[b])
        o, l = ref_dense(q[None, q0:q1], k[None, k0:k1], v[None, k0:k1], sinks, scale, causal, (wl, wr), softcap, sl,
                         normalize=False)
        outs.append(o[0])
        lses.append(l[0])
    Hq, D = q.shape[1], v.shape[2]
    out = torch.cat(outs, 0) if outs else q.new_zeros((0, Hq, D), dtype=torch.float64)
    lse = torch.cat(lses, 1) if lses else q.new_zeros((Hq, 0), dtype=torch.float64)
    return out, lse


def sink_identity(out, lse, sinks, head_axis):
    """(b).  out / lse: numpy results WITHOUT sinks, out shaped lse.shape + (D,) (the head at `head_axis` of both), sinks
    [Hq] numpy.  Returns (out_s, lse_s) in fp64: out * sigmoid(LSE - s), logaddexp(LSE, s); a sink of -inf changes
    nothing."""
    out = np.asarray(out, dtype=np.float64)
    lse = np.asarray(lse, dtype=np.float64)
    assert out.shape[:-1] == lse.shape, (out.shape, lse.shape)
    s = np.asarray(sinks, dtype=np.float64)
    sh = [1] * lse.ndim
    sh[head_axis] = -1
    s_l = np.broadcast_to(s.reshape(sh), lse.shape)
    none = np.isneginf(s_l)
    with np.errstate(over="ignore", invalid="ignore"):
        frac = np.where(none, 1.0, 1.0 / (1.0 + np.exp(np.where(none, 0.0, s_l - lse))))
        lse_s = np.where(none, lse, np.logaddexp(lse, s_l))
    return out * frac[..., None], lse_s


def sink_identity_bhs(out_bhsd, lse_bhs, sinks):
    """(b) for the dense oracle's layout: out [B, H, S, D] + lse [B, H, S]"""
    return sink_identity(out_bhsd, lse_bhs, sinks, 1)


def sink_identity_bshd(out_bshd, lse_bhs, sinks):
    """(b) for out [B, S, H, D] (kv-cache oracle) + lse [B, H, S]"""
    o, l = sink_identity(np.swapaxes(out_bshd, 1, 2), lse_bhs, sinks, 1)
    return np.swapaxes(o, 1, 2), l


def sink_identity_thd(out_thd, lse_ht, sinks):
    """(b) for the varlen oracle's layout: out [T, H, D] + lse [H, T]"""
    o, l = sink_identity(np.swapaxes(out_thd, 0, 1), lse_ht, sinks, 0)
    return np.swapaxes(o, 0, 1), l
