"""The merge rule of attention states over DISJOINT key sets, stated in numpy fp64 (a plain helper module, like sink_ref.py):

    LSE = logsumexp_s(lse_s),    out = sum_s exp(lse_s - LSE) out_s.

A part whose lse_s is -inf contributes nothing, whatever its out_s holds (NaN included); if every part is -inf the row gives
out = 0 and LSE = -inf.  This is the checker of fa_merge_states (csrc/fa_merge.hip) and of the shared-prefix operator; it shares
no code with either, nor with sharding.merge_attention_shards."""
import numpy as np


def merge_ref(outs, lses):
    """outs[s] [..., D], lses[s] [...] (the same leading shape) -> (out [..., D], lse [...]) in fp64"""
    outs = [np.asarray(o, dtype=np.float64) for o in outs]
    lses = [np.asarray(l, dtype=np.float64) for l in lses]
    for o, l in zip(outs, lses):
        assert o.shape[:-1] == l.shape and o.shape == outs[0].shape, (o.shape, l.shape)
    L = np.stack(lses)                                            # [n, ...]
    m = L.max(axis=0)
    has = np.isfinite(m)                                          # (LSEs are finite or -inf)
    m0 = np.where(has, m, 0.0)
    with np.errstate(invalid="ignore"):
        e = np.where(np.isneginf(L), 0.0, np.exp(L - m0))
    den = e.sum(axis=0)
    lse = np.where(has, m0 + np.log(np.where(has, den, 1.0)), -np.inf)
    out = np.zeros_like(outs[0])
    for o, es in zip(outs, e):
        w = es / np.where(has, den, 1.0)
        out += np.where((w > 0)[..., None], o, 0.0) * w[..., None]      # (a dead part's NaN never meets its zero weight)
    return out, lse


def merge_ref_bshd(outs, lses):
    """the operators' layouts: outs[s] [B, S, H, D], lses[s] [B, H, S] -> (out [B, S, H, D], lse [B, H, S])"""
    out, lse = merge_ref([np.swapaxes(np.asarray(o, dtype=np.float64), 1, 2) for o in outs], lses)
    return np.swapaxes(out, 1, 2), lse


def merge_gate(ref, outs, lses, dtype):
    """The out gate of the device merge on 16-bit inputs, elementwise (derived, not fitted): the rounding of the result to the
    output dtype - 2^-8 |ref| for bf16, 2^-10 |ref| + 2^-24 for fp16, the output-rounding terms of fp8_gate.OUT_ROUND - plus
    n 2^-22 max_s |out_s| for the fp32 weights and sums (n parts: each weight is a few fp32 roundings, each fma one more).
    outs / lses in the layout of merge_ref; parts with lse_s = -inf do not enter the maximum."""
    from fp8_gate import OUT_ROUND
    rel, ab = OUT_ROUND[dtype]
    big = np.zeros_like(np.asarray(ref, dtype=np.float64))
    for o, l in zip(outs, lses):
        live = np.isfinite(np.asarray(l, dtype=np.float64))[..., None]
        big = np.maximum(big, np.where(live, np.abs(np.where(live, np.asarray(o, dtype=np.float64), 0.0)), 0.0))
    return rel * np.abs(ref) + ab + len(outs) * 2.0 ** -22 * big
