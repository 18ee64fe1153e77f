"""fp64 reference of the backward of the per-head RMSNorm + RoPE for the tests of fa_qk_norm_rope_bwd (a plain helper module, like
qk_norm_ref.py: no fixtures), and the error bounds the tests hold the kernel to.  u = 2^-24 is fp32's unit roundoff.

  forward64()      torch float64, differentiable: y = x rsqrt(mean(x^2) + eps) (offset + w), z = rope(y) at the positions, NO
                   rounding anywhere - the composition that backward_ref() is validated against through torch autograd.
  backward_ref()   numpy fp64 on the 16-bit inputs as they are:
                       dy = conj_rope(dz)  (dy = dz where the forward left the element unrotated)
                       no weight:  dx = dy
                       weight:     xhat = x rstd, a = dy g, c = mean_d(a xhat), dx = rstd (a - xhat c), dw = sum_rows,heads dy xhat
                   together with the magnitudes the bounds are stated in: M = |dz cos| + |dz_partner sin| (|dz| where unrotated),
                   A = rstd (|g| M + |xhat| mean_d(|g| M |xhat|)) and S[d] = sum_rows,heads |dy xhat|.
  backward_ref_torch(), dx_worst_torch()   the same formulas (one function serves both) and the dx bound in torch float64 on
                   the tensors' device, for the one large shape of the tests and for tools/qk_norm_bwd_sweep.py.
  dx_bound()       |got - ref| <= 0.5 ulp16(ref) + K_x(D) u A,  K_x(D) = 5 D / 2 + 26.  Counted from the kernel's operation order:
                     rstd   the sum of D exact squares through at most D - 1 fp32 additions, the division by D, the sum with eps,
                            the root (which halves what came before) and the reciprocal: (D + 1) / 2 + 2 roundings, relative;
                     xhat   = x rstd, one more: D / 2 + 3.5;
                     dy     the two products of 16-bit values are exact in fp32 and the fused multiply-add rounds once: u |dy| <= u M;
                     a      = dy g with g = offset + w: two more, 3 u |g| M in all;
                     dot    D terms a xhat through at most D roundings of partial sums: (3 + D / 2 + 3.5 + D) u sum |g| M |xhat|;
                     c      = dot / D, one more: (3 D / 2 + 7.5) u mean(|g| M |xhat|);
                     t      = fma(-xhat, c, a): with P = |g| M and Q = |xhat| mean(|g| M |xhat|) the errors of c, xhat and a and the
                            rounding of t (|t| <= P + Q) give (2 D + 12) u Q + 4 u P;
                     dx     = rstd t: the error of rstd and one rounding, (D / 2 + 3.5) u (P + Q), on top.
                   The largest coefficient is Q's, 5 D / 2 + 15.5; the 10.5 up to 26 cover the second-order terms.  A bounds the
                   magnitudes that enter the cancellation a - xhat c, not |ref|.
  dx_bound_plain() a tensor without a weight: 0.5 ulp16(ref) + u |ref| - dy is the correctly rounded fp32 value of the exact sum of
                   two exact products, then rounded to the io type.
  plan()           the launch plan of csrc/fa_qk_norm_rope_bwd.hip restated (qnb_plan: the constants below are the kernel's) and
                   the longest chain of sequential fp32 additions one dw sum passes through:
                       L = steps x U ceil(rows_per_step x heads_per_row / (slots_per_pass x U))    a lane's registers, row by row
                         + slots_per_pass - 1                                                      the workgroup's lanes through LDS
                         + ceil(grid / 16) + 15                                                    the partial rows, 16 runs, then the runs
  dw_bound()       |got - ref| <= 0.5 ulp_w(ref) + gamma(L + c) S,  gamma(n) = n u / (1 - n u);  c = D / 2 + 5 is the per-term
                   count: dy once, xhat D / 2 + 3.5 (above), rounded up; the product is fused into the addition that L counts.
                   ulp_w is the weight dtype's (fp32 weights: fp32's): dw is rounded once from the final fp32 sum.
Derived, not measured."""
import numpy as np
import torch

import qk_norm_ref as N

U = 2.0 ** -24
THREADS, ITEMS, STEP_LANES, MAX_GROUP_ROWS, GRID_CAP, FIN_SEGS = 256, 2, 2048, 64, 1024, 16      # csrc/fa_qk_norm_rope_bwd.hip


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _rope64(y, pos, cos, sin, interleaved):
    """torch: rotate y [T, H, D] at pos [T] (rows outside the table and columns >= rotary_dim stay)"""
    if cos is None or cos.shape[0] == 0:
        return y
    S, h = cos.shape
    rd = 2 * h
    at = (pos >= 0) & (pos < S)
    p = torch.where(at, pos, torch.zeros_like(pos))
    c, s = cos[p][:, None, :], sin[p][:, None, :]
    if interleaved:
        y0, y1 = y[..., 0:rd:2], y[..., 1:rd:2]
    else:
        y0, y1 = y[..., :h], y[..., h:rd]
    z0, z1 = y0 * c - y1 * s, y0 * s + y1 * c
    z = torch.stack([z0, z1], dim=-1).flatten(-2) if interleaved else torch.cat([z0, z1], dim=-1)
    z = torch.cat([z, y[..., rd:]], dim=-1)
    return torch.where(at[:, None, None], z, y)


def forward64(x, w, pos, cos, sin, interleaved, eps, offset):
    """x [T, H, D], w [D] or None, cos / sin [S, rd / 2] or None: float64 tensors (x and w may require grad) -> z, no rounding"""
    y = x
    if w is not None:
        ms = (x * x).mean(dim=-1, keepdim=True)
        y = x * torch.rsqrt(ms + float(np.float32(eps))) * (float(np.float32(offset)) + w)
    return _rope64(y, pos, cos, sin, interleaved)


def _backward(xp, dz, x, w, pos, cos, sin, interleaved, eps, offset):
    """the formulas, on fp64 numpy arrays (xp = np) or float64 torch tensors (xp = torch)"""
    dy, M = dz * 1.0, xp.abs(dz)
    if cos is not None and cos.shape[0] > 0:
        S, h = cos.shape
        rd = 2 * h
        at = (pos >= 0) & (pos < S)
        p = xp.where(at, pos, pos * 0)
        c, s = cos[p][:, None, :], sin[p][:, None, :]
        if interleaved:
            i0, i1 = slice(0, rd, 2), slice(1, rd, 2)
        else:
            i0, i1 = slice(0, h), slice(h, rd)
        z0, z1 = dz[..., i0], dz[..., i1]
        rot = at[:, None, None]
        dy[..., i0] = xp.where(rot, z0 * c + z1 * s, z0)
        dy[..., i1] = xp.where(rot, z1 * c - z0 * s, z1)
        M[..., i0] = xp.where(rot, xp.abs(z0 * c) + xp.abs(z1 * s), xp.abs(z0))
        M[..., i1] = xp.where(rot, xp.abs(z1 * c) + xp.abs(z0 * s), xp.abs(z1))
    if w is None:
        return {"dx": dy, "absdy": xp.abs(dy)}
    D = x.shape[-1]
    g = float(np.float32(offset)) + w
    rstd = 1.0 / xp.sqrt(xp.mean(x * x, axis=-1, keepdims=True) + float(np.float32(eps)))
    xhat = x * rstd
    a = dy * g
    c = xp.sum(a * xhat, axis=-1, keepdims=True) / D
    dx = rstd * (a - xhat * c)
    dw = xp.sum(dy * xhat, axis=(0, 1))
    P = xp.abs(g) * M
    A = rstd * (P + xp.abs(xhat) * xp.mean(P * xp.abs(xhat), axis=-1, keepdims=True))
    return {"dx": dx, "dw": dw, "A": A, "S": xp.sum(xp.abs(dy * xhat), axis=(0, 1))}


def backward_ref(dz, x, w, pos, cos, sin, interleaved, eps, offset):
    """tensors as the kernel gets them -> dict of fp64 arrays: dx [T, H, D]; with a weight also dw [D], A [T, H, D], S [D];
    without one absdy = |dy|"""
    pos = None if pos is None else pos.detach().cpu().numpy().astype(np.int64)
    return _backward(np, _np(dz), _np(x), _np(w), pos, _np(cos), _np(sin), interleaved, eps, offset)


def backward_ref_torch(dz, x, w, pos, cos, sin, interleaved, eps, offset):
    """backward_ref() in torch float64 on the tensors' device, for shapes where the numpy arrays would be gigabytes: the same
    formulas (one function), a dict of float64 tensors"""
    d = lambda t: None if t is None else t.detach().double()      # noqa: E731
    return _backward(torch, d(dz), d(x), d(w), None if pos is None else pos.long(), d(cos), d(sin), interleaved, eps, offset)


def dx_worst_torch(got, ref, A, dtype):
    """worst(got, ref["dx"], dx_bound(...)) on the device, from backward_ref_torch()'s tensors"""
    emin, mant = N.EMIN[dtype], N.MANT[dtype]
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin)))
    bound = 0.5 * torch.exp2(e.clamp_min(emin) - mant) + k_x(ref.shape[-1]) * U * A
    g = got.double()
    assert bool(torch.isfinite(g).all()), "non-finite values in the kernel's output"
    return float(((g - ref).abs() / bound).max())


def k_x(D):
    return 2.5 * D + 26


def dx_bound(ref, A, D, dtype):
    return 0.5 * N.ulp16(ref, dtype) + k_x(D) * U * A


def dx_bound_plain(ref, dtype):
    return 0.5 * N.ulp16(ref, dtype) + U * np.abs(ref)


def plan(T, Hq, Hk, D):
    """the kernel's launch plan for T rows of Hq + Hk heads that are worked on, and L (module docstring)"""
    G = 1
    while 8 * G < D:
        G *= 2
    hpr = Hq + Hk
    rows = min(MAX_GROUP_ROWS, max(1, -(-STEP_LANES // (hpr * G))))
    groups = -(-T // rows)
    grid = min(groups, GRID_CAP)
    spp = THREADS // G
    steps = -(-groups // grid)
    per_step = ITEMS * -(-(rows * hpr) // (spp * ITEMS))
    L = steps * per_step + (spp - 1) + -(-grid // FIN_SEGS) + FIN_SEGS - 1
    return {"G": G, "group_rows": rows, "grid": grid, "slots_per_pass": spp, "steps": steps, "L": L,
            "workspace_bytes": grid * 2 * D * 4}


def ulp32(ref):
    a = np.abs(np.asarray(ref, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 23)


def dw_bound(ref, S, L, D, wdtype):
    n = (L + D / 2 + 5) * U
    half_ulp = 0.5 * (ulp32(ref) if wdtype == torch.float32 else N.ulp16(ref, wdtype))
    return half_ulp + n / (1 - n) * S


def worst(got, ref, bound):
    """max over elements of |got - ref| / bound; a non-finite output fails"""
    g = got.detach().double().cpu().numpy()
    assert g.shape == ref.shape, (g.shape, ref.shape)
    assert np.isfinite(g).all(), "non-finite values in the kernel's output"
    return float(np.max(np.abs(g - ref) / bound))

