"""fp64 reference of fa_add_norm / fa_add_norm_bwd for the tests (a plain helper module, like qk_norm_bwd_ref.py: no fixtures), and
the error bounds the tests hold the kernels to.  Everything is torch float64 on the tensors' own device.  u = 2^-24 is fp32's unit
roundoff.

  add_ref()        z = (float(x) + float(residual)) rounded once to residual_out's dtype: the ONE fp32 add and ONE rounding of the
                   op, restated exactly (an IEEE fp32 add is the same everywhere).
  forward64()      differentiable float64 composition without any rounding: xhat = z rstd (LayerNorm: (z - mean) rstd),
                   y = xhat (offset + w) + b - what backward_ref() is validated against through torch autograd.
  norm_ref()       y in fp64 from the STORED z, with the magnitude M of the forward bound; leave_out names one term to drop
                   ('eps', 'bias', 'offset', 'mean'): the tests show that each dropped term violates the bound.
  backward_ref()   the analytic formulas of the op: a = dy g, c = mean(a xhat), dz = rstd (a - xhat c) (LayerNorm: c1 = mean(a),
                   dz = rstd ((a - c1) - xhat c2)), dz += dres_out, dw = sum_rows dy xhat, db = sum_rows dy; with the magnitudes
                   A (dz), Sw (dw) and Sb (db) of the bounds.
  depth(N)         the longest chain of dependent fp32 roundings one row sum passes through, from csrc/fa_rowsum.h's order:
                   8 in a lane's piece (a product and 7 fused additions), pieces - 1 for the lane's pieces, log2(lanes) butterfly
                   stages, waves - 1 through LDS.  At most 24 (N = 16384).  A sum of terms t_i computed in that order is within
                   depth u sum |t_i| of the exact sum.
  Forward bound    |out - y| <= 0.5 ulp16(y) + k_fwd(N) u M,  k_fwd = 2 (d + 8), d = depth(N).  Counted:
                     RMSNorm   ss: d u relative (positive terms); / N, + eps: 2 more, the root halves them and adds 1, the reciprocal
                               1: rstd within (d / 2 + 3) u; xhat = z rstd: d / 2 + 4; g = offset + w: 1; the product (fused with
                               the bias add where there is one) rounds once more: (d / 2 + 7) u (|xhat g| + |b|).  M = |xhat g| + |b|.
                     LayerNorm mean: the sum within d u sum|z|, / N one more: (d + 1) u mean|z|.  z - mean rounds once: the
                               deviation is off by u |dev| + (d + 1) u mean|z|.  That absolute part is what enters z - mean; with
                               R = mean|z| rstd (>= 1 up to eps; several units for a row whose mean is several standard
                               deviations) it moves the variance by at most 2 (d + 1) u R relative, so rstd is within
                               (d / 2 + 4 + (d + 1) R) u and xhat within u ((d / 2 + 6 + (d + 1) R) |xhat| + (d + 1) R).  With g and
                               the fused product: u (d + 8) ((1 + R) |xhat g| + R |g| + |b|).  M = (1 + R) |xhat g| + R |g| + |b|.
                   The factor 2 in k_fwd: rounding the perturbed value v instead of y costs at most 0.5 ulp16(y) + 2 |v - y| (v may
                   lie in the binade above y's).
  Backward bound   |dx - dz| <= 0.5 ulp(dz) + k_bwd(N) u A,  k_bwd = 6 d + 44 (ulp of dx's / dres's dtype).  Counted as
                   qk_norm_bwd_ref.dx_bound with depth(N) in the place of the head dimension:
                     RMSNorm   P = |a|, Q = |xhat| mean|a xhat|: the errors of c ((3 d / 2 + 6.5) u), xhat, a (2 u) and the fused
                               multiply-add give (2 d + 11) u Q + 3 u P, times rstd ((d / 2 + 3.5) u more): (5 d / 2 + 14.5) u Q +
                               (d / 2 + 6.5) u P; the fused add of dres_out rounds once more.  A = rstd (P + Q) + |dres_out|.
                     LayerNorm with the deviation's absolute error as in the forward and C1 = mean|a|: every coefficient is at most
                               (3 d + 21) (1 + R) on A = rstd (1 + R) (P + Q + C1 (1 + |xhat|) + mean|a xhat|) + |dres_out|.
                   Doubled as in the forward, plus 2 for the last fused add.
  dw / db bound    |got - ref| <= 0.5 ulp_w(ref) + gamma(L + d + 8) S,  gamma(n) = n u / (1 - n u): L is the longest chain of
                   sequential additions of the launch plan (plan(): a lane's registers row by row, N <= 256 the workgroup's
                   lanes through LDS, N > 256 ceil(run / RW) rows of one of the RW groups of the workgroup and RW - 1 to
                   add the groups, then the partial rows in 16 runs and the runs), d + 8 bounds the relative error of one term
                   (xhat's, above).  S = sum_rows |dy| |xhat| (LayerNorm: sum_rows |dy| (|xhat| + R) (1 + R)); db: sum_rows |dy|.
Derived, not measured."""
import math

import torch

import qk_norm_ref as N16

U = 2.0 ** -24
SMALL_MAX, THREADS, MAX_PARTS, FIN_SEGS = 256, 256, 256, 16        # csrc/fa_rowsum.h, csrc/fa_add_norm_bwd.hip


def row_shape(n):
    """csrc/fa_rowsum.h row_shape(): (lanes that own a row, pieces per lane, waves)"""
    if n <= SMALL_MAX:
        g = 1
        while 8 * g < n:
            g *= 2
        return g, 1, 1
    np_ = n // 8
    threads = THREADS if np_ >= THREADS else (np_ + 63) // 64 * 64
    per = -(-np_ // threads)
    pieces = 1 if per <= 1 else 2 if per <= 2 else 4 if per <= 4 else 8
    return threads, pieces, threads // 64


def depth(n):
    lanes, pieces, waves = row_shape(n)
    return 8 + (pieces - 1) + int(math.log2(min(lanes, 64))) + (waves - 1)


def k_fwd(n):
    return 2 * (depth(n) + 8)


def k_bwd(n):
    return 6 * depth(n) + 44


def plan(rows, n, has_dbias):
    """csrc/fa_add_norm_bwd.hip anb_plan() with a weight gradient: partial rows P, the run length, the workspace, and L"""
    lanes, pieces, _ = row_shape(n)
    small = n <= SMALL_MAX
    spp = THREADS // lanes if small else 1
    units = -(-rows // spp)
    run = -(-units // MAX_PARTS)
    parts = -(-units // run)
    # rows in flight per workgroup (n > 256): group g adds the rows g, g + rw, .. of the run, then the groups are added in order
    rw = 1 if small else {1: 4, 2: 2 if has_dbias else 4, 4: 2, 8: 1}[pieces]
    L = -(-run // rw) + (rw - 1) + (spp - 1 if small else 0) + -(-parts // FIN_SEGS) + FIN_SEGS - 1
    return {"parts": parts, "run": run, "rows_in_flight": rw, "L": L, "workspace_bytes": parts * (2 if has_dbias else 1) * n * 4}


def add_ref(x, residual, ro_dtype):
    if residual is None:
        return x.to(ro_dtype)
    return (x.float() + residual.float()).to(ro_dtype)


def _d(t):
    return None if t is None else t.detach().double()


def _f32(v):
    """a scalar as the kernel receives it: rounded to fp32"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def forward64(z, w, b, eps, offset, is_rms):
    """differentiable, no rounding; z [rows, N] float64"""
    if is_rms:
        xhat = z * torch.rsqrt((z * z).mean(-1, keepdim=True) + eps)
    else:
        dev = z - z.mean(-1, keepdim=True)
        xhat = dev * torch.rsqrt((dev * dev).mean(-1, keepdim=True) + eps)
    y = xhat * (offset + w)
    return y if b is None else y + b


def _stats(z, eps, is_rms, leave_out=None):
    """(dev, rstd, R): dev = z (RMSNorm) or z - mean; R = mean|z| rstd (0 for RMSNorm)"""
    eps = 0.0 if leave_out == "eps" else _f32(eps)
    if is_rms or leave_out == "mean":
        dev = z
    else:
        dev = z - z.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((dev * dev).mean(-1, keepdim=True) + eps)
    R = torch.zeros_like(rstd) if is_rms else z.abs().mean(-1, keepdim=True) * rstd
    return dev, rstd, R


def norm_ref(z, w, b, eps, offset, is_rms, leave_out=None):
    """(y, M) float64 from the stored z [rows, N] of any dtype"""
    z, w, b = _d(z), _d(w), _d(b)
    dev, rstd, R = _stats(z, eps, is_rms, leave_out)
    g = (0.0 if leave_out == "offset" else _f32(offset)) + w
    xhat = dev * rstd
    y = xhat * g
    if b is not None and leave_out != "bias":
        y = y + b
    M = (1 + R) * (xhat * g).abs() + R * g.abs() + (0.0 if b is None else b.abs())
    return y, M


def fwd_bound(y, M, n, dtype):
    return 0.5 * ulp(y, dtype) + k_fwd(n) * U * M


def backward_ref(dy, z, w, dres_out, eps, offset, is_rms):
    """{"dz", "dw", "db", "A", "Sw", "Sb"} float64"""
    dy, z, w, dro = _d(dy), _d(z), _d(w), _d(dres_out)
    dev, rstd, R = _stats(z, eps, is_rms)
    g = _f32(offset) + w
    xhat = dev * rstd
    a = dy * g
    c2 = (a * xhat).mean(-1, keepdim=True)
    Q = xhat.abs() * (a * xhat).abs().mean(-1, keepdim=True)
    if is_rms:
        dz = rstd * (a - xhat * c2)
        A = rstd * (a.abs() + Q)
    else:
        c1 = a.mean(-1, keepdim=True)
        C1 = a.abs().mean(-1, keepdim=True)
        dz = rstd * ((a - c1) - xhat * c2)
        A = rstd * (1 + R) * (a.abs() + Q + C1 * (1 + xhat.abs()) + (a * xhat).abs().mean(-1, keepdim=True))
    if dro is not None:
        dz = dz + dro
        A = A + dro.abs()
    Sw = (dy.abs() * (xhat.abs() + R) * (1 + R)).sum(0)
    return {"dz": dz, "dw": (dy * xhat).sum(0), "db": dy.sum(0), "A": A, "Sw": Sw, "Sb": dy.abs().sum(0)}


def ulp(ref, dtype):
    """the spacing of `dtype` at |ref| (float64 tensor)"""
    a = ref.abs()
    if dtype == torch.float32:
        emin, mant = -126, 23
    else:
        emin, mant = N16.EMIN[dtype], N16.MANT[dtype]
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** emin)))
    return torch.exp2(torch.clamp(e, min=emin) - mant)


def dz_bound(ref, A, n, dtype):
    return 0.5 * ulp(ref, dtype) + k_bwd(n) * U * A


def dw_bound(ref, S, L, n, wdtype):
    m = (L + depth(n) + 8) * U
    return 0.5 * ulp(ref, wdtype) + m / (1 - m) * S


def worst(got, ref, bound):
    """max over elements of |got - ref| / bound; a non-finite output fails"""
    g = got.detach().double().to(ref.device)
    assert torch.isfinite(g).all(), "non-finite values in the kernel's output"
    assert g.shape == ref.shape, (g.shape, ref.shape)
    return float(((g - ref).abs() / bound).max())
