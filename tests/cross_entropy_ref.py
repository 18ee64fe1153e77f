"""fp64 reference of fa_cross_entropy / fa_cross_entropy_bwd for the tests (a plain helper module, like add_norm_ref.py: no
fixtures), the error bounds the tests hold the kernels to, the launch plan restated, and the inputs both test files use.
Everything is torch float64 on the tensors' own device.  u = 2^-24 is fp32's unit roundoff.  ls = label_smoothing, zs =
lse_square_scale; the scalars enter as the fp32 values the kernel receives.

  forward_ref()    the op's formulas, literally, without any rounding:
                       l_j = scale x_j;  m = max_j l_j;  s = sum_j exp(l_j - m);  lse = m + log(s)
                       loss = lse - (1 - ls) l_label - (ls / V) sum_j l_j   (the sum skips l_j = -inf; absent at ls = 0)
                       z = zs lse^2;  loss += z;   label == ignore_index: loss = z = 0;  label outside [0, V): NaN
                   A row whose maximum is not finite gives NaN through l_j - m, as the kernel does.  leave_out names one term
                   to drop ('scale', 'smoothing', 'zloss', 'zfactor') and label_shift moves every label by one column: the
                   tests show that each violates the bounds.
  backward_ref()   from the SAVED lse (the op recomputes nothing but p_j from it):  p_j = exp(l_j - lse),  F = 1 + 2 zs lse,
                       dx_j = dloss scale (p_j F - (1 - ls) [j == label] - ls / V);   ignored row: 0;  bad label: NaN
  plan()           csrc/fa_cross_entropy.hip restated: CHUNK(dtype), nchunks, the workspace bytes, the backward's chunks, and
                   `steps`, the longest chain of merges one term passes through: CHUNK / 2048 pieces of a lane, 6 butterfly
                   stages, 3 waves through LDS, nchunks - 1 chunks, and the term's own exp.

Bounds, counted from the kernel's operations (csrc/fa_lse.h).  E_EXP u and E_LOG u are the relative errors assumed for
v_exp_f32 and the library logf: 1 ulp = 2 u each.  That is what AMD's published ISA guides state for V_EXP_F32 as far as we
recall, but no copy of the manual could be consulted while this was written, so the figure is an assumption, checked the only
way left: the GPU test prints the worst error / bound ratio against this reference (profiles/cross_entropy.txt records it), and
E_EXP must stay at least twice what that ratio needs.
  lse     one term e_j = exp(l_j - b): l_j = fl(scale x_j) is off by u |l_j| (moves lse by at most u L1, L1 = sum_j p_j |l_j|);
          the difference rounds once and the product with log2(e) - itself rounded - twice more: 3 u |l_j - b| in the exponent;
          v_exp_f32 adds E_EXP u.  Every later change of the maximum multiplies the running sum by e(m_old - m_new), whose
          exponent errors add up to 3 u |m_final - b|: in all 3 u |l_j - m| per term, weighted by p_j: 3 u W, W = sum_j p_j
          |l_j - m|.  Each merge step costs one product and one addition rounding and one exp: (E_EXP + 2) u per step; the 8
          additions inside a piece 8 u.  So s is within (3 W + (E_EXP + 2) steps + 8) u relative.  log: E_LOG u |log s|, and the
          relative error of s enters as is; the final addition rounds to fp32.
              |lse - ref| <= 0.5 ulp32(ref) + 2 u (L1 + 3 W + (E_EXP + 2) steps + 8 + (E_LOG + 1) |log s|)  =: B_lse
          (the factor 2: rounding the perturbed value instead of the exact one costs 0.5 ulp + 2 |v - y|, as in add_norm_ref).
  losses  l_label and 1 - ls round once each: 2 u (1 - ls) |l_label|; the two fused multiply-adds and the addition of z round
          to at most u M each, M = |lse| + (1 - ls) |l_label| + (ls / V) sum |l_j| + z; ls / V rounds once, every l_j once and
          their fixed-order sum has depth steps + 8: (steps + 10) u (ls / V) sum |l_j|; z = fl(fl(zs lse) lse): 2 u z and
          2 zs |lse| B_lse from lse itself.
              |loss - ref| <= 0.5 ulp32(ref) + (1 + 2 zs |lse|) B_lse + 2 u (5 M + (steps + 10) (ls / V) sum |l_j|)
              |z - ref|    <= 0.5 ulp32(ref) + 2 zs |lse| B_lse (1 + B_lse / |lse|) + 4 u z
  dlogits p_j: u |l_j| from l_j, 3 u |l_j - lse| from the difference and the product, E_EXP u from the exp; F and p F round
          once each: p F is within (|l_j| + 3 |l_j - lse| + E_EXP + 2) u.  1 - ls and ls / V round once each, the two
          subtractions once each, g = dloss scale once and the last product once, all relative to at most
          A = |g| (p F + (1 - ls) [j == label] + ls / V), the magnitudes entering the cancellation: 6 u A.  A p_j below 2^-126
          may be flushed to zero by v_exp_f32: |g| F 2^-126.
              |dx - ref| <= 0.5 ulp_x(ref) + 2 u (|g| p F (|l_j| + 3 |l_j - lse| + E_EXP + 2) + 6 A) + |g| F 2^-126
Derived, not measured - except for the check of E_EXP described above."""
import torch

from add_norm_ref import U, ulp

E_EXP = 2.0                                               # v_exp_f32: 1 ulp assumed (see above)
E_LOG = 2.0                                               # logf: 1 ulp
THREADS, STEP = 256, 2048                                 # csrc/fa_cross_entropy.hip: CE_THREADS, CE_STEP
CHUNK = {torch.float16: 32768, torch.bfloat16: 32768, torch.float32: 16384}
BWD_CHUNK = 8192
IGNORE = -100


def _f32(v):
    """a scalar as the kernel receives it: rounded to fp32"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def plan(rows, V, dtype):
    chunk = CHUNK[dtype]
    nchunks = -(-V // chunk)
    return {"chunk": chunk, "nchunks": nchunks, "workspace_bytes": 0 if nchunks == 1 else rows * nchunks * 16,
            "bwd_nchunks": -(-V // BWD_CHUNK), "steps": chunk // STEP + 6 + 3 + (nchunks - 1) + 1}


def forward_ref(x, labels, ls=0.0, scale=1.0, zs=0.0, ignore=IGNORE, leave_out=None, label_shift=0):
    """{"lse", "loss", "z"} float64 [rows] and the magnitudes of the bounds {"L1", "W", "logs", "M", "S"}; x [rows, V]"""
    ls, scale, zs = _f32(ls), _f32(scale), _f32(zs)
    V = x.shape[1]
    l = (1.0 if leave_out == "scale" else scale) * x.detach().double()
    m = l.max(-1, keepdim=True).values
    e = torch.exp(l - m)
    s = e.sum(-1, keepdim=True)
    lse = (m + torch.log(s)).squeeze(-1)
    p = e / s
    finite = ~(torch.isinf(l) & (l < 0))
    l0 = torch.where(finite, l, torch.zeros_like(l))
    lab = labels.long() + label_shift
    ign = labels.long() == ignore
    bad = ~ign & ((lab < 0) | (lab >= V))
    ll = l.gather(1, lab.clamp(0, V - 1)[:, None]).squeeze(-1)
    loss = lse - (1 - ls) * ll
    if ls > 0 and leave_out != "smoothing":
        loss = loss - (ls / V) * l0.sum(-1)
    z = zs * lse * lse
    if leave_out != "zloss":
        loss = loss + z
    nan = torch.full_like(loss, float("nan"))
    zero = torch.zeros_like(loss)
    loss = torch.where(ign, zero, torch.where(bad, nan, loss))
    z = torch.where(ign, zero, torch.where(bad, nan, z))
    S = l0.abs().sum(-1)
    return {"lse": lse, "loss": loss, "z": z,
            "L1": (p * l0.abs()).sum(-1), "W": (p * torch.where(finite, (l - m).abs(), torch.zeros_like(l))).sum(-1),
            "logs": torch.log(s).abs().squeeze(-1), "S": S,
            "M": lse.abs() + (1 - ls) * ll.abs() + (ls / V) * S + z.abs()}


def lse_bound(ref, steps):
    k = ref["L1"] + 3 * ref["W"] + (E_EXP + 2) * steps + 8 + (E_LOG + 1) * ref["logs"]
    return 0.5 * ulp(ref["lse"], torch.float32) + 2 * U * k


def loss_bound(ref, steps, ls, zs, V):
    ls, zs = _f32(ls), _f32(zs)
    B = lse_bound(ref, steps)
    return (0.5 * ulp(ref["loss"], torch.float32) + (1 + 2 * zs * ref["lse"].abs()) * B
            + 2 * U * (5 * ref["M"] + (steps + 10) * (ls / V) * ref["S"]))


def z_bound(ref, steps, zs):
    zs = _f32(zs)
    B = lse_bound(ref, steps)
    return (0.5 * ulp(ref["z"], torch.float32) + 2 * zs * ref["lse"].abs() * B * (1 + B / ref["lse"].abs().clamp(min=1e-30))
            + 4 * U * ref["z"].abs())


def backward_ref(dloss, x, labels, lse, ls=0.0, scale=1.0, zs=0.0, ignore=IGNORE, leave_out=None, label_shift=0):
    """(dx float64 [rows, V], bound-less magnitudes {"gpF", "A", "k", "gF"}) from the SAVED lse [rows] (any float dtype)"""
    ls, scale, zs = _f32(ls), _f32(scale), _f32(zs)
    V = x.shape[1]
    sc = 1.0 if leave_out == "scale" else scale
    l = sc * x.detach().double()
    lse = lse.detach().double()[:, None]
    g = (dloss.detach().double() * sc)[:, None]
    F = torch.ones_like(lse) if leave_out == "zfactor" else 1 + 2 * zs * lse
    p = torch.exp(l - lse)
    lab = labels.long() + label_shift
    ign = (labels.long() == ignore)[:, None]
    bad = ~ign & ((lab < 0) | (lab >= V))[:, None]
    onehot = torch.zeros_like(l)
    onehot.scatter_(1, lab.clamp(0, V - 1)[:, None], 1.0)
    c = 0.0 if leave_out == "smoothing" else ls / V
    dx = g * (p * F - (1 - ls) * onehot - c)
    dx = torch.where(ign, torch.zeros_like(dx), torch.where(bad, torch.full_like(dx, float("nan")), dx))
    fin = torch.isfinite(l)
    dist = torch.where(fin, l.abs() + 3 * (l - lse).abs(), torch.zeros_like(l))
    mags = {"gpF": g.abs() * p * F.abs(), "A": g.abs() * (p * F.abs() + (1 - ls) * onehot + ls / V),
            "k": dist + E_EXP + 2, "gF": (g.abs() * F.abs()).expand_as(l)}
    return dx, mags


def dx_bound(dx, mags, dtype):
    return 0.5 * ulp(dx, dtype) + 2 * U * (mags["gpF"] * mags["k"] + 6 * mags["A"]) + mags["gF"] * 2.0 ** -126


def worst(got, ref, bound, rows=None, wrong=False):
    """max over elements of |got - ref| / bound; `rows`: a bool mask of the rows to look at.  NaN / inf must sit where the
    reference has them (checked by the caller for the rows it leaves out); here every value must be finite - unless `got` is a
    deliberately wrong value (wrong=True: a non-finite one counts as infinitely far off)"""
    g = got.detach().double().to(ref.device)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    if rows is not None:
        g, ref, bound = g[rows], ref[rows], bound[rows]
    if g.numel() == 0:
        return 0.0
    if wrong and not torch.isfinite(g).all():
        return float("inf")
    assert torch.isfinite(g).all() and torch.isfinite(ref).all(), "non-finite values where finite ones are expected"
    return float(((g - ref).abs() / bound).max())


def inputs(rows, V, dtype, seed=0, chunk=None):
    """(x [rows, V] of dtype, labels int64 [rows], dloss fp32 [rows]) on the CPU: rows of logit magnitude 1e-3, 1 and 30 side by
    side; every third label is ignore_index, some sit on column 0 and on column V - 1; rows 1, 3, 5 (mod 7) hold -inf over the
    first piece, over a leading run of 20 columns and over the whole first chunk (V <= chunk: the second piece) - never over
    the label's column, and never over the whole row"""
    chunk = CHUNK[dtype] if chunk is None else chunk
    g = torch.Generator().manual_seed(1000 + seed)
    r = torch.arange(rows)
    scale = torch.tensor([1e-3, 1.0, 30.0])[(r + r // 3) % 3][:, None]      # (every magnitude also among the rows that are not ignored)
    x = (torch.randn(rows, V, generator=g) * scale).to(dtype)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[r % 5 == 0] = 0
    labels[r % 5 == 1] = V - 1
    for k, (lo, hi) in ((1, (0, 8)), (3, (0, 20)), (5, (0, chunk) if V > chunk else (8, 16))):
        hi = min(hi, V - 1)
        if hi > lo:
            sel = r % 7 == k
            x[sel, lo:hi] = float("-inf")
            labels[sel] = V - 1
    labels[r % 3 == 2] = IGNORE
    dloss = torch.randn(rows, generator=g) * 2.0
    return x, labels, dloss
