"""fp64 reference of fa_act_mul / fa_act_mul_bwd for the tests (a plain helper module, like cross_entropy_ref.py: no fixtures), the
error bounds the tests hold the kernels to, the launch plan restated, and the inputs both test files use.  Everything is torch
float64 on the tensors' own device (the GPU tests keep the large cases there).  U = 2^-24 is fp32's unit roundoff.

  forward_ref()    out = act(g) u (u None: act(g)) without any rounding, and B, the bound on |kernel - out|
  backward_ref()   dgate = d u act'(g), dup = d act(g), and their bounds.  leave_out names a term to get wrong ('silu_term': silu'
                   without its g (1 - s) term; 'dup_act': dup from act' instead of act): the CPU tests show that each violates
                   the bounds.
  worst(), used()  the error as a fraction of the bound, and of the bound's fp32 part alone
  plan()           csrc/fa_act_mul.hip's act_plan restated: the columns of a run, runs per row, items, grid.

Accuracy assumed for what is not a correctly rounded fp32 operation, in units of U:
  E_EXP = 2   v_exp_f32: 1 ulp.  What AMD's ISA guides state for V_EXP_F32 as far as we recall; no copy could be consulted, so it
              is an ASSUMPTION, the same one cross_entropy_ref.py makes, checked the same way: the GPU test prints the worst
              error / bound ratio per activation (profiles/act_mul.txt records it).
  E_RCP = 2   v_rcp_f32: 1 ulp.  The same source, the same status: an ASSUMPTION.
  E_ERF = 32  the device library's erff: 16 ulp, the ceiling the OpenCL C specification sets for erf, which the ROCm device
              library is built to; HIP's own table quotes a smaller figure that we could not consult.  An ASSUMPTION likewise.
  FLUSH = 2^-126   v_exp_f32 and v_rcp_f32 may flush a result below the smallest normal number to zero.
Bounds, counted from the kernel's operations in the order flash_attn_mi355/act_mul.py states (D x: the absolute error of the
fp32 value x; every fp32 operation adds U |result|; first order in U, and the final factor 2 covers the rest):
  e = e(t)       the exponent t log2e is off by |t| (rel(t) + 2 U) log2e - log2e rounded, the product rounded - which moves e by
                 that times ln 2:  rel(e) = |t| (rel(t) + 2 U) + E_EXP U.         silu: t = -g exact, rel(t) = 0
  s = sig(t)     1 + e moves by e rel(e) and rounds; rcp adds E_RCP U:  D s = s ((1 - s) rel(e) + (1 + E_RCP) U) + FLUSH
  silu           a = g s:  D a = |g| D s + U |a|;   om = 1 - s:  D om = D s + U om;   t2 = fma(g, om, 1):  D t2 = |g| D om + U |t2|
                 - t2 passes through 0 at g = -1.28: the magnitudes entering that cancellation are 1 and |g| om -;
                 a' = s t2:  D a' = D s |t2| + s D t2 + U |a'|
  gelu_tanh      q = g g: U;  p = fma(C3, q, 1):  D p = 2 U C3 q + U p;  w = (K2 g) p:  rel(w) = 3 U + D p / p;  s = sig(w) with
                 t = -w, rel(t) = rel(w);  a as for silu;  r = g om:  D r = |g| D om + U |r|;  p3 = fma(3 C3, q, 1) like p;
                 wp = K2 p3:  D wp = K2 D p3 + 2 U wp;  t2 = fma(r, wp, 1):  D t2 = D r wp + |r| D wp + U |t2|;  a' = s t2 as above
  gelu           x = g sqrt(1/2): 2 U |x|, which moves erf by at most 2 U |x| (2 / sqrt(pi)) exp(-x^2);  erff: E_ERF U |erf|;
                 ph = fma(.5, erf, .5):  D ph = D erf / 2 + U ph  - for negative g this is the cancellation 1 + erf: its error is
                 absolute, of the size U, however small ph is -;  a = g ph:  D a = |g| D ph + U |a|;
                 h = (g g)(-.5): U;  e(h): rel = |h| 3 U + E_EXP U;  pdf = e c: + 2 U, + FLUSH;  a' = fma(g, pdf, ph):
                 D a' = |g| D pdf + D ph + U |a'|
  relu, relu2    exact, but for r r: U a
  out            a u:  D = D a |u| + U |a u|          (u None: D a)
  dgate          (d u) a':  D = |d u| (D a' + 2 U |a'|)        (u None: d a':  |d| D a' + U |d a'|)
  dup            d a:  D = |d| D a + U |d a|
  in all         |kernel - ref| <= 0.5 ulp16(ref) + 2 D + FLUSH   (ulp16: the io type's spacing at |ref|, the subnormal spacing
                 below its smallest normal number; rounding the perturbed value instead of the exact one costs 0.5 ulp + 2 D, as
                 in add_norm_ref.py)
Derived, not measured."""
import math

import torch

from add_norm_ref import U, ulp

E_EXP, E_RCP, E_ERF = 2.0, 2.0, 32.0
FLUSH = 2.0 ** -126
ACTIVATIONS = ("silu", "gelu", "gelu_tanh", "relu", "relu2")
K2 = 2.0 * math.sqrt(2.0 / math.pi)
C3 = 0.044715
THREADS, UNROLL, GRID_CAP = 256, 4, 65536                # csrc/fa_act_mul.hip: ACT_THREADS, ACT_UNROLL, FA_ACT_GRID_CAP
STEP = 8 * THREADS                                       # columns a workgroup takes side by side


def plan(rows, N):
    P = -(-N // 8)
    nchunks = -(-P // (UNROLL * THREADS))
    chunk = -(-(-(-P // nchunks)) // 64) * 64
    nchunks = -(-P // chunk)
    items = rows * nchunks
    return {"run_columns": 8 * chunk, "nchunks": nchunks, "items": items, "grid": min(items, GRID_CAP)}


def second_trip_n(rows):
    """the smallest N (a multiple of 8, plus 8) at which `rows` rows are more items than the grid cap: the kernel's stride loop
    takes a second trip"""
    N = (GRID_CAP // rows) * 8 * UNROLL * THREADS + 8
    assert plan(rows, N)["items"] > GRID_CAP >= plan(rows, N - 8 * UNROLL * THREADS)["items"]
    return N


def _sig(t, rel_t):
    """(s, D s, 1 - s) of s = 1 / (1 + exp(-t)); rel_t: the relative error of t"""
    s = torch.sigmoid(t)
    om = torch.sigmoid(-t)                                   # 1 - s without cancellation
    rel_e = t.abs() * (rel_t + 2 * U) + E_EXP * U
    return s, s * (om * rel_e + (1 + E_RCP) * U) + FLUSH, om


def act_ref(g, activation):
    """(a, a', D a, D a') float64: act(g), act'(g) and the absolute errors the kernel's fp32 evaluation may have"""
    g = g.detach().double()
    ag = g.abs()
    zero = torch.zeros_like(g)
    if activation in ("silu", "gelu_tanh"):
        if activation == "silu":
            t, rel_t, wp, Dwp = g, zero, None, None
        else:
            q = g * g
            p = 1 + C3 * q
            Dp = 2 * U * C3 * q + U * p
            t = K2 * g * p
            rel_t = 3 * U + Dp / p
            p3 = 1 + 3 * C3 * q
            wp = K2 * p3
            Dwp = K2 * (2 * U * 3 * C3 * q + U * p3) + 2 * U * wp
        s, Ds, om = _sig(t, rel_t)
        a = g * s
        Da = ag * Ds + U * a.abs()
        Dom = Ds + U * om
        if activation == "silu":
            t2 = 1 + g * om
            Dt2 = ag * Dom + U * t2.abs()
        else:
            r = g * om
            Dr = ag * Dom + U * r.abs()
            t2 = 1 + r * wp
            Dt2 = Dr * wp + r.abs() * Dwp + U * t2.abs()
        d = s * t2
        Dd = Ds * t2.abs() + s * Dt2 + U * d.abs()
        return a, d, Da, Dd
    if activation == "gelu":
        x = g * math.sqrt(0.5)
        erf = torch.erf(x)
        Derf = 2 * U * x.abs() * (2 / math.sqrt(math.pi)) * torch.exp(-x * x) + E_ERF * U * erf.abs()
        ph = 0.5 * torch.erfc(-x)                            # 0.5 (1 + erf) without cancellation
        Dph = 0.5 * Derf + U * ph
        a = g * ph
        Da = ag * Dph + U * a.abs()
        h = -0.5 * g * g
        pdf = torch.exp(h) / math.sqrt(2 * math.pi)
        Dpdf = pdf * (h.abs() * 3 * U + E_EXP * U + 2 * U) + FLUSH
        d = ph + g * pdf
        Dd = ag * Dpdf + Dph + U * d.abs()
        return a, d, Da, Dd
    r = torch.where(g <= 0, zero, g)
    if activation == "relu":
        return r, torch.where(g <= 0, zero, torch.where(g > 0, torch.ones_like(g), g)), zero, zero
    assert activation == "relu2", activation
    return r * r, 2 * r, U * r * r, zero


def forward_ref(gate, up=None, activation="silu"):
    """(out float64, D: the fp32 error term of the bound)"""
    a, _, Da, _ = act_ref(gate, activation)
    if up is None:
        return a, Da
    u = up.detach().double()
    out = a * u
    return out, Da * u.abs() + U * out.abs()


def backward_ref(dout, gate, up=None, activation="silu", leave_out=None):
    """(dgate, dup or None, D dgate, D dup or None) float64"""
    a, d, Da, Dd = act_ref(gate, activation)
    if leave_out == "silu_term":
        assert activation == "silu"
        d = torch.sigmoid(gate.detach().double())
    do = dout.detach().double()
    if up is None:
        dgate = do * d
        return dgate, None, do.abs() * Dd + U * dgate.abs(), None
    u = up.detach().double()
    du = do * u
    dgate = du * d
    dup = do * (d if leave_out == "dup_act" else a)
    return dgate, dup, du.abs() * (Dd + 2 * U * d.abs()), do.abs() * Da + U * dup.abs()


def bound(ref, D, dtype):
    return 0.5 * ulp(ref, dtype) + 2 * D + FLUSH


def worst(got, ref, bnd, wrong=False, dtype=None):
    """max over elements of |got - ref| / bound; every value must be finite - unless `got` is a deliberately wrong value
    (wrong=True: a non-finite one counts as infinitely far off).  dtype: where |ref| reaches the type's largest finite number
    (fp16: relu2 of a large gate) the result must be that number or the infinity of ref's sign, and is not compared further"""
    g = got.detach().double().to(ref.device)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    if dtype is not None:
        fmax = float(torch.finfo(dtype).max)
        over = ref.abs() >= fmax * (1 - 2.0 ** -11)
        if bool(over.any()):
            ok = bool(((g[over].abs() >= fmax * (1 - 2.0 ** -10)) & (torch.sign(g[over]) == torch.sign(ref[over]))).all())
            if wrong and not ok:
                return float("inf")
            assert ok, "a result that should have reached the type's largest number did not"
            g, ref, bnd = g[~over], ref[~over], bnd[~over]
    if g.numel() == 0:
        return 0.0
    if wrong and not torch.isfinite(g).all():
        return float("inf")
    assert torch.isfinite(g).all() and torch.isfinite(ref).all(), "non-finite values where finite ones are expected"
    return float(((g - ref).abs() / bnd).max())


def used(got, ref, D, dtype):
    """how much of the fp32 part of the bound is used: max over elements of (|got - ref| - 0.5 ulp16(ref)) / (2 D + FLUSH), 0 where
    no element is further off than the final rounding alone allows.  The 0.5 ulp16 term is most of every bound, so worst() sits
    near 1 for any correctly rounded result; this is the figure that says how far the assumed accuracies are from what is seen."""
    g = got.detach().double().to(ref.device)
    fin = torch.isfinite(g) & (ref.abs() < float(torch.finfo(dtype).max) * (1 - 2.0 ** -11))
    ex = ((g - ref).abs() - 0.5 * ulp(ref, dtype)) / (2 * D + FLUSH)
    return max(float(ex[fin].max()), 0.0) if bool(fin.any()) else 0.0


def inputs(rows, N, dtype, seed=0, device="cpu"):
    """(gate, up, dout) [rows, N] of dtype: the gate covers [-12, 12] densely - a grid of rows x N values, shuffled, plus +-30 and
    +-100 and +-0 where there is room -, up and dout are normal with a few large and tiny magnitudes"""
    gen = torch.Generator(device="cpu").manual_seed(4000 + seed)
    n = rows * N
    gate = (torch.rand(n, generator=gen, dtype=torch.float64) * 24 - 12)
    gate[::7] = torch.linspace(-12, 12, gate[::7].numel(), dtype=torch.float64)
    special = torch.tensor([30.0, -30.0, 100.0, -100.0, 0.0, -0.0, -1.28, 12.0, -12.0], dtype=torch.float64)
    k = min(n, special.numel())
    pos = torch.arange(k) * (n // k)                          # (spread over the tensor; after the grid, so none is lost)
    gate[pos] = special[:k]
    scale = torch.tensor([1.0, 1e-3, 37.0])[torch.randint(0, 3, (n,), generator=gen)].double()
    up = torch.randn(n, generator=gen, dtype=torch.float64) * scale
    dout = torch.randn(n, generator=gen, dtype=torch.float64) * 2
    return tuple(t.view(rows, N).to(dtype).to(device) for t in (gate, up, dout))
