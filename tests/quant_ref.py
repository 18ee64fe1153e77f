"""Torch restatement of the fp8-e4m3 quantisation rule of fa_quant_fp8 / fa_add_norm_quant / fa_act_mul_quant for their tests (a
plain helper module, like kv_store_ref.py: no fixtures).  fp32 throughout, on the device of its input; y are the 16-bit values:

    a      = fmaxf(+0, |y_0|, |y_1|, ..)        over the row, or over each aligned group of 128 columns; a NaN is skipped
    a'     = fminf(a, scale_ub) if scale_ub is given else a
    scale  = fmaxf(a' / 448, 2^-64)
    inv    = 1 / scale
    code_j = e4m3(fminf(fmaxf(y_j * inv, -448), 448))          torch's cast: round to nearest even

  quant_ref()      (codes, scales); scales None for mode "static".  The keyword switches build the WRONG variants the CPU tests
                   hold the reference apart from: divide (y / scale instead of y * inv), no_abs (amax without fabs), fp8_max (240
                   in place of 448), group (64 columns in place of 128).
  nearest_e4m3()   the code nearest to a float64 value among the 254 finite e4m3 values, ties to the even code, saturating - by
                   search, without torch's cast.
  inputs()         the rows the tests use: magnitudes from 1e-3 to 300 mixed, a share of exact zeros and of -0.
  same_bits()      bit-exact equality (integer views: -0 != +0, NaN == NaN)."""
import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
FLOOR = 2.0 ** -64
GROUP = 128
_INT_OF = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, FP8: torch.uint8,
           torch.uint8: torch.uint8}


def _f32(v, like):
    return torch.tensor(float(v), dtype=torch.float32, device=like.device)


def amax(y, *, no_abs=False):
    """fmaxf(+0, ..) over the last dimension: fp32, a NaN skipped"""
    m = y.float() if no_abs else y.float().abs()
    m = torch.where(torch.isnan(m), torch.zeros_like(m), m)
    return torch.clamp(m.amax(dim=-1), min=0.0)


def scale_of(a, scale_ub=None, fp8_max=FP8_MAX):
    ap = a if scale_ub is None else torch.fmin(a, _f32(scale_ub, a))
    return torch.fmax(ap / _f32(fp8_max, a), _f32(FLOOR, a))


def encode(y, scale, *, divide=False, fp8_max=FP8_MAX):
    """codes of y with `scale` (fp32, broadcast against y): fmaxf / fminf clamp (a NaN product gives -448), torch's RNE cast"""
    t = y.float() / scale if divide else y.float() * (_f32(1.0, y) / scale)
    t = torch.fmin(torch.fmax(t, _f32(-fp8_max, y)), _f32(fp8_max, y))
    return t.to(FP8)


def quant_ref(y, mode="row", scale=None, scale_ub=None, *, divide=False, no_abs=False, fp8_max=FP8_MAX, group=GROUP):
    N = y.shape[-1]
    if mode == "static":
        return encode(y, _f32(scale, y), divide=divide, fp8_max=fp8_max), None
    if mode == "row":
        s = scale_of(amax(y, no_abs=no_abs), scale_ub, fp8_max)
        return encode(y, s.unsqueeze(-1), divide=divide, fp8_max=fp8_max), s
    assert mode == "group" and N % group == 0
    yg = y.reshape(y.shape[:-1] + (N // group, group))
    s = scale_of(amax(yg, no_abs=no_abs), scale_ub, fp8_max)
    return encode(yg, s.unsqueeze(-1), divide=divide, fp8_max=fp8_max).reshape(y.shape), s


def decode_table():
    """float64 values of the 256 codes (0x7F / 0xFF: NaN)"""
    return torch.arange(256, dtype=torch.uint8).view(FP8).double()


def nearest_e4m3(t):
    """codes (uint8) nearest to the float64 values t: by distance over the 127 finite magnitudes, a tie to the even code,
    saturating at 448; the sign bit is t's (so -0 and a negative value that rounds to zero give 0x80)"""
    mags = decode_table()[:127]                                   # 0x00 .. 0x7E: ascending
    d = (t.abs().clamp(max=FP8_MAX).unsqueeze(-1) - mags).abs()
    best = d.min(dim=-1, keepdim=True).values
    cand = d == best
    even = cand & (torch.arange(127) % 2 == 0)
    pick = torch.where(even.any(dim=-1), even.int().argmax(dim=-1), cand.int().argmax(dim=-1))
    return (pick + 128 * torch.signbit(t).int()).to(torch.uint8)


def inputs(rows, N, dtype, seed=0, device="cpu"):
    """[rows, N]: normal values whose magnitudes mix 1e-3, 1, 37 and 300 by column block and row, 3 % exact zeros, 1 % -0"""
    g = torch.Generator().manual_seed(1000 * seed + N + 7 * rows)
    x = torch.randn(rows, N, generator=g)
    mag = torch.tensor([1e-3, 1.0, 37.0, 300.0])[torch.randint(0, 4, (rows, N), generator=g)]
    row = torch.tensor([0.01, 1.0, 5.0])[torch.randint(0, 3, (rows, 1), generator=g)]
    x = x * mag * row
    u = torch.rand(rows, N, generator=g)
    x = torch.where(u < 0.03, torch.zeros(()), x)
    x = torch.where(u < 0.01, -torch.zeros(()), x)
    return x.to(dtype).to(device)


def same_bits(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(_INT_OF[a.dtype]), b.view(_INT_OF[b.dtype])))


def assert_same(got, want, name):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (name, got.dtype, want.dtype, got.shape, want.shape)
    ne = got.view(_INT_OF[got.dtype]) != want.view(_INT_OF[want.dtype]).to(got.device)
    if bool(ne.any()):
        idx = torch.nonzero(ne)
        first = tuple(int(i) for i in idx[0])
        raise AssertionError(f"{name}: the bits of {idx.shape[0]} of {ne.numel()} elements differ; first at {first}: got "
                             f"{float(got[first].float())}, expected {float(want[first].float())}")
