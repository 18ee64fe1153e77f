"""fp64 reference of the rotary embedding for the tests of fa_rotary (a plain helper module, like merge_ref.py: no fixtures).

  rotary_ref()      y = rope(x, pos) in fp64 on the 16-bit inputs as they are, per (batch, row): rows whose position falls outside
                    the cos / sin table stay unrotated.  Also returns the magnitude term |x0 c| + |x1 s| of every element, which
                    the error bound needs.
  bound()           the derived per-element bound: one rounding of the exact result to the io type, the fp32 evaluation of two
                    products and one fused add, half of fp16's subnormal spacing.
  rotate_torch()    the same rotation written in differentiable torch (fp32): what a user composes today from rotate_half."""
import numpy as np
import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}       # unit roundoff of the io type
F = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}              # half the subnormal spacing (bf16 has fp32's exponent range)


def positions(batch, seqlen, seqlen_offsets=0, cu_seqlens=None):
    """int64 [B, S] positions (dense) or [T] (packed: cu_seqlens as a list of ints)"""
    offs = np.zeros(batch, dtype=np.int64) + np.asarray(seqlen_offsets, dtype=np.int64)
    if cu_seqlens is None:
        return np.arange(seqlen, dtype=np.int64)[None, :] + offs[:, None]
    pos = np.zeros(cu_seqlens[-1], dtype=np.int64)
    for b in range(batch):
        n = cu_seqlens[b + 1] - cu_seqlens[b]
        pos[cu_seqlens[b]:cu_seqlens[b + 1]] = np.arange(n) + offs[b]
    return pos


def rotary_ref(x, cos, sin, pos, interleaved, conjugate=False):
    """x [..., H, D] tensor (16-bit or wider), cos / sin [seqlen_ro, rd / 2] tensors, pos: int array of x's leading shape.
    Returns (y, mag) as fp64 arrays of x's shape; mag = |x0 c| + |x1 s| (first of a pair) / |x0 s| + |x1 c| (second), 0 elsewhere."""
    x = x.detach().double().cpu().numpy()
    c_tab = cos.detach().double().cpu().numpy()
    s_tab = sin.detach().double().cpu().numpy() * (-1.0 if conjugate else 1.0)
    seqlen_ro, half = c_tab.shape
    rd = 2 * half
    pos = np.asarray(pos)
    ok = (pos >= 0) & (pos < seqlen_ro)
    safe = np.where(ok, pos, 0)
    c = c_tab[safe][..., None, :]                                  # [..., 1, half]
    s = s_tab[safe][..., None, :]
    if interleaved:
        x0, x1 = x[..., 0:rd:2], x[..., 1:rd:2]
    else:
        x0, x1 = x[..., :half], x[..., half:rd]
    y0, y1 = x0 * c - x1 * s, x0 * s + x1 * c
    m0, m1 = np.abs(x0 * c) + np.abs(x1 * s), np.abs(x0 * s) + np.abs(x1 * c)
    okb = ok[..., None, None]
    y0, y1 = np.where(okb, y0, x0), np.where(okb, y1, x1)
    m0, m1 = np.where(okb, m0, 0.0), np.where(okb, m1, 0.0)
    y, mag = x.copy(), np.zeros_like(x)
    if interleaved:
        y[..., 0:rd:2], y[..., 1:rd:2] = y0, y1
        mag[..., 0:rd:2], mag[..., 1:rd:2] = m0, m1
    else:
        y[..., :half], y[..., half:rd] = y0, y1
        mag[..., :half], mag[..., half:rd] = m0, m1
    return y, mag


def bound(y64, mag, dtype):
    """|y - y64| <= u |y64| + 2^-22 (|x0 c| + |x1 s|) + f per element.
    u |y64|: the one rounding of the kernel's fp32 result to the io type (round to nearest: half an ulp <= u |y|).
    2^-22 mag: the fp32 evaluation - the inner product rounds once (2^-24 of its magnitude), the fused multiply-add once more
    (2^-24 of the result, itself <= mag), and the rounding point of the io type can move by the fp32 error: 4 x 2^-24 covers them.
    f: results below the smallest normal fp16 number are rounded to a multiple of 2^-24."""
    return U[dtype] * np.abs(y64) + 2.0 ** -22 * mag + F[dtype]


def worst_ratio(y, y64, mag, dtype):
    """max over elements of |y - y64| / bound (elements with a zero bound must be exact)"""
    err = np.abs(y.detach().double().cpu().numpy() - y64)
    b = bound(y64, mag, dtype)
    exact = b == 0
    assert np.all(err[exact] == 0), "an element with a zero bound (0 in, 0 out) is not exact"
    return float(np.max(err[~exact] / b[~exact])) if np.any(~exact) else 0.0


def table_defect(cos, sin, pos, interleaved, head_dim):
    """|c^2 + s^2 - 1| per element ([..., 1, D] fp64, 0 behind rotary_dim and for rows outside the table): cos / sin rounded to 16 bits
    are no longer a rotation, so rotating with s and then with -s returns (c^2 + s^2) x, not x"""
    c = cos.detach().double().cpu().numpy()
    s = sin.detach().double().cpu().numpy()
    seqlen_ro, half = c.shape
    pos = np.asarray(pos)
    ok = (pos >= 0) & (pos < seqlen_ro)
    safe = np.where(ok, pos, 0)
    d = np.where(ok[..., None], np.abs(c[safe] ** 2 + s[safe] ** 2 - 1.0), 0.0)      # [..., half]
    out = np.zeros(pos.shape + (1, head_dim))
    if interleaved:
        out[..., 0, 0:2 * half:2], out[..., 0, 1:2 * half:2] = d, d
    else:
        out[..., 0, :half], out[..., 0, half:2 * half] = d, d
    return out


def rotate_torch(x, cos, sin, pos, interleaved):
    """differentiable fp32 torch restatement (the rotate_half composition): x [..., H, D], pos LongTensor of x's leading shape,
    every position inside the table"""
    half = cos.shape[1]
    rd = 2 * half
    c = cos.float()[pos][..., None, :]
    s = sin.float()[pos][..., None, :]
    xf = x.float()
    if interleaved:
        x0, x1 = xf[..., 0:rd:2], xf[..., 1:rd:2]
        rot = torch.stack((x0 * c - x1 * s, x0 * s + x1 * c), dim=-1).flatten(-2)
    else:
        x0, x1 = xf[..., :half], xf[..., half:rd]
        rot = torch.cat((x0 * c - x1 * s, x0 * s + x1 * c), dim=-1)
    return torch.cat((rot, xf[..., rd:]), dim=-1)
