"""fa_mx_quant / fa_mx_dequant's rule (include/fa_mi355.h) as a plain fp64 / integer definition"""
import numpy as np

E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])


def quant(w, rule="floor"):
    """w float64 [..., N, K], "nk" -> (blocks uint8 [..., N, K / 2], scales uint8 [..., N, K / 32])"""
    x = w.reshape(*w.shape[:-1], -1, 32)
    bad = ~np.isfinite(x).all(-1)
    ax = np.where(bad[..., None], 0.0, np.abs(x))
    amax = ax.max(-1)
    m, e = np.frexp(amax)                                   # amax = (2 m) 2^(e - 1), 1 <= 2 m < 2
    b = e - 1 - 2 + 127 + ((2 * m > 1.5) if rule == "rceil" else 0)
    byte = np.where(bad, 255, np.where(amax == 0, 127, np.clip(b, 2, 252)))
    y = np.minimum(np.ldexp(ax, (127 - np.where(bad, 127, byte))[..., None]), 6.0)
    d = np.abs(y[..., None] - E2M1[:8])
    lo = d.argmin(-1)                                       # the first of two equally near codes
    nxt = np.take_along_axis(d, np.minimum(lo + 1, 7)[..., None], -1)[..., 0]
    code = lo + ((lo < 7) & (nxt == d.min(-1)) & (lo % 2 == 1))          # a tie goes to the even one
    code = np.where(bad[..., None], 0, code | (np.signbit(x) << 3)).astype(np.uint8).reshape(w.shape)
    return code[..., 0::2] | (code[..., 1::2] << 4), byte.astype(np.uint8)


def dequant(blocks, scales):
    """uint8 [..., N, K / 2], [..., N, K / 32] -> float64 [..., N, K]; a scale byte of 255: NaN"""
    codes = np.stack([blocks & 15, blocks >> 4], axis=-1).reshape(*blocks.shape[:-1], -1)
    s = np.repeat(scales.astype(np.int64), 32, axis=-1)
    return np.where(s == 255, np.nan, np.ldexp(E2M1[codes], s - 127))
