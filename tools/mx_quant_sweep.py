"""quant_mxfp4 / dequant_mxfp4 (csrc/fa_mx_quant.hip) against the eager torch composition that computes the same bits, at the
expert-weight sizes of the MXFP4 GEMM sweeps: writes profiles/mx_quant.txt.

Per cell: the bit-equality assertion first, then a warm-up and medians of evented calls, the op and the eager composition
alternated in the same run.  The rate is algorithmic bytes (2.53125 per element: 2 of w, 1 / 2 of codes, 1 / 32 of scales) over
the median.  The eager composition runs over 32 experts at a time so that its fp32 temporaries fit beside the largest case.

    python tools/mx_quant_sweep.py [--iters 9] [--warmup 3] [--out profiles/mx_quant.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v100_amd"))
from flash_attn_mi355 import quant  # noqa: E402

CASES = [(32, 5760, 2880), (128, 5760, 2880), (256, 4096, 7168)]          # E, N, K: gpt-oss gate-up at 32 / 128 experts, 7168 -> 4096
CHUNK = 32
E2M1 = [0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6]


def eager_quant(w, layout):
    """the "floor" rule in torch ops, the kernel's bits: w [E, N, K] or ("kn") [E, K, N] bf16"""
    outs = []
    for e0 in range(0, w.shape[0], CHUNK):
        c = w[e0:e0 + CHUNK]
        c = c if layout == "nk" else c.transpose(1, 2)
        E, N, K = c.shape
        x = c.float().reshape(E, N, K // 32, 32)
        ax = x.abs()
        amax = ax.amax(-1)
        bad = ~torch.isfinite(amax)
        byte = ((amax.view(torch.int32) >> 23) - 2).clamp(2, 252)
        byte = torch.where(bad, 255, torch.where(amax == 0, 127, byte))
        mul = ((254 - torch.where(bad, 127, byte)) << 23).to(torch.int32).view(torch.float32)
        y = (ax * mul[..., None]).clamp(max=6.0)
        u = y.view(torch.int32)
        kept = ((u + 0x1fffff + ((u >> 22) & 1)) >> 22) - 252
        code = torch.where(y < 2, (y + 4194304.0).view(torch.int32) & 7, kept) | ((x.view(torch.int32) >> 28) & 8)
        code = torch.where(bad[..., None], 0, code).to(torch.uint8).view(E, N, K)
        outs.append((code[..., 0::2] | (code[..., 1::2] << 4), byte.to(torch.uint8)))
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


def eager_dequant(blocks, scales, layout):
    lut = torch.tensor(E2M1, dtype=torch.float32, device=blocks.device)
    outs = []
    for e0 in range(0, blocks.shape[0], CHUNK):
        b, s = blocks[e0:e0 + CHUNK], scales[e0:e0 + CHUNK]
        codes = torch.stack([b & 15, b >> 4], -1).view(*b.shape[:2], -1)
        v = torch.ldexp(lut[codes.int()].view(*s.shape, 32), (s.int() - 127)[..., None]).view(codes.shape).to(torch.bfloat16)
        outs.append(v if layout == "nk" else v.transpose(1, 2).contiguous())
    return torch.cat(outs)


def timed(fns, iters, warmup):
    """median milliseconds of each of `fns`, called in turn"""
    ms = [[] for _ in fns]
    for it in range(warmup + iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= warmup:
                ms[i].append(a.elapsed_time(b))
    return [statistics.median(m) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_quant.txt"))
    a = ap.parse_args()
    lines = [f"# tools/mx_quant_sweep.py: {torch.cuda.get_device_name(0)}, bf16, scale_rule floor; medians of {a.iters} evented calls after "
             f"{a.warmup} warm-up rounds, op and eager alternated; GB/s = 2.53125 bytes x E N K / median",
             "# op layout E N K | op ms  op GB/s | eager ms  eager GB/s | eager / op"]
    for E, N, K in CASES:
        g = torch.Generator(device="cuda").manual_seed(E + N)
        w = torch.randn(E, N, K, device="cuda", dtype=torch.bfloat16, generator=g)
        for layout in ("nk", "kn"):
            wl = w if layout == "nk" else w.transpose(1, 2).contiguous()
            blocks, scales = quant.quant_mxfp4(wl, w_layout=layout)
            eb, es = eager_quant(wl, layout)
            assert torch.equal(blocks, eb) and torch.equal(scales, es), f"quant {layout} {E} {N} {K}: bits differ from eager"
            out = quant.dequant_mxfp4(blocks, scales, w_layout=layout)
            assert torch.equal(out.view(torch.int16), eager_dequant(blocks, scales, layout).view(torch.int16)), f"dequant {layout}"
            del eb, es
            ob = (torch.empty_like(blocks), torch.empty_like(scales))
            cells = [("quant", lambda: quant.quant_mxfp4(wl, w_layout=layout, out=ob), lambda: eager_quant(wl, layout)),
                     ("dequant", lambda: quant.dequant_mxfp4(blocks, scales, w_layout=layout, out=out),
                      lambda: eager_dequant(blocks, scales, layout))]
            for name, op, eager in cells:
                t_op, t_eager = timed([op, eager], a.iters, a.warmup)
                gb = 2.53125 * E * N * K / 1e9
                lines.append(f"{name:8s} {layout} {E:4d} {N} {K} | {t_op:9.3f} {gb / t_op * 1e3:8.0f} | {t_eager:9.3f} {gb / t_eager * 1e3:8.0f} | "
                             f"{t_eager / t_op:6.1f}")
                print(lines[-1], flush=True)
            del wl, blocks, scales, out, ob
        del w
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
