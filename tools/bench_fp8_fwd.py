"""fp8-e4m3 q / k / v forward (csrc/fa_fwd_fp8.hip) against the bf16 forward on the same data, in one process, alternating.

Each leg: >= 60 ms of warm-up calls (an idle MI355X runs its first ~35 ms of launches on a clock ramp), then `--ms` of calls
between two device events; the two legs alternate `--rounds` times and the median per call is reported.  The bf16 leg is the
shipped forward (the hand-scheduled D = 128 kernel where it applies).  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_fp8_fwd.py --prof` (fewer calls, no timing).

FLOPs are the bench's convention: 4 B H Sq Sk D, halved for causal.  Peaks (MI355X_MICROARCH.md): fp8 ~5 PF, bf16 ~2.5 PF dense.

    python tools/bench_fp8_fwd.py [--ms 400] [--rounds 3] [--prof]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v100_amd"))
import torch  # noqa: E402

import flash_attn  # noqa: E402

PEAK_FP8, PEAK_BF16 = 5.0e15, 2.5e15
F8 = torch.float8_e4m3fn


def _time(fn, ms, settle_ms=60.0):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); fn(); e.record(); e.synchronize()
    one = max(s.elapsed_time(e), 1e-3)
    for _ in range(int(settle_ms / one) + 2):
        fn()
    n = max(10, int(ms / one))
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / n


def dense(B, S, H, D, causal):
    g = torch.Generator(device="cpu").manual_seed(421)
    q8, k8, v8 = ((torch.randn(B, S, H, D, generator=g)).to(F8).cuda() for _ in range(3))
    q16, k16, v16 = q8.bfloat16(), k8.bfloat16(), v8.bfloat16()
    fl = 4.0 * B * H * S * S * D * (0.5 if causal else 1.0)
    name = f"dense B{B} H{H} S{S} D{D} {'causal' if causal else 'non-causal'}"
    return name, fl, (lambda: flash_attn.flash_attn_func(q8, k8, v8, causal=causal),
                      lambda: flash_attn.flash_attn_func(q16, k16, v16, causal=causal))


def varlen(H=16, D=128):
    g = torch.Generator().manual_seed(421)
    lens = torch.randint(256, 4097, (16,), generator=g)
    cu = torch.zeros(17, dtype=torch.int32)
    cu[1:] = lens.cumsum(0)
    T, mx = int(cu[-1]), int(lens.max())
    cu = cu.cuda()
    q8, k8, v8 = (torch.randn(T, H, D, generator=g).to(F8).cuda() for _ in range(3))
    q16, k16, v16 = q8.bfloat16(), k8.bfloat16(), v8.bfloat16()
    fl = sum(4.0 * H * int(L) * int(L) * D * 0.5 for L in lens)
    return (f"varlen 16 seqs 256-4096 (T {T}) H{H} D{D} causal", fl,
            (lambda: flash_attn.flash_attn_varlen_func(q8, k8, v8, cu, cu, mx, mx, causal=True),
             lambda: flash_attn.flash_attn_varlen_func(q16, k16, v16, cu, cu, mx, mx, causal=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", type=float, default=400.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prof", action="store_true", help="a few calls per leg for a rocprofv3 kernel trace, no timing")
    a = ap.parse_args()
    cases = [dense(8, 4096, 16, 128, True), dense(8, 4096, 16, 128, False), dense(16, 2048, 32, 64, True), varlen()]
    print(f"# {torch.cuda.get_device_name()}; fp8 vs bf16 forward, alternating, {a.rounds} rounds x {a.ms:.0f} ms per leg")
    for name, fl, (f8, f16) in cases:
        if a.prof:
            for _ in range(20):
                f8(); f16()
            torch.cuda.synchronize()
            continue
        t8, t16 = [], []
        for _ in range(a.rounds):
            t8.append(_time(f8, a.ms))
            t16.append(_time(f16, a.ms))
        m8, m16 = statistics.median(t8), statistics.median(t16)
        tf8, tf16 = fl / m8 / 1e9, fl / m16 / 1e9
        print(f"{name}: fp8 {m8:.4f} ms ({tf8:.0f} TFLOP/s, {tf8 * 1e12 / PEAK_FP8:.1%} of fp8 peak, {tf8 * 1e12 / PEAK_BF16:.1%} "
              f"of bf16 peak) [{min(t8):.4f}-{max(t8):.4f}]   bf16 {m16:.4f} ms ({tf16:.0f} TFLOP/s, {tf16 * 1e12 / PEAK_BF16:.1%} "
              f"of bf16 peak) [{min(t16):.4f}-{max(t16):.4f}]   fp8 / bf16 speed-up {m16 / m8:.2f}x", flush=True)


if __name__ == "__main__":
    main()
