"""fa_moe_gemm_mxfp4_dgrad (flash_attn_mi355.moe.moe_gemm_mxfp4_dgrad on csrc/fa_moe_gemm_mxfp4_dgrad.hip) next to the path a user
has without it: moe_gemm's "kn" form on the same weights dequantised to bf16 OUTSIDE the timed region - which flatters that path:
it neither pays for the dequantisation nor for the 2 E N K bytes the copy occupies.

bf16 dy, align 1, softmax routing of random logits: (E, K_top) {(32, 4), (128, 4)} x (K -> N) {2880 -> 2880, 2880 -> 5760} (the
forward's hidden -> N; the data gradient maps dy [rows, N] to dx [rows, K]) x T {128, 8192, 65536}.  Per point, alternated in one
process on the same tensors:
    mxfp4    moe_gemm_mxfp4_dgrad(dy, w_blocks, w_scales, offsets)
    bf16     moe_gemm(dy, dequantised w [E, N, K], offsets, w_layout="kn")
Before anything is timed, each group asserts at T = 128 and at T = 8192 (both plans), on the timing data, that the two legs
agree bit for bit.  Timing data: weights N(0, 1) 2^[-4, 4] through quant_mxfp4, dy N(0, 1).
Reported: us per call, median [min .. max] of `--rounds` rounds of >= 3 evented calls after a warm-up (call time, not kernel
time); TFLOP/s = 2 rows N K / time; bf16 / mxfp4; the bytes the dequantised copy would occupy, 2 E N K.  Every group runs in a
child process of its own under a time limit; the sweep stops at the first one that fails or runs out of time.

    python tools/moe_gemm_mxfp4_dgrad_sweep.py [--only 32x4x2880x5760,..] [--tokens 128,8192] [--ms 30] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--ms", type=float, default=30.0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--group-timeout", type=int, default=300)
ap.add_argument("--tokens", default="128,8192,65536")
ap.add_argument("--only", default=None, help="comma-separated groups E x K_top x K x N instead of the whole list")
ap.add_argument("--group", default=None, help="(child) E x K_top x K x N - measure it and print one JSON line per T")
args = ap.parse_args()

GROUPS = [f"{E}x{Kt}x{K}x{N}" for (E, Kt) in ((32, 4), (128, 4)) for (K, N) in ((2880, 2880), (2880, 5760))]
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "flash-attention-v100_amd")


def _time(fn, ms):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    s.record(); fn(); e.record(); e.synchronize()
    one = max(s.elapsed_time(e), 1e-3)
    for _ in range(min(int(ms / 2 / one), 200)):
        fn()
    n = max(3, min(int(ms / one), 2000))
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / n * 1e3


def group(name):
    sys.path.insert(0, PKG)
    import torch
    from flash_attn_mi355 import moe as M, quant as Q
    E, Kt, K, N = (int(v) for v in name.split("x"))
    bf = torch.bfloat16
    gd = torch.Generator(device="cuda").manual_seed(E + K + N)
    w = torch.empty(E, N, K, device="cuda", dtype=bf)
    for e in range(E):                                           # an expert at a time: no fp32 copy of the whole tensor
        w[e].copy_(torch.empty(N, K, device="cuda").normal_(generator=gd) * torch.exp2(torch.randint(-4, 5, (N, 1), device="cuda", generator=gd).float()))
    blocks, scales = Q.quant_mxfp4(w)
    Q.dequant_mxfp4(blocks, scales, out=w)                       # the bf16 leg's weights: what the codes say, exactly

    def point(T):
        logits = torch.empty(T, E, device="cuda").normal_(generator=gd).to(bf)
        _, ids = M.moe_route_forward(logits, Kt)
        _, _, offsets = M.moe_sort(ids, E)
        dy = torch.empty(T * Kt, N, device="cuda").normal_(generator=gd).to(bf)
        out = torch.empty(T * Kt, K, device="cuda", dtype=bf)
        return offsets, {"mxfp4": lambda: M.moe_gemm_mxfp4_dgrad(dy, blocks, scales, offsets, out=out),
                         "bf16": lambda: M.moe_gemm(dy, w, offsets, w_layout="kn", out=out)}

    for T in (128, 8192):                                        # both plans, before anything is timed
        _, legs = point(T)
        got = legs["mxfp4"]().clone()
        assert torch.equal(got.view(torch.int16), legs["bf16"]().view(torch.int16)), f"{name}: T {T}: mxfp4 dgrad differs from moe_gemm 'kn'"
        del legs, got
    torch.cuda.empty_cache()

    for T in (int(t) for t in args.tokens.split(",")):
        offsets, legs = point(T)
        times = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg, fn in legs.items():
                times[leg].append(_time(fn, args.ms))
        res = {"group": name, "T": T, "rows": T * Kt, "block_m": M.moe_gemm_mxfp4_dgrad_plan(T * Kt, N, K, E)[0],
               "legs": {leg: [statistics.median(t), min(t), max(t)] for leg, t in times.items()}}
        print("POINT " + json.dumps(res), flush=True)
        del legs, offsets
        torch.cuda.empty_cache()


def run_child(name):
    cmd = [sys.executable, os.path.abspath(__file__), "--group", name, "--ms", str(args.ms), "--rounds", str(args.rounds),
           "--tokens", args.tokens]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.group_timeout)
    except subprocess.TimeoutExpired:
        print(f"{name}: no result within {args.group_timeout} s - sweep stopped", flush=True)
        return None
    lines = [json.loads(l[6:]) for l in r.stdout.splitlines() if l.startswith("POINT ")]
    if r.returncode != 0 or not lines:
        print(f"{name}: exit status {r.returncode} - sweep stopped\n{r.stdout[-2000:]}", flush=True)
        return None
    return lines


fmt = lambda t: f"{t[0]:10.1f} [{t[1]:10.1f} .. {t[2]:10.1f}]"                     # noqa: E731


def main():
    if args.group:
        return group(args.group)
    print(f"# fa_moe_gemm_mxfp4_dgrad against fa_moe_gemm 'kn' on weights dequantised outside the timed region, bf16 dy, align 1; "
          f"groups E x K_top x K x N (dy [rows, N] -> dx [rows, K]); us per call: median [min .. max] of {args.rounds} rounds of >= 3 "
          f"calls (~{args.ms:.0f} ms), legs alternated", flush=True)
    for name in (args.only.split(",") if args.only else GROUPS):
        pts = run_child(name)
        if pts is None:
            return 1
        E, Kt, K, N = (int(v) for v in name.split("x"))
        print(f"{name}: bit for bit against moe_gemm 'kn' on the dequantised weights at T = 128 and 8192: ok; the dequantised copy "
              f"this op does without: 2 E N K = {2 * E * N * K / 2 ** 30:.2f} GiB (codes and scales: {E * N * K * 17 / 32 / 2 ** 30:.2f} GiB)", flush=True)
        for p in pts:
            q, b = p["legs"]["mxfp4"], p["legs"]["bf16"]
            print(f"  T {p['T']:6d} (block_m {p['block_m']:3d}, {p['rows']:7d} rows)  mxfp4 {fmt(q)} us | "
                  f"{2.0 * p['rows'] * K * N / q[0] / 1e6:7.1f} TFLOP/s | bf16 {fmt(b)} us | bf16 / mxfp4 "
                  f"{b[0] / q[0]:5.2f} x{'   <- mxfp4 dgrad is SLOWER' if b[0] < q[0] else ''}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
