"""fa_moe_gemm_mxfp4 (flash_attn_mi355.moe.moe_gemm_mxfp4 on csrc/fa_moe_gemm_mxfp4.hip) next to the path a user has without
it: moe_gemm on the same weights dequantised to bf16.

bf16 x, "nk", align 1, softmax routing of random logits: (E, K_top) {(32, 4), (128, 4), (256, 8)} x (hidden -> N)
{2880 -> 5760, 2880 -> 2880, 7168 -> 4096} x T {1, 8, 128, 8192}.  Per point, alternated in one process on the same tensors:
    mxfp4    moe_gemm_mxfp4(xp, w_blocks, w_scales, offsets)     (xp = moe_permute's output, made outside the timed region)
    bf16     moe_gemm(xp, dequantised w, offsets)
Before anything is timed, each (E, K_top, shape) asserts at T = 128 on witness data - every code, scale bytes 126 ... 128, x
integers in [-3, 3]: every fp32 partial sum is exact - that mxfp4 equals the exact product rounded once AND moe_gemm on the
dequantised weights, bit for bit.  Timing data: random codes, scale bytes 118 ... 122, x N(0, 1).
Reported: us per call, median [min .. max] of `--rounds` rounds of >= 3 evented calls after a warm-up (call time, not kernel
time); the weight stream of the mxfp4 call = live experts x N x hidden x 17 / 32 bytes (codes and scales) over time; bf16 / mxfp4,
bounded by 3.76 where weights are all that moves.  Every (E, K_top, shape) runs in a child process of its own under a time limit;
the sweep stops at the first one that fails or runs out of time.

    python tools/moe_gemm_mxfp4_sweep.py [--only 32x4x2880x5760,..] [--tokens 1,8,128] [--ms 30] [--rounds 3]
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
ap.add_argument("--tokens", default="1,8,128,8192")
ap.add_argument("--only", default=None, help="comma-separated groups E x K_top x hidden x N instead of the whole list")
ap.add_argument("--group", default=None, help="(child) E x K_top x hidden x N - measure it and print one JSON line per T")
args = ap.parse_args()

GROUPS = [f"{E}x{K}x{H}x{N}" for (E, K) in ((32, 4), (128, 4), (256, 8)) for (H, N) in ((2880, 5760), (2880, 2880), (7168, 4096))]
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
    from flash_attn_mi355 import moe as M
    E, K, H, N = (int(v) for v in name.split("x"))
    bf = torch.bfloat16
    gd = torch.Generator(device="cuda").manual_seed(E + H + N)
    lut = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], device="cuda")
    blocks = torch.empty(E, N, H // 2, device="cuda", dtype=torch.uint8)
    scales = torch.empty(E, N, H // 32, device="cuda", dtype=torch.uint8)
    w = torch.empty(E, N, H, device="cuda", dtype=bf)

    def fill(lo, hi):
        """random codes and scale bytes lo ... hi; w = their bf16 dequantisation (exact), an expert at a time"""
        blocks.copy_(torch.randint(0, 256, blocks.shape, device="cuda", generator=gd, dtype=torch.uint8))
        scales.copy_(torch.randint(lo, hi + 1, scales.shape, device="cuda", generator=gd, dtype=torch.uint8))
        for e in range(E):
            codes = torch.stack([blocks[e] & 15, blocks[e] >> 4], dim=-1).reshape(N, H).long()
            w[e].copy_(lut[codes] * torch.exp2(scales[e].float() - 127).repeat_interleave(32, dim=-1))

    def routed(T):
        logits = torch.empty(T, E, device="cuda").normal_(generator=gd).to(bf)
        _, ids = M.moe_route_forward(logits, K)
        return M.moe_sort(ids, E)

    # the witness assertion: the fp32 product of the dequantised weights, every partial sum exact, rounded once is THE answer
    fill(126, 128)
    x = torch.randint(-3, 4, (128, H), device="cuda", generator=gd).to(bf)
    sorted_slot, pos, offsets = routed(128)
    xp = M.moe_permute_forward(x, sorted_slot, K)
    off = offsets.tolist()
    want = torch.zeros(xp.shape[0], N, device="cuda", dtype=bf)
    for e in range(E):
        if off[e + 1] > off[e]:
            want[off[e]:off[e + 1]] = (xp[off[e]:off[e + 1]].float() @ w[e].float().t()).to(bf)
    got = M.moe_gemm_mxfp4(xp, blocks, scales, offsets)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{name}: mxfp4 differs from the exact product"
    assert torch.equal(got.view(torch.int16), M.moe_gemm(xp, w, offsets).view(torch.int16)), f"{name}: mxfp4 differs from moe_gemm"
    del want, got, xp, x
    fill(118, 122)

    for T in (int(t) for t in args.tokens.split(",")):
        x = torch.empty(T, H, device="cuda").normal_(generator=gd).to(bf)
        sorted_slot, pos, offsets = routed(T)
        xp = M.moe_permute_forward(x, sorted_slot, K)
        off = offsets.tolist()
        out = torch.empty(xp.shape[0], N, device="cuda", dtype=bf)
        legs = {"mxfp4": lambda: M.moe_gemm_mxfp4(xp, blocks, scales, offsets, out=out),
                "bf16": lambda: M.moe_gemm(xp, w, offsets, out=out)}
        times = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg, fn in legs.items():
                times[leg].append(_time(fn, args.ms))
        live = sum(1 for e in range(E) if off[e + 1] > off[e])
        res = {"group": name, "T": T, "rows": T * K, "live_experts": live, "block_m": M.moe_gemm_mxfp4_plan(xp.shape[0], N, H, E)[0],
               "legs": {leg: [statistics.median(t), min(t), max(t)] for leg, t in times.items()}}
        print("POINT " + json.dumps(res), flush=True)
        del x, xp, out, sorted_slot, pos, offsets
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
    print(f"# fa_moe_gemm_mxfp4 against fa_moe_gemm on the dequantised weights, bf16 x, 'nk', align 1; groups E x K_top x hidden x N; us "
          f"per call: median [min .. max] of {args.rounds} rounds of >= 3 calls (~{args.ms:.0f} ms), legs alternated; weight stream = live "
          f"experts x N x hidden x 17 / 32 bytes / time", flush=True)
    for name in (args.only.split(",") if args.only else GROUPS):
        pts = run_child(name)
        if pts is None:
            return 1
        E, K, H, N = (int(v) for v in name.split("x"))
        print(f"{name}: witness data bit for bit (exact product, moe_gemm on dequantised weights) at T = 128: ok", flush=True)
        for p in pts:
            q, b = p["legs"]["mxfp4"], p["legs"]["bf16"]
            wbytes = p["live_experts"] * N * H * 17 / 32
            print(f"  T {p['T']:5d} (block_m {p['block_m']:3d}, {p['live_experts']:3d} live experts)  mxfp4 {fmt(q)} us | weights "
                  f"{wbytes / q[0] / 1e6:5.2f} TB/s | {2.0 * p['rows'] * H * N / q[0] / 1e6:7.1f} TFLOP/s | bf16 {fmt(b)} us | bf16 / mxfp4 "
                  f"{b[0] / q[0]:5.2f} x{'   <- mxfp4 LOSES' if b[0] < q[0] else ''}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
