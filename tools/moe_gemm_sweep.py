"""fa_moe_gemm (flash_attn_mi355.moe.moe_gemm on csrc/fa_moe_gemm.hip) next to what a user runs without it: a Python loop of
torch.mm over the segments of expert_offsets.

bf16, "nk" weights, align 1, softmax routing of random logits: (E, K_top) {(8, 2), (128, 8), (256, 8)} x (hidden -> N)
{4096 -> 28672, 2880 -> 5760, 7168 -> 4096} x T {1, 8, 128, 8192, 65536}.  Per point, alternated in one process on the same tensors:
    gemm         moe_gemm(xp, w, offsets)                                   (xp = moe_permute's output, made outside the timed region)
    loop         for e: torch.mm(xp[o[e]:o[e + 1]], w[e].T, out=out[..])    o = offsets.tolist() read OUTSIDE the timed region - the
                                                                            synchronisation a real caller pays in every layer is
                                                                            not in this number: the baseline is flattered
    gather       moe_gemm(x, w, offsets, sorted_slot=.., top_k=K)           the fused gather
    permute+gemm moe_permute_forward + moe_gemm                             what the gather replaces
Before anything is timed, each (E, K_top, shape) fills x and w with moe_gemm_ref's witness integers and asserts at T = 128 that
gemm and gather equal the exact fp32 products bit for bit.  Timing data are N(0, 1) / sqrt(hidden).
Reported: us per call, median [min .. max] of `--rounds` rounds of >= 3 evented calls after a warm-up (call time, not kernel time);
TFLOP/s over the real T K rows; weight bytes (experts with at least one row) x N x hidden x 2 over time, next to the 6.45 TB/s
fa_merge_states streams at.  Every (E, K_top, shape) runs in a child process of its own under a time limit; the sweep stops at
the first one that fails or runs out of time.

    python tools/moe_gemm_sweep.py [--only 8x2x2880x5760,..] [--tokens 1,8,128] [--ms 30] [--rounds 3]
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
ap.add_argument("--group-timeout", type=int, default=400)
ap.add_argument("--tokens", default="1,8,128,8192,65536")
ap.add_argument("--only", default=None, help="comma-separated groups E x K_top x hidden x N instead of the whole list")
ap.add_argument("--group", default=None, help="(child) E x K_top x hidden x N - measure it and print one JSON line per T")
args = ap.parse_args()

STREAM = 6.45e12
GROUPS = [f"{E}x{K}x{H}x{N}" for (E, K) in ((8, 2), (128, 8), (256, 8)) for (H, N) in ((4096, 28672), (2880, 5760), (7168, 4096))]
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
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    import torch
    from flash_attn_mi355 import moe as M
    E, K, H, N = (int(v) for v in name.split("x"))
    bf = torch.bfloat16
    gd = torch.Generator(device="cuda").manual_seed(E + H + N)
    w = torch.empty(E, N, H, device="cuda", dtype=bf)

    def routed(T):
        logits = torch.empty(T, E, device="cuda").normal_(generator=gd).to(bf)
        _, ids = M.moe_route_forward(logits, K)
        return M.moe_sort(ids, E)

    def loop(xp, off, out):
        for e in range(E):
            if off[e + 1] > off[e]:
                torch.mm(xp[off[e]:off[e + 1]], w[e].t(), out=out[off[e]:off[e + 1]])
        return out

    # the witness assertion: integers in [-3, 3], every fp32 partial sum exact, so the fp32 product rounded once is THE answer
    T0 = 128
    for e in range(E):
        w[e].copy_(torch.randint(-3, 4, (N, H), device="cuda", generator=gd))
    x = torch.randint(-3, 4, (T0, H), device="cuda", generator=gd).to(bf)
    sorted_slot, pos, offsets = routed(T0)
    xp = M.moe_permute_forward(x, sorted_slot, K)
    off = offsets.tolist()
    want = torch.zeros(xp.shape[0], N, device="cuda", dtype=bf)
    for e in range(E):
        if off[e + 1] > off[e]:
            want[off[e]:off[e + 1]] = (xp[off[e]:off[e + 1]].float() @ w[e].float().t()).to(bf)
    for got, what in ((M.moe_gemm(xp, w, offsets), "gemm"), (M.moe_gemm(x, w, offsets, sorted_slot=sorted_slot, top_k=K), "gather")):
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{name}: {what} differs from the exact product"
    del want, xp, x
    for e in range(E):
        w[e].normal_(generator=gd).mul_(H ** -0.5)

    for T in (int(t) for t in args.tokens.split(",")):
        x = torch.empty(T, H, device="cuda").normal_(generator=gd).to(bf)
        sorted_slot, pos, offsets = routed(T)
        xp = M.moe_permute_forward(x, sorted_slot, K)
        off = offsets.tolist()
        out = torch.empty(xp.shape[0], N, device="cuda", dtype=bf)
        legs = {
            "gemm": lambda: M.moe_gemm(xp, w, offsets, out=out),
            "loop": lambda: loop(xp, off, out),
            "gather": lambda: M.moe_gemm(x, w, offsets, sorted_slot=sorted_slot, top_k=K, out=out),
            "permute+gemm": lambda: M.moe_gemm(M.moe_permute_forward(x, sorted_slot, K), w, offsets, out=out),
        }
        times = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg, fn in legs.items():
                times[leg].append(_time(fn, args.ms))
        live = sum(1 for e in range(E) if off[e + 1] > off[e])
        res = {"group": name, "T": T, "rows": T * K, "live_experts": live, "block_m": M.moe_gemm_plan(xp.shape[0], N, H, E)[0],
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
    print(f"# fa_moe_gemm, bf16, 'nk', align 1; groups E x K_top x hidden x N; us per call: median [min .. max] of {args.rounds} rounds of "
          f">= 3 calls (~{args.ms:.0f} ms), legs alternated; the loop's offsets are read to the host outside the timed region; TFLOP/s over "
          f"the real T K_top rows; weight stream = live experts x N x hidden x 2 bytes / time, share of {STREAM / 1e12:.2f} TB/s", flush=True)
    for name in (args.only.split(",") if args.only else GROUPS):
        pts = run_child(name)
        if pts is None:
            return 1
        E, K, H, N = (int(v) for v in name.split("x"))
        print(f"{name}: witness data bit for bit (gemm, gather) at T = 128: ok", flush=True)
        for p in pts:
            g, lp, ga, pg = (p["legs"][k] for k in ("gemm", "loop", "gather", "permute+gemm"))
            flop = 2.0 * p["rows"] * H * N
            wbytes = p["live_experts"] * N * H * 2
            print(f"  T {p['T']:6d} (block_m {p['block_m']:3d}, {p['live_experts']:3d} live experts)", flush=True)
            print(f"    gemm         {fmt(g)} us | {flop / g[0] / 1e6:7.1f} TFLOP/s | weights {wbytes / g[0] / 1e6:6.2f} TB/s "
                  f"({100 * wbytes / (g[0] * 1e-6) / STREAM:5.1f} %)", flush=True)
            print(f"    loop         {fmt(lp)} us | {flop / lp[0] / 1e6:7.1f} TFLOP/s | loop / gemm {lp[0] / g[0]:6.2f} x"
                  f"{'   <- the op LOSES' if lp[0] < g[0] else ''}", flush=True)
            print(f"    gather       {fmt(ga)} us | permute+gemm {fmt(pg)} us | permute+gemm / gather {pg[0] / ga[0]:5.2f} x"
                  f"{'   <- the gather LOSES' if pg[0] < ga[0] else ''}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
