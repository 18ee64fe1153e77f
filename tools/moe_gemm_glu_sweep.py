"""fa_moe_gemm_glu (flash_attn_mi355.moe.moe_gemm_glu, the GLU instantiations of csrc/fa_moe_gemm.hip) next to the two launches it
replaces: moe_gemm into h [M_max, 2 I] and act_and_mul of h.

bf16, "nk" weights, align 1, softmax routing of random logits: tools/moe_gemm_sweep.py's groups (E, K_top) {(8, 2), (128, 8),
(256, 8)} x (hidden -> 2 I) {4096 -> 28672, 2880 -> 5760, 7168 -> 4096} x T {1, 8, 128, 8192, 65536} - the packed gate-up weight
has that sweep's N columns, so the GEMM's shapes are the ones measured there and I = N / 2.  Per point, alternated in one process
on the same tensors, after every T of the group has been run once (the warm-up of every shape):
    fused     moe_gemm_glu(xp, w, offsets, out=out)
    two       act_mul_forward(h[:, :I], h[:, I:], out=out) with h = moe_gemm(xp, w, offsets, out=h)      (h allocated outside)
Before anything is timed, each (group, T) asserts that the two legs' outputs are equal bit for bit.
Reported: us per call, median [min .. max] of `--rounds` rounds of >= 3 evented calls (call time, not kernel time); two / fused;
TFLOP/s of the fused leg over the real T K_top rows (2 rows hidden 2 I); weight bytes (experts with at least one row) x 2 I x
hidden x 2 over the fused leg's time, next to the 6.45 TB/s fa_merge_states streams at.  Every group runs in a child process of
its own under a time limit; the sweep stops at the first one that fails or runs out of time.

    python tools/moe_gemm_glu_sweep.py [--only 8x2x2880x5760,..] [--tokens 1,8,128] [--ms 30] [--rounds 3]
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
ap.add_argument("--activation", default="silu")
ap.add_argument("--only", default=None, help="comma-separated groups E x K_top x hidden x 2I instead of the whole list")
ap.add_argument("--group", default=None, help="(child) E x K_top x hidden x 2I - measure it and print one JSON line per T")
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
    import torch
    from flash_attn_mi355 import act_mul as A
    from flash_attn_mi355 import moe as M
    E, K, H, N = (int(v) for v in name.split("x"))
    I, act, bf = N // 2, args.activation, torch.bfloat16
    gd = torch.Generator(device="cuda").manual_seed(E + H + N)
    w = torch.empty(E, N, H, device="cuda", dtype=bf)
    for e in range(E):
        w[e].normal_(generator=gd).mul_(H ** -0.5)
    points = []
    for T in (int(t) for t in args.tokens.split(",")):
        x = torch.empty(T, H, device="cuda").normal_(generator=gd).to(bf)
        _, ids = M.moe_route_forward(torch.empty(T, E, device="cuda").normal_(generator=gd).to(bf), K)
        sorted_slot, pos, offsets = M.moe_sort(ids, E)
        xp = M.moe_permute_forward(x, sorted_slot, K)
        h = torch.empty(xp.shape[0], N, device="cuda", dtype=bf)
        out = torch.empty(xp.shape[0], I, device="cuda", dtype=bf)
        legs = {"fused": lambda xp=xp, offsets=offsets, out=out: M.moe_gemm_glu(xp, w, offsets, activation=act, out=out),
                "two": lambda xp=xp, offsets=offsets, out=out, h=h: A.act_mul_forward(
                    *A._halves(M.moe_gemm(xp, w, offsets, out=h)), activation=act, out=out)}
        # the bit-equality assertion, which is also this shape's warm-up
        a = legs["fused"]().clone()
        b = legs["two"]()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{name} T {T}: fused differs from moe_gemm + act_mul"
        off = offsets.tolist()
        points.append((T, sum(1 for e in range(E) if off[e + 1] > off[e]), M.moe_gemm_glu_plan(xp.shape[0], I, H, E)[0], legs))
        del a, b
    for T, live, bm, legs in points:
        times = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg, fn in legs.items():
                times[leg].append(_time(fn, args.ms))
        res = {"group": name, "T": T, "rows": T * K, "live_experts": live, "block_m": bm,
               "legs": {leg: [statistics.median(t), min(t), max(t)] for leg, t in times.items()}}
        print("POINT " + json.dumps(res), flush=True)


def run_child(name):
    cmd = [sys.executable, os.path.abspath(__file__), "--group", name, "--ms", str(args.ms), "--rounds", str(args.rounds),
           "--tokens", args.tokens, "--activation", args.activation]
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
    print(f"# fa_moe_gemm_glu ({args.activation}) against moe_gemm + act_mul, bf16, 'nk', align 1; groups E x K_top x hidden x 2I; us per "
          f"call: median [min .. max] of {args.rounds} rounds of >= 3 calls (~{args.ms:.0f} ms), legs alternated after a warm-up of every "
          f"shape; TFLOP/s and weight stream (live experts x 2I x hidden x 2 bytes / time, share of {STREAM / 1e12:.2f} TB/s) of the "
          f"fused leg", flush=True)
    for name in (args.only.split(",") if args.only else GROUPS):
        pts = run_child(name)
        if pts is None:
            return 1
        E, K, H, N = (int(v) for v in name.split("x"))
        print(f"{name}: fused == moe_gemm + act_mul bit for bit at every T: ok", flush=True)
        for p in pts:
            f, t = p["legs"]["fused"], p["legs"]["two"]
            flop, wbytes = 2.0 * p["rows"] * H * N, p["live_experts"] * N * H * 2
            print(f"  T {p['T']:6d} (block_m {p['block_m']:3d}, {p['live_experts']:3d} live experts)  fused {fmt(f)} us | two {fmt(t)} us | "
                  f"two / fused {t[0] / f[0]:5.2f} x{'   <- the fused op is SLOWER' if t[0] < f[0] else ''} | "
                  f"{flop / f[0] / 1e6:7.1f} TFLOP/s | weights {wbytes / f[0] / 1e6:5.2f} TB/s ({100 * wbytes / (f[0] * 1e-6) / STREAM:5.1f} %)",
                  flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
