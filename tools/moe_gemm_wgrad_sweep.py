"""fa_moe_gemm_wgrad (flash_attn_mi355.moe.moe_gemm_wgrad on csrc/fa_moe_gemm_wgrad.hip) next to what a user runs without it: a
Python loop of torch.mm over the segments of expert_offsets, and torch._grouped_mm where this torch build runs it.

The forward sweep's prefill cells (tools/moe_gemm_sweep.py): bf16, "nk", align 1, softmax routing of random logits, (E, K_top)
{(8, 2), (128, 8), (256, 8)} x (hidden -> N) {4096 -> 28672, 2880 -> 5760, 7168 -> 4096} x T {8192, 65536}.  Per point, alternated
in one process on the same tensors:
    wgrad        moe_gemm_wgrad(dy, xp, offsets, out=dw)                      bf16 dw
    loop         for e: torch.mm(dy[o[e]:o[e + 1]].T, xp[o[e]:o[e + 1]], out=dw[e])    o = offsets.tolist() read OUTSIDE the timed
                                                                              region: the baseline is flattered by a synchronisation
    grouped_mm   torch._grouped_mm(dy.T, xp, offs=offsets[1:])                 where it runs (tried once at a small shape; else said)
    fp32+=       moe_gemm_wgrad(.., dw_dtype=fp32, out=dw32, accumulate=True)  the main-grad form (left out where dw32 passes 32 GiB)
    gather       moe_gemm_wgrad(dy, x, offsets, sorted_slot=.., top_k=K)       the fused gather
    permute+     moe_permute_forward + moe_gemm_wgrad                          what the gather replaces
    skew         one expert holds half the rows, the rest share the other half: wgrad and loop.  One accumulator chain per tile
                 makes this the bad case.
Before anything is timed, each group fills dy and x with integers in [-3, 3] and asserts at T = 128 that wgrad and gather equal
the exact fp32 products bit for bit.  Timing data are N(0, 1).  Reported: us per call, median [min .. max] of `--rounds` rounds of
>= 3 evented calls after a warm-up (call time, not kernel time); TFLOP/s over the real T K_top rows.  Every group runs in a child
process of its own under a time limit; the sweep stops at the first one that fails or runs out of time.

    python tools/moe_gemm_wgrad_sweep.py [--only 8x2x2880x5760,..] [--tokens 8192] [--ms 30] [--rounds 3] [--out profiles/moe_gemm_wgrad.txt]
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
ap.add_argument("--tokens", default="8192,65536")
ap.add_argument("--only", default=None, help="comma-separated groups E x K_top x hidden x N instead of the whole list")
ap.add_argument("--group", default=None, help="(child) E x K_top x hidden x N - measure it and print one JSON line per T")
ap.add_argument("--out", default=None, help="also append the report to this file")
args = ap.parse_args()

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
    from flash_attn_mi355 import moe as M
    E, K, H, N = (int(v) for v in name.split("x"))
    bf = torch.bfloat16
    gd = torch.Generator(device="cuda").manual_seed(E + H + N)

    def routed(T):
        logits = torch.empty(T, E, device="cuda").normal_(generator=gd).to(bf)
        _, ids = M.moe_route_forward(logits, K)
        return M.moe_sort(ids, E)

    def loop(dy, xp, off, dw):
        for e in range(E):
            if off[e + 1] > off[e]:
                torch.mm(dy[off[e]:off[e + 1]].t(), xp[off[e]:off[e + 1]], out=dw[e])
            else:
                dw[e].zero_()
        return dw

    # the witness assertion: integers in [-3, 3], every fp32 partial sum exact, so the fp32 product rounded once is THE answer
    T0 = 128
    x = torch.randint(-3, 4, (T0, H), device="cuda", generator=gd).to(bf)
    sorted_slot, pos, offsets = routed(T0)
    dy = torch.randint(-3, 4, (sorted_slot.shape[0], N), device="cuda", generator=gd).to(bf)
    xp = M.moe_permute_forward(x, sorted_slot, K)
    off = offsets.tolist()
    want = torch.zeros(E, N, H, device="cuda", dtype=bf)
    for e in range(E):
        if off[e + 1] > off[e]:
            want[e] = (dy[off[e]:off[e + 1]].float().t() @ xp[off[e]:off[e + 1]].float()).to(bf)
    for got, what in ((M.moe_gemm_wgrad(dy, xp, offsets), "wgrad"), (M.moe_gemm_wgrad(dy, x, offsets, sorted_slot=sorted_slot, top_k=K), "gather")):
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{name}: {what} differs from the exact product"
    grouped = None
    try:
        got = torch._grouped_mm(dy.t(), xp, offs=offsets[1:].contiguous())
        torch.cuda.synchronize()
        grouped = "ok" if got.shape == want.shape else f"shape {tuple(got.shape)}"
    except Exception as exc:  # noqa: BLE001
        grouped = f"{type(exc).__name__}: {str(exc).splitlines()[0][:160]}"
    print("GROUPED " + json.dumps(grouped), flush=True)
    del want, xp, x, dy

    for T in (int(t) for t in args.tokens.split(",")):
        x = torch.empty(T, H, device="cuda").normal_(generator=gd).to(bf)
        sorted_slot, pos, offsets = routed(T)
        rows = sorted_slot.shape[0]
        dy = torch.empty(rows, N, device="cuda", dtype=bf).normal_(generator=gd)
        xp = M.moe_permute_forward(x, sorted_slot, K)
        off = offsets.tolist()
        ends = offsets[1:].contiguous()
        dw = torch.empty(E, N, H, device="cuda", dtype=bf)
        big = E * N * H * 4 > 2 ** 35                                # (an fp32 dw past 32 GiB: that leg and grouped_mm's own output are left out)
        dw32 = None if big else torch.zeros(E, N, H, device="cuda", dtype=torch.float32)
        half = rows // 2
        rest = [half + (rows - half) * i // (E - 1) for i in range(E)]
        skew = torch.tensor([0] + rest, dtype=torch.int32, device="cuda")
        skew_l = skew.tolist()
        legs = {
            "wgrad": lambda: M.moe_gemm_wgrad(dy, xp, offsets, out=dw),
            "loop": lambda: loop(dy, xp, off, dw),
            "gather": lambda: M.moe_gemm_wgrad(dy, x, offsets, sorted_slot=sorted_slot, top_k=K, out=dw),
            "permute+": lambda: M.moe_gemm_wgrad(dy, M.moe_permute_forward(x, sorted_slot, K), offsets, out=dw),
            "skew wgrad": lambda: M.moe_gemm_wgrad(dy, xp, skew, out=dw),
            "skew loop": lambda: loop(dy, xp, skew_l, dw),
        }
        if not big:
            legs["fp32+="] = lambda: M.moe_gemm_wgrad(dy, xp, offsets, dw_dtype=torch.float32, out=dw32, accumulate=True)
        if grouped == "ok" and not big:
            legs["grouped_mm"] = lambda: torch._grouped_mm(dy.t(), xp, offs=ends)
        times = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg, fn in legs.items():
                times[leg].append(_time(fn, args.ms))
        live = sum(1 for e in range(E) if off[e + 1] > off[e])
        res = {"group": name, "T": T, "rows": rows, "live_experts": live, "longest": max(off[e + 1] - off[e] for e in range(E)),
               "grid": list(M.moe_gemm_wgrad_plan(N, H, E)[3:]),
               "legs": {leg: [statistics.median(t), min(t), max(t)] for leg, t in times.items()}}
        print("POINT " + json.dumps(res), flush=True)
        del x, xp, dy, dw, dw32, sorted_slot, pos, offsets
        torch.cuda.empty_cache()


def run_child(name):
    cmd = [sys.executable, os.path.abspath(__file__), "--group", name, "--ms", str(args.ms), "--rounds", str(args.rounds),
           "--tokens", args.tokens]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.group_timeout)
    except subprocess.TimeoutExpired:
        return None, None, f"{name}: no result within {args.group_timeout} s - sweep stopped"
    lines = [json.loads(l[6:]) for l in r.stdout.splitlines() if l.startswith("POINT ")]
    grouped = [json.loads(l[8:]) for l in r.stdout.splitlines() if l.startswith("GROUPED ")]
    if r.returncode != 0 or not lines:
        return None, None, f"{name}: exit status {r.returncode} - sweep stopped\n{r.stdout[-2000:]}"
    return lines, (grouped[0] if grouped else None), None


fmt = lambda t: f"{t[0]:10.1f} [{t[1]:10.1f} .. {t[2]:10.1f}]"                     # noqa: E731


def main():
    if args.group:
        return group(args.group)
    sink = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    say(f"# fa_moe_gemm_wgrad, bf16, 'nk', align 1; groups E x K_top x hidden x N; us per call: median [min .. max] of {args.rounds} rounds "
        f"of >= 3 calls (~{args.ms:.0f} ms), legs alternated; the loop's offsets are read to the host outside the timed region; TFLOP/s "
        f"over the real T K_top rows")
    for name in (args.only.split(",") if args.only else GROUPS):
        pts, grouped, err = run_child(name)
        if pts is None:
            say(err)
            return 1
        E, K, H, N = (int(v) for v in name.split("x"))
        say(f"{name}: witness data bit for bit (wgrad, gather) at T = 128: ok; torch._grouped_mm: "
            f"{'runs' if grouped == 'ok' else 'does not run here (' + str(grouped) + ')'}")
        for p in pts:
            L = p["legs"]
            w = L["wgrad"]
            flop = 2.0 * p["rows"] * H * N
            tf = lambda t: flop / t[0] / 1e6                                       # noqa: E731
            lose = lambda other: "   <- the op LOSES" if other[0] < w[0] else ""   # noqa: E731
            say(f"  T {p['T']:6d} ({p['rows']} rows, {p['live_experts']:3d} live experts, longest segment {p['longest']}, grid {p['grid']})")
            say(f"    wgrad        {fmt(w)} us | {tf(w):7.1f} TFLOP/s")
            say(f"    loop         {fmt(L['loop'])} us | {tf(L['loop']):7.1f} TFLOP/s | loop / wgrad {L['loop'][0] / w[0]:6.2f} x{lose(L['loop'])}")
            if "grouped_mm" in L:
                g = L["grouped_mm"]
                say(f"    grouped_mm   {fmt(g)} us | {tf(g):7.1f} TFLOP/s | grouped_mm / wgrad {g[0] / w[0]:6.2f} x{lose(g)}")
            if "fp32+=" in L:
                a = L["fp32+="]
                say(f"    fp32 +=      {fmt(a)} us | {tf(a):7.1f} TFLOP/s | fp32 += / wgrad {a[0] / w[0]:6.2f} x")
            else:
                say("    fp32 +=      not run: an fp32 dw of more than 32 GiB (grouped_mm's fresh output left out with it)")
            ga, pg = L["gather"], L["permute+"]
            say(f"    gather       {fmt(ga)} us | permute+wgrad {fmt(pg)} us | permute+wgrad / gather {pg[0] / ga[0]:5.2f} x"
                f"{'   <- the gather LOSES' if pg[0] < ga[0] else ''}")
            sw, sl = L["skew wgrad"], L["skew loop"]
            say(f"    skew wgrad   {fmt(sw)} us | {tf(sw):7.1f} TFLOP/s | skew / even {sw[0] / w[0]:5.2f} x | skew loop {fmt(sl)} us | "
                f"loop / wgrad {sl[0] / sw[0]:6.2f} x{'   <- the op LOSES' if sl[0] < sw[0] else ''}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
