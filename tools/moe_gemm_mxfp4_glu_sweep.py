"""fa_moe_gemm_mxfp4_glu (flash_attn_mi355.moe.moe_gemm_mxfp4_glu, the GLU kernels of csrc/fa_moe_gemm_mxfp4.hip) next to what a
user runs without it, at the gate-up layer of gpt-oss: hidden 2880 -> I 2880 (weights of 5760 rows), top-4, E {32, 128} x T {1, 8,
128, 8192}, bf16 x, align 1, softmax routing of random logits, bf16 bias.  Per point, alternated in one process on the same tensors
(xp = moe_permute's output, made outside the timed region; every leg writes preallocated outputs):
    silu / packed             fused     moe_gemm_mxfp4_glu(xp, .., activation="silu", gate_up="packed")
                              unfused   h = moe_gemm_mxfp4(xp, ..);  act_mul_forward(h[:, :I], h[:, I:])
    swiglu_oai / interleaved  fused     moe_gemm_mxfp4_glu(xp, ..)                                     (the defaults)
                              unfused   h = moe_gemm_mxfp4(xp, ..);  the clamped SwiGLU in PyTorch on h[:, 0::2], h[:, 1::2]
    gemm                      moe_gemm_mxfp4(xp, ..) alone: the first launch of both unfused legs (N = 5760 of
                              tools/moe_gemm_mxfp4_sweep.py)
Before anything is timed each E asserts at T = 128 that fused silu / packed equals its unfused leg bit for bit and that fused
swiglu_oai / interleaved is within one bf16 ulp of the PyTorch leg evaluated in fp64 on h.
Reported: us per call, median [min .. max] of `--rounds` rounds of >= 3 evented calls after a warm-up (call time, not kernel
time).  Every E runs in a child process of its own under a time limit; the sweep stops at the first one that fails.

    python tools/moe_gemm_mxfp4_glu_sweep.py [--experts 32,128] [--tokens 1,8,128] [--ms 30] [--rounds 3]
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
ap.add_argument("--group-timeout", type=int, default=240)
ap.add_argument("--tokens", default="1,8,128,8192")
ap.add_argument("--experts", default="32,128")
ap.add_argument("--group", type=int, default=None, help="(child) E - measure it and print one JSON line per T")
args = ap.parse_args()

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "flash-attention-v100_amd")
H, I, TOPK, ALPHA, LIMIT = 2880, 2880, 4, 1.702, 7.0


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


def group(E):
    sys.path.insert(0, PKG)
    import torch
    from flash_attn_mi355 import moe as M
    from flash_attn_mi355.act_mul import act_mul_forward
    bf = torch.bfloat16
    gd = torch.Generator(device="cuda").manual_seed(E)
    blocks = torch.randint(0, 256, (E, 2 * I, H // 2), device="cuda", generator=gd, dtype=torch.uint8)
    scales = torch.randint(118, 123, (E, 2 * I, H // 32), device="cuda", generator=gd, dtype=torch.uint8)
    bias = torch.empty(E, 2 * I, device="cuda").normal_(generator=gd).to(bf)

    def oai(h, out, dtype=torch.float32):
        """the clamped SwiGLU as HF gpt-oss writes it, on the de-interleaved views of h"""
        g, u = h[:, 0::2].to(dtype).clamp(max=LIMIT), h[:, 1::2].to(dtype).clamp(-LIMIT, LIMIT)
        return out.copy_((u + 1) * (g * torch.sigmoid(g * ALPHA)))

    def ordered(t):
        """bf16 -> integers in the order of the values: neighbours differ by 1"""
        b = t.view(torch.int16).int()
        return torch.where(b < 0, -(b & 0x7fff), b)

    for T, check in [(128, True)] + [(int(t), False) for t in args.tokens.split(",")]:    # h has a spread of about 2.5 units
        x = torch.empty(T, H, device="cuda").normal_(generator=gd).to(bf)
        logits = torch.empty(T, E, device="cuda").normal_(generator=gd).to(bf)
        sorted_slot, pos, offsets = M.moe_sort(M.moe_route_forward(logits, TOPK)[1], E)
        xp = M.moe_permute_forward(x, sorted_slot, TOPK)
        h = torch.empty(xp.shape[0], 2 * I, device="cuda", dtype=bf)
        out, ref = torch.empty(xp.shape[0], I, device="cuda", dtype=bf), torch.empty(xp.shape[0], I, device="cuda", dtype=bf)
        gemm = lambda: M.moe_gemm_mxfp4(xp, blocks, scales, offsets, bias=bias, out=h)                                  # noqa: E731
        legs = {"silu fused": lambda: M.moe_gemm_mxfp4_glu(xp, blocks, scales, offsets, activation="silu", gate_up="packed", bias=bias, out=out),
                "silu unfused": lambda: act_mul_forward(gemm()[:, :I], h[:, I:], out=ref),
                "oai fused": lambda: M.moe_gemm_mxfp4_glu(xp, blocks, scales, offsets, bias=bias, out=out),
                "oai unfused": lambda: oai(gemm(), ref),
                "gemm": gemm}
        if check:
            legs["silu fused"](), legs["silu unfused"]()
            assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), f"E {E}: fused silu differs from moe_gemm_mxfp4 + act_mul"
            legs["oai fused"]()
            d = (ordered(oai(gemm(), ref, torch.float64)) - ordered(out)).abs()
            assert int(d.max()) <= 1, f"E {E}: fused swiglu_oai is {int(d.max())} bf16 ulps from fp64"
            continue
        times = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg, fn in legs.items():
                times[leg].append(_time(fn, args.ms))
        off = offsets.tolist()
        res = {"E": E, "T": T, "live_experts": sum(1 for e in range(E) if off[e + 1] > off[e]),
               "block_m": M.moe_gemm_mxfp4_glu_plan(xp.shape[0], I, H, E)[0],
               "legs": {leg: [statistics.median(t), min(t), max(t)] for leg, t in times.items()}}
        print("POINT " + json.dumps(res), flush=True)
        del x, xp, h, out, ref, sorted_slot, pos, offsets
        torch.cuda.empty_cache()


fmt = lambda t: f"{t[0]:8.1f} [{t[1]:8.1f} .. {t[2]:8.1f}]"                         # noqa: E731


def main():
    if args.group:
        return group(args.group)
    print(f"# fa_moe_gemm_mxfp4_glu against moe_gemm_mxfp4 + activation, hidden {H} -> I {I}, top-{TOPK}, bf16 x and bias, plain form; us per "
          f"call: median [min .. max] of {args.rounds} rounds of >= 3 calls (~{args.ms:.0f} ms), legs alternated", flush=True)
    for E in (int(e) for e in args.experts.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--group", str(E), "--ms", str(args.ms), "--rounds", str(args.rounds),
               "--tokens", args.tokens]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.group_timeout)
        except subprocess.TimeoutExpired:
            print(f"E {E}: no result within {args.group_timeout} s - sweep stopped", flush=True)
            return 1
        pts = [json.loads(l[6:]) for l in r.stdout.splitlines() if l.startswith("POINT ")]
        if r.returncode != 0 or not pts:
            print(f"E {E}: exit status {r.returncode} - sweep stopped\n{r.stdout[-2000:]}", flush=True)
            return 1
        print(f"E {E}: at T = 128 fused silu / packed == moe_gemm_mxfp4 + act_mul bit for bit, fused swiglu_oai / interleaved within one "
              f"bf16 ulp of fp64 on h: ok", flush=True)
        for p in pts:
            L = p["legs"]
            print(f"  T {p['T']:5d} (block_m {p['block_m']:3d}, {p['live_experts']:3d} live experts)  gemm alone {fmt(L['gemm'])} us", flush=True)
            for act in ("silu", "oai"):
                f, u = L[act + " fused"], L[act + " unfused"]
                print(f"      {'silu / packed           ' if act == 'silu' else 'swiglu_oai / interleaved'}  fused {fmt(f)} us | unfused {fmt(u)} us | "
                      f"unfused / fused {u[0] / f[0]:5.2f} x{'   <- fused LOSES' if u[0] < f[0] else ''}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
