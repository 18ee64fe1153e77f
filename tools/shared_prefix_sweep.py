"""Shared-prefix decode (flash_attn_mi355/cascade.py) next to the plain kv-cache op over caches that physically hold
prefix + suffix per sequence, and the merge kernel alone against the HBM figure.

Shapes: bf16 q, H 32/8, D 128, T 1 (single-token decode, nothing appended), B 8 / 32 / 128, shared prefix 2 k / 8 k / 32 k tokens,
256 own tokens per sequence, 16-bit and fp8-e4m3 suffix caches (contiguous).  Per point, three legs:
  cascade   flash_attn_with_shared_prefix: prefix pass (fa_fwd over all B rows) + suffix pass + fa_merge_states
  baseline  flash_attn_with_kvcache over [B, S_p + 256, H_k, D] caches - the path this operator leaves untouched
  merge     fa_merge_states alone on the two (out, lse) pairs of the point; bytes = 3 x B x H x (D x 2 + 4) (two parts read,
            one result written, LSEs included) over its time, as a share of the 8 TB/s HBM peak the README quotes decode against
At these shapes the merge moves 0.2 - 3.4 MB: its leg is a launch, not a stream.  One more line therefore times the merge alone on
two [64, 1024, 32, 128] bf16 states (1.6 GB moved): the kernel's streaming rate.
Each leg: a warm-up of >= 60 ms of calls, then `--ms` of calls between two device events; the legs alternate `--rounds` times;
median [min .. max] us per call.  Every point runs in a child process of its own under a time limit (`--point-timeout`
seconds); the sweep stops at the first point that fails or runs out of time - nothing is started on a device that has just
faulted.

    python tools/shared_prefix_sweep.py [--ms 100] [--rounds 5] [--batches 8,32,128] [--prefix 2048,8192,32768]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--ms", type=float, default=100.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", default="8,32,128")
ap.add_argument("--prefix", default="2048,8192,32768")
ap.add_argument("--suffix", type=int, default=256)
ap.add_argument("--kv", default="bf16,fp8")
ap.add_argument("--point-timeout", type=int, default=120)
ap.add_argument("--point", default=None, help="(child) B,S_p,kv - or 'merge' - : measure one point and print one JSON line")
args = ap.parse_args()

HBM_PEAK = 8.0e12                                      # bytes / s, the peak README.md quotes the decode rates against
H, HK, D = 32, 8, 128


def _time(fn, ms, settle_ms=60.0):
    import torch
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
    return s.elapsed_time(e) / n * 1e3


def point(B, S_p, kv):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flash-attention-v100_amd"))
    import torch
    import flash_attn_mi355 as fa
    from flash_attn_mi355 import cascade
    g = torch.Generator(device="cuda").manual_seed(B + S_p)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=torch.bfloat16, generator=g)
    q = rnd(B, 1, H, D)
    pk, pv = rnd(S_p, HK, D), rnd(S_p, HK, D)
    cap = args.suffix + 16
    sk, sv = rnd(B, cap, HK, D), rnd(B, cap, HK, D)
    kw = {}
    if kv == "fp8":
        q8 = lambda t: (t.float() * 0.5).to(torch.float8_e4m3fn)
        kw = dict(k_descale=2.0, v_descale=2.0)
    else:
        q8 = lambda t: t
    sk_c, sv_c = q8(sk), q8(sv)
    # the baseline's caches: every sequence holds the prefix and its own tokens
    fk = torch.cat([q8(pk)[None].expand(B, S_p, HK, D), sk_c], dim=1).contiguous()
    fv = torch.cat([q8(pv)[None].expand(B, S_p, HK, D), sv_c], dim=1).contiguous()
    lens = torch.full((B,), args.suffix, dtype=torch.int32, device="cuda")
    lens_full = lens + S_p
    o_p, lse_p = fa.flash_attn_func(q.view(1, B, H, D), pk[None], pv[None], return_attn_probs=True)[:2]
    o_s, lse_s = fa.flash_attn_with_kvcache(q, sk_c, sv_c, cache_seqlens=lens, causal=True, return_softmax_lse=True, **kw)
    parts_o, parts_l = [o_p.view(B, 1, H, D), o_s], [lse_p[0].view(H, B, 1).permute(1, 0, 2), lse_s]
    legs = {
        "cascade": lambda: cascade.flash_attn_with_shared_prefix(q, pk, pv, sk_c, sv_c, cache_seqlens=lens, **kw),
        "baseline": lambda: fa.flash_attn_with_kvcache(q, fk, fv, cache_seqlens=lens_full, causal=True, **kw),
        "merge": lambda: cascade.merge_attention_states(parts_o, parts_l),
    }
    # same answer first (the baseline's fp8 cache quantises the prefix, the cascade keeps it in 16 bits: reported, not gated)
    a, b = legs["cascade"]().float(), legs["baseline"]().float()
    diff = float((a - b).abs().max() / b.abs().max())
    res = {m: [] for m in legs}
    for _ in range(args.rounds):
        for m, fn in legs.items():
            res[m].append(_time(fn, args.ms))
    out = {"B": B, "S_p": S_p, "kv": kv, "maxrel_vs_baseline": diff,
           "merge_bytes": 3 * B * H * (D * 2 + 4)}
    for m, ts in res.items():
        out[m] = [statistics.median(ts), min(ts), max(ts)]
    print("POINT " + json.dumps(out), flush=True)


def merge_point():
    """the merge alone at a size that streams: two [64, 1024, 32, 128] bf16 states -> one"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flash-attention-v100_amd"))
    import torch
    from flash_attn_mi355 import cascade
    B, S = 64, 1024
    g = torch.Generator(device="cuda").manual_seed(1)
    outs = [torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2)]
    lses = [torch.randn(B, H, S, device="cuda", generator=g) * 3 for _ in range(2)]
    ts = [_time(lambda: cascade.merge_attention_states(outs, lses), args.ms) for _ in range(args.rounds)]
    print("POINT " + json.dumps({"merge": [statistics.median(ts), min(ts), max(ts)], "merge_bytes": 3 * B * S * H * (D * 2 + 4)}), flush=True)


def run_child(point_arg):
    """one point in a process of its own under the time limit -> its dict, or None (the caller stops the sweep)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--point", point_arg, "--ms", str(args.ms), "--rounds", str(args.rounds),
           "--suffix", str(args.suffix)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.point_timeout)
    except subprocess.TimeoutExpired:
        print(f"{point_arg}: no result within {args.point_timeout} s - sweep stopped", flush=True)
        return None
    line = [l for l in r.stdout.splitlines() if l.startswith("POINT ")]
    if r.returncode != 0 or not line:
        print(f"{point_arg}: exit status {r.returncode} - sweep stopped\n{r.stdout[-2000:]}", flush=True)
        return None
    return json.loads(line[0][6:])


def main():
    if args.point == "merge":
        return merge_point()
    if args.point:
        b, s, kv = args.point.split(",")
        return point(int(b), int(s), kv)
    print(f"# shared-prefix decode: bf16 q, H {H}/{HK}, D {D}, T 1, suffix {args.suffix} tokens; us per call: median [min .. max] of "
          f"{args.rounds} rounds x {args.ms:.0f} ms; merge: bytes moved / time, share of {HBM_PEAK / 1e12:.0f} TB/s", flush=True)
    for B in map(int, args.batches.split(",")):
        for S_p in map(int, args.prefix.split(",")):
            for kv in args.kv.split(","):
                p = run_child(f"{B},{S_p},{kv}")
                if p is None:
                    return 1
                fmt = lambda t: f"{t[0]:8.1f} [{t[1]:8.1f} .. {t[2]:8.1f}]"
                rate = p["merge_bytes"] / (p["merge"][0] * 1e-6)
                print(f"B {B:3d} S_p {S_p:5d} {kv:4s} | cascade {fmt(p['cascade'])} | baseline {fmt(p['baseline'])} | "
                      f"baseline / cascade {p['baseline'][0] / p['cascade'][0]:5.2f} x | merge {fmt(p['merge'])} "
                      f"{rate / 1e9:7.1f} GB/s ({100 * rate / HBM_PEAK:4.1f} %) | max-rel vs baseline {p['maxrel_vs_baseline']:.1e}", flush=True)
    p = run_child("merge")
    if p is None:
        return 1
    rate = p["merge_bytes"] / (p["merge"][0] * 1e-6)
    print(f"merge alone, 2 x [64, 1024, {H}, {D}] bf16 -> 1 ({p['merge_bytes'] / 1e9:.2f} GB moved): {p['merge'][0]:8.1f} "
          f"[{p['merge'][1]:8.1f} .. {p['merge'][2]:8.1f}] us, {rate / 1e12:5.2f} TB/s ({100 * rate / HBM_PEAK:4.1f} % of "
          f"{HBM_PEAK / 1e12:.0f} TB/s)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
