"""QK-norm in front of the fused serving prologue (flash_attn_mi355.qk_norm.qk_norm_rope_and_store_kv on
csrc/fa_qk_norm_rope_store.hip: a per-head RMSNorm of q and k, the rotation at per-token positions, K / V stored by slot, one
launch) next to what a user runs without it: a torch eager RMSNorm on the q heads and on the k heads, then rope_and_store_kv.

Shapes (bf16, Hq 32, Hk 8, D 128, page 16, NeoX rotation of the whole head, bf16 weights 1 + 0.2 randn, eps 1e-6):
128 rows (128 sequences of one token: a decode step, the floor of a call - launch plus the Python layer), 8192 rows (8 ragged
sequences: a prefill chunk) and 65536 rows (8 x 8192), which moves 1.1 - 1.3 GB: more than the 256 MiB last-level cache holds, so
its rate is the kernel's streaming rate.  q, k and v are the head slices of one packed [T, Hq + 2 Hk, D] buffer and are changed IN
PLACE.  Per shape, into a bf16 and into an fp8-e4m3 cache:
  fused      qk_norm_rope_and_store_kv(q, k, v, positions, cos, sin, k_cache, v_cache, slot_mapping, q_weight=, k_weight=): one launch
  baseline   the HF module's RMSNorm in torch eager on q and on k, written back in place - x.float(), pow(2).mean(-1), rsqrt,
             the product, the cast to bf16, times the weight - then rope_and_store_kv on the same views
  rope only  rope_and_store_kv alone on the same views: what the prologue costs without the norm, so fused - rope only is the
             cost of the norm
Before anything is timed, every case runs `fused` and the library's own composition qk_rms_norm (out of place) +
rope_and_store_kv once on clones of the same inputs and asserts that q, k and both caches hold the same bits.
Bytes: q and k read and written once, v read once, the cache rows written once, positions and slot_mapping (16 bytes per row), one
cos and one sin row per row, the two weights once.  Rate = bytes / median time, for `fused` and for `baseline` (the baseline moves
more than that; the figure says what it achieves on the same problem), as a share of the 8 TB/s HBM peak the README quotes.
Each leg: a warm-up of >= 60 ms of calls (past the clock ramp), then `--ms` of calls between two device events; the legs
alternate `--rounds` times; median [min .. max] us per call.  Every shape runs in a child process of its own under a time limit
(`--point-timeout` seconds); the sweep stops at the first one that fails or runs out of time - nothing is started on a device
that has just faulted.  Kernel time apart from the call is not measured (no profiler run).

    python tools/qk_norm_sweep.py [--ms 100] [--rounds 5]
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
ap.add_argument("--point-timeout", type=int, default=240)
ap.add_argument("--point", default=None, help="(child) shape name: measure it and print one JSON line")
args = ap.parse_args()

HBM_PEAK = 8.0e12                                      # bytes / s, the peak README.md quotes rates against
PAGE, HQ, HK, D, EPS = 16, 32, 8, 128, 1e-6
SHAPES = {"decode_128": [1] * 128, "prefill_8192": [700, 1500, 3, 2048, 1024, 917, 1000, 1000],       # new tokens per sequence
          "prefill_65536": [8192] * 8}


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


def point(name):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flash-attention-v100_amd"))
    import torch
    from flash_attn_mi355.qk_norm import qk_norm_rope_and_store_kv, qk_rms_norm
    from flash_attn_mi355.rope_store import rope_and_store_kv
    lens = SHAPES[name]
    B, T = len(lens), sum(lens)
    g = torch.Generator().manual_seed(T)
    L = torch.randint(0, 2048, (B,), generator=g).tolist()                     # tokens already cached per sequence
    pages = [(l + n + PAGE - 1) // PAGE for l, n in zip(L, lens)]
    nblk = sum(pages) + 8
    perm = iter(torch.randperm(nblk, generator=g).tolist())
    slots, pos = [], []
    for b in range(B):
        table = [next(perm) for _ in range(pages[b])]
        for i in range(lens[b]):
            p = L[b] + i
            pos.append(p)
            slots.append(table[p // PAGE] * PAGE + p % PAGE)
    slot_d, pos_d = torch.tensor(slots, dtype=torch.int64).cuda(), torch.tensor(pos, dtype=torch.int64).cuda()
    gd = torch.Generator(device="cuda").manual_seed(T)
    qkv0 = torch.randn(T, HQ + 2 * HK, D, device="cuda", dtype=torch.bfloat16, generator=gd)
    w = (1.0 + 0.2 * torch.randn(2, D, generator=g)).bfloat16().cuda()
    qw, kw_ = w[0].contiguous(), w[1].contiguous()
    seqlen_ro = max(l + n for l, n in zip(L, lens))
    ang = torch.arange(seqlen_ro, dtype=torch.float32)[:, None] / (10000 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))[None, :]
    cos, sin = torch.cos(ang).bfloat16().cuda(), torch.sin(ang).bfloat16().cuda()
    kd, vd = 0.0625, 0.03125
    out = {"shape": name, "cases": []}
    for cache in ("bf16", "fp8"):
        fp8 = cache == "fp8"
        cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16
        kw = dict(k_descale=kd, v_descale=vd) if fp8 else {}

        def make(leg):
            qkv = qkv0.clone()
            q, k, v = qkv[:, :HQ], qkv[:, HQ:HQ + HK], qkv[:, HQ + HK:]
            kc = torch.zeros((nblk, PAGE, HK, D), dtype=torch.bfloat16, device="cuda").to(cdt)
            vc = torch.zeros_like(kc)

            def fused():
                qk_norm_rope_and_store_kv(q, k, v, pos_d, cos, sin, kc, vc, slot_d, q_weight=qw, k_weight=kw_, eps=EPS, **kw)

            def hf_norm(x, weight):
                h = x.float()
                h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS)
                x.copy_(weight * h.to(x.dtype))

            def baseline():
                hf_norm(q, qw)
                hf_norm(k, kw_)
                rope_and_store_kv(q, k, v, pos_d, cos, sin, kc, vc, slot_d, **kw)

            def rope_only():
                rope_and_store_kv(q, k, v, pos_d, cos, sin, kc, vc, slot_d, **kw)

            def composed():                                                    # (the bit check's arbiter, not timed)
                qn, kn = qk_rms_norm(q, k, qw, kw_, EPS)
                qo, ko = rope_and_store_kv(qn, kn, v, pos_d, cos, sin, kc, vc, slot_d, inplace=False, **kw)
                q.copy_(qo); k.copy_(ko)

            return {"fused": fused, "baseline": baseline, "rope-only": rope_only, "composed": composed}[leg], (qkv, kc, vc)

        (f_a, st_a), (f_b, st_b) = make("fused"), make("composed")
        f_a(); f_b()
        torch.cuda.synchronize()
        same = all(bool(torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.uint8),
                                    b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.uint8))) for a, b in zip(st_a, st_b))
        assert same, f"{name} {cache}: the fused call and qk_rms_norm + rope_and_store_kv leave different bits"
        assert not torch.equal(st_a[0], qkv0) and bool((st_a[1].float() != 0).any())           # (both did change q / k and store)
        del st_b, f_b
        legs = {leg: make(leg)[0] for leg in ("fused", "baseline", "rope-only")}
        times = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg, fn in legs.items():
                times[leg].append(_time(fn, args.ms))
        nbytes = (2 * T * (HQ + HK) * D * 2 + T * HK * D * 2 + 2 * T * HK * D * (1 if fp8 else 2) + T * 16 + 2 * T * (D // 2) * 2
                  + 2 * D * 2)
        out["cases"].append({"cache": cache, "same_bits_as_composition": same, "bytes": nbytes,
                             **{leg: [statistics.median(t), min(t), max(t)] for leg, t in times.items()}})
    print("POINT " + json.dumps(out), flush=True)


def run_child(name):
    """one shape in a process of its own under the time limit -> its dict, or None (the caller stops the sweep)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--point", name, "--ms", str(args.ms), "--rounds", str(args.rounds)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.point_timeout)
    except subprocess.TimeoutExpired:
        print(f"{name}: no result within {args.point_timeout} s - sweep stopped", flush=True)
        return None
    line = [l for l in r.stdout.splitlines() if l.startswith("POINT ")]
    if r.returncode != 0 or not line:
        print(f"{name}: exit status {r.returncode} - sweep stopped\n{r.stdout[-2000:]}", flush=True)
        return None
    return json.loads(line[0][6:])


def main():
    if args.point:
        return point(args.point)
    print(f"# QK RMSNorm + RoPE + KV-cache store, bf16 packed qkv in place, Hq {HQ}, Hk {HK}, D {D}, page {PAGE}, NeoX rotary_dim {D}, "
          f"bf16 weights; us per call: median [min .. max] of {args.rounds} rounds x {args.ms:.0f} ms; rate: algorithmic bytes / median, "
          f"share of {HBM_PEAK / 1e12:.0f} TB/s; baseline: torch eager RMSNorm on q and on k (fp32 inside, HF form) + rope_and_store_kv; "
          f"rope only: rope_and_store_kv alone (no norm); kernel time apart from the call: not measured", flush=True)
    for name, lens in SHAPES.items():
        p = run_child(name)
        if p is None:
            return 1
        print(f"{name}: {sum(lens)} rows in {len(lens)} sequences", flush=True)
        fmt = lambda t: f"{t[0]:7.1f} [{t[1]:7.1f} .. {t[2]:7.1f}]"
        for c in p["cases"]:
            rf, rb = c["bytes"] / (c["fused"][0] * 1e-6), c["bytes"] / (c["baseline"][0] * 1e-6)
            print(f"  {c['cache']:4s} cache | fused {fmt(c['fused'])} us | baseline {fmt(c['baseline'])} us | rope only {fmt(c['rope-only'])} us | "
                  f"baseline / fused {c['baseline'][0] / c['fused'][0]:5.2f} x | fused - rope only {c['fused'][0] - c['rope-only'][0]:+7.1f} us | "
                  f"{c['bytes'] / 1e6:7.2f} MB: fused {rf / 1e12:5.2f} TB/s ({100 * rf / HBM_PEAK:4.1f} % of peak), "
                  f"baseline {rb / 1e12:5.2f} TB/s ({100 * rb / HBM_PEAK:4.1f} %) | "
                  f"same bits as qk_rms_norm + rope_and_store_kv: {c['same_bits_as_composition']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
