"""KV-cache gather (flash_attn_mi355.kv_gather.gather_kv_cache on csrc/fa_kv_gather.hip) next to the torch eager composition a user
writes without it, and against the HBM figure.

Shapes (bf16 output, page 16, Hk 8, D 128): 8192 rows (8 ragged runs), a decode-sized 128 rows (128 runs of one token: the floor
of a call - launch plus the Python layer) and 65536 rows (8 x 8192), which moves 0.4 - 0.5 GB: more than the 256 MiB last-level
cache holds and far above the floor, so its rate is the kernel's streaming rate.  Every run starts at a random position of its
sequence (seq_offsets).  Per shape, the cases cache {bf16, fp8-e4m3} x addressing {seq: cu_seqlens + seq_offsets + block_table,
slot: slot_mapping}, each with two legs:
  ours   gather_kv_cache into a preallocated pair (out=), one launch
  eager  seq: per sequence, index the cache through its block-table row, reshape to [pages x page, Hk, D], slice the run, then
         one `cat` over the sequences (K, then V); slot: `index_select` on the flattened cache with the int64 slots (K, then V);
         for an fp8 cache followed by `.float() * descale` and `.to(bfloat16)` of K and of V
Every case first checks that both legs leave the same bits.
Bytes: the cache rows read once, k and v written once, plus the tables the kernel reads (slot: 8 bytes per row; seq: cu_seqlens,
seq_offsets and one block-table entry per page touched).  Rate = bytes / median time, as a share of the 8 TB/s HBM peak the README
quotes, next to fa_kv_store's 6.48 TB/s (bf16) / 5.20 TB/s (fp8) at 65536 rows (profiles/kv_store.txt).  The 8192-row problem
moves 50 - 70 MB, which the last-level cache can hold between calls: its rate says how close to the floor a chunk is, not what
the kernel streams at.
Each leg: a warm-up of >= 60 ms of calls (past the clock ramp), then `--ms` of calls between two device events; the legs
alternate `--rounds` times; median [min .. max] us per call.  Every shape runs in a child process of its own under a time limit
(`--point-timeout` seconds); the sweep stops at the first one that fails or runs out of time - nothing is started on a device
that has just faulted.  FA_MI355_LIB selects an experiment build of the library (the variant with ordinary cache loads:
`build.py --variant <out.so> FA_KV_GATHER_NT_LOADS=0`); the header line names it.

    python tools/kv_gather_sweep.py [--ms 100] [--rounds 5]
"""
import argparse
import itertools
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
STORE_TBS = {"bf16": 6.48, "fp8": 5.20}                # fa_kv_store at 65536 rows, sequence mode, profiles/kv_store.txt
PAGE, HK, D = 16, 8, 128
SHAPES = {"rows_8192": [700, 1500, 3, 2048, 1024, 917, 1000, 1000], "rows_128": [1] * 128,            # rows read per sequence
          "rows_65536": [8192] * 8}
CASES = list(itertools.product(("bf16", "fp8"), ("seq", "slot")))


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
    from flash_attn_mi355.kv_gather import gather_kv_cache
    lens = SHAPES[name]
    B, T = len(lens), sum(lens)
    assert T in (8192, 128, 65536)
    g = torch.Generator().manual_seed(T)
    L = torch.randint(0, 2048, (B,), generator=g).tolist()                     # first position read per sequence
    pages = [(l + n + PAGE - 1) // PAGE for l, n in zip(L, lens)]
    nblk = sum(pages) + 8
    perm = iter(torch.randperm(nblk, generator=g).tolist())
    bt = torch.zeros((B, max(pages)), dtype=torch.int32)
    slots, touched = [], 0
    for b in range(B):
        for j in range(pages[b]):
            bt[b, j] = next(perm)
        for i in range(lens[b]):
            p = L[b] + i
            slots.append(int(bt[b, p // PAGE]) * PAGE + p % PAGE)
        touched += (L[b] + lens[b] - 1) // PAGE - L[b] // PAGE + 1
    cu = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32).cuda()
    Ld, btd = torch.tensor(L, dtype=torch.int32).cuda(), bt.cuda()
    rows_bt = [btd[b, :pages[b]].long() for b in range(B)]                     # (made once: the eager leg's own index tensors)
    slot_d = torch.tensor(slots, dtype=torch.int64).cuda()
    gd = torch.Generator(device="cuda").manual_seed(T)
    kd, vd = 0.0625, 0.03125
    out = {"shape": name, "cases": []}
    for cache, mode in CASES:
        fp8 = cache == "fp8"
        kc = torch.randn(nblk, PAGE, HK, D, device="cuda", dtype=torch.bfloat16, generator=gd)
        vc = torch.randn(nblk, PAGE, HK, D, device="cuda", dtype=torch.bfloat16, generator=gd)
        if fp8:
            kc, vc = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
        kw = dict(dtype=torch.bfloat16, k_descale=kd, v_descale=vd) if fp8 else {}
        k = torch.empty(T, HK, D, device="cuda", dtype=torch.bfloat16)
        v = torch.empty_like(k)
        res = {}

        def ours():
            if mode == "seq":
                gather_kv_cache(kc, vc, cu_seqlens=cu, seq_offsets=Ld, block_table=btd, out=(k, v), **kw)
            else:
                gather_kv_cache(kc, vc, slot_mapping=slot_d, out=(k, v), **kw)

        def eager_one(c, d):
            if mode == "seq":
                x = torch.cat([c[rows_bt[b]].reshape(-1, HK, D)[L[b]:L[b] + lens[b]] for b in range(B)])
            else:
                x = c.view(-1, HK, D).index_select(0, slot_d)
            return (x.float() * d).to(torch.bfloat16) if fp8 else x

        def eager():
            res["k"], res["v"] = eager_one(kc, kd), eager_one(vc, vd)

        ours(); eager()
        torch.cuda.synchronize()
        same = bool(torch.equal(k.view(torch.int16), res["k"].view(torch.int16)) and torch.equal(v.view(torch.int16), res["v"].view(torch.int16)))
        t_ours, t_eager = [], []
        for _ in range(args.rounds):
            t_ours.append(_time(ours, args.ms))
            t_eager.append(_time(eager, args.ms))
        nbytes = 2 * T * HK * D * (1 if fp8 else 2) + 2 * T * HK * D * 2
        nbytes += T * 8 if mode == "slot" else (2 * B + 1 + touched) * 4
        out["cases"].append({"cache": cache, "mode": mode, "same_bits_as_eager": same, "bytes": nbytes,
                             "ours": [statistics.median(t_ours), min(t_ours), max(t_ours)],
                             "eager": [statistics.median(t_eager), min(t_eager), max(t_eager)]})
        if not same:
            break
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
    lib = os.environ.get("FA_MI355_LIB")
    print(f"# KV-cache gather, bf16 k / v out, page {PAGE}, Hk {HK}, D {D}; library: {os.path.basename(lib) if lib else 'the product build'}; "
          f"us per call: median [min .. max] of {args.rounds} rounds x {args.ms:.0f} ms; rate: algorithmic bytes / median, share of "
          f"{HBM_PEAK / 1e12:.0f} TB/s (fa_kv_store at 65536 rows: {STORE_TBS['bf16']} TB/s into bf16, {STORE_TBS['fp8']} TB/s into fp8)",
          flush=True)
    for name, lens in SHAPES.items():
        p = run_child(name)
        if p is None:
            return 1
        print(f"{name}: {sum(lens)} rows in {len(lens)} sequences", flush=True)
        fmt = lambda t: f"{t[0]:7.1f} [{t[1]:7.1f} .. {t[2]:7.1f}]"
        for c in p["cases"]:
            rate = c["bytes"] / (c["ours"][0] * 1e-6)
            label = f"{c['cache']:4s} {c['mode']:4s}"
            print(f"  {label:9s} | fa_kv_gather {fmt(c['ours'])} us | eager {fmt(c['eager'])} us | eager / fa_kv_gather "
                  f"{c['eager'][0] / c['ours'][0]:5.2f} x | {c['bytes'] / 1e6:6.2f} MB, {rate / 1e12:5.2f} TB/s "
                  f"({100 * rate / HBM_PEAK:4.1f} % of peak, {rate / 1e12 / STORE_TBS[c['cache']]:4.2f} x fa_kv_store's rate) | "
                  f"same bits as eager: {c['same_bits_as_eager']}", flush=True)
            if not c["same_bits_as_eager"]:
                print("the two legs differ - sweep stopped", flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
