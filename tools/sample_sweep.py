"""Token sampling (flash_attn_mi355.sample.sample on csrc/fa_sample.hip) next to what a caller runs without it: the eager torch
composition - sort, softmax, cumsum, mask, then the draw (the same inverse CDF from the same uniform numbers, so both sides do the
same job; without a filter the eager side needs no sort).

Grid: rows {1, 8, 64, 256, 1024} x V {32000, 128256, 151936, 262144} in bf16 and fp32 (randn x 3), temperature 0.8, four filter
settings: none, top-k 50, top-p 0.9, all three (top-k 50, min-p 0.01, top-p 0.9).  Per cell the two legs alternate `--rounds`
times in one process; each leg is a warm-up of >= `--settle` ms of calls, then `--ms` of calls between two device events; median
us per call.  Columns: the fused time, the eager time, eager / fused, the logits bytes the fused op reads per row - its sweeps
(csrc/fa_sample.hip: 1 for the statistics, 1 for the masses with min-p or with top-p alone, key bits / 8 per radix select, 1 + 1/16
for the draw) x V x the element size - and the share of the 8 TB/s HBM peak that rows x those bytes / time comes to (an IMPLIED
figure: sweeps after the first are served by the caches where the row fits them; from V 32768 on a row is cut over several
workgroups and every sweep is a launch of its own - the same sweeps).  A second table prices the LDS-add contention
of the select's histogram: top-k 50 at 64 x 151936 bf16 over rows whose keys fall into many bins, few bins and one bin.
`same ids` is the share of rows on which both sides drew the same token: 1 without a filter (up to fp32 sums in another order);
with a filter it means nothing - the eager side inverts the CDF in sorted order, the op in index order (the same distribution,
another map from u to the token).  Every cell with eager / fused <= 1 is listed at the end.  Each (V, dtype) group runs in a child process of its own under a time
limit; the sweep stops at the first one that fails - nothing is started on a device that has just faulted.

    python tools/sample_sweep.py [--ms 40] [--rounds 3] [--out profiles/sample.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--ms", type=float, default=40.0)
ap.add_argument("--settle", type=float, default=20.0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--group-timeout", type=int, default=150)
ap.add_argument("--out", default=None, help="also write the tables to this file")
ap.add_argument("--group", default=None, help="(child) V:dtype or 'contention': measure it and print JSON lines")
args = ap.parse_args()

HBM_PEAK = 8.0e12
ROWS = [1, 8, 64, 256, 1024]
VOCABS = [32000, 128256, 151936, 262144]
DTYPES = ["bf16", "fp32"]
SETTINGS = [("none", dict()), ("top-k 50", dict(top_k=50)), ("top-p 0.9", dict(top_p=0.9)),
            ("all three", dict(top_k=50, min_p=0.01, top_p=0.9))]
TEMP = 0.8
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "flash-attention-v100_amd")


def sweeps(dtype, kw):
    """how often the fused op reads a row's logits"""
    sel = 2 if dtype == "bf16" else 4
    k, p, mp = "top_k" in kw, "top_p" in kw, "min_p" in kw
    return 1 + (1 if (mp or (p and not k)) else 0) + sel * (int(k) + int(p)) + 1 + 1.0 / 16


def _time(fn, ms, settle_ms):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); fn(); e.record(); e.synchronize()
    one = max(s.elapsed_time(e), 1e-3)
    for _ in range(int(settle_ms / one) + 2):
        fn()
    n = max(5, int(ms / one))
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / n * 1e3


def _eager(x, u, top_k=0, top_p=1.0, min_p=0.0):
    import torch
    z = x.float() / TEMP
    if not top_k and top_p >= 1.0 and not min_p:
        cdf = torch.softmax(z, -1).cumsum(-1)
        return torch.searchsorted(cdf, u[:, None] * cdf[:, -1:]).clamp_(max=x.shape[-1] - 1).squeeze(-1)
    s, idx = torch.sort(z, -1, descending=True)
    if top_k:
        s[:, top_k:] = float("-inf")
    pr = torch.softmax(s, -1)
    if min_p:
        pr = pr.masked_fill(pr < min_p * pr[:, :1], 0.0)
        pr = pr / pr.sum(-1, keepdim=True)
    if top_p < 1.0:
        cum = pr.cumsum(-1)
        pr = pr.masked_fill(cum - pr > top_p, 0.0)
    cdf = pr.cumsum(-1)
    j = torch.searchsorted(cdf, u[:, None] * cdf[:, -1:]).clamp_(max=x.shape[-1] - 1)
    return idx.gather(1, j).squeeze(-1)


def _cell(S, x, u, kw, dtype, name):
    import torch
    fused = lambda: S.sample_forward(x, u, temperature=TEMP, **kw)      # noqa: E731
    eager = lambda: _eager(x, u, **kw)                                    # noqa: E731
    a, b = fused()[0], eager()
    torch.cuda.synchronize()
    agree = float((a.long() == b).float().mean())                        # (meaningful without a filter only: the docstring)
    tf, te = [], []
    for _ in range(args.rounds):
        tf.append(_time(fused, args.ms, args.settle))
        te.append(_time(eager, args.ms, args.settle))
    return dict(name=name, fused=statistics.median(tf), eager=statistics.median(te), agree=agree)


def group(spec):
    sys.path.insert(0, PKG)
    import torch
    import flash_attn_mi355.sample as S
    if spec == "contention":
        rows, V = 64, 151936
        g = torch.Generator(device="cuda").manual_seed(1)
        kinds = {
            "randn x 3 (a dozen exponent bins, runs of 1 - 3)": torch.randn(rows, V, device="cuda", generator=g) * 3,
            "randn x 2^[-8, 8] (some 40 bins)": torch.randn(rows, V, device="cuda", generator=g)
            * torch.exp2(torch.randint(-8, 9, (rows, V), device="cuda", generator=g).float()),
            "uniform [1, 2) (ONE bin in the first sweep)": 1 + torch.rand(rows, V, device="cuda", generator=g),
            "+-[1, 2) alternating (two bins, every run of length 1)": (1 + torch.rand(rows, V, device="cuda", generator=g))
            * (1 - 2 * (torch.arange(V, device="cuda") % 2)).float(),
        }
        u = torch.rand(rows, device="cuda", generator=g)
        for name, x in kinds.items():
            x = x.bfloat16()
            t = [_time(lambda: S.sample_forward(x, u, temperature=TEMP, top_k=50), args.ms, args.settle) for _ in range(args.rounds)]
            t0 = [_time(lambda: S.sample_forward(x, u, temperature=TEMP), args.ms, args.settle) for _ in range(args.rounds)]
            print(json.dumps(dict(name=name, topk=statistics.median(t), none=statistics.median(t0))), flush=True)
        return
    V, dtype = spec.split(":")
    V = int(V)
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator(device="cuda").manual_seed(V)
    for rows in ROWS:
        x = (torch.randn(rows, V, device="cuda", generator=g) * 3).to(tdt)
        u = torch.rand(rows, device="cuda", generator=g)
        for name, kw in SETTINGS:
            r = _cell(S, x, u, kw, dtype, name)
            r.update(rows=rows, V=V, dtype=dtype, bytes_per_row=sweeps(dtype, kw) * V * x.element_size())
            print(json.dumps(r), flush=True)
        del x


def main():
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def run(spec):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--group", spec, "--ms", str(args.ms), "--settle",
                                str(args.settle), "--rounds", str(args.rounds)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               text=True, timeout=args.group_timeout)
        except subprocess.TimeoutExpired:
            emit(f"group {spec} did not finish in {args.group_timeout} s (hung); the sweep stops here")
            return None
        if p.returncode != 0:
            emit(f"group {spec} failed ({p.returncode}); the sweep stops here\n{p.stderr[-2000:]}")
            return None
        return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]

    emit(f"fa_sample vs eager torch (sort, softmax, cumsum, mask, draw); temperature {TEMP}; median of {args.rounds} rounds of "
         f"{args.ms:.0f} ms; us per call")
    emit(f"{'dtype':5} {'V':>7} {'rows':>5}  {'setting':10} {'fused us':>10} {'eager us':>10} {'eager/fused':>11} "
         f"{'KiB read/row':>12} {'% of 8 TB/s':>11} {'same ids':>8}")
    slower = []
    ok = True
    for dtype in DTYPES:
        for V in VOCABS:
            res = run(f"{V}:{dtype}")
            if res is None:
                ok = False
                break
            for r in res:
                ratio = r["eager"] / r["fused"]
                share = r["rows"] * r["bytes_per_row"] / (r["fused"] * 1e-6) / HBM_PEAK * 100
                emit(f"{r['dtype']:5} {r['V']:7d} {r['rows']:5d}  {r['name']:10} {r['fused']:10.1f} {r['eager']:10.1f} {ratio:11.2f} "
                     f"{r['bytes_per_row'] / 1024:12.0f} {share:11.2f} {r['agree']:8.3f}")
                if ratio <= 1.0:
                    slower.append(f"{r['dtype']} V {r['V']} rows {r['rows']} {r['name']}: {ratio:.2f}")
        if not ok:
            break
    if ok:
        emit()
        emit("cells where the fused op is not faster than eager: " + ("none" if not slower else ""))
        for s in slower:
            emit("  " + s)
        emit()
        emit("LDS-add contention of the select histogram (8 copies per bin, equal-bin runs merged in the lane): 64 x 151936 bf16, us")
        emit(f"{'logits':58} {'top-k 50':>9} {'no filter':>9} {'the two selects sweeps':>22}")
        res = run("contention")
        ok = res is not None
        for r in res or []:
            emit(f"{r['name']:58} {r['topk']:9.1f} {r['none']:9.1f} {r['topk'] - r['none']:22.1f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    if args.group:
        group(args.group)
    else:
        sys.exit(main())
