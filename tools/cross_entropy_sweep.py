"""Softmax cross-entropy over the vocabulary (flash_attn.losses.cross_entropy.CrossEntropyLoss on csrc/fa_cross_entropy.hip) next to
what a user runs without it: torch eager `F.cross_entropy(logits.float(), labels)`.

bf16 logits (randn), labels uniform over the vocabulary with every 16th one ignore_index, mean reduction.  Two tables:

  --chunks   the forward alone for CHUNK16 (columns per forward workgroup, csrc/fa_cross_entropy.hip) of 2048 .. 32768 at rows
             {128, 8192} x V {32000, 128256, 262144}: the product library for its own CHUNK, `tools/variants/libfa_mi355_ce<CHUNK>.so`
             (built beforehand, no GPU needed, by `--build-variants`) for the others, each in a child process that loads it
             through FA_MI355_LIB.  The choice recorded in profiles/cross_entropy.txt comes from this table.
  (default)  rows {128, 8192, 65536} x V {32000, 50257, 128256, 262144} where the eager baseline fits the memory, and V = 50257
             once more as a [:, :50257] view of a buffer padded to 50264 (every row 16-byte aligned) beside the contiguous
             layout (every odd row misaligned).  Per shape three legs, each alternated in the same run with its eager counterpart on
             the same tensors:
               fwd       CrossEntropyLoss()(x, y)                      | F.cross_entropy(x.float(), y)
               fwd+bwd   the same and torch.autograd.grad to x          | the same through the eager composition
               bwd       cross_entropy_backward(dloss, x, y, lse) alone                  | (no eager counterpart: autograd's backward
                                                                                           cannot be called without its forward)
             and once, untimed: torch.cuda.max_memory_allocated above the logits for fwd+bwd with inplace_backward=True, for
             fwd+bwd out of place, and for eager.
Before anything is timed every point asserts lse, losses and dlogits of its first and last 64 rows within the derived bounds of
tests/cross_entropy_ref.py against the fp64 formulas (a row's bits do not depend on the batch).
Bytes: the logits read once forward; read and written once backward; labels, the three outputs and the chunk partials once.
Rate = bytes / median time, against the 8 TB/s HBM peak and the 6.45 TB/s fa_merge_states streams at.
Each leg: a warm-up of >= 60 ms of calls, then `--ms` of calls between two device events; the legs alternate `--rounds` times;
median [min .. max] us per call.  Every point runs in a child process of its own under a time limit (`--point-timeout` seconds);
the sweep stops at the first one that fails or runs out of time - nothing is started on a device that has just faulted.

    python tools/cross_entropy_sweep.py [--chunks] [--ms 100] [--rounds 5]
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
ap.add_argument("--chunks", action="store_true", help="the CHUNK table instead of the shape table")
ap.add_argument("--build-variants", action="store_true", help="build tools/variants/libfa_mi355_ce<CHUNK>.so (no GPU needed) and exit")
ap.add_argument("--eager-limit-gb", type=float, default=150.0, help="skip the eager legs where 8 fp32 copies of the logits exceed it")
ap.add_argument("--point", default=None, help="(child) rows x V[p] [@CHUNK]: measure it and print one JSON line")
args = ap.parse_args()

HBM_PEAK, STREAM = 8.0e12, 6.45e12                     # bytes / s: the peak README.md quotes, and what fa_merge_states streams at
CHUNKS = [2048, 4096, 8192, 16384, 32768]
CHUNK_SHAPES = [(rows, v) for v in (32000, 128256, 262144) for rows in (128, 8192)]
SHAPES = [(rows, v) for v in (32000, 50257, 128256, 262144) for rows in (128, 8192, 65536)]
PAD_TO = 50264
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "flash-attention-v100_amd")
VARIANTS = os.path.join(HERE, "variants")


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
    sys.path.insert(0, PKG)
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    import torch
    import torch.nn.functional as F
    import cross_entropy_ref as R
    from flash_attn.losses.cross_entropy import CrossEntropyLoss
    from flash_attn_mi355 import cross_entropy as C
    shape, _, chunk = name.partition("@")
    padded = shape.endswith("p")
    rows, V = (int(v) for v in shape.rstrip("p").split("x"))
    bf = torch.bfloat16
    if chunk:
        R.CHUNK[bf] = int(chunk)                            # (the library loaded through FA_MI355_LIB was built with it)
    gd = torch.Generator(device="cuda").manual_seed(rows + V)
    if padded:
        x = torch.empty(rows, PAD_TO, device="cuda", dtype=bf).normal_(generator=gd)[:, :V]
    else:
        x = torch.empty(rows, V, device="cuda", dtype=bf).normal_(generator=gd)
    y = torch.randint(0, V, (rows,), device="cuda", generator=gd)
    y[::16] = -100
    plan = R.plan(rows, V, bf)

    # the bounds first, on the first and last 64 rows of the whole batch's results
    losses, _, lse = C.cross_entropy_forward(x, y)
    dl = torch.full((rows,), 1.0 / rows, device="cuda")
    dx = C.cross_entropy_backward(dl, x, y, lse)
    torch.cuda.synchronize()
    sel = torch.cat([torch.arange(min(64, rows)), torch.arange(max(rows - 64, 0), rows)]).unique().cuda()
    ref = R.forward_ref(x[sel], y[sel])
    rdx, mags = R.backward_ref(dl[sel], x[sel], y[sel], lse[sel])
    worst = {"lse": R.worst(lse[sel], ref["lse"], R.lse_bound(ref, plan["steps"])),
             "loss": R.worst(losses[sel], ref["loss"], R.loss_bound(ref, plan["steps"], 0.0, 0.0, V)),
             "dx": R.worst(dx[sel], rdx, R.dx_bound(rdx, mags, bf))}
    assert all(v <= 1.0 for v in worst.values()), f"{name}: outside the derived bounds: {worst}"
    del ref, rdx, mags, dx, losses
    torch.cuda.empty_cache()

    t2 = rows * V * 2
    small = rows * (8 + 3 * 4) + 2 * plan["workspace_bytes"]
    nbytes = {"fwd": t2 + small, "bwd": 2 * t2 + rows * 16, "fwd+bwd": 3 * t2 + small + rows * 16}
    stat = lambda t: [statistics.median(t), min(t), max(t)]                        # noqa: E731
    if chunk:
        t = [_time(lambda: C.cross_entropy_forward(x, y), args.ms) for _ in range(args.rounds)]
        print("POINT " + json.dumps({"shape": name, "worst": worst, "nchunks": plan["nchunks"], "bytes": nbytes,
                                     "legs": {"fwd": {"fused": stat(t)}}}), flush=True)
        return

    with_eager = 8 * rows * V * 4 <= args.eager_limit_gb * 1e9
    mod = CrossEntropyLoss()
    xg = x.detach().requires_grad_(True)
    legs = {
        "fwd": (lambda: mod(x, y), lambda: F.cross_entropy(x.float(), y)),
        "fwd+bwd": (lambda: torch.autograd.grad(mod(xg, y), xg), lambda: torch.autograd.grad(F.cross_entropy(xg.float(), y), xg)),
        "bwd": (lambda: C.cross_entropy_backward(dl, x, y, lse), None),
    }
    times = {leg: ([], []) for leg in legs}
    for _ in range(args.rounds):
        for leg, (fused, base) in legs.items():
            times[leg][0].append(_time(fused, args.ms))
            if base is not None and with_eager:
                times[leg][1].append(_time(base, args.ms))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before
    mem = {"fused": peak(legs["fwd+bwd"][0])}
    if with_eager:
        mem["eager"] = peak(legs["fwd+bwd"][1])
    inpl = CrossEntropyLoss(inplace_backward=True)
    mem["fused-inplace"] = peak(lambda: torch.autograd.grad(inpl(xg, y), xg))     # (last: it overwrites the logits)
    out = {"shape": name, "worst": worst, "nchunks": plan["nchunks"], "bytes": nbytes, "logits_bytes": t2, "mem": mem,
           "legs": {leg: {"fused": stat(t[0]), "eager": stat(t[1]) if t[1] else None} for leg, t in times.items()}}
    print("POINT " + json.dumps(out), flush=True)


def run_child(name, lib=None):
    """one point in a process of its own under the time limit -> its dict, or None (the caller stops the sweep)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--point", name, "--ms", str(args.ms), "--rounds", str(args.rounds),
           "--eager-limit-gb", str(args.eager_limit_gb)]
    env = dict(os.environ)
    if lib:
        env["FA_MI355_LIB"] = lib
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.point_timeout, env=env)
    except subprocess.TimeoutExpired:
        print(f"{name}: no result within {args.point_timeout} s - sweep stopped", flush=True)
        return None
    line = [l for l in r.stdout.splitlines() if l.startswith("POINT ")]
    if r.returncode != 0 or not line:
        print(f"{name}: exit status {r.returncode} - sweep stopped\n{r.stdout[-2000:]}", flush=True)
        return None
    return json.loads(line[0][6:])


def product_chunk():
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    import torch
    import cross_entropy_ref as R
    return R.CHUNK[torch.bfloat16]


def build_variants():
    sys.path.insert(0, PKG)
    import build
    os.makedirs(VARIANTS, exist_ok=True)
    for c in CHUNKS:
        if c != product_chunk():
            print(build.build(defines=[f"FA_CE_CHUNK16={c}", "FA_CE_CHUNK32=2048"], out=os.path.join(VARIANTS, f"libfa_mi355_ce{c}.so")))
    return 0


fmt = lambda t: f"{t[0]:9.1f} [{t[1]:9.1f} .. {t[2]:9.1f}]"                        # noqa: E731


def rate(nbytes, us):
    r = nbytes / (us * 1e-6)
    return f"{nbytes / 1e6:9.2f} MB: {r / 1e12:5.2f} TB/s ({100 * r / HBM_PEAK:4.1f} % of peak, {100 * r / STREAM:4.1f} % of the stream rate)"


def chunk_table():
    print(f"# forward alone, bf16, us per call: median [min .. max] of {args.rounds} rounds x {args.ms:.0f} ms; rate: algorithmic bytes / "
          f"median", flush=True)
    prod = product_chunk()
    for rows, v in CHUNK_SHAPES:
        for c in CHUNKS:
            lib = None if c == prod else os.path.join(VARIANTS, f"libfa_mi355_ce{c}.so")
            if lib and not os.path.exists(lib):
                print(f"rows {rows} V {v} CHUNK {c}: {lib} is not built (--build-variants) - left out", flush=True)
                continue
            p = run_child(f"{rows}x{v}@{c}", lib)
            if p is None:
                return 1
            t = p["legs"]["fwd"]["fused"]
            print(f"rows {rows:5d} V {v:6d} CHUNK {c:5d}{' *' if c == prod else '  '} {p['nchunks']:3d} chunks  fwd {fmt(t)} us | "
                  f"{rate(p['bytes']['fwd'], t[0])}", flush=True)
    return 0


def main():
    if args.point:
        return point(args.point)
    if args.build_variants:
        return build_variants()
    if args.chunks:
        return chunk_table()
    print(f"# softmax cross-entropy, bf16 logits, mean reduction; us per call: median [min .. max] of {args.rounds} rounds x "
          f"{args.ms:.0f} ms, fused and eager alternated; rate: algorithmic bytes / median, share of {HBM_PEAK / 1e12:.0f} TB/s peak and of "
          f"{STREAM / 1e12:.2f} TB/s (fa_merge_states); eager: F.cross_entropy(logits.float(), labels); 'p': a [:, :V] view of rows "
          f"padded to {PAD_TO}", flush=True)
    names = []
    for rows, v in SHAPES:
        names.append(f"{rows}x{v}")
        if v == 50257:
            names.append(f"{rows}x{v}p")
    for name in names:
        p = run_child(name)
        if p is None:
            return 1
        print(f"{name}: {p['nchunks']} chunks; worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in p["worst"].items()), flush=True)
        for leg, t in p["legs"].items():
            eager = f"eager {fmt(t['eager'])} us | eager / fused {t['eager'][0] / t['fused'][0]:6.2f} x" if t["eager"] else "eager not run"
            print(f"  {leg:8s} fused {fmt(t['fused'])} us | {eager} | {rate(p['bytes'][leg], t['fused'][0])}", flush=True)
        lb = p["logits_bytes"]
        print("  peak memory above the logits, fwd+bwd: " + ", ".join(f"{k} {v / 1e6:.1f} MB ({v / lb:.2f} x the logits)"
                                                                       for k, v in p["mem"].items()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
