"""The gated activation of the MLP (flash_attn_mi355.act_mul on csrc/fa_act_mul.hip) next to what a user runs without it: the torch
eager composition `F.silu(gate) * up` and its autograd backward.

bf16, a packed [rows, 2N] input (gate first), rows {128, 8192, 65536} x N {14336, 11008} - widths whose column tail would show a
loss - with SiLU, and the erf GELU once at 8192 x 14336.  Per point these legs, each alternated in the same run with its eager
counterpart on the same tensors:
    fwd          act_and_mul(x)                                             | F.silu(x[:, :N]) * x[:, N:]
    fwd+bwd      the same and torch.autograd.grad to x                      | the same through the eager composition
    bwd          act_mul_backward(dout, gate, up, out=halves of one dx)     | (no eager counterpart: autograd's backward cannot be
    bwd-inplace  act_mul_backward(dout, gate, up, inplace=True) on a copy   |  called without its forward)
and once, untimed: torch.cuda.max_memory_allocated above the input for fwd+bwd - fused, fused with inplace_backward, eager.
Before anything is timed every point asserts out, dgate and dup of its first and last 64 rows within the derived bounds of
tests/act_mul_ref.py against the fp64 formulas (an element's bits depend on its own operands alone).
Bytes: forward 2 reads + 1 write of rows x N x 2 bytes; backward 3 reads + 2 writes.  Rate = bytes / median time, against the 8 TB/s
HBM peak, the 6.45 TB/s fa_merge_states streams at (profiles/shared_prefix_decode.txt) and the 6.2 TB/s of the add-norm forward.
Each leg: a warm-up of >= 60 ms of calls, then `--ms` of calls between two device events; the legs alternate `--rounds` times;
median [min .. max] us per call - call time: kernel time apart from the call is not measured here.  Every point runs in a child
process of its own under a time limit (`--point-timeout` seconds); the sweep stops at the first one that fails or runs out of time -
nothing is started on a device that has just faulted.
`--loads ordinary` runs the same sweep on `tools/variants/libfa_mi355_act_ld.so` (FA_ACT_NT_LOADS=0: ordinary instead of
nontemporal loads), built beforehand, no GPU needed, by `--build-variants`.

    python tools/act_mul_sweep.py [--loads nt|ordinary] [--only 8192x14336:silu,..] [--ms 100] [--rounds 5]
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
ap.add_argument("--loads", choices=["nt", "ordinary"], default="nt")
ap.add_argument("--build-variants", action="store_true", help="build tools/variants/libfa_mi355_act_ld.so (no GPU needed) and exit")
ap.add_argument("--only", default=None, help="comma-separated points (rows x N : activation) instead of the whole list")
ap.add_argument("--point", default=None, help="(child) rows x N : activation - measure it and print one JSON line")
args = ap.parse_args()

HBM_PEAK, STREAM, ADD_NORM = 8.0e12, 6.45e12, 6.2e12
POINTS = [f"{rows}x{n}:silu" for n in (14336, 11008) for rows in (128, 8192, 65536)] + ["8192x14336:gelu"]
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "flash-attention-v100_amd")
VARIANT = os.path.join(HERE, "variants", "libfa_mi355_act_ld.so")


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
    import act_mul_ref as R
    from flash_attn_mi355 import act_mul as M
    shape, _, act = name.partition(":")
    rows, N = (int(v) for v in shape.split("x"))
    bf = torch.bfloat16
    eager_act = {"silu": F.silu, "gelu": F.gelu}[act]
    gd = torch.Generator(device="cuda").manual_seed(rows + N)
    x = (torch.empty(rows, 2 * N, device="cuda", dtype=torch.float32).normal_(generator=gd) * 2).to(bf)
    dout = torch.empty(rows, N, device="cuda", dtype=torch.float32).normal_(generator=gd).to(bf)
    gate, up = x[:, :N], x[:, N:]

    # the bounds first, on the first and last 64 rows of the whole batch's results
    out = M.act_mul_forward(gate, up, activation=act)
    dx = torch.empty_like(x)
    M.act_mul_backward(dout, gate, up, activation=act, out=(dx[:, :N], dx[:, N:]))
    torch.cuda.synchronize()
    sel = torch.cat([torch.arange(min(64, rows)), torch.arange(max(rows - 64, 0), rows)]).unique().cuda()
    ro, Do = R.forward_ref(gate[sel], up[sel], act)
    rg, rp, Dg, Dp = R.backward_ref(dout[sel], gate[sel], up[sel], act)
    worst = {"out": R.worst(out[sel], ro, R.bound(ro, Do, bf)), "dgate": R.worst(dx[sel, :N], rg, R.bound(rg, Dg, bf)),
             "dup": R.worst(dx[sel, N:], rp, R.bound(rp, Dp, bf))}
    assert all(v <= 1.0 for v in worst.values()), f"{name}: outside the derived bounds: {worst}"
    del ro, Do, rg, rp, Dg, Dp, out
    torch.cuda.empty_cache()

    t2 = rows * N * 2
    nbytes = {"fwd": 3 * t2, "bwd": 5 * t2, "bwd-inplace": 5 * t2, "fwd+bwd": 8 * t2}
    stat = lambda t: [statistics.median(t), min(t), max(t)]                        # noqa: E731
    xg = x.detach().requires_grad_(True)
    xc = x.clone()                                          # (the in-place leg rewrites it call after call: timing only)
    eager = lambda t: eager_act(t[:, :N]) * t[:, N:]        # noqa: E731
    legs = {
        "fwd": (lambda: M.act_and_mul(x, activation=act), lambda: eager(x)),
        "fwd+bwd": (lambda: torch.autograd.grad(M.act_and_mul(xg, activation=act), xg, dout),
                    lambda: torch.autograd.grad(eager(xg), xg, dout)),
        "bwd": (lambda: M.act_mul_backward(dout, gate, up, activation=act, out=(dx[:, :N], dx[:, N:])), None),
        "bwd-inplace": (lambda: M.act_mul_backward(dout, xc[:, :N], xc[:, N:], activation=act, inplace=True), None),
    }
    times = {leg: ([], []) for leg in legs}
    for _ in range(args.rounds):
        for leg, (fused, base) in legs.items():
            times[leg][0].append(_time(fused, args.ms))
            if base is not None:
                times[leg][1].append(_time(base, args.ms))
    del xc, dx

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before
    mem = {"fused": peak(legs["fwd+bwd"][0]), "eager": peak(legs["fwd+bwd"][1])}
    xi = x.clone()                                          # (a non-leaf would be the usual case; the clone stands for it)

    def inplace():
        leaf = xi.requires_grad_(True)
        torch.autograd.grad(M.act_and_mul(leaf * 1, activation=act, inplace_backward=True), leaf, dout)
    mem["fused-inplace (incl. the non-leaf copy of x it overwrites)"] = peak(inplace)
    res = {"point": name, "worst": worst, "plan": R.plan(rows, N), "bytes": nbytes, "input_bytes": 2 * t2, "mem": mem,
           "legs": {leg: {"fused": stat(t[0]), "eager": stat(t[1]) if t[1] else None} for leg, t in times.items()}}
    print("POINT " + json.dumps(res), flush=True)


def run_child(name, lib=None):
    """one point in a process of its own under the time limit -> its dict, or None (the caller stops the sweep)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--point", name, "--ms", str(args.ms), "--rounds", str(args.rounds)]
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


def build_variants():
    sys.path.insert(0, PKG)
    import build
    os.makedirs(os.path.dirname(VARIANT), exist_ok=True)
    print(build.build(defines=["FA_ACT_NT_LOADS=0"], out=VARIANT))
    return 0


fmt = lambda t: f"{t[0]:9.1f} [{t[1]:9.1f} .. {t[2]:9.1f}]"                        # noqa: E731


def rate(nbytes, us):
    r = nbytes / (us * 1e-6)
    return (f"{nbytes / 1e6:9.2f} MB: {r / 1e12:5.2f} TB/s ({100 * r / HBM_PEAK:4.1f} % of peak, {100 * r / STREAM:4.1f} % of the merge "
            f"stream, {100 * r / ADD_NORM:4.1f} % of the add-norm forward)")


def main():
    if args.point:
        return point(args.point)
    if args.build_variants:
        return build_variants()
    lib = None
    if args.loads == "ordinary":
        lib = VARIANT
        if not os.path.exists(lib):
            print(f"{lib} is not built (--build-variants)")
            return 1
    print(f"# act(gate) * up, bf16, packed [rows, 2N] input, {args.loads} loads; us per call: median [min .. max] of {args.rounds} rounds x "
          f"{args.ms:.0f} ms, fused and eager alternated; rate: algorithmic bytes / median, share of {HBM_PEAK / 1e12:.0f} TB/s peak, of "
          f"{STREAM / 1e12:.2f} TB/s (fa_merge_states) and of {ADD_NORM / 1e12:.1f} TB/s (add-norm forward); eager: act(x[:, :N]) * x[:, N:] "
          f"and its autograd", flush=True)
    for name in (args.only.split(",") if args.only else POINTS):
        p = run_child(name, lib)
        if p is None:
            return 1
        pl = p["plan"]
        print(f"{name}: {pl['nchunks']} runs of {pl['run_columns']} columns per row, {pl['items']} items on {pl['grid']} workgroups; "
              f"worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in p["worst"].items()), flush=True)
        for leg, t in p["legs"].items():
            eager = f"eager {fmt(t['eager'])} us | eager / fused {t['eager'][0] / t['fused'][0]:6.2f} x" if t["eager"] else "eager not run"
            print(f"  {leg:11s} fused {fmt(t['fused'])} us | {eager} | {rate(p['bytes'][leg], t['fused'][0])}", flush=True)
        ib = p["input_bytes"]
        print("  peak memory above the input, fwd+bwd: " + ", ".join(f"{k} {v / 1e6:.1f} MB ({v / ib:.2f} x the input)"
                                                                      for k, v in p["mem"].items()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
