"""Residual add + RMSNorm over the hidden size (flash_attn_mi355.add_norm on csrc/fa_add_norm.hip / fa_add_norm_bwd.hip) next to what
a user runs without it: the torch eager composition of the HF modules.

bf16, bf16 weights 1 + 0.2 randn, eps 1e-6, contiguous tensors; rows 128 (a call floor), 8192 and 65536; N 4096 and 8192.  Per shape
four legs, each alternated in the same run with its eager counterpart on the same tensors:
  fwd        add_norm(x, w, residual=r, prenorm=True): out and residual_out, out of place
  fwd-inpl   fused_add_rms_norm_(x, r, w): vLLM's form, x and r rewritten where they are
  bwd        add_norm_backward(dy, z, w): dx (which is dres as well) and dweight - two launches, the partial slab
  bwd-nodw   the same with need_dw=False: one launch, no workspace
  eager fwd  z = x + r; h = z.float(); y = w * (h * rsqrt(h.pow(2).mean(-1) + eps)).to(bf16)   (fwd-inpl: the same, then x.copy_(y),
             r.copy_(z) - what in place costs a user without the op)
  eager bwd  torch.autograd.grad through that composition, graph built once, for (x, r, w) and for (x, r) alone
Before anything is timed every case asserts the forward (and, for the backward legs, dx and dweight) within the derived bounds of
tests/add_norm_ref.py against the fp64 formulas (torch float64 on the device).
Bytes: forward x, r, out, residual_out and the weight once; backward dy, z and dx once, the weight and dweight once, the partial
slab written and read once.  Rate = bytes / median time, against the 8 TB/s HBM peak and against the 6.45 TB/s fa_merge_states
streams at.
Each leg: a warm-up of >= 60 ms of calls, then `--ms` of calls between two device events; the legs alternate `--rounds` times;
median [min .. max] us per call.  Every shape runs in a child process of its own under a time limit (`--point-timeout` seconds);
the sweep stops at the first one that fails or runs out of time - nothing is started on a device that has just faulted.

    python tools/add_norm_sweep.py [--ms 100] [--rounds 5]
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
ap.add_argument("--point", default=None, help="(child) rows x N: measure it and print one JSON line")
args = ap.parse_args()

HBM_PEAK, STREAM = 8.0e12, 6.45e12                     # bytes / s: the peak README.md quotes, and what fa_merge_states streams at
EPS = 1e-6
SHAPES = [(rows, n) for n in (4096, 8192) for rows in (128, 8192, 65536)]
HERE = os.path.dirname(os.path.abspath(__file__))


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
    sys.path.insert(0, os.path.join(HERE, "..", "flash-attention-v100_amd"))
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    import torch
    import add_norm_ref as R
    from flash_attn_mi355 import add_norm as A
    rows, n = (int(v) for v in name.split("x"))
    bf = torch.bfloat16
    gd = torch.Generator(device="cuda").manual_seed(rows + n)
    mk = lambda: torch.randn(rows, n, device="cuda", dtype=bf, generator=gd)       # noqa: E731
    x, r, dy = mk(), mk(), mk()
    w = (1.0 + 0.2 * torch.randn(n, device="cuda", generator=gd)).to(bf)

    # check 1 (and the backward's bounds) first
    out, z = A.add_norm_forward(x, w, None, r, eps=EPS, prenorm=True)
    dx, _, dw, _ = A.add_norm_backward(dy, z, w, eps=EPS)
    torch.cuda.synchronize()
    assert torch.equal(z, R.add_ref(x, r, bf))
    worst = {}
    y, M = R.norm_ref(z, w, None, EPS, 0.0, True)
    worst["out"] = R.worst(out, y, R.fwd_bound(y, M, n, bf))
    del y, M
    ref = R.backward_ref(dy, z, w, None, EPS, 0.0, True)
    plan = R.plan(rows, n, False)
    worst["dx"] = R.worst(dx, ref["dz"], R.dz_bound(ref["dz"], ref["A"], n, bf))
    worst["dweight"] = R.worst(dw, ref["dw"], R.dw_bound(ref["dw"], ref["Sw"], plan["L"], n, bf))
    assert all(v <= 1.0 for v in worst.values()), f"{name}: outside the derived bounds: {worst}"
    del ref, out, dx, dw
    torch.cuda.empty_cache()

    xi, ri = x.clone(), r.clone()                          # the in-place legs rewrite these (values drift; the time does not)

    def eager(x_, r_, w_):
        z_ = x_ + r_
        h = z_.float()
        return w_ * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS)).to(bf), z_

    def eager_inplace():
        y_, z_ = eager(xi, ri, w)
        xi.copy_(y_)
        ri.copy_(z_)

    leaves = [t.detach().clone().requires_grad_(True) for t in (x, r, w)]
    y_l, _ = eager(*leaves)
    legs = {
        "fwd": (lambda: A.add_norm_forward(x, w, None, r, eps=EPS, prenorm=True), lambda: eager(x, r, w)),
        "fwd-inpl": (lambda: A.fused_add_rms_norm_(xi, ri, w, EPS), eager_inplace),
        "bwd": (lambda: A.add_norm_backward(dy, z, w, eps=EPS), lambda: torch.autograd.grad(y_l, leaves, dy, retain_graph=True)),
        "bwd-nodw": (lambda: A.add_norm_backward(dy, z, w, eps=EPS, need_dw=False),
                     lambda: torch.autograd.grad(y_l, leaves[:2], dy, retain_graph=True)),
    }
    times = {leg: ([], []) for leg in legs}
    for _ in range(args.rounds):
        for leg, (fused, base) in legs.items():
            times[leg][0].append(_time(fused, args.ms))
            times[leg][1].append(_time(base, args.ms))
            xi.copy_(x); ri.copy_(r)
    t2 = rows * n * 2
    nbytes = {"fwd": 4 * t2 + 2 * n, "fwd-inpl": 4 * t2 + 2 * n, "bwd": 3 * t2 + 4 * n + 2 * plan["workspace_bytes"], "bwd-nodw": 3 * t2 + 2 * n}
    stat = lambda t: [statistics.median(t), min(t), max(t)]                        # noqa: E731
    out = {"shape": name, "worst": worst, "parts": plan["parts"], "L": plan["L"], "bytes": nbytes,
           "legs": {leg: {"fused": stat(t[0]), "eager": stat(t[1])} for leg, t in times.items()}}
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
    print(f"# residual add + RMSNorm, bf16, bf16 weights, eps {EPS}; us per call: median [min .. max] of {args.rounds} rounds x "
          f"{args.ms:.0f} ms, fused and eager alternated; rate: algorithmic bytes / median, share of {HBM_PEAK / 1e12:.0f} TB/s peak and of "
          f"{STREAM / 1e12:.2f} TB/s (fa_merge_states); eager: the HF-form torch composition (fp32 inside), backward graph built once",
          flush=True)
    fmt = lambda t: f"{t[0]:8.1f} [{t[1]:8.1f} .. {t[2]:8.1f}]"                    # noqa: E731
    for rows, n in SHAPES:
        p = run_child(f"{rows}x{n}")
        if p is None:
            return 1
        print(f"rows {rows} N {n}: {p['parts']} partial rows, L {p['L']}; worst error / bound: "
              + ", ".join(f"{k} {v:.3f}" for k, v in p["worst"].items()), flush=True)
        for leg, t in p["legs"].items():
            rate = p["bytes"][leg] / (t["fused"][0] * 1e-6)
            print(f"  {leg:8s} fused {fmt(t['fused'])} us | eager {fmt(t['eager'])} us | eager / fused {t['eager'][0] / t['fused'][0]:6.2f} x | "
                  f"{p['bytes'][leg] / 1e6:8.2f} MB: {rate / 1e12:5.2f} TB/s ({100 * rate / HBM_PEAK:4.1f} % of peak, "
                  f"{100 * rate / STREAM:4.1f} % of the stream rate)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
