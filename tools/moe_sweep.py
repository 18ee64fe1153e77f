"""The MoE routing and data-movement ops (flash_attn_mi355.moe on csrc/fa_moe.hip) next to what a user runs without them: the torch
eager composition topk + softmax, stable argsort + bincount + cumsum, index_select and a weighted fp32 index_add_.

bf16, softmax routing with renormalisation, align 1 (the eager composition has no padding), identity experts (y = xp):
T {128, 8192, 65536} x (E, K) {(8, 2), (128, 8), (256, 8)} x N {4096, 7168}.  Per point these legs, each alternated in the same
run with its eager counterpart on the same tensors:
    route        moe_route_forward(logits, K)                 | topk(logits.float(), K) + softmax over the K values
    sort         moe_sort(ids, E)                             | argsort(stable) + bincount + cumsum
    permute      moe_permute_forward(x, sorted_slot, K)       | x.index_select(0, order // K)
    combine      moe_combine_forward(xp, w, pos)              | zeros fp32 [T, N] .index_add_(0, order // K, xp.float() * w[order]) .to(bf16)
    route_bwd    moe_route_backward(dw, logits, ids)          | (no eager counterpart: autograd's backward cannot be called
    combine_bwd  moe_combine_backward(dout, xp, w, pos)       |  without its forward)
    chain        route -> sort -> permute -> combine through torch.ops                      | the four eager steps
    chain+bwd    the same and torch.autograd.grad to x and the logits                        | the same through eager autograd
and once, untimed: torch.cuda.max_memory_allocated above the inputs for chain and chain+bwd, and the number of device kernels of one
chain+bwd call (torch.profiler).  Before anything is timed every point asserts: ids and weights of the first and last 64 rows
against tests/moe_ref.py (ids exact, weights within the counted bound), the sort against a stable argsort of all slots,
permute against index_select bit for bit, combine within its bound on the same rows.
Bytes are algorithmic: what the op must read and write once.  Rate = bytes / median time, against the 8 TB/s HBM peak and the
6.45 TB/s fa_merge_states streams at (profiles/shared_prefix_decode.txt).  Each leg: a warm-up of >= `--settle` ms of calls, then
`--ms` of calls between two device events; the legs alternate `--rounds` times; median [min .. max] us per call - call time.
Every point runs in a child process of its own under a time limit; the sweep stops at the first one that fails or runs out of time.

    python tools/moe_sweep.py [--only 8192x128x8x4096,..] [--ms 40] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--ms", type=float, default=40.0)
ap.add_argument("--settle", type=float, default=30.0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--point-timeout", type=int, default=240)
ap.add_argument("--only", default=None, help="comma-separated points T x E x K x N instead of the whole list")
ap.add_argument("--point", default=None, help="(child) T x E x K x N - measure it and print one JSON line")
args = ap.parse_args()

HBM_PEAK, STREAM = 8.0e12, 6.45e12
POINTS = [f"{T}x{E}x{K}x{N}" for N in (4096, 7168) for (E, K) in ((8, 2), (128, 8), (256, 8)) for T in (128, 8192, 65536)]
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "flash-attention-v100_amd")
LEGS = ("route", "sort", "permute", "combine", "route_bwd", "combine_bwd", "chain", "chain+bwd")


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


def point(name):
    sys.path.insert(0, PKG)
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    import numpy as np
    import torch
    import moe_ref as R
    from flash_attn_mi355 import moe as M
    import flash_attn_mi355.torch_ops  # noqa: F401
    ns = torch.ops.flash_attn_mi355
    T, E, K, N = (int(v) for v in name.split("x"))
    bf = torch.bfloat16
    gd = torch.Generator(device="cuda").manual_seed(T + E + N)
    logits = (torch.empty(T, E, device="cuda").normal_(generator=gd) * 2).to(bf)
    x = torch.empty(T, N, device="cuda").normal_(generator=gd).to(bf)
    dout = torch.empty(T, N, device="cuda").normal_(generator=gd).to(bf)
    dwt = torch.empty(T, K, device="cuda").normal_(generator=gd)

    def e_route(lg):
        tw, ti = torch.topk(lg.float(), K, dim=-1)
        return torch.softmax(tw, dim=-1), ti

    def e_sort(ti):
        flat = ti.reshape(-1)
        order = torch.argsort(flat, stable=True)
        return order, torch.cumsum(torch.bincount(flat, minlength=E), 0)

    def e_permute(xx, order):
        return xx.index_select(0, order // K)

    def e_combine(yp, w, order):
        acc = torch.zeros(T, N, device="cuda", dtype=torch.float32)
        return acc.index_add_(0, order // K, yp.float() * w.reshape(-1)[order][:, None]).to(bf)

    def e_chain(lg, xx):
        w, ti = e_route(lg)
        order, _ = e_sort(ti)
        return e_combine(e_permute(xx, order), w, order)

    def f_chain(lg, xx):
        w, ids = ns.moe_route(lg, K, "softmax", True, None, 1.0)
        sorted_slot, pos, _ = ns.moe_sort(ids, E, 1)
        return ns.moe_combine(ns.moe_permute(xx, sorted_slot, K, None, pos), w, pos)

    # correctness first
    w, ids = M.moe_route_forward(logits, K)
    sorted_slot, pos, offsets = M.moe_sort(ids, E)
    xp = M.moe_permute_forward(x, sorted_slot, K)
    out = M.moe_combine_forward(xp, w, pos)
    torch.cuda.synchronize()
    sel = torch.cat([torch.arange(min(64, T)), torch.arange(max(T - 64, 0), T)]).unique().cuda()
    lw = R.widen(logits[sel])
    w_ref, ids_ref, _ = R.route_ref(lw, K)
    assert (ids[sel].cpu().numpy() == ids_ref).all(), f"{name}: ids differ from the reference"
    worst = {"weights": float((np.abs(R.widen(w[sel]) - w_ref) / R.route_weight_bound(lw, w_ref, ids_ref, scoring="softmax",
                                                                                      renormalize=True)).max())}
    order, ends = e_sort(ids.long())
    assert torch.equal(sorted_slot.long(), order) and torch.equal(offsets[1:].long(), ends), f"{name}: the sort differs"
    assert torch.equal(xp.view(torch.int16), e_permute(x, order).view(torch.int16)), f"{name}: permute is not a copy"
    rows_of_sel = xp.index_select(0, pos[sel].reshape(-1).long())             # (only the rows these tokens read leave the device)
    ref, mag = R.combine_ref(R.widen(rows_of_sel), R.widen(w[sel]), np.arange(sel.numel() * K).reshape(-1, K))
    err32 = K * R.U * mag
    worst["combine"] = float((np.abs(R.widen(out[sel]) - ref) / (R.half_ulp16(np.abs(ref) + err32, "bfloat16") + err32 + R.TINY)).max())
    assert all(v <= 1.0 for v in worst.values()), f"{name}: outside the derived bounds: {worst}"
    ew, eti = e_route(logits)
    del ref, mag, err32, out
    torch.cuda.empty_cache()

    S, Mr = T * K, sorted_slot.shape[0]
    nbytes = {"route": T * E * 2 + S * 8, "sort": S * 4 + (Mr + S + E + 1) * 4, "permute": 2 * Mr * N * 2 + Mr * 4,
              "combine": S * N * 2 + T * N * 2 + S * 8, "route_bwd": 2 * T * E * 2 + S * 8,
              "combine_bwd": (T * N * 2 + Mr * N * 2 + S * 8) + (S * N * 2 + T * N * 2 + S * 8)}
    nbytes["chain"] = sum(nbytes[k] for k in ("route", "sort", "permute", "combine"))
    nbytes["chain+bwd"] = nbytes["chain"] + nbytes["route_bwd"] + nbytes["combine_bwd"] + nbytes["combine"]
    lg_g, x_g = logits.detach().requires_grad_(True), x.detach().requires_grad_(True)
    legs = {
        "route": (lambda: M.moe_route_forward(logits, K), lambda: e_route(logits)),
        "sort": (lambda: M.moe_sort(ids, E), lambda: e_sort(eti)),
        "permute": (lambda: M.moe_permute_forward(x, sorted_slot, K), lambda: e_permute(x, order)),
        "combine": (lambda: M.moe_combine_forward(xp, w, pos), lambda: e_combine(xp, ew, order)),
        "route_bwd": (lambda: M.moe_route_backward(dwt, logits, ids), None),
        "combine_bwd": (lambda: M.moe_combine_backward(dout, xp, w, pos), None),
        "chain": (lambda: f_chain(logits, x), lambda: e_chain(logits, x)),
        "chain+bwd": (lambda: torch.autograd.grad(f_chain(lg_g, x_g), (x_g, lg_g), dout),
                      lambda: torch.autograd.grad(e_chain(lg_g, x_g), (x_g, lg_g), dout)),
    }
    times = {leg: ([], []) for leg in legs}
    for _ in range(args.rounds):
        for leg, (fused, base) in legs.items():
            times[leg][0].append(_time(fused, args.ms, args.settle))
            if base is not None:
                times[leg][1].append(_time(base, args.ms, args.settle))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    def kernels(fn):
        try:
            from torch.profiler import ProfilerActivity, profile
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
        except Exception as exc:                              # the count is a side note: say so instead of failing the point
            return f"not measured ({type(exc).__name__})"
    mem = {leg: {"fused": peak(legs[leg][0]), "eager": peak(legs[leg][1])} for leg in ("chain", "chain+bwd")}
    launches = {"fused": kernels(legs["chain+bwd"][0]), "eager": kernels(legs["chain+bwd"][1])}
    stat = lambda t: [statistics.median(t), min(t), max(t)]                        # noqa: E731
    res = {"point": name, "worst": worst, "bytes": nbytes, "input_bytes": T * E * 2 + T * N * 2, "mem": mem, "launches": launches,
           "legs": {leg: {"fused": stat(t[0]), "eager": stat(t[1]) if t[1] else None} for leg, t in times.items()}}
    print("POINT " + json.dumps(res), flush=True)


def run_child(name):
    """one point in a process of its own under the time limit -> its dict, or None (the caller stops the sweep)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--point", name, "--ms", str(args.ms), "--rounds", str(args.rounds),
           "--settle", str(args.settle)]
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


fmt = lambda t: f"{t[0]:9.1f} [{t[1]:9.1f} .. {t[2]:9.1f}]"                        # noqa: E731


def rate(nbytes, us):
    r = nbytes / (us * 1e-6)
    return f"{nbytes / 1e6:10.2f} MB: {r / 1e12:5.2f} TB/s ({100 * r / HBM_PEAK:4.1f} % of peak, {100 * r / STREAM:4.1f} % of the merge stream)"


def main():
    if args.point:
        return point(args.point)
    print(f"# MoE routing ops, bf16, softmax + renormalise, align 1, identity experts; points T x E x K x N; us per call: median "
          f"[min .. max] of {args.rounds} rounds x {args.ms:.0f} ms, fused and eager alternated; rate: algorithmic bytes / median, share "
          f"of {HBM_PEAK / 1e12:.0f} TB/s peak and of {STREAM / 1e12:.2f} TB/s (fa_merge_states)", flush=True)
    for name in (args.only.split(",") if args.only else POINTS):
        p = run_child(name)
        if p is None:
            return 1
        print(f"{name}: worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in p["worst"].items()), flush=True)
        for leg in LEGS:
            t = p["legs"][leg]
            eager = f"eager {fmt(t['eager'])} us | eager / fused {t['eager'][0] / t['fused'][0]:6.2f} x" if t["eager"] else "eager not run"
            print(f"  {leg:11s} fused {fmt(t['fused'])} us | {eager} | {rate(p['bytes'][leg], t['fused'][0])}", flush=True)
        ib = p["input_bytes"]
        for leg, m in p["mem"].items():
            print(f"  peak memory above the inputs, {leg}: " + ", ".join(f"{k} {v / 1e6:.1f} MB ({v / ib:.2f} x the inputs)"
                                                                          for k, v in m.items()), flush=True)
        print(f"  device kernels of one chain+bwd call: fused {p['launches']['fused']}, eager {p['launches']['eager']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
