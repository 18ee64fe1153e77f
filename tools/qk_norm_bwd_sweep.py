"""The backward of QK-norm + RoPE (flash_attn_mi355.qk_norm.qk_norm_rope_backward on csrc/fa_qk_norm_rope_bwd.hip: dq, dk and both
weight gradients from the gradients of q_out / k_out and the saved pre-norm q / k, one launch plus a small second one for dw) next
to what a user runs without it: the torch eager autograd backward of the HF-form composition.

Set-up of tools/qk_norm_sweep.py (bf16, Hq 32, Hk 8, D 128, NeoX rotation of the whole head, bf16 weights 1 + 0.2 randn, eps 1e-6,
the same ragged positions): 128 rows (a call floor), 8192 rows and 65536 rows.  Out of place, contiguous tensors.  Per shape:
  fused      qk_norm_rope_backward(dq_out, dk_out, q, k, positions, cos, sin, q_weight, k_weight): all four outputs
  no dw      the same call with need_dw=False: one launch, no accumulation, no workspace - fused - no dw is what dw costs
  baseline   torch.autograd.grad through the eager composition the forward sweep's baseline uses - the HF module's RMSNorm
             (x.float(), pow(2).mean(-1), rsqrt, the product, the cast to bf16, times the weight) - followed by the HF rotation
             (x cos + rotate_half(x) sin at the gathered positions), for q and for k, gradients for q, k and both weights.  The
             graph is built once; only the backward is timed.
Before anything is timed, every case runs `fused` once and asserts that dq, dk, dq_weight and dk_weight are within the derived
bounds of tests/qk_norm_bwd_ref.py against the fp64 formulas (torch float64 on the device).
Bytes: x and dz read once, dx written once, the positions (8 bytes per row), one cos and one sin row per row, the weights and
their gradients once, the partial slab written and read once.  Rate = bytes / median time as a share of the 8 TB/s HBM peak the
README quotes.
Each leg: a warm-up of >= 60 ms of calls (past the clock ramp), then `--ms` of calls between two device events; the legs
alternate `--rounds` times; median [min .. max] us per call.  The second kernel's share is read from one torch.profiler pass over
a few fused calls after the timing (device time per kernel name); where the profiler gives no kernel records it is reported as
not measured.  Every shape runs in a child process of its own under a time limit (`--point-timeout` seconds); the sweep stops at
the first one that fails or runs out of time - nothing is started on a device that has just faulted.

    python tools/qk_norm_bwd_sweep.py [--ms 100] [--rounds 5]
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
HQ, HK, D, EPS = 32, 8, 128, 1e-6
SHAPES = {"decode_128": [1] * 128, "prefill_8192": [700, 1500, 3, 2048, 1024, 917, 1000, 1000],       # new tokens per sequence
          "prefill_65536": [8192] * 8}
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


def _kernel_share(fn):
    """device time of the second kernel / device time of both kernels over a few calls, or None"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
        main = fin = 0.0
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            t = getattr(ev, "cuda_time_total", 0.0) if t is None else t
            if "qk_norm_rope_bwd_finish_kernel" in ev.key:
                fin += t
            elif "qk_norm_rope_bwd_kernel" in ev.key:
                main += t
        return [fin / 5, main / 5] if main > 0 and fin > 0 else None
    except Exception:                                   # noqa: BLE001  (a missing profiler back end: reported as not measured)
        return None


def point(name):
    sys.path.insert(0, os.path.join(HERE, "..", "flash-attention-v100_amd"))
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    import torch
    import qk_norm_bwd_ref as B
    from flash_attn_mi355.qk_norm import qk_norm_rope_backward
    lens = SHAPES[name]
    Bn, T = len(lens), sum(lens)
    g = torch.Generator().manual_seed(T)
    L = torch.randint(0, 2048, (Bn,), generator=g).tolist()                    # tokens already cached per sequence
    pos_d = torch.tensor([L[b] + i for b in range(Bn) for i in range(lens[b])], dtype=torch.int64).cuda()
    gd = torch.Generator(device="cuda").manual_seed(T)
    mk = lambda h: torch.randn(T, h, D, device="cuda", dtype=torch.bfloat16, generator=gd)       # noqa: E731
    q, k, dzq, dzk = mk(HQ), mk(HK), mk(HQ), mk(HK)
    w = (1.0 + 0.2 * torch.randn(2, D, generator=g)).bfloat16().cuda()
    qw, kw = w[0].contiguous(), w[1].contiguous()
    seqlen_ro = max(l + n for l, n in zip(L, lens))
    ang = torch.arange(seqlen_ro, dtype=torch.float32)[:, None] / (10000 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))[None, :]
    cos, sin = torch.cos(ang).bfloat16().cuda(), torch.sin(ang).bfloat16().cuda()

    def fused():
        return qk_norm_rope_backward(dzq, dzk, q, k, pos_d, cos, sin, qw, kw, EPS)

    def no_dw():
        return qk_norm_rope_backward(dzq, dzk, q, k, pos_d, cos, sin, qw, kw, EPS, need_dw=False)

    # the bounds first
    dq, dk, dqw, dkw = fused()
    torch.cuda.synchronize()
    plan = B.plan(T, HQ, HK, D)
    worst = {}
    for dx, dw, dz, x, wt, nm in ((dq, dqw, dzq, q, qw, "q"), (dk, dkw, dzk, k, kw, "k")):
        ref = B.backward_ref_torch(dz, x, wt, pos_d, cos, sin, False, EPS, 0.0)
        dw_ref, S = ref["dw"].cpu().numpy(), ref["S"].cpu().numpy()
        worst["d" + nm] = B.dx_worst_torch(dx, ref["dx"], ref["A"], torch.bfloat16)
        worst["d" + nm + "_weight"] = B.worst(dw, dw_ref, B.dw_bound(dw_ref, S, plan["L"], D, torch.bfloat16))
        del ref
    assert all(v <= 1.0 for v in worst.values()), f"{name}: outside the derived bounds: {worst}"
    del dq, dk, dqw, dkw
    torch.cuda.empty_cache()

    # the eager composition, its graph built once
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, qw, kw)]
    c2 = torch.cat([cos[pos_d], cos[pos_d]], dim=-1)[:, None, :]
    s2 = torch.cat([sin[pos_d], sin[pos_d]], dim=-1)[:, None, :]

    def hf(x, weight):
        h = x.float()
        h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS)
        y = weight * h.to(x.dtype)
        return y * c2 + torch.cat([-y[..., D // 2:], y[..., :D // 2]], dim=-1) * s2

    outs = [hf(leaves[0], leaves[2]), hf(leaves[1], leaves[3])]

    def baseline():
        return torch.autograd.grad(outs, leaves, [dzq, dzk], retain_graph=True)

    legs = {"fused": fused, "no-dw": no_dw, "baseline": baseline}
    times = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg, fn in legs.items():
            times[leg].append(_time(fn, args.ms))
    nbytes = 3 * T * (HQ + HK) * D * 2 + T * 8 + 2 * T * (D // 2) * 2 + 4 * D * 2 + 2 * plan["workspace_bytes"]
    out = {"shape": name, "bytes": nbytes, "worst": worst, "grid": plan["grid"], "L": plan["L"], "share": _kernel_share(fused),
           **{leg: [statistics.median(t), min(t), max(t)] for leg, t in times.items()}}
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
    print(f"# QK RMSNorm + RoPE backward, bf16, out of place, Hq {HQ}, Hk {HK}, D {D}, NeoX rotary_dim {D}, bf16 weights; us per call: "
          f"median [min .. max] of {args.rounds} rounds x {args.ms:.0f} ms; rate: algorithmic bytes / median, share of "
          f"{HBM_PEAK / 1e12:.0f} TB/s; baseline: torch eager autograd backward of the HF-form RMSNorm (fp32 inside) + HF rotation, graph "
          f"built once; no dw: need_dw=False", flush=True)
    for name, lens in SHAPES.items():
        p = run_child(name)
        if p is None:
            return 1
        print(f"{name}: {sum(lens)} rows in {len(lens)} sequences, {p['grid']} workgroups", flush=True)
        fmt = lambda t: f"{t[0]:7.1f} [{t[1]:7.1f} .. {t[2]:7.1f}]"
        rf, rb = p["bytes"] / (p["fused"][0] * 1e-6), p["bytes"] / (p["baseline"][0] * 1e-6)
        share = "not measured" if p["share"] is None else \
            f"{p['share'][0]:.1f} us of {p['share'][0] + p['share'][1]:.1f} us device time ({100 * p['share'][0] / (p['share'][0] + p['share'][1]):.1f} %)"
        print(f"  fused {fmt(p['fused'])} us | no dw {fmt(p['no-dw'])} us | baseline {fmt(p['baseline'])} us | "
              f"baseline / fused {p['baseline'][0] / p['fused'][0]:5.2f} x | fused - no dw {p['fused'][0] - p['no-dw'][0]:+7.1f} us | "
              f"second kernel: {share} | {p['bytes'] / 1e6:7.2f} MB: fused {rf / 1e12:5.2f} TB/s ({100 * rf / HBM_PEAK:4.1f} % of peak), "
              f"baseline {rb / 1e12:5.2f} TB/s ({100 * rb / HBM_PEAK:4.1f} %) | worst error / bound: "
              + ", ".join(f"{k} {v:.3f}" for k, v in p["worst"].items()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
