"""Cost of attention sinks: the same call with and without sinks, in one process, alternating.

Shapes (gpt-oss: head dim 64, 64 query heads over 8 kv heads, every other layer a 128-token sliding window):
  prefill   B 1, S 8192, H 64/8, D 64, causal and window (128, 0): forward, and forward + backward (q, k, v, sinks)
  decode    B 64, 8 k context, paged (pages of 64) bf16 and fp8 caches, one query token
  d128      B 1, S 8192, H 32/8, D 128, causal: with sinks the forward runs fa_fwd_kernel instead of the hand-scheduled body
The fp32 sinks are [H_q] logits drawn from N(0, 1).  Each leg: >= 60 ms of warm-up calls, then `--ms` of calls between
two device events; the legs alternate `--rounds` times and the median per call is reported.

    python tools/bench_sinks.py [--ms 300] [--rounds 3] [--only prefill,decode,d128]
"""
import argparse
import statistics
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v100_amd"))
import torch  # noqa: E402

import flash_attn_mi355 as fa  # noqa: E402


def _time(fn, ms, settle_ms=60.0):
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
    return s.elapsed_time(e) / n


def _pair(name, base, sink, args):
    tb, ts = [], []
    for _ in range(args.rounds):
        tb.append(_time(base, args.ms))
        ts.append(_time(sink, args.ms))
    b, s = statistics.median(tb), statistics.median(ts)
    print(f"{name:44s} no sink {b * 1e3:9.1f} us   sinks {s * 1e3:9.1f} us   ratio {s / b:6.3f}", flush=True)


def prefill(args, D=64, Hq=64, Hk=8, S=8192, label="prefill"):
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(1, S, Hq, D, device="cuda", dtype=torch.bfloat16, generator=g)
    k = torch.randn(1, S, Hk, D, device="cuda", dtype=torch.bfloat16, generator=g)
    v = torch.randn(1, S, Hk, D, device="cuda", dtype=torch.bfloat16, generator=g)
    do = torch.randn_like(q)
    sinks = torch.randn(Hq, device="cuda", generator=g)
    masks = [("causal", dict(causal=True))] + ([("window (128, 0)", dict(window_size=(128, 0)))] if D == 64 else [])
    for mname, kw in masks:
        _pair(f"{label} D{D} H{Hq}/{Hk} S{S} {mname} fwd",
              lambda: fa.flash_attn_func(q, k, v, **kw), lambda: fa.flash_attn_sinks_func(q, k, v, sinks, **kw), args)
        qg, kg, vg = (t.detach().requires_grad_() for t in (q, k, v))
        sg = sinks.detach().requires_grad_()

        def base():
            o = fa.flash_attn_func(qg, kg, vg, **kw)
            torch.autograd.grad(o, (qg, kg, vg), do)

        def sink():
            o = fa.flash_attn_sinks_func(qg, kg, vg, sg, **kw)
            torch.autograd.grad(o, (qg, kg, vg, sg), do)

        _pair(f"{label} D{D} H{Hq}/{Hk} S{S} {mname} fwd+bwd", base, sink, args)


def decode(args, B=64, ctx=8192, Hq=64, Hk=8, D=64, page=64):
    g = torch.Generator(device="cuda").manual_seed(1)
    pps = ctx // page
    nblk = B * pps
    q = torch.randn(B, 1, Hq, D, device="cuda", dtype=torch.bfloat16, generator=g)
    kc = torch.randn(nblk, page, Hk, D, device="cuda", dtype=torch.bfloat16, generator=g)
    vc = torch.randn(nblk, page, Hk, D, device="cuda", dtype=torch.bfloat16, generator=g)
    bt = torch.randperm(nblk, device="cuda", generator=g).reshape(B, pps).to(torch.int32)
    lens = torch.full((B,), ctx - 1, dtype=torch.int32, device="cuda")
    sinks = torch.randn(Hq, device="cuda", generator=g)
    for cname, kcc, vcc, kw in (("bf16", kc, vc, {}),
                                ("fp8", kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn), dict(k_descale=1.0, v_descale=1.0))):
        _pair(f"decode B{B} ctx{ctx} H{Hq}/{Hk} D{D} paged {cname}",
              lambda: fa.flash_attn_with_kvcache(q, kcc, vcc, cache_seqlens=lens, block_table=bt, **kw),
              lambda: fa.flash_attn_with_kvcache(q, kcc, vcc, cache_seqlens=lens, block_table=bt, sinks=sinks, **kw), args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="prefill,decode,d128")
    args = ap.parse_args()
    print(torch.cuda.get_device_name(), flush=True)
    only = args.only.split(",")
    if "prefill" in only:
        prefill(args)
    if "decode" in only:
        decode(args)
    if "d128" in only:
        prefill(args, D=128, Hq=32, Hk=8, label="d128")


if __name__ == "__main__":
    main()
