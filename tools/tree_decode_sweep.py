"""Cost of a tree-masked speculative decoding step next to the causal multi-token step of the same shape.

Shapes: B 1 / 16 / 128, H 32/8 and 64/8, T_q 8 / 32 / 64 over 4 k and 32 k keys, D 128, paged (pages of 256), bf16 and
fp8-e4m3 caches; plus the single-token step (T_q 1, causal column only) as a guard for the kernels a tree never reaches.
Per shape: the causal step (`causal=True`, K / V of the T_q tokens appended by the call) and the tree step (same call with
a random tree's mask as packed words; no rotary in either, so depths play no part).  Each leg: >= 60 ms of warm-up calls,
then `--ms` of calls between two device events; the legs alternate `--rounds` times; median, min and max per call are
printed, so the spread of repeated runs of one leg is on the same line as the difference between legs.

    python tools/tree_decode_sweep.py [--ms 150] [--rounds 5] [--modes causal,tree] [--pkg DIR] [--batches 1,16,128]

`--pkg DIR` imports flash_attn_mi355 from another build of the package (e.g. a checkout of the parent commit, whose
flash_attn_with_kvcache has no tree_mask: run it with --modes causal) for the before / after columns.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--ms", type=float, default=150.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--modes", default="causal,tree")
ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flash-attention-v100_amd"))
ap.add_argument("--batches", default="1,16,128")
ap.add_argument("--ctx", default="4096,32768")
ap.add_argument("--tq", default="1,8,32,64")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.pkg))
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
    return s.elapsed_time(e) / n * 1e3


def random_tree_words(B, T, seed):
    """packed visibility words [B, T, ceil(T / 32)] of random trees (parent[t] < t; a node sees itself and its ancestors)"""
    rng = np.random.default_rng(seed)
    W = (T + 31) // 32
    words = np.zeros((B, T, W), dtype=np.uint32)
    for b in range(B):
        for t in range(T):
            par = -1 if t == 0 else int(rng.integers(-1, t))
            if par >= 0:
                words[b, t] = words[b, par]
            words[b, t, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    return torch.from_numpy(words.view(np.int32)).cuda()


def main():
    modes = args.modes.split(",")
    page, D, Hk = 256, 128, 8
    print(f"# {torch.cuda.get_device_name(0)}; package {os.path.abspath(args.pkg)}; us per call: median [min .. max] of {args.rounds} rounds x {args.ms:.0f} ms")
    for B in map(int, args.batches.split(",")):
        for ctx in map(int, args.ctx.split(",")):
            pps = (ctx + 64 + page - 1) // page
            g = torch.Generator(device="cuda").manual_seed(B + ctx)
            kc16 = torch.randn(B * pps, page, Hk, D, device="cuda", dtype=torch.bfloat16, generator=g)
            vc16 = torch.randn(B * pps, page, Hk, D, device="cuda", dtype=torch.bfloat16, generator=g)
            bt = torch.randperm(B * pps, device="cuda", generator=g).to(torch.int32).reshape(B, pps)
            for kv in ("bf16", "fp8"):
                kw = {}
                if kv == "fp8":
                    kc, vc = (kc16.float() * 0.5).to(torch.float8_e4m3fn), (vc16.float() * 0.5).to(torch.float8_e4m3fn)
                    kw = dict(k_descale=2.0, v_descale=2.0)
                else:
                    kc, vc = kc16, vc16
                for Hq in (32, 64):
                    for T in map(int, args.tq.split(",")):
                        lens = torch.full((B,), ctx - T, dtype=torch.int32, device="cuda")
                        q = torch.randn(B, T, Hq, D, device="cuda", dtype=torch.bfloat16, generator=g)
                        kn = torch.randn(B, T, Hk, D, device="cuda", dtype=torch.bfloat16, generator=g)
                        vn = torch.randn(B, T, Hk, D, device="cuda", dtype=torch.bfloat16, generator=g)
                        legs = {}
                        if "causal" in modes:
                            legs["causal"] = lambda: fa.flash_attn_with_kvcache(q, kc, vc, k=kn, v=vn, cache_seqlens=lens, block_table=bt,
                                                                                causal=True, **kw)
                        if "tree" in modes and T >= 2:
                            words = random_tree_words(B, T, T + B)
                            legs["tree"] = lambda: fa.flash_attn_with_kvcache(q, kc, vc, k=kn, v=vn, cache_seqlens=lens, block_table=bt,
                                                                              tree_mask=words, **kw)
                        res = {m: [] for m in legs}
                        for _ in range(args.rounds):
                            for m, fn in legs.items():
                                res[m].append(_time(fn, args.ms))
                        line = f"B {B:3d} H {Hq}/{Hk} T_q {T:2d} ctx {ctx:5d} {kv:4s}"
                        for m, ts in res.items():
                            line += f" | {m} {statistics.median(ts):9.1f} [{min(ts):9.1f} .. {max(ts):9.1f}]"
                        print(line, flush=True)
                if kv == "fp8":
                    del kc, vc
            del kc16, vc16


if __name__ == "__main__":
    main()
