"""The fused serving prologue (flash_attn_mi355.rope_store.rope_and_store_kv on csrc/fa_rope_store.hip: q and k rotated at per-token
positions, K / V stored by slot, one launch) next to this library's two-launch composition on the same tensors, and to the torch
eager composition a user writes without either.

Shapes (bf16, Hq 32, Hk 8, D 128, page 16, NeoX rotation of the whole head): 128 rows (128 sequences of one token: a decode step,
the floor of a call - launch plus the Python layer), 8192 rows (8 ragged sequences: a prefill chunk) and 65536 rows (8 x 8192),
which moves 1.1 - 1.3 GB: more than the 256 MiB last-level cache holds, so its rate is the kernel's streaming rate.  q, k and v
are the head slices of one packed [T, Hq + 2 Hk, D] buffer and are rotated IN PLACE.  The positions are those of a ragged batch
(cache_seqlens[b] + i), so that the two-launch baseline can express them.  Per shape, into a bf16 and into an fp8-e4m3 cache:
  fused       rope_and_store_kv(q, k, v, positions, cos, sin, k_cache, v_cache, slot_mapping): one launch
  two-launch  apply_rotary_emb in place over the q + k heads of the packed buffer as one view (cu_seqlens + seqlen_offsets:
              fa_rotary), then store_kv_cache(k, v, ..., slot_mapping=) (fa_kv_store)
  eager       torch: cos / sin rows gathered by position, the rotate-half formula in fp32 on q and on k, written back; for an fp8
              cache the divide, clamp and cast of K and V; index_copy_ of K and of V on the flattened cache
Before anything is timed, every case runs `fused` and `two-launch` once on clones of the same inputs and asserts that the packed
buffer and both caches hold the same bits.
Bytes: q and k read and written once, v read once, the cache rows written once, positions and slot_mapping (16 bytes per row), one
cos and one sin row per row.  Rate = bytes / median time of `fused`, as a share of the 8 TB/s HBM peak the README quotes.
Each leg: a warm-up of >= 60 ms of calls (past the clock ramp), then `--ms` of calls between two device events; the legs
alternate `--rounds` times; median [min .. max] us per call.  Every shape runs in a child process of its own under a time limit
(`--point-timeout` seconds); the sweep stops at the first one that fails or runs out of time - nothing is started on a device
that has just faulted.  FA_MI355_LIB selects an experiment build of the library (the variant with nontemporal q_out / k_out
stores: `build.py --variant <out.so> FA_ROPE_STORE_NT_OUT=1`); the header line names it.

    python tools/rope_store_sweep.py [--ms 100] [--rounds 5]
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
PAGE, HQ, HK, D = 16, 32, 8, 128
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
    from flash_attn.layers.rotary import apply_rotary_emb
    from flash_attn_mi355.kv_store import store_kv_cache
    from flash_attn_mi355.rope_store import rope_and_store_kv
    lens = SHAPES[name]
    B, T = len(lens), sum(lens)
    assert T in (8192, 128, 65536)
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
    cu = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32).cuda()
    Ld = torch.tensor(L, dtype=torch.int32).cuda()
    slot_d, pos_d = torch.tensor(slots, dtype=torch.int64).cuda(), torch.tensor(pos, dtype=torch.int64).cuda()
    gd = torch.Generator(device="cuda").manual_seed(T)
    qkv0 = torch.randn(T, HQ + 2 * HK, D, device="cuda", dtype=torch.bfloat16, generator=gd)
    seqlen_ro = max(l + n for l, n in zip(L, lens))
    ang = torch.arange(seqlen_ro, dtype=torch.float32)[:, None] / (10000 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))[None, :]
    cos, sin = torch.cos(ang).bfloat16().cuda(), torch.sin(ang).bfloat16().cuda()
    kd, vd = 0.0625, 0.03125
    rot = dict(interleaved=False, inplace=True, seqlen_offsets=Ld, cu_seqlens=cu, max_seqlen=max(lens))
    out = {"shape": name, "cases": []}
    for cache in ("bf16", "fp8"):
        fp8 = cache == "fp8"
        cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16
        kw = dict(k_descale=kd, v_descale=vd) if fp8 else {}
        ibits = torch.uint8 if fp8 else torch.int16                            # (index_copy_ on integer views: same bytes)

        def make(leg):
            qkv = qkv0.clone()
            q, k, v, qk = qkv[:, :HQ], qkv[:, HQ:HQ + HK], qkv[:, HQ + HK:], qkv[:, :HQ + HK]
            kc = torch.zeros((nblk, PAGE, HK, D), dtype=torch.bfloat16, device="cuda").to(cdt)
            vc = torch.zeros_like(kc)
            kf, vf = kc.view(ibits).view(-1, HK, D), vc.view(ibits).view(-1, HK, D)

            def fused():
                rope_and_store_kv(q, k, v, pos_d, cos, sin, kc, vc, slot_d, **kw)

            def two_launch():
                apply_rotary_emb(qk, cos, sin, **rot)
                store_kv_cache(k, v, kc, vc, slot_mapping=slot_d, **kw)

            def eager():
                c, s = cos[pos_d].float()[:, None, :], sin[pos_d].float()[:, None, :]
                x = qk.float()
                x0, x1 = x[..., :D // 2], x[..., D // 2:]
                qk.copy_(torch.cat((x0 * c - x1 * s, x0 * s + x1 * c), dim=-1))
                kk, vv = k, v
                if fp8:
                    kk = (kk.float() / kd).clamp(-448, 448).to(cdt)
                    vv = (vv.float() / vd).clamp(-448, 448).to(cdt)
                kf.index_copy_(0, slot_d, kk.contiguous().view(ibits))
                vf.index_copy_(0, slot_d, vv.contiguous().view(ibits))

            return {"fused": fused, "two-launch": two_launch, "eager": eager}[leg], (qkv, kc, vc)

        (f_a, st_a), (f_b, st_b) = make("fused"), make("two-launch")
        f_a(); f_b()
        torch.cuda.synchronize()
        same = all(bool(torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.uint8),
                                    b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.uint8))) for a, b in zip(st_a, st_b))
        assert same, f"{name} {cache}: the fused call and the two-launch composition leave different bits"
        assert not torch.equal(st_a[0], qkv0) and bool((st_a[1].float() != 0).any())           # (both did rotate and store)
        legs = {leg: make(leg)[0] for leg in ("fused", "two-launch", "eager")}
        times = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg, fn in legs.items():
                times[leg].append(_time(fn, args.ms))
        nbytes = 2 * T * (HQ + HK) * D * 2 + T * HK * D * 2 + 2 * T * HK * D * (1 if fp8 else 2) + T * 16 + 2 * T * (D // 2) * 2
        out["cases"].append({"cache": cache, "same_bits_as_two_launch": same, "bytes": nbytes,
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
    lib = os.environ.get("FA_MI355_LIB")
    print(f"# fused RoPE + KV-cache store, bf16 packed qkv in place, Hq {HQ}, Hk {HK}, D {D}, page {PAGE}, NeoX rotary_dim {D}; library: "
          f"{os.path.basename(lib) if lib else 'the product build'}; us per call: median [min .. max] of {args.rounds} rounds x "
          f"{args.ms:.0f} ms; rate: algorithmic bytes / median of the fused call, share of {HBM_PEAK / 1e12:.0f} TB/s; kernel time apart "
          f"from the call: not measured", flush=True)
    for name, lens in SHAPES.items():
        p = run_child(name)
        if p is None:
            return 1
        print(f"{name}: {sum(lens)} rows in {len(lens)} sequences", flush=True)
        fmt = lambda t: f"{t[0]:7.1f} [{t[1]:7.1f} .. {t[2]:7.1f}]"
        for c in p["cases"]:
            rate = c["bytes"] / (c["fused"][0] * 1e-6)
            print(f"  {c['cache']:4s} cache | fused {fmt(c['fused'])} us | two-launch {fmt(c['two-launch'])} us | eager {fmt(c['eager'])} us | "
                  f"two-launch / fused {c['two-launch'][0] / c['fused'][0]:5.2f} x | eager / fused {c['eager'][0] / c['fused'][0]:6.2f} x | "
                  f"{c['bytes'] / 1e6:7.2f} MB, {rate / 1e12:5.2f} TB/s ({100 * rate / HBM_PEAK:4.1f} % of peak) | "
                  f"same bits as two-launch: {c['same_bits_as_two_launch']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
