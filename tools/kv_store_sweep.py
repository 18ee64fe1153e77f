"""KV-cache store (flash_attn_mi355.kv_store.store_kv_cache on csrc/fa_kv_store.hip) next to the torch eager composition a user
writes without it, and against the HBM figure.

Shapes (bf16, page 16, Hk 8, D 128): a prefill chunk of 8192 rows (8 ragged sequences), a decode-sized batch of 128 rows (128
sequences of one token: the floor of a call - launch plus the Python layer) and 65536 rows (8 x 8192), which moves 0.4 - 0.8 GB:
more than the 256 MiB last-level cache holds and far above the floor, so its rate is the kernel's streaming rate.  Per shape, the cases cache {bf16, fp8-e4m3} x addressing {seq: cu_seqlens +
cache_seqlens + block_table, slot: slot_mapping} x RoPE on K {no, yes (NeoX, rotary_dim = D)}, each with two legs:
  ours   store_kv_cache, one launch (slot mode has no fused rotation: apply_rotary_emb - fa_rotary - out of place, then the store)
  eager  index_copy_ on the flattened cache with a precomputed int64 row index (K, then V), preceded for an fp8 cache by the
         divide, clamp and cast of K and of V, and with RoPE by apply_rotary_emb on K (this library's kernel: the rotation itself
         is not what is compared)
Bytes: k and v read once, the cache rows written once, plus the tables the kernel reads (slot: 8 bytes per row; seq: cu_seqlens,
cache_seqlens and one block-table entry per page touched; RoPE: one cos and one sin row per position).  Rate = bytes / median
time, as a share of the 8 TB/s HBM peak the README quotes, next to the 6.45 TB/s fa_merge_states streams at
(profiles/shared_prefix_decode.txt) and fa_rotary's out-of-place 5.69 - 5.83 TB/s (profiles/rotary.txt).  The 8192-row problem
moves 50 - 100 MB, which the 256 MiB last-level cache can hold between calls, and a call of it takes little more than the
128-row floor: its rate says how close to the floor a prefill chunk is, not what the kernel streams at.
Each leg: a warm-up of >= 60 ms of calls (past the clock ramp), then `--ms` of calls between two device events; the legs
alternate `--rounds` times; median [min .. max] us per call.  Every shape runs in a child process of its own under a time limit
(`--point-timeout` seconds); the sweep stops at the first one that fails or runs out of time - nothing is started on a device
that has just faulted.  FA_MI355_LIB selects an experiment build of the library (the nontemporal-store variant:
`build.py --variant <out.so> FA_KV_STORE_NT_STORES=1`); the header line names it.

    python tools/kv_store_sweep.py [--ms 100] [--rounds 5]
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
MERGE_TBS = 6.45                                       # fa_merge_states alone, profiles/shared_prefix_decode.txt
ROTARY_TBS = (5.69, 5.83)                              # fa_rotary out of place, profiles/rotary.txt
PAGE, HK, D = 16, 8, 128
SHAPES = {"prefill_8192": [700, 1500, 3, 2048, 1024, 917, 1000, 1000], "decode_128": [1] * 128,       # new tokens per sequence
          "prefill_65536": [8192] * 8}
CASES = list(itertools.product(("bf16", "fp8"), ("seq", "slot"), (False, True)))


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
    lens = SHAPES[name]
    B, T = len(lens), sum(lens)
    assert T in (8192, 128, 65536)
    g = torch.Generator().manual_seed(T)
    L = torch.randint(0, 2048, (B,), generator=g).tolist()                     # tokens already cached per sequence
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
    slot_d = torch.tensor(slots, dtype=torch.int64).cuda()
    gd = torch.Generator(device="cuda").manual_seed(T)
    qkv = torch.randn(T, 32 + 2 * HK, D, device="cuda", dtype=torch.bfloat16, generator=gd)
    k, v = qkv[:, 32:32 + HK], qkv[:, 32 + HK:]                                # views of a packed qkv, as a model produces them
    seqlen_ro = max(l + n for l, n in zip(L, lens))
    ang = torch.arange(seqlen_ro, dtype=torch.float32)[:, None] / (10000 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))[None, :]
    cos, sin = torch.cos(ang).bfloat16().cuda(), torch.sin(ang).bfloat16().cuda()
    kd, vd = 0.0625, 0.03125
    out = {"shape": name, "cases": []}
    for cache, mode, rope in CASES:
        fp8 = cache == "fp8"
        cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16
        kc = torch.zeros((nblk, PAGE, HK, D), dtype=torch.bfloat16, device="cuda").to(cdt)
        vc = torch.zeros_like(kc)
        kc_e, vc_e = torch.zeros_like(kc), torch.zeros_like(kc)
        kw = dict(k_descale=kd, v_descale=vd) if fp8 else {}
        rot = dict(interleaved=False, seqlen_offsets=Ld, cu_seqlens=cu, max_seqlen=max(lens))

        def ours():
            if mode == "seq":
                r = dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False) if rope else {}
                store_kv_cache(k, v, kc, vc, cu_seqlens=cu, cache_seqlens=Ld, block_table=btd, **r, **kw)
            else:
                store_kv_cache(apply_rotary_emb(k, cos, sin, **rot) if rope else k, v, kc, vc, slot_mapping=slot_d, **kw)

        ibits = torch.uint8 if fp8 else torch.int16                            # (index_copy_ on integer views: same bytes)
        kf, vf = kc_e.view(ibits).view(-1, HK, D), vc_e.view(ibits).view(-1, HK, D)

        def eager():
            kk = apply_rotary_emb(k, cos, sin, **rot) if rope else k
            vv = v
            if fp8:
                kk = (kk.float() / kd).clamp(-448, 448).to(cdt)
                vv = (vv.float() / vd).clamp(-448, 448).to(cdt)
            kf.index_copy_(0, slot_d, kk.view(ibits))
            vf.index_copy_(0, slot_d, vv.view(ibits))

        ours(); eager()
        torch.cuda.synchronize()
        same = bool(torch.equal(kc.view(ibits), kc_e.view(ibits)) and torch.equal(vc.view(ibits), vc_e.view(ibits)))
        t_ours, t_eager = [], []
        for _ in range(args.rounds):
            t_ours.append(_time(ours, args.ms))
            t_eager.append(_time(eager, args.ms))
        nbytes = 2 * T * HK * D * 2 + 2 * T * HK * D * (1 if fp8 else 2)
        nbytes += T * 8 if mode == "slot" else (2 * B + 1 + touched) * 4
        if rope:
            nbytes += 2 * T * (D // 2) * 2 + (2 * T * HK * D * 2 if mode == "slot" else 0)   # slot: fa_rotary reads K and writes it once more
        out["cases"].append({"cache": cache, "mode": mode, "rope": rope, "same_bits_as_eager": same, "bytes": nbytes,
                             "ours": [statistics.median(t_ours), min(t_ours), max(t_ours)],
                             "eager": [statistics.median(t_eager), min(t_eager), max(t_eager)]})
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
    print(f"# KV-cache store, bf16 k / v, page {PAGE}, Hk {HK}, D {D}; library: {os.path.basename(lib) if lib else 'the product build'}; "
          f"us per call: median [min .. max] of {args.rounds} rounds x {args.ms:.0f} ms; rate: algorithmic bytes / median, share of "
          f"{HBM_PEAK / 1e12:.0f} TB/s (fa_merge_states alone: {MERGE_TBS} TB/s; fa_rotary out of place: {ROTARY_TBS[0]} - {ROTARY_TBS[1]} TB/s)",
          flush=True)
    for name, lens in SHAPES.items():
        p = run_child(name)
        if p is None:
            return 1
        print(f"{name}: {sum(lens)} rows in {len(lens)} sequences", flush=True)
        fmt = lambda t: f"{t[0]:7.1f} [{t[1]:7.1f} .. {t[2]:7.1f}]"
        for c in p["cases"]:
            rate = c["bytes"] / (c["ours"][0] * 1e-6)
            label = f"{c['cache']:4s} {c['mode']:4s} {'rope' if c['rope'] else 'plain'}"
            print(f"  {label:15s} | fa_kv_store {fmt(c['ours'])} us | eager {fmt(c['eager'])} us | eager / fa_kv_store "
                  f"{c['eager'][0] / c['ours'][0]:5.2f} x | {c['bytes'] / 1e6:6.2f} MB, {rate / 1e12:5.2f} TB/s "
                  f"({100 * rate / HBM_PEAK:4.1f} % of peak, {rate / 1e12 / MERGE_TBS:4.2f} x the merge kernel's rate) | "
                  f"same bits as eager: {c['same_bits_as_eager']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
