"""Standalone rotary embedding (flash_attn.layers.rotary on csrc/fa_rotary.hip) next to the torch eager rotate_half composition a
user writes without it, and against the HBM figure.

Shapes (bf16, NeoX pairs, rotary_dim = D): the config-2 shape B 8, S 4096, H 16, D 128 as a packed [B, S, 3, H, D] qkv, and a GQA
prefill shape B 4, S 8192, Hq 32 / Hk 8, D 128 as [B, S, Hq + 2 Hk, D].  Per shape, three cases, each with two legs:
  qkv_inplace  apply_rotary_emb_qkv_ (q and k in place, one launch)   | eager: rotate_half on the q and k views, copied back
  out_of_place apply_rotary_emb on q (a fresh tensor)                 | eager: rotate_half on q
  backward     the backward of apply_rotary_emb on q (one launch)     | eager: autograd through rotate_half
Bytes: in place 2 x the rotated bytes (read + write) plus the cos / sin table once; out of place and backward the same (read x
or dout, write a fresh tensor).  Rate = bytes / median time, as a share of the 8 TB/s HBM peak the README quotes, next to the
6.45 TB/s fa_merge_states streams at (profiles/shared_prefix_decode.txt), the nearest kernel of the same kind.
Each leg: a warm-up of >= 60 ms of calls (past the clock ramp), then `--ms` of calls between two device events; the legs
alternate `--rounds` times; median [min .. max] us per call.  Every shape runs in a child process of its own under a time limit
(`--point-timeout` seconds); the sweep stops at the first one that fails or runs out of time - nothing is started on a device
that has just faulted.

    python tools/rotary_sweep.py [--ms 100] [--rounds 5]
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
ap.add_argument("--point-timeout", type=int, default=150)
ap.add_argument("--point", default=None, help="(child) shape name: measure it and print one JSON line")
args = ap.parse_args()

HBM_PEAK = 8.0e12                                      # bytes / s, the peak README.md quotes rates against
MERGE_TBS = 6.45                                       # fa_merge_states alone, profiles/shared_prefix_decode.txt
SHAPES = {"config2": (8, 4096, 16, 16, 128), "gqa_prefill": (4, 8192, 32, 8, 128)}     # B, S, Hq, Hk, D


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
    from flash_attn.layers.rotary import RotaryEmbedding, apply_rotary_emb, apply_rotary_emb_qkv_
    B, S, Hq, Hk, D = SHAPES[name]
    g = torch.Generator(device="cuda").manual_seed(S)
    qkv = torch.randn(B, S, Hq + 2 * Hk, D, device="cuda", dtype=torch.bfloat16, generator=g)
    emb = RotaryEmbedding(D, device="cuda")
    emb._update_cos_sin_cache(S, device=qkv.device, dtype=qkv.dtype)
    cos, sin = emb._cos_cached, emb._sin_cached
    q = qkv[:, :, :Hq]
    qk = qkv[:, :, :Hq + Hk]
    dout = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16, generator=g)
    cos_e = torch.cat((cos, cos), dim=-1)[None, :, None, :]          # the eager composition's [1, S, 1, D] tables
    sin_e = torch.cat((sin, sin), dim=-1)[None, :, None, :]

    def rotate_half(x):
        x1, x2 = x.chunk(2, dim=-1)
        return torch.cat((-x2, x1), dim=-1)

    def eager(x):
        return x * cos_e + rotate_half(x) * sin_e

    def eager_inplace():
        qk.copy_(eager(qk))

    q_leaf = q.detach().clone().requires_grad_()
    y_ours = apply_rotary_emb(q_leaf, cos, sin)
    y_eager = eager(q_leaf)
    legs = {
        "qkv_inplace": (lambda: apply_rotary_emb_qkv_(qkv, cos, sin, num_heads_q=Hq), eager_inplace, qk.numel()),
        "out_of_place": (lambda: apply_rotary_emb(q, cos, sin), lambda: eager(q), q.numel()),
        "backward": (lambda: torch.autograd.grad(y_ours, q_leaf, dout, retain_graph=True),
                     lambda: torch.autograd.grad(y_eager, q_leaf, dout, retain_graph=True), q.numel()),
    }
    # same answer first (the eager composition rounds after every elementwise step: reported, not gated)
    a, b = apply_rotary_emb(q, cos, sin).float(), eager(q).float()
    out = {"shape": name, "maxrel_vs_eager": float((a - b).abs().max() / b.abs().max())}
    res = {m: ([], []) for m in legs}
    for _ in range(args.rounds):
        for m, (ours, theirs, _) in legs.items():
            res[m][0].append(_time(ours, args.ms))
            res[m][1].append(_time(theirs, args.ms))
    for m, (t_ours, t_eager) in res.items():
        out[m] = {"ours": [statistics.median(t_ours), min(t_ours), max(t_ours)],
                  "eager": [statistics.median(t_eager), min(t_eager), max(t_eager)],
                  "bytes": 2 * legs[m][2] * 2 + 2 * cos.numel() * 2}
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
    print(f"# rotary embedding, bf16, NeoX, rotary_dim = D; us per call: median [min .. max] of {args.rounds} rounds x {args.ms:.0f} ms; "
          f"rate: algorithmic bytes / median, share of {HBM_PEAK / 1e12:.0f} TB/s (fa_merge_states alone: {MERGE_TBS} TB/s)", flush=True)
    for name, (B, S, Hq, Hk, D) in SHAPES.items():
        p = run_child(name)
        if p is None:
            return 1
        print(f"{name}: B {B} S {S} H {Hq}/{Hk} D {D}; max-rel vs eager {p['maxrel_vs_eager']:.1e}", flush=True)
        fmt = lambda t: f"{t[0]:8.1f} [{t[1]:8.1f} .. {t[2]:8.1f}]"
        for case in ("qkv_inplace", "out_of_place", "backward"):
            c = p[case]
            rate = c["bytes"] / (c["ours"][0] * 1e-6)
            print(f"  {case:12s} | fa_rotary {fmt(c['ours'])} us | eager {fmt(c['eager'])} us | eager / fa_rotary "
                  f"{c['eager'][0] / c['ours'][0]:5.2f} x | {c['bytes'] / 1e6:7.1f} MB, {rate / 1e12:5.2f} TB/s "
                  f"({100 * rate / HBM_PEAK:4.1f} % of peak, {rate / 1e12 / MERGE_TBS:4.2f} x the merge kernel's rate)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
