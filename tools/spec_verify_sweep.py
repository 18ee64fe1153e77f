"""Speculative-decoding verification (flash_attn_mi355.spec_decode on csrc/fa_spec_verify.hip) next to what a caller runs without
it: the eager torch composition of the same rules from the same uniform numbers - softmax into fp32, gather, compare, clamp of
p - q, cumsum, searchsorted, and a vectorised walk without a Python loop over requests.

Grid: B {1, 8, 64, 256} x V {32000, 128256, 151936}, bf16 logits (randn x 3), temperature 0.8.
  mode B  a chain of 4 and of 8 drafts per request (T = 5, 9), fp32 draft_probs (the softmax of the target logits plus noise, so
          that most drafts are accepted and the residual is a real distribution): `verify`, and `accept_forward` (fa_spec_accept)
          alone with its algorithmic bytes - per child node the target row twice (statistics, masses) and the draft row once, the
          one chunk that the last step sweeps again, and the workspace written and read - over the median, as a share of the
          8 TB/s HBM peak (fa_merge_states reaches 6.45 TB/s, profiles/merge_states.txt)
  mode A  a 32-node binary tree (depth 5), draft ids that follow the target's own draws on half of the nodes: `verify`
Per cell the legs alternate `--rounds` times in one process; each leg is a warm-up of >= `--settle` ms of calls, then `--ms` of
calls between two device events; median us per call.  The results are asserted first: accept, recovered and the emitted tokens of
the op agrees with the eager composition run in fp64 on at least 98 % of the nodes and requests (what is left: a uniform number within
the fp32 rounding of the masses of a threshold).  The share printed is the agreement with the fp32 composition that is timed: its
cumsum over V terms carries an error wider than many of the tail tokens' intervals, so a few per cent of its draws land on a
neighbouring token.  Every cell with eager / fused <= 1 is listed at the end.  Each V runs in
a child process of its own under a time limit; the sweep stops at the first one that fails - nothing is started on a device that
has just faulted.

    python tools/spec_verify_sweep.py [--ms 20] [--rounds 3] [--out profiles/spec_verify.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--ms", type=float, default=20.0)
ap.add_argument("--settle", type=float, default=10.0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--group-timeout", type=int, default=170)
ap.add_argument("--out", default=None, help="also write the tables to this file")
ap.add_argument("--group", default=None, help="(child) V: measure it and print JSON lines")
args = ap.parse_args()

HBM_PEAK = 8.0e12
BATCHES = [1, 8, 64, 256]
DRAFTS = [4, 8]
VOCABS = [32000, 128256, 151936]
TREE_T = 32
TEMP = 0.8
CHUNK = 16384
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "flash-attention-v100_amd")


def accept_bytes(B, T, V):
    """what fa_spec_accept moves for a chain: bf16 target rows, fp32 draft rows"""
    C = -(-V // CHUNK)
    again = min(V, CHUNK)
    return B * (T - 1) * (2 * V * 2 + V * 4 + again * (2 + 4) + 3 * 48 * C)


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


def _draw(p, u):
    """inverse CDF in index order: the first index whose running sum exceeds u x the total"""
    import torch
    cdf = p.cumsum(-1)
    return torch.searchsorted(cdf, u.unsqueeze(-1) * cdf[..., -1:], right=True).clamp_(max=p.shape[-1] - 1).squeeze(-1)


def _eager_chain(x, q, d, us, ua, ur, dt=None):
    """mode B on a chain: (accept [B, T - 1], recovered [B, T - 1], out_tokens [B, T], num_out [B]); dt: torch.float64 for the
    assertion, fp32 as timed"""
    import torch
    dt = dt or torch.float32
    B, T, V = x.shape
    p = torch.softmax(x.to(dt) / TEMP, -1)
    pp, qq, dd = p[:, :-1], q[:, 1:].to(dt), d[:, 1:].long()
    pd = pp.gather(-1, dd.unsqueeze(-1)).squeeze(-1)
    qd = qq.gather(-1, dd.unsqueeze(-1)).squeeze(-1)
    acc = ua[:, 1:].to(dt) * qd < pd
    rec = _draw((pp - qq).clamp_(min=0), ur[:, 1:].to(dt))
    bonus = _draw(p[:, -1], us[:, -1].to(dt))
    n_acc = acc.long().cumprod(-1).sum(-1)                              # the accepted prefix
    last = torch.cat([rec, bonus.unsqueeze(-1)], -1).gather(-1, n_acc.unsqueeze(-1))
    idx = torch.arange(T, device=x.device).unsqueeze(0)
    cand = torch.cat([dd, dd[:, :1]], -1)
    out = torch.where(idx < n_acc.unsqueeze(-1), cand, torch.where(idx == n_acc.unsqueeze(-1), last, torch.full_like(cand, -1)))
    return acc, rec, out, n_acc + 1


def _eager_tree(x, d, par, depth, us, dt=None):
    """mode A on a shared tree: (out_tokens [B, T], num_out [B]); the loop runs over the tree's depth, not over requests"""
    import torch
    dt = dt or torch.float32
    B, T, V = x.shape
    ids = _draw(torch.softmax(x.to(dt) / TEMP, -1), us.to(dt))
    rows = torch.arange(B, device=x.device)
    c = torch.zeros(B, dtype=torch.long, device=x.device)
    alive = torch.ones(B, dtype=torch.bool, device=x.device)
    out = torch.full((B, T), -1, dtype=torch.long, device=x.device)
    num = torch.zeros(B, dtype=torch.long, device=x.device)
    for step in range(depth + 1):
        y = ids[rows, c]
        out[:, step] = torch.where(alive, y, out[:, step])
        num += alive.long()
        match = (par.unsqueeze(0) == c.unsqueeze(-1)) & (d.long() == y.unsqueeze(-1))
        match[:, 0] = False
        alive = alive & match.any(-1)
        c = torch.where(alive, match.float().argmax(-1), c)
    return out, num


def group(V):
    sys.path.insert(0, PKG)
    import torch
    import flash_attn_mi355.sample as S
    import flash_attn_mi355.spec_decode as D
    g = torch.Generator(device="cuda").manual_seed(V)
    rnd = lambda *shape: torch.rand(*shape, device="cuda", generator=g)   # noqa: E731
    for B in BATCHES:
        for drafts in DRAFTS:
            T = drafts + 1
            x = (torch.randn(B, T, V, device="cuda", generator=g) * 3).bfloat16()
            q = torch.zeros(B, T, V, device="cuda")          # row t drafts what follows node t - 1: the target's row t - 1 plus noise
            q[:, 1:] = torch.softmax(x[:, :-1].float() / TEMP + torch.randn(B, drafts, V, device="cuda", generator=g), -1)
            d = torch.zeros(B, T, dtype=torch.int32, device="cuda")
            d[:, 1:] = torch.multinomial(q[:, 1:].reshape(-1, V), 1, generator=g).view(B, drafts).int()
            us, ua, ur = rnd(B, T), rnd(B, T), rnd(B, T)
            fused = lambda: D.verify_forward(x, d, q, None, TEMP, us, ua, ur)                        # noqa: E731
            accept = lambda: D.accept_forward(x, q, d, ua, ur, temperature=TEMP)                     # noqa: E731
            eager = lambda: _eager_chain(x, q, d, us, ua, ur)                                        # noqa: E731
            (tok, num, _), (a, r), (ea, er, eo, en) = fused(), accept(), eager()
            torch.cuda.synchronize()
            share = lambda ea, er, eo: dict(accept=float((a[:, 1:] != 0).eq(ea).float().mean()),                # noqa: E731
                                            recovered=float(r[:, 1:].long().eq(er).float().mean()),
                                            tokens=float(tok.long().eq(eo).all(-1).float().mean()))
            agree = share(ea, er, eo)
            exact = share(*_eager_chain(x, q, d, us, ua, ur, torch.float64)[:3])
            assert min(exact.values()) >= 0.98 or B * drafts < 64, exact
            assert bool((num >= 1).all()) and bool((num <= T).all())
            tf, ta, te = [], [], []
            for _ in range(args.rounds):
                tf.append(_time(fused, args.ms, args.settle))
                ta.append(_time(accept, args.ms, args.settle))
                te.append(_time(eager, args.ms, args.settle))
            print(json.dumps(dict(mode="B", B=B, T=T, V=V, fused=statistics.median(tf), accept_us=statistics.median(ta),
                                  eager=statistics.median(te), bytes=accept_bytes(B, T, V), accepted=float(num.float().mean()) - 1,
                                  **agree)), flush=True)
            del x, q
        T = TREE_T
        par = torch.tensor([-1] + [(t - 1) // 2 for t in range(1, T)], dtype=torch.int32, device="cuda")
        x = (torch.randn(B, T, V, device="cuda", generator=g) * 3).bfloat16()
        us = rnd(B, T)
        ids = S.sample_forward(x, us, temperature=TEMP)[0]
        d = torch.randint(0, V, (B, T), device="cuda", generator=g, dtype=torch.int32)
        follow = torch.arange(T, device="cuda") % 2 == 1                 # the odd children carry the target's own draw
        d = torch.where(follow.unsqueeze(0), ids[:, par.clamp(min=0).long()], d)
        fused = lambda: D.verify_forward(x, d, None, par, TEMP, us, None, None)                      # noqa: E731
        eager = lambda: _eager_tree(x, d, par.long(), 5, us)                                          # noqa: E731
        (tok, num, _), (eo, en) = fused(), eager()
        torch.cuda.synchronize()
        same = float(tok.long().eq(eo).all(-1).float().mean())
        exact = float(tok.long().eq(_eager_tree(x, d, par.long(), 5, us, torch.float64)[0]).all(-1).float().mean())
        assert exact >= 0.98 or B < 64, exact
        tf, te = [], []
        for _ in range(args.rounds):
            tf.append(_time(fused, args.ms, args.settle))
            te.append(_time(eager, args.ms, args.settle))
        print(json.dumps(dict(mode="A", B=B, T=T, V=V, fused=statistics.median(tf), eager=statistics.median(te), tokens=same,
                              accepted=float(num.float().mean()) - 1)), flush=True)
        del x


def main():
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def run(V):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--group", str(V), "--ms", str(args.ms), "--settle",
                                str(args.settle), "--rounds", str(args.rounds)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               text=True, timeout=args.group_timeout)
        except subprocess.TimeoutExpired:
            emit(f"V {V} did not finish in {args.group_timeout} s (hung); the sweep stops here")
            return None
        if p.returncode != 0:
            emit(f"V {V} failed ({p.returncode}); the sweep stops here\n{p.stderr[-2000:]}")
            return None
        return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]

    emit(f"spec_decode.verify vs eager torch (softmax, gather, compare, clamp, cumsum, searchsorted, vectorised walk); bf16 logits, "
         f"fp32 draft_probs, temperature {TEMP}; median of {args.rounds} rounds of {args.ms:.0f} ms; us per call")
    emit(f"{'mode':4} {'V':>7} {'B':>4} {'T':>3} {'verify us':>10} {'eager us':>10} {'eager/verify':>12} {'accept us':>10} "
         f"{'accept MB':>10} {'TB/s':>6} {'% of 8 TB/s':>11} {'accepted':>8} {'same accept / recovered / tokens':>32}")
    slower, ok = [], True
    for V in VOCABS:
        res = run(V)
        if res is None:
            ok = False
            break
        for r in res:
            ratio = r["eager"] / r["fused"]
            if r["mode"] == "B":
                tbs = r["bytes"] / (r["accept_us"] * 1e-6) / 1e12
                emit(f"{r['mode']:4} {r['V']:7d} {r['B']:4d} {r['T']:3d} {r['fused']:10.1f} {r['eager']:10.1f} {ratio:12.2f} "
                     f"{r['accept_us']:10.1f} {r['bytes'] / 1e6:10.1f} {tbs:6.2f} {tbs * 1e12 / HBM_PEAK * 100:11.1f} {r['accepted']:8.2f} "
                     f"{r['accept']:10.3f} {r['recovered']:10.3f} {r['tokens']:10.3f}")
            else:
                emit(f"{r['mode']:4} {r['V']:7d} {r['B']:4d} {r['T']:3d} {r['fused']:10.1f} {r['eager']:10.1f} {ratio:12.2f} "
                     f"{'':10} {'':10} {'':6} {'':11} {r['accepted']:8.2f} {'':10} {'':10} {r['tokens']:10.3f}")
            if ratio <= 1.0:
                slower.append(f"mode {r['mode']} V {r['V']} B {r['B']} T {r['T']}: {ratio:.2f}")
    if ok:
        emit()
        emit("cells where verify is not faster than eager: " + ("none" if not slower else ""))
        for s in slower:
            emit("  " + s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    if args.group:
        group(int(args.group))
    else:
        sys.exit(main())
