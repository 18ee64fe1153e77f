"""fp8-e4m3 quantisation fused behind add_norm and act_mul (flash_attn_mi355.quant on csrc/fa_quant.hip) next to the ways of getting
the same codes without it.

bf16; add-norm (RMSNorm with a bf16 residual, residual_out written) at N {4096, 8192} and act-mul (SiLU, packed [rows, 2N] input) at
N {11008, 14336}, rows {128, 8192, 65536}, row and group mode.  Four contenders per point, alternated in the same run on the same
tensors:
    (a) 16-bit op + eager   the 16-bit op, then torch: amax, division, clamp, cast (what a user runs today)
    (b) 16-bit op + quant   the 16-bit op, then quant_fp8
    (c) fused               add_norm_quant / act_and_mul_quant
    (d) 16-bit op alone     add_norm_forward / act_mul_forward (unchanged by this work: profiles/add_norm.txt, profiles/act_mul.txt)
Before anything is timed every point asserts, bit for bit, (c) == (b) for codes, scales and residual_out, and (b)'s codes and scales
== tests/quant_ref.py's on the first and last 64 rows.
Bytes (algorithmic, for the fused forms): the inputs read once, residual_out written once, codes (1 byte an element) and fp32
scales written once.  Rate = bytes / median time, beside the 8 TB/s HBM peak and the 6.45 TB/s fa_merge_states streams at
(profiles/shared_prefix_decode.txt).
Each leg: a warm-up of >= 60 ms of calls, then `--ms` of calls between two device events; the legs alternate `--rounds` times;
median [min .. max] us per call.  Every point runs in a child process of its own under a time limit; the sweep stops at the first
one that fails or runs out of time - nothing is started on a device that has just faulted.
`--wide 1024` runs the act-mul points on `tools/variants/libfa_mi355_quant_wide.so` (FA_QUANT_WIDE_PIECES=1024: rows of more than
8192 columns are owned by 1024 lanes with 2 pieces each instead of 256 lanes with 8), built beforehand, no GPU needed, by
`--build-variants`.

    python tools/quant_sweep.py [--wide 2048|1024] [--only add_norm:8192x4096,act_mul:128x11008,..] [--ms 60] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--ms", type=float, default=60.0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--point-timeout", type=int, default=240)
ap.add_argument("--wide", choices=["2048", "1024"], default="2048")
ap.add_argument("--build-variants", action="store_true", help="build tools/variants/libfa_mi355_quant_wide.so (no GPU needed) and exit")
ap.add_argument("--only", default=None, help="comma-separated points (op : rows x N) instead of the whole list")
ap.add_argument("--point", default=None, help="(child) op : rows x N - measure it and print one JSON line")
args = ap.parse_args()

HBM_PEAK, STREAM = 8.0e12, 6.45e12
POINTS = ([f"add_norm:{rows}x{n}" for n in (4096, 8192) for rows in (128, 8192, 65536)]
          + [f"act_mul:{rows}x{n}" for n in (11008, 14336) for rows in (128, 8192, 65536)])
MODES = ("row", "group")
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "flash-attention-v100_amd")
VARIANT = os.path.join(HERE, "variants", "libfa_mi355_quant_wide.so")


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
    import quant_ref as R
    from flash_attn_mi355 import act_mul as M
    from flash_attn_mi355 import add_norm as A
    from flash_attn_mi355 import quant as Q
    op, _, shape = name.partition(":")
    rows, N = (int(v) for v in shape.split("x"))
    bf, f8 = torch.bfloat16, torch.float8_e4m3fn
    gd = torch.Generator(device="cuda").manual_seed(rows + N)
    rnd = lambda *s: torch.empty(*s, device="cuda", dtype=torch.float32).normal_(generator=gd)      # noqa: E731
    if op == "add_norm":
        x, res = rnd(rows, N).to(bf), (rnd(rows, N) * 3).to(bf)
        w = (1 + 0.1 * rnd(N)).to(bf)
        plain = lambda: A.add_norm_forward(x, w, None, res)                                          # noqa: E731
        fused = lambda mode: Q.add_norm_quant(x, res, w, mode=mode)                                  # noqa: E731
        in_bytes, extra_out = 2 * rows * N * 2, rows * N * 2
    else:
        x = (rnd(rows, 2 * N) * 2).to(bf)
        plain = lambda: (M.act_mul_forward(x[:, :N], x[:, N:], activation="silu"), None)             # noqa: E731
        fused = lambda mode: Q.act_and_mul_quant(x, activation="silu", mode=mode) + (None,)          # noqa: E731
        in_bytes, extra_out = 2 * rows * N * 2, 0

    def eager(y, mode):
        yf = y.float()
        g = yf.view(rows, -1, 128) if mode == "group" else yf.view(rows, 1, N)
        s = (g.abs().amax(dim=-1, keepdim=True) / 448.0).clamp(min=2.0 ** -64)
        return (g / s).clamp(-448, 448).to(f8).view(rows, N), s

    res_out = {}
    sel = torch.cat([torch.arange(min(64, rows)), torch.arange(max(rows - 64, 0), rows)]).unique().cuda()
    for mode in MODES:
        # the bit-for-bit checks first
        y, ro = plain()
        b = Q.quant_fp8(y, mode=mode)
        c = fused(mode)
        torch.cuda.synchronize()
        R.assert_same(c[0], b[0], f"{name} {mode}: fused codes")
        R.assert_same(c[1], b[1], f"{name} {mode}: fused scales")
        if ro is not None:
            R.assert_same(c[2], ro, f"{name} {mode}: residual_out")
        rc, rs = R.quant_ref(y[sel].cpu(), mode)
        R.assert_same(b[0][sel].cpu(), rc, f"{name} {mode}: codes against the reference")
        R.assert_same(b[1][sel].cpu(), rs, f"{name} {mode}: scales against the reference")
        del b, c, rc, rs, ro
        legs = {"a": lambda: eager(plain()[0], mode), "b": lambda: Q.quant_fp8(plain()[0], mode=mode), "c": lambda: fused(mode),
                "d": plain}
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                times[k].append(_time(fn, args.ms))
        nscales = rows * (N // 128 if mode == "group" else 1)
        res_out[mode] = {"us": {k: [statistics.median(t), min(t), max(t)] for k, t in times.items()},
                         "fused_bytes": in_bytes + extra_out + rows * N + 4 * nscales,
                         "plain_bytes": in_bytes + extra_out + rows * N * 2}
        del y
        torch.cuda.empty_cache()
    print("POINT " + json.dumps({"point": name, "modes": res_out}), flush=True)


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
    print(build.build(defines=["FA_QUANT_WIDE_PIECES=1024"], out=VARIANT))
    return 0


fmt = lambda t: f"{t[0]:8.1f} [{t[1]:8.1f} .. {t[2]:8.1f}]"                          # noqa: E731


def rate(nbytes, us):
    r = nbytes / (us * 1e-6)
    return f"{nbytes / 1e6:8.2f} MB: {r / 1e12:5.2f} TB/s ({100 * r / HBM_PEAK:4.1f} % of peak, {100 * r / STREAM:4.1f} % of the merge stream)"


def main():
    if args.point:
        return point(args.point)
    if args.build_variants:
        return build_variants()
    lib, points = None, POINTS
    if args.wide == "1024":
        lib, points = VARIANT, [p for p in POINTS if p.startswith("act_mul")]
        if not os.path.exists(lib):
            print(f"{lib} is not built (--build-variants)")
            return 1
    print(f"# fp8-e4m3 quantisation behind add_norm (RMSNorm + bf16 residual) and act_mul (SiLU, packed input), bf16; rows wider than "
          f"8 x {args.wide} columns on 1024 lanes; us per call: median [min .. max] of {args.rounds} rounds x {args.ms:.0f} ms, the four "
          f"contenders alternated; (a) 16-bit op + eager torch quantisation, (b) 16-bit op + quant_fp8, (c) fused, (d) 16-bit op alone; "
          f"rate: algorithmic bytes / median, share of {HBM_PEAK / 1e12:.0f} TB/s peak and of {STREAM / 1e12:.2f} TB/s (fa_merge_states); "
          f"(c) == (b) and (b) == the reference asserted bit for bit before timing", flush=True)
    for name in (args.only.split(",") if args.only else points):
        p = run_child(name, lib)
        if p is None:
            return 1
        for mode, m in p["modes"].items():
            us = m["us"]
            print(f"{name} {mode:5s}: (a) {fmt(us['a'])}  (b) {fmt(us['b'])}  (c) {fmt(us['c'])}  (d) {fmt(us['d'])} us | "
                  f"b / c {us['b'][0] / us['c'][0]:5.2f} x, a / c {us['a'][0] / us['c'][0]:5.2f} x, d / c {us['d'][0] / us['c'][0]:5.2f} x", flush=True)
            print(f"    (c) {rate(m['fused_bytes'], us['c'][0])} | (d) {rate(m['plain_bytes'], us['d'][0])}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
