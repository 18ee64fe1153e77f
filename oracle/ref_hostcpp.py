"""Build and run the reference's host C++ attention check (TEST INFRASTRUCTURE ONLY, build container only).

The reference tree carries a plain host-side forward and backward over std::vector<float> with free M, N, D, scale and
causal - `cpu_attention_forward` (O and LSE = max + logf(sum_exp)) and `cpu_attention_backward` - in
utils/sass/mma_kernel/backward_kernel.cu.  They are the only place the reference states an LSE, and a gradient
formulation independent of test.py's.  This module

  1. reads that file at run time and cuts the two functions out BY NAME with brace matching,
  2. writes them, next to a copy of the project's own harness oracle/ref_hostcpp_main.cpp, to oracle/_ref/ (ignored by
     git: no reference text is ever committed),
  3. compiles with  g++ -O2 -ffp-contract=off  (no fused multiply-adds, so the results do not depend on the host's ISA
     and the fixtures regenerate byte for byte),
  4. runs the binary on inputs that come from Python.

tests/golden/make_golden.py uses it to write the hostcpp_*.npz fixtures.  Nothing that runs on a GPU machine - no test,
smoke() or bench.py - imports this module: the tests read the fixtures only.
"""
import os
import shutil
import subprocess
import tempfile

import numpy as np

REF = "/root/reference"
REF_FILE = os.path.join(REF, "utils", "sass", "mma_kernel", "backward_kernel.cu")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "_ref")
HARNESS = os.path.join(HERE, "ref_hostcpp_main.cpp")
FUNCTIONS = ("cpu_attention_backward", "cpu_attention_forward")
CXXFLAGS = ("-O2", "-ffp-contract=off", "-std=c++14")


def cut_function(src, name):
    """The text of the definition `void <name>(...) {...}` in `src`, found by name and brace matching."""
    start = src.find(f"void {name}(")
    if start < 0:
        raise RuntimeError(f"{name} not found in {REF_FILE}")
    if src.find(f"void {name}(", start + 1) >= 0:
        raise RuntimeError(f"{name} is defined more than once in {REF_FILE}")
    # the parameter list, then the body (the functions hold no braces in strings, character literals or comments)
    depth, i = 0, src.index("(", start)
    while True:
        depth += {"(": 1, ")": -1}.get(src[i], 0)
        i += 1
        if depth == 0:
            break
    body = src.index("{", i)
    if src[i:body].strip():
        raise RuntimeError(f"{name}: a declaration, not a definition")
    depth, i = 0, body
    while True:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
        if depth == 0:
            return src[start:i]


def build():
    """Cut, write and compile; returns the path of the binary under oracle/_ref/."""
    if not os.path.isfile(REF_FILE):
        raise SystemExit(f"oracle/ref_hostcpp.py: the reference tree is not present ({REF_FILE}); "
                         "this recipe runs in the build container only")
    cxx = shutil.which("g++")
    if cxx is None:
        raise SystemExit("oracle/ref_hostcpp.py: g++ not found")
    src = open(REF_FILE).read()
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, "ref_hostcpp_cut.inc"), "w") as f:
        f.write("\n\n".join(cut_function(src, n) for n in FUNCTIONS) + "\n")
    shutil.copyfile(HARNESS, os.path.join(OUT_DIR, "ref_hostcpp_main.cpp"))
    exe = os.path.join(OUT_DIR, "ref_hostcpp")
    subprocess.run([cxx, *CXXFLAGS, "-o", exe, os.path.join(OUT_DIR, "ref_hostcpp_main.cpp")], check=True)
    return exe


def run(exe, q, k, v, do, scale, causal):
    """q, do [M,D], k, v [N,D] -> dict of fp32 arrays o [M,D], lse [M], dq [M,D], dk, dv [N,D]."""
    q, k, v, do = (np.ascontiguousarray(x, dtype=np.float32) for x in (q, k, v, do))
    (M, D), N = q.shape, k.shape[0]
    assert k.shape == (N, D) and v.shape == (N, D) and do.shape == (M, D)
    with tempfile.TemporaryDirectory(dir=OUT_DIR) as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            for x in (q, k, v, do):
                f.write(x.tobytes())
        # %.9g round-trips an fp32 value through strtof
        subprocess.run([exe, str(M), str(N), str(D), "%.9g" % np.float32(scale), str(int(bool(causal))), fin, fout],
                       check=True)
        raw = np.fromfile(fout, dtype=np.float32)
    sizes = (("o", (M, D)), ("lse", (M,)), ("dq", (M, D)), ("dk", (N, D)), ("dv", (N, D)))
    assert raw.size == sum(int(np.prod(s)) for _, s in sizes), raw.size
    res, at = {}, 0
    for name, shape in sizes:
        n = int(np.prod(shape))
        res[name] = raw[at:at + n].reshape(shape).copy()
        at += n
    return res


if __name__ == "__main__":
    print(build())
