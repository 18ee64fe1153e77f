"""CPU: the fp64 oracle against the reference's host C++ check functions (`cpu_attention_forward`, which returns O and
LSE = max + logf(sum_exp), and `cpu_attention_backward`, in the reference's utils/sass/mma_kernel/backward_kernel.cu).

tests/golden/make_golden.py ran them (oracle/ref_hostcpp.py cuts them out by name and compiles them) on inputs that are
exact in fp16 and bf16 and stored what they returned in tests/golden/hostcpp_*.npz.  This is the pin of the oracle's LSE -
every GPU LSE assertion compares a kernel with the oracle - and a second pin of its gradients, independent of test.py's
`ref_mha_backward` (tests/test_oracle_golden.py).  Only the fixtures are read here.

Gates: O 2e-6 and gradients 2e-5, as tests/test_oracle_golden.py holds the same fp32-against-fp64 comparison to; LSE 4e-6 =
8 fp32 ulps at values in [4, 8) (ulp 4.8e-7), which covers expf, logf and a sequential fp32 sum of at most 300 terms.
"""
import glob
import os

import numpy as np
import pytest
import torch

import oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLD, "hostcpp_*.npz")))
GATE = {"o": 2e-6, "lse": 4e-6, "dq": 2e-5, "dk": 2e-5, "dv": 2e-5}
# the shapes and masks the fixtures must cover: (M, N, D, causal)
CASES = {(128, 128, 128, False), (128, 128, 128, True), (200, 200, 64, True), (130, 130, 256, True), (65, 65, 40, True),
         (192, 192, 96, False), (77, 300, 128, False), (300, 129, 64, False), (1, 65, 64, False)}


def _oracle(g, o_saved=None):
    """The oracle's o, lse, dq, dk, dv on a fixture's inputs; the backward gets the fixture's fp32 O as the saved output, as
    the host C++ takes D_row from its own."""
    q, k, v, do = (g[n].astype(np.float64) for n in ("q", "k", "v", "do"))
    scale, causal = float(g["scale"]), bool(g["causal"])
    # top-left causal mask, only used with M == N, where it is the bottom-right one
    o, lse, _ = oracle.attn_fwd(q, k, v, scale, causal=causal, normalize=False)
    dq, dk, dv, _ = oracle.attn_bwd(do, q, k, v, g["o"] if o_saved is None else o_saved, lse, scale, causal=causal,
                                    normalize=False)
    return {"o": o, "lse": lse.astype(np.float64), "dq": dq, "dk": dk, "dv": dv}


def _misses(res, g):
    """names of the outputs outside their gate, with the worst difference"""
    bad = {}
    for n, gate in GATE.items():
        assert res[n].shape == g[n].shape, (n, res[n].shape, g[n].shape)
        d = float(np.abs(res[n] - g[n].astype(np.float64)).max())
        if not d < gate:
            bad[n] = d
    return bad


def test_fixture_set_is_complete():
    got = set()
    for p in FIXTURES:
        g = np.load(p)
        got.add((g["q"].shape[2], g["k"].shape[2], g["q"].shape[3], bool(g["causal"])))
    assert got == CASES


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_oracle_matches_host_cpp(path):
    g = np.load(path)
    assert _misses(_oracle(g), g) == {}


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_comparison_is_decisive(path):
    """the same comparison refuses an LSE off by 2e-5 or in base 2, a dS without `scale` and a D_row from a zero O"""
    g = np.load(path)
    good = _oracle(g)
    assert set(_misses(dict(good, lse=good["lse"] + 2e-5), g)) == {"lse"}
    assert set(_misses(dict(good, lse=good["lse"] / np.log(2.0)), g)) == {"lse"}
    # dS = P (dP - D) * scale feeds dQ = dS K and dK = dS^T Q, both linear in it; dV does not see it
    s = float(g["scale"])
    assert set(_misses(dict(good, dq=good["dq"] / s, dk=good["dk"] / s), g)) == {"dq", "dk"}
    # D_row = rowsum(O * dO).  The non-causal 128^3 fixture alone cannot see it: its inputs are the reference file's own
    # +-0.1 range, O is a mean of 128 such values, and dropping D_row moves dQ by 1.3e-5 and dK by 5.4e-6 (of gradients up
    # to 0.02), inside the 2e-5 gate.  Its causal twin (short rows: 8e-4) and every randn-scale fixture (0.03 .. 2.7) see it.
    if float(np.abs(g["q"]).max()) > 0.1 or bool(g["causal"]):
        assert set(_misses(_oracle(g, o_saved=np.zeros_like(g["o"])), g)) == {"dq", "dk"}


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_fixture_hygiene(path):
    g = np.load(path)
    assert set(g.files) == {"q", "k", "v", "do", "o", "lse", "dq", "dk", "dv", "scale", "causal"}
    M, N, D = g["q"].shape[2], g["k"].shape[2], g["q"].shape[3]
    assert g["q"].shape == g["do"].shape == g["o"].shape == g["dq"].shape == (1, 1, M, D)
    assert g["k"].shape == g["v"].shape == g["dk"].shape == g["dv"].shape == (1, 1, N, D)
    assert g["lse"].shape == (1, 1, M)
    assert not bool(g["causal"]) or M == N      # the host C++ masks top-left
    for n in ("q", "k", "v", "do"):             # both kernel dtypes see the very numbers the C++ saw
        assert g[n].dtype == np.float16
        t = torch.from_numpy(g[n].astype(np.float32))
        assert torch.equal(t.to(torch.float16).float(), t) and torch.equal(t.to(torch.bfloat16).float(), t), n
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert g[n].dtype == np.float32 and np.isfinite(g[n]).all(), n
    assert os.path.getsize(path) < 1 << 20
