"""GPU: a fixed sample of the seeded differential fuzz of the grouped expert GEMM family (tests/moe_gemm_fuzz.py) - moe_gemm,
moe_gemm_glu, moe_gemm_wgrad, moe_gemm_mxfp4 and moe_gemm_mxfp4_glu bit for bit against fp64 on witness data, and against each
other on random data.  tests/test_moe_gemm_fuzz_cpu.py asserts what this sample covers.
Larger sweeps: `python tests/moe_gemm_fuzz.py --kind gemm --seed 7 --n 400` (profiles/moe_gemm_fuzz.txt records one)."""
import pytest

import moe_gemm_fuzz as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", F.KINDS)
def test_random_cases_agree_bit_for_bit(kind):
    F.run(kind, F.SAMPLE_SEED, F.SAMPLE_N[kind])


# cases that larger sweeps logged, pinned by (kind, seed, i): none so far
@pytest.mark.parametrize("kind,seed,i", [])
def test_logged_failures_agree(kind, seed, i):
    print(F.run_one(kind, seed, i))
