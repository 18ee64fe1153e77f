"""CPU: attention sinks - the fa_ext_params mirror and the five *_ext entry points of the C ABI, their argument checks (no
device work happens before them), the Python argument checks, and the agreement of the two fp64 references of
tests/sink_ref.py ((a) direct, (b) the identity on the oracle) on random cases with rows without keys and extreme sinks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import oracle
from sink_ref import ref_dense, ref_varlen, sink_identity_bhs, sink_identity_thd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_OPS = ["fa_fwd_ext", "fa_varlen_fwd_ext", "fa_fwd_kvcache_ext", "fa_bwd_ext", "fa_varlen_bwd_ext"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


def test_ext_params_mirror_matches_header(lib):
    src = open(os.path.join(ROOT, "include", "fa_mi355.h")).read()
    body = re.search(r"typedef struct fa_ext_params \{(.*?)\} fa_ext_params;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [stmt.split()[-1].lstrip("*") for stmt in body.split(";") if stmt.strip()]
    assert fields == [f[0] for f in lib.FaExtParams._fields_] == ["struct_size", "sinks", "dsinks"]
    assert ctypes.sizeof(lib.FaExtParams) == 24
    # fa_params is untouched: ABI 4, q_descale / o_dtype last
    assert lib.lib.fa_abi_version() == 4
    assert [f[0] for f in lib.FaParams._fields_][-2:] == ["q_descale", "o_dtype"]
    for name in EXT_OPS:
        assert re.search(rf"int {name}\(const fa_params\* p, const fa_ext_params\* ext, void\* stream\);", src), name


def test_ext_symbols_exported(lib):
    for name in EXT_OPS:
        assert hasattr(lib.lib, name), name
        assert name in lib.EXPORTS


def _params(lib, buf, dtype=None):
    p = lib.FaParams()
    addr = (ctypes.addressof(buf) + 15) & ~15
    p.q = p.k = p.v = p.o = p.lse = p.dout = p.softmax_d = addr
    p.batch, p.nheads_q, p.nheads_k, p.head_dim, p.seqlen_q, p.seqlen_k = 1, 2, 2, 64, 4, 4
    p.q_row_stride = p.k_row_stride = p.v_row_stride = p.o_row_stride = p.do_row_stride = 128
    p.q_head_stride = p.k_head_stride = p.v_head_stride = p.o_head_stride = p.do_head_stride = 64
    p.dtype = p.kv_dtype = lib.FA_BF16 if dtype is None else dtype
    p.o_dtype = lib.FA_BF16
    p.softmax_scale = 0.125
    p.window_left = p.window_right = -1
    return p, addr


def test_ext_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * 65536)()

    def fails(op, p, e, match):
        rc = getattr(lib.lib, op)(ctypes.byref(p), ctypes.byref(e), None)
        assert rc != 0, op
        msg = lib.lib.fa_last_error().decode()
        assert re.search(match, msg), (op, rc, msg)
        return rc

    p, addr = _params(lib, buf)
    sinks = addr + 4096
    for op in EXT_OPS:
        e = lib.FaExtParams()
        e.struct_size = 8                                         # too small
        e.sinks = sinks
        assert fails(op, p, e, "struct_size") == -1
        e = lib.FaExtParams()
        e.struct_size = ctypes.sizeof(lib.FaExtParams)
        e.dsinks = sinks                                          # dsinks without sinks
        assert fails(op, p, e, "dsinks") == -1
    for op in ("fa_fwd_ext", "fa_varlen_fwd_ext", "fa_fwd_kvcache_ext"):
        e = lib.ext_params()
        e.sinks, e.dsinks = sinks, sinks + 64                     # dsinks on a forward op
        assert fails(op, p, e, "dsinks") == -1
    for op in EXT_OPS:
        e = lib.ext_params()
        e.sinks = sinks
        pd, _ = _params(lib, buf)
        pd.p_dropout = 0.1
        assert fails(op, pd, e, "sinks.*dropout") == -2
        pm, _ = _params(lib, buf)
        pm.dmask = addr
        assert fails(op, pm, e, "sinks.*dropout") == -2
        p8, _ = _params(lib, buf, dtype=lib.FA_FP8_E4M3)
        assert fails(op, p8, e, "sinks.*fp8") == -2


def test_python_argument_errors_before_allocation():
    import flash_attn_mi355 as fa
    q = torch.zeros(1, 4, 2, 64, dtype=torch.bfloat16)
    k = v = torch.zeros(1, 4, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="shape"):
        fa.flash_attn_sinks_func(q, k, v, torch.zeros(3))
    with pytest.raises(RuntimeError, match="floating"):
        fa.flash_attn_sinks_func(q, k, v, torch.zeros(2, dtype=torch.int32))
    q8 = torch.zeros(1, 4, 2, 64).to(torch.float8_e4m3fn)
    with pytest.raises(RuntimeError, match="fp8"):
        fa.flash_attn_sinks_func(q8, q8, q8, torch.zeros(2))
    cu = torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="dropout"):
        fa.flash_attn_varlen_func(q[0], k[0], v[0], cu, cu, 4, 4, dropout_p=0.1, sinks=torch.zeros(2))
    with pytest.raises(RuntimeError, match="fp8"):
        fa.flash_attn_varlen_func(q8[0], q8[0], q8[0], cu, cu, 4, 4, sinks=torch.zeros(2))
    with pytest.raises(RuntimeError, match="shape"):
        fa.flash_attn_with_kvcache(q, k, v, sinks=torch.zeros(2, 1))
    if torch.cuda.is_available():                                  # (a GPU run: the device check)
        with pytest.raises(RuntimeError, match="device"):
            fa.flash_attn_sinks_func(q.cuda(), k.cuda(), v.cuda(), torch.zeros(2))


def test_sinks_keyword_only_on_varlen_and_kvcache():
    import inspect
    import flash_attn
    import flash_attn_mi355 as fa
    for fn in (flash_attn.flash_attn_varlen_func, flash_attn.flash_attn_with_kvcache):
        prm = inspect.signature(fn).parameters["sinks"]
        assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default is None
    assert "flash_attn_sinks_func" in fa.__all__ and "flash_attn_sinks_func" not in flash_attn.__all__
    assert list(inspect.signature(fa.flash_attn_sinks_func).parameters)[:4] == ["q", "k", "v", "sinks"]


SINK_VALUES = [float("-inf"), -80.0, -30.0, 0.0, 0.7, 30.0, 80.0]


@pytest.mark.parametrize("case", range(6))
def test_direct_and_identity_references_agree(case):
    rng = np.random.default_rng(100 + case)
    B, Hk = 2, 2
    Hq = Hk * int(rng.choice([1, 2]))
    Sq, Sk = [(7, 5), (5, 9), (12, 12), (9, 3), (6, 6), (4, 11)][case]
    D = 16
    causal = bool(case % 2 == 0)
    window = [(-1, -1), (2, 0), (-1, -1), (1, 1), (3, -1), (-1, -1)][case]
    softcap = 0.0 if case < 4 else 5.0
    alibi = torch.from_numpy(rng.uniform(0.1, 0.6, size=Hq)) if case in (2, 5) else None
    q = torch.from_numpy(rng.standard_normal((B, Sq, Hq, D)))
    k = torch.from_numpy(rng.standard_normal((B, Sk, Hk, D)))
    v = torch.from_numpy(rng.standard_normal((B, Sk, Hk, D)))
    sinks = np.array([SINK_VALUES[(case + h) % len(SINK_VALUES)] for h in range(Hq)])
    scale = D ** -0.5
    out_a, lse_a = ref_dense(q, k, v, torch.from_numpy(sinks), scale, causal, window, softcap, alibi)
    t = lambda x: x.numpy().transpose(0, 2, 1, 3)
    o, lse, _ = oracle.attn_fwd(t(q), t(k), t(v), scale, causal=causal, window=window, softcap=softcap,
                                alibi_slopes=None if alibi is None else alibi.numpy())
    # (the oracle's LSE is fp32: compare at fp32 resolution)
    out_b, lse_b = sink_identity_bhs(o, lse.astype(np.float64), sinks)
    np.testing.assert_allclose(t(out_a.detach()), out_b, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(lse_a.detach().numpy(), lse_b, rtol=1e-6, atol=1e-5)
    assert np.isfinite(out_b).all()
    # rows without keys: out 0, LSE = s_h
    no_keys = np.isneginf(lse)
    if no_keys.any():
        assert np.all(out_b[no_keys] == 0)
        assert np.array_equal(lse_b[no_keys], np.broadcast_to(sinks[None, :, None], lse.shape)[no_keys])
    # a sink of +inf: out 0, LSE +inf; +80: out ~ 0 and a finite LSE ~ 80
    s2 = sinks.copy()
    s2[0] = np.inf
    out_c, lse_c = sink_identity_bhs(o, lse.astype(np.float64), s2)
    out_d, lse_d = ref_dense(q, k, v, torch.from_numpy(s2), scale, causal, window, softcap, alibi)
    assert np.all(out_c[:, 0] == 0) and np.all(np.isposinf(lse_c[:, 0]))
    assert torch.all(out_d[:, :, 0] == 0) and torch.all(torch.isposinf(lse_d[:, 0]))


def test_sink_minus_inf_is_no_sink_and_varlen_matches():
    rng = np.random.default_rng(7)
    cu = [0, 3, 3, 9]
    cuk = [0, 5, 6, 8]
    Hq, Hk, D = 4, 2, 8
    q = torch.from_numpy(rng.standard_normal((9, Hq, D)))
    k = torch.from_numpy(rng.standard_normal((8, Hk, D)))
    v = torch.from_numpy(rng.standard_normal((8, Hk, D)))
    sinks = np.array([-np.inf, 0.3, 80.0, -2.0])
    o_a, l_a = ref_varlen(q, k, v, cu, cuk, torch.from_numpy(sinks), 0.3, causal=True)
    o, lse = oracle.varlen_fwd(q.numpy(), k.numpy(), v.numpy(), np.array(cu), np.array(cuk), 6, 5, 0.3, causal=True)
    o_b, l_b = sink_identity_thd(o, lse.astype(np.float64), sinks)
    np.testing.assert_allclose(o_a.numpy(), o_b, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(l_a.numpy(), l_b, rtol=1e-6, atol=1e-5)
    # the -inf head is the oracle's result unchanged
    np.testing.assert_array_equal(o_b[:, 0], o[:, 0])
    np.testing.assert_array_equal(l_b[0], lse[0].astype(np.float64))


def test_direct_reference_gradient_of_sinks():
    """(a)'s autograd dsinks equals the closed form -sum exp(s - LSE) D with D = rowsum(dO o O)."""
    rng = np.random.default_rng(3)
    q = torch.from_numpy(rng.standard_normal((2, 6, 4, 8)))
    k = torch.from_numpy(rng.standard_normal((2, 4, 2, 8)))
    v = torch.from_numpy(rng.standard_normal((2, 4, 2, 8)))
    s = torch.tensor([0.5, -1.0, 2.0, 0.0], dtype=torch.float64, requires_grad=True)
    out, lse = ref_dense(q, k, v, s, 0.35, causal=True)
    do = torch.from_numpy(rng.standard_normal(out.shape))
    (ds,) = torch.autograd.grad(out, s, do)
    Dr = (do * out).sum(-1).permute(0, 2, 1)                       # [B, H, S]
    closed = -(torch.exp(s.view(1, -1, 1) - lse) * Dr).sum((0, 2))
    torch.testing.assert_close(ds, closed.detach(), rtol=1e-10, atol=1e-12)
