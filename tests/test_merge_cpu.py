"""CPU: the C ABI of fa_merge_states (struct mirror, every rejection before any launch) and the merge rule itself - the fp64
statement in merge_ref.py against the oracle's attention over the concatenated keys."""
import ctypes

import numpy as np
import pytest

import oracle
from oracle.attention import score_matrix
from merge_ref import merge_ref, merge_ref_bshd


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


def test_ctypes_struct_matches_the_library(lib):
    assert ctypes.sizeof(lib.FaMergeParams) == lib.lib.fa_merge_params_size()
    assert ctypes.sizeof(lib.FaMergeState) == 64 and lib.FA_MERGE_MAX_PARTS == 8
    assert "fa_merge_states" in lib.EXPORTS and "fa_merge_params_size" in lib.EXPORTS
    assert lib.FaMergeParams._fields_[0][0] == "struct_size"           # first, as in fa_ext_params
    assert lib.lib.fa_abi_version() == 4                               # additive: the ABI version did not move


def _valid(lib, n=2, D=64, dtype=None):
    """a block that passes every check (host addresses: nothing may be launched from it); returns (params, keep-alive)"""
    buf = (ctypes.c_char * 8192)()
    base = (ctypes.addressof(buf) + 15) & ~15
    m = lib.FaMergeParams()
    m.struct_size = ctypes.sizeof(lib.FaMergeParams)
    m.n_parts, m.batch, m.seqlen, m.nheads, m.head_dim = n, 1, 2, 2, D
    m.dtype = lib.FA_BF16 if dtype is None else dtype
    for i in range(n + 1):
        st = m.out if i == n else m.parts[i]
        st.o, st.lse = base + 256 * i, base + 4096 + 64 * i
        st.o_batch_stride, st.o_row_stride, st.o_head_stride = 2 * 2 * D, 2 * D, D
        st.lse_batch_stride, st.lse_head_stride, st.lse_row_stride = 4, 2, 1
    return m, buf


def _rejected(lib, m, match):
    rc = lib.lib.fa_merge_states(ctypes.byref(m), None)
    assert rc == -1, rc
    msg = lib.lib.fa_last_error().decode()
    assert msg and match in msg, msg
    with pytest.raises(RuntimeError, match=match):
        lib.call_merge(m, 0)


def test_every_rejection_without_a_device(lib):
    m, _k = _valid(lib)
    m.struct_size -= 8
    _rejected(lib, m, "struct_size")
    for n in (0, 1, 9, -3):
        m, _k = _valid(lib)
        m.n_parts = n
        _rejected(lib, m, "n_parts")
    for field in ("o", "lse"):
        for which in ("part0", "part1", "out"):
            m, _k = _valid(lib)
            st = m.out if which == "out" else m.parts[int(which[-1])]
            setattr(st, field, None)
            _rejected(lib, m, "NULL")
    for D in (0, 4, 12, 100, 264, -8):
        m, _k = _valid(lib)
        m.head_dim = D
        _rejected(lib, m, "head_dim")
    for dt in (lib.FA_FP8_E4M3, 7, -1):
        m, _k = _valid(lib, dtype=dt)
        _rejected(lib, m, "fp16 or bf16")
    for which in ("part1", "out"):
        m, _k = _valid(lib)
        st = m.out if which == "out" else m.parts[1]
        st.lse += 2
        _rejected(lib, m, "4-byte aligned")
    for field in ("o", "lse"):                       # in-place merges: the output's base equals a part's
        for p in (0, 2):
            m, _k = _valid(lib, n=3)
            setattr(m.out, field, getattr(m.parts[p], field))
            _rejected(lib, m, "alias")
    m, _k = _valid(lib)                              # an o that is not even 8-byte aligned (base, then a stride)
    m.parts[0].o += 4
    _rejected(lib, m, "multiple of 8 bytes")
    m, _k = _valid(lib)
    m.out.o_row_stride += 2
    _rejected(lib, m, "multiple of 8 bytes")
    m, _k = _valid(lib)
    m.batch = -1
    _rejected(lib, m, "non-negative")
    assert lib.lib.fa_merge_states(None, None) == -1


def test_an_empty_problem_is_accepted_without_a_launch(lib):
    m, _k = _valid(lib)
    m.seqlen = 0
    assert lib.lib.fa_merge_states(ctypes.byref(m), None) == 0


def test_python_layer_rejects_cpu_tensors_and_bad_lists(lib):
    import torch
    from flash_attn_mi355 import cascade
    import flash_attn
    import flash_attn_mi355
    o, l = torch.zeros(1, 2, 2, 64, dtype=torch.bfloat16), torch.zeros(1, 2, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        cascade.merge_attention_states([o, o], [l, l])
    with pytest.raises(RuntimeError, match="GPU"):
        cascade.flash_attn_with_shared_prefix(o, o[0], o[0], o, o)
    # additive: nothing joins the pinned export lists
    for name in ("merge_attention_states", "flash_attn_with_shared_prefix"):
        assert name not in flash_attn.__all__ and name not in flash_attn_mi355.__all__ and hasattr(cascade, name)


def test_fake_op_gives_the_shapes_without_a_device(lib):
    import torch
    import flash_attn_mi355.torch_ops  # noqa: F401
    outs = [torch.empty(2, 3, 4, 64, dtype=torch.float16, device="meta") for _ in range(3)]
    lses = [torch.empty(2, 4, 3, dtype=torch.float32, device="meta") for _ in range(3)]
    out, lse = torch.ops.flash_attn_mi355.merge_states(outs, lses)
    assert out.shape == (2, 3, 4, 64) and out.dtype == torch.float16
    assert lse.shape == (2, 4, 3) and lse.dtype == torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# the merge rule
# ---------------------------------------------------------------------------------------------------------------------
def _attn64(q, k, v, scale, wr, softcap=0.0):
    """oracle.attn_fwd on [B, H, S, D] with a right window `wr` (-1: none) and fp64 LSEs: the oracle returns its LSE in fp32, which
    would cap the identity below at 1e-7.  Built from the oracle's own score_matrix and checked against attn_fwd right here."""
    B, Hq, Sq, D = q.shape
    G = Hq // k.shape[1]
    out, lse = np.zeros((B, Hq, Sq, v.shape[3])), np.full((B, Hq, Sq), -np.inf)
    for b in range(B):
        for h in range(Hq):
            s, vis = score_matrix(q[b, h], k[b, h // G], scale, False, -1, wr, softcap, None)
            m = np.where(vis.any(axis=1), np.max(s, axis=1, initial=-np.inf), 0.0)
            e = np.where(vis, np.exp(s - m[:, None]), 0.0)
            l = e.sum(axis=1)
            has = l > 0
            out[b, h] = (e / np.where(has, l, 1.0)[:, None]) @ v[b, h // G]
            lse[b, h] = np.where(has, m + np.log(np.where(has, l, 1.0)), -np.inf)
    o_ref, lse_ref, _ = oracle.attn_fwd(q, k, v, scale, window=(-1, wr), softcap=softcap, normalize=False)
    assert np.abs(out - o_ref).max() <= 1e-14 and np.array_equal(lse.astype(np.float32), lse_ref)
    return out, lse


@pytest.mark.parametrize("Sq,Sk,cuts,Hq,Hk,softcap", [
    (5, 9, (6,), 4, 2, 0.0),             # keys 6 .. 8 under the causal mask: rows 0 and 1 see none of the second part
    (7, 7, (2, 4), 2, 2, 0.0),           # three parts; the first rows see only the first
    (3, 40, (17,), 6, 2, 15.0),          # every row sees both parts, softcap
    (6, 6, (1, 2, 3, 4, 5), 2, 1, 0.0),  # six one-key parts
])
def test_split_identity_against_the_oracle(Sq, Sk, cuts, Hq, Hk, softcap):
    """attention over [K1; K2; ...] = merge of attention over K1, K2, ... to 1e-12, rows without a visible key in a part included.
    The full problem is bottom-right causal; a part holding keys [a, b) sees it as a right window of Sk - b keys."""
    rng = np.random.default_rng(Sq * 100 + Sk)
    B, D = 2, 16
    q = rng.standard_normal((B, Hq, Sq, D))
    k = rng.standard_normal((B, Hk, Sk, D))
    v = rng.standard_normal((B, Hk, Sk, D))
    scale = D ** -0.5
    o_full, lse_full = _attn64(q, k, v, scale, 0, softcap)
    o_causal, lse_causal, _ = oracle.attn_fwd(q, k, v, scale, causal=True, softcap=softcap)
    assert np.array_equal(o_full, o_causal) or np.abs(o_full - o_causal).max() <= 1e-14     # (a window of 0 IS the causal mask)
    edges = (0,) + tuple(cuts) + (Sk,)
    parts = [_attn64(q, k[:, :, a:b], v[:, :, a:b], scale, Sk - b, softcap) for a, b in zip(edges[:-1], edges[1:])]
    dead = sum(int(np.isneginf(l).sum()) for _, l in parts)
    if softcap == 0.0:
        assert dead > 0                                                   # the cases are built to contain such rows
    out, lse = merge_ref([o for o, _ in parts], [l for _, l in parts])
    assert np.abs(out - o_full).max() <= 1e-12
    assert np.abs(lse - lse_full).max() <= 1e-12
    assert np.abs(lse - lse_causal).max() <= 1e-5                          # (the oracle's own fp32 LSE)
    # a dead part may hold anything: NaN in its out changes nothing
    poisoned = [np.where(np.isneginf(l)[..., None], np.nan, o) for o, l in parts]
    out2, lse2 = merge_ref(poisoned, [l for _, l in parts])
    assert np.array_equal(out2, out) and np.array_equal(lse2, lse)


def test_merge_rule_edge_rows():
    o = [np.full((1, 2, 4), 3.0), np.full((1, 2, 4), np.nan), np.full((1, 2, 4), -5.0)]
    l = [np.array([[0.5, -np.inf]]), np.array([[-np.inf, -np.inf]]), np.array([[-np.inf, -np.inf]])]
    out, lse = merge_ref(o, l)
    assert np.array_equal(out[0, 0], np.full(4, 3.0)) and lse[0, 0] == 0.5          # one finite part: that part
    assert np.array_equal(out[0, 1], np.zeros(4)) and np.isneginf(lse[0, 1])        # none: 0 / -inf
    ob, lb = merge_ref_bshd([np.swapaxes(x[None], 1, 2) for x in o], [x[None] for x in l])
    assert ob.shape == (1, 2, 1, 4) and lb.shape == (1, 1, 2) and np.array_equal(ob[0, :, 0], out[0])


def test_merge_ref_agrees_with_merge_attention_shards():
    """the torch merge of the context-parallel wrapper keeps its implementation; both state the same rule"""
    import torch
    from flash_attn_mi355.sharding import merge_attention_shards
    rng = np.random.default_rng(5)
    outs = [rng.standard_normal((2, 3, 4, 8)) for _ in range(3)]
    lses = [rng.standard_normal((2, 4, 3)) * 3 for _ in range(3)]
    lses[1][0, 1, :] = -np.inf
    lses[0][1, :, 2] = lses[1][1, :, 2] = lses[2][1, :, 2] = -np.inf
    ref_o, ref_l = merge_ref_bshd(outs, lses)
    got_o, got_l = merge_attention_shards([torch.from_numpy(o).float() for o in outs], [torch.from_numpy(x).float() for x in lses])
    assert np.abs(got_o.double().numpy() - ref_o).max() <= 1e-5
    assert np.array_equal(np.isneginf(got_l.numpy()), np.isneginf(ref_l))
    fin = np.isfinite(ref_l)
    assert np.abs(got_l.double().numpy()[fin] - ref_l[fin]).max() <= 1e-5
