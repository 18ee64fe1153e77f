"""CPU: tree attention masks of the kv-cache op - the fa_tree_params mirror and the fa_fwd_kvcache_tree entry point, every
argument check of the C ABI (reached without a device), FA_FLAG_TREE_MASK and the workspace query, the Python argument
checks, the fake implementation of the torch.library op, and the agreement of the two fp64 references of tests/tree_ref.py
((a) direct, (b) the ancestor-chain identity on the oracle) on random trees."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import tree_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


def test_tree_params_mirror_matches_header(lib):
    src = open(os.path.join(ROOT, "include", "fa_mi355.h")).read()
    body = re.search(r"typedef struct fa_tree_params \{(.*?)\} fa_tree_params;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [stmt.split()[-1].lstrip("*") for stmt in body.split(";") if stmt.strip()]
    assert fields == [f[0] for f in lib.FaTreeParams._fields_] == [
        "struct_size", "mask", "mask_batch_stride", "mask_words", "depths", "depths_batch_stride"]
    assert ctypes.sizeof(lib.FaTreeParams) == lib.lib.fa_tree_params_size() == 48
    assert re.search(r"int fa_fwd_kvcache_tree\(const fa_params\* p, const fa_ext_params\* ext, const fa_tree_params\* tree, "
                     r"void\* stream\);", src)
    assert re.search(r"#define FA_FLAG_TREE_MASK 16\b", src) and lib.FA_FLAG_TREE_MASK == 16
    assert hasattr(lib.lib, "fa_fwd_kvcache_tree") and "fa_fwd_kvcache_tree" in lib.EXPORTS
    # additive: the sinks block, fa_params and the ABI version are what they were
    assert ctypes.sizeof(lib.FaExtParams) == 24
    assert lib.lib.fa_abi_version() == 4 == lib.FA_ABI_VERSION
    assert [f[0] for f in lib.FaParams._fields_][-2:] == ["q_descale", "o_dtype"]
    # what the header leaves out of scope is said there
    for words in ("ALiBi", "varlen", "T_q > 64", "backward"):
        assert words in src[src.index("Tree attention masks"):src.index("typedef struct fa_tree_params")], words


def _params(lib, buf, Tq=4, Tn=4, H=2, Hk=2, D=64, S=64):
    p = lib.FaParams()
    addr = (ctypes.addressof(buf) + 15) & ~15
    p.q = p.k = p.v = p.o = p.lse = addr
    p.batch, p.nheads_q, p.nheads_k, p.head_dim, p.seqlen_q, p.seqlen_k = 1, H, Hk, D, Tq, S
    p.q_row_stride = p.o_row_stride = H * D
    p.k_row_stride = p.v_row_stride = Hk * D
    p.q_head_stride = p.k_head_stride = p.v_head_stride = p.o_head_stride = D
    p.k_batch_stride = p.v_batch_stride = S * Hk * D
    p.dtype = p.kv_dtype = lib.FA_BF16
    p.softmax_scale = 0.125
    p.window_left = p.window_right = -1
    p.cache_seqlens = addr
    if Tn:
        p.k_new = p.v_new = addr
        p.knew_row_stride = p.vnew_row_stride = Hk * D
        p.knew_head_stride = p.vnew_head_stride = D
        p.seqlen_new = Tn
    p.flags = lib.FA_FLAG_TREE_MASK
    return p, addr


def _tree(lib, addr, Tq=4, depths=False):
    t = lib.FaTreeParams()
    t.struct_size = ctypes.sizeof(lib.FaTreeParams)
    t.mask = addr + 4096
    t.mask_words = (Tq + 31) // 32
    if depths:
        t.depths = addr + 8192
    return t


def test_tree_argument_errors_without_gpu(lib):
    """Every check runs on the host before any device work: the calls below would fault or launch otherwise (the
    pointers name host memory and there may be no device at all)."""
    buf = (ctypes.c_char * 65536)()
    fn = lib.lib.fa_fwd_kvcache_tree

    def fails(p, t, match, code=-1):
        rc = fn(ctypes.byref(p), None, None if t is None else ctypes.byref(t), None)
        msg = lib.lib.fa_last_error().decode()
        assert rc == code and re.search(match, msg), (rc, msg)

    p, addr = _params(lib, buf)
    t = _tree(lib, addr)
    t.struct_size = 8
    fails(p, t, "struct_size")
    # the flag and the block come together
    fails(p, None, "FA_FLAG_TREE_MASK is set but no tree block")
    t = _tree(lib, addr); t.mask = None
    fails(p, t, "FA_FLAG_TREE_MASK is set but no tree block")
    p.flags = 0
    fails(p, _tree(lib, addr), "FA_FLAG_TREE_MASK is not set")
    # ... the flag through the entry points without a tree argument
    p, addr = _params(lib, buf)
    assert lib.lib.fa_fwd_kvcache(ctypes.byref(p), None) == -1
    assert "FA_FLAG_TREE_MASK" in lib.lib.fa_last_error().decode()
    e = lib.ext_params()
    assert lib.lib.fa_fwd_kvcache_ext(ctypes.byref(p), ctypes.byref(e), None) == -1
    # ... on every other op it is an unknown bit, and 64 stays one here
    for op in ("fa_fwd", "fa_varlen_fwd", "fa_bwd", "fa_varlen_bwd"):
        assert getattr(lib.lib, op)(ctypes.byref(p), None) == -1, op
        assert "unknown bits" in lib.lib.fa_last_error().decode(), op
    p.flags = lib.FA_FLAG_TREE_MASK | 64
    fails(p, _tree(lib, addr), "unknown bits")
    p.flags = 64
    fails(p, None, "unknown bits")
    # sizes
    for Tq in (1, 65):
        p, addr = _params(lib, buf, Tq=Tq, Tn=Tq, S=128)
        fails(p, _tree(lib, addr, Tq), r"seqlen_q must be in \[2, 64\]")
    p, addr = _params(lib, buf, Tq=33, Tn=33)
    t = _tree(lib, addr, 33); t.mask_words = 1
    fails(p, t, "mask_words")
    p, addr = _params(lib, buf)
    t = _tree(lib, addr); t.mask_words = 2
    fails(p, t, "mask_words")
    t = _tree(lib, addr); t.mask = addr + 4098
    fails(p, t, "4-byte aligned")
    t = _tree(lib, addr, depths=True); t.depths = addr + 8193
    fails(p, t, "4-byte aligned")
    t = _tree(lib, addr); t.mask_batch_stride = -4
    fails(p, t, "batch strides must be >= 0")
    t = _tree(lib, addr, depths=True); t.depths_batch_stride = -4
    fails(p, t, "batch strides must be >= 0")
    p, addr = _params(lib, buf, Tq=4, Tn=2)
    fails(p, _tree(lib, addr), "seqlen_new must be 0 or seqlen_q")
    for wl, wr in ((8, -1), (-1, 0), (3, 3)):
        p, addr = _params(lib, buf)
        p.window_left, p.window_right = wl, wr
        fails(p, _tree(lib, addr), "window_size")
    p, addr = _params(lib, buf)
    p.alibi_slopes = addr
    fails(p, _tree(lib, addr), "ALiBi", code=-2)
    p, addr = _params(lib, buf)
    p.rotary_cos = p.rotary_sin = addr
    p.rotary_dim, p.seqlen_ro = 32, 64
    fails(p, _tree(lib, addr), "depths are required")


def test_tree_null_block_is_the_ext_op(lib):
    """tree == NULL (or mask == NULL) without the flag: fa_fwd_kvcache_ext's own checks answer, word for word"""
    buf = (ctypes.c_char * 65536)()
    p, addr = _params(lib, buf)
    p.flags = 0
    p.p_dropout = 0.5
    assert lib.lib.fa_fwd_kvcache_ext(ctypes.byref(p), None, None) == -1
    want = lib.lib.fa_last_error().decode()
    assert lib.lib.fa_fwd_kvcache_tree(ctypes.byref(p), None, None, None) == -1
    assert lib.lib.fa_last_error().decode() == want and "dropout" in want
    t = _tree(lib, addr); t.mask = None
    assert lib.lib.fa_fwd_kvcache_tree(ctypes.byref(p), None, ctypes.byref(t), None) == -1
    assert lib.lib.fa_last_error().decode() == want


def test_workspace_query_follows_the_flag(lib):
    """B 16, H 64/8, T_q 64, D 128, bf16 cache: 16 row blocks against 8 general-path passes and 1024 general-path workgroups
    (>= 2 x the CU count of any gfx950 part, 256 without a device) - decode_takes() says no, the general path runs and
    needs no workspace.  With FA_FLAG_TREE_MASK the decode kernels run: 4 requested splits x rows x (D + 1) floats."""
    B, H, Hk, Tq, D, S = 16, 64, 8, 64, 128, 4096
    p = lib.FaParams()
    p.dtype = p.kv_dtype = lib.FA_BF16
    p.batch, p.nheads_q, p.nheads_k, p.seqlen_q, p.seqlen_k, p.head_dim = B, H, Hk, Tq, S, D
    p.q_batch_stride, p.q_row_stride, p.q_head_stride = Tq * H * D, H * D, D
    for n in ("k", "v"):
        setattr(p, n + "_batch_stride", S * Hk * D); setattr(p, n + "_row_stride", Hk * D); setattr(p, n + "_head_stride", D)
    p.is_causal = 1
    p.window_left = p.window_right = -1
    p.seqlen_new = Tq
    p.num_splits = 4
    q = lib.lib.fa_fwd_kvcache_workspace_bytes
    assert q(ctypes.byref(p)) == 0
    p.flags = lib.FA_FLAG_TREE_MASK
    assert q(ctypes.byref(p)) == 4 * B * H * Tq * (D + 1) * 4
    p.num_splits = 1
    assert q(ctypes.byref(p)) == 0


def test_python_argument_errors():
    import flash_attn_mi355 as fa
    f = fa.flash_attn_with_kvcache
    B, T, H, D = 2, 4, 2, 64
    q = torch.zeros(B, T, H, D, dtype=torch.bfloat16)
    kc = torch.zeros(B, 64, H, D, dtype=torch.bfloat16)
    k = torch.zeros(B, T, H, D, dtype=torch.bfloat16)
    m = torch.ones(T, T, dtype=torch.bool).tril()
    sl = torch.zeros(B, dtype=torch.int32)
    cos = torch.zeros(64, 16, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="tree_depths needs tree_mask"):
        f(q, kc, kc, tree_depths=torch.zeros(T, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="shape"):
        f(q, kc, kc, tree_mask=torch.ones(T, T + 1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="shape"):
        f(q, kc, kc, tree_mask=torch.ones(B + 1, T, T, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="shape"):
        f(q, kc, kc, tree_mask=torch.ones(T, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="dtype"):
        f(q, kc, kc, tree_mask=torch.ones(T, T))
    with pytest.raises(RuntimeError, match="2 .. 64"):
        f(q[:, :1], kc, kc, tree_mask=torch.ones(1, 1, dtype=torch.bool))
    q65 = torch.zeros(1, 65, H, D, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="2 .. 64"):
        f(q65, kc[:1], kc[:1], tree_mask=torch.ones(65, 65, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="window_size"):
        f(q, kc, kc, tree_mask=m, window_size=(8, 0))
    with pytest.raises(RuntimeError, match="ALiBi"):
        f(q, kc, kc, tree_mask=m, alibi_slopes=torch.zeros(H))
    with pytest.raises(RuntimeError, match="tokens"):
        f(q, kc, kc, k=k[:, :2], v=k[:, :2], cache_seqlens=sl, tree_mask=m)
    with pytest.raises(RuntimeError, match="needs tree_depths"):
        f(q, kc, kc, k=k, v=k, cache_seqlens=sl, rotary_cos=cos, rotary_sin=cos, tree_mask=m)
    with pytest.raises(RuntimeError, match="int32"):
        f(q, kc, kc, k=k, v=k, cache_seqlens=sl, rotary_cos=cos, rotary_sin=cos, tree_mask=m, tree_depths=torch.zeros(T))
    with pytest.raises(RuntimeError, match="shape"):
        f(q, kc, kc, k=k, v=k, cache_seqlens=sl, rotary_cos=cos, rotary_sin=cos, tree_mask=m,
          tree_depths=torch.zeros(T + 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):                   # (all tree checks passed: the device check answers)
        f(q, kc, kc, k=k, v=k, cache_seqlens=sl, tree_mask=m, causal=True)


def test_keywords_and_plan_key():
    import flash_attn
    import flash_attn_mi355 as fa
    from flash_attn_mi355 import flash_attn_interface as fi
    prm = inspect.signature(flash_attn.flash_attn_with_kvcache).parameters
    for name in ("tree_mask", "tree_depths"):
        assert prm[name].kind is inspect.Parameter.KEYWORD_ONLY and prm[name].default is None
    assert list(prm)[-2:] == ["tree_mask", "tree_depths"] and list(prm)[19:-2] == ["k_descale", "v_descale", "sinks"]
    assert "tree_mask" not in " ".join(flash_attn.__all__) and fa.flash_attn_with_kvcache is flash_attn.flash_attn_with_kvcache
    # a tree call and a causal call of one geometry never share a plan; the mask's and the depths' geometry count
    q = torch.zeros(2, 4, 2, 64, dtype=torch.bfloat16)
    kc = torch.zeros(2, 64, 2, 64, dtype=torch.bfloat16)
    sl = torch.zeros(2, dtype=torch.int32)

    def key(**kw):
        return fi._kv_plan_key(q, kc, kc, q, q, None, None, sl, None, None, None, None, True, (-1, -1), 0.0, True, None, 0,
                               None, None, None, **kw)
    mb = torch.ones(4, 4, dtype=torch.bool)
    d = torch.zeros(4, dtype=torch.int32)
    keys = [key(), key(tree_mask=mb), key(tree_mask=mb.expand(2, 4, 4).contiguous()), key(tree_mask=mb.to(torch.int32)[:, :1].contiguous()),
            key(tree_mask=mb, tree_depths=d), key(tree_mask=mb, tree_depths=d.expand(2, 4).contiguous())]
    assert len(set(keys)) == len(keys)
    assert key(tree_mask=mb.clone()) == key(tree_mask=mb)
    assert key(tree_mask=mb.t()[::1].expand(2, 4, 4)) is None        # (not contiguous: the slow path)


def test_pack_round_trip_and_library_packing():
    from flash_attn_mi355 import flash_attn_interface as fi
    rng = np.random.default_rng(5)
    for T in (2, 7, 31, 32, 33, 63, 64):
        m = rng.random((3, T, T)) < 0.5
        m[0, :, T - 1] = True                                        # (bit 31 / 63: the sign bit of a word)
        w = tr.pack_mask(m)
        assert w.dtype == np.int32 and w.shape == (3, T, (T + 31) // 32)
        assert np.array_equal(tr.unpack_mask(w, T), m)
        got = fi._pack_tree_mask(torch.from_numpy(m))
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), w)
        assert np.array_equal(fi._pack_tree_mask(torch.from_numpy(m[1])).numpy(), w[1])


def test_fake_op_shapes():
    import flash_attn_mi355.torch_ops  # noqa: F401
    op = torch.ops.flash_attn_mi355.fwd_kvcache_tree
    q = torch.empty(3, 8, 8, 128, dtype=torch.float16, device="meta")
    kc = torch.empty(3, 1024, 2, 128, dtype=torch.float16, device="meta")
    kn = torch.empty(3, 8, 2, 128, dtype=torch.float16, device="meta")
    m = torch.empty(8, 8, dtype=torch.bool, device="meta")
    sl = torch.empty(3, dtype=torch.int32, device="meta")
    o, l = op(q, kc, kc.clone(), kn, kn, sl, None, None, None, None, None, m, None, 0.1, 0.0, True, 0)
    assert o.shape == q.shape and o.dtype == q.dtype and l.shape == (3, 8, 8) and l.dtype == torch.float32
    # no existing op's schema changed
    assert "tree" not in str(torch.ops.flash_attn_mi355.fwd_kvcache.default._schema)


@pytest.mark.parametrize("case", range(6))
def test_direct_and_chain_references_agree(case):
    """(a) == (b) on random trees (parent[t] < t): out to 1e-12.  The LSE bound is forced by the oracle: (b) is built on
    oracle.kvcache.kvcache_fwd, which returns its LSE as float32, so the two can only agree to fp32 resolution there (2^-23).  Covers paged and contiguous caches, cache_batch_idx, leftpad, rotary with depth positions, softcap, fp8."""
    rng = np.random.default_rng(40 + case)
    B, Hk, D = 2, 2, 16
    Hq = Hk * [1, 2, 4][case % 3]
    T = [2, 7, 12, 33, 5, 9][case]
    paged = case in (1, 4)
    rot = case in (0, 1, 3, 5)
    fp8 = case == 4
    softcap = 4.0 if case == 2 else 0.0
    Smax = 96
    pars = [tr.random_parents(T, rng) for _ in range(B)]
    mask = np.stack([tr.mask_from_parents(p) for p in pars])
    depths = np.stack([tr.depths_from_parents(p) for p in pars])
    # depth of a node = its chain's length - 1
    assert np.array_equal(depths, mask.sum(-1) - 1)
    if case == 5:
        mask, depths = mask[0], depths[0]                            # one tree for the batch
    r16 = lambda *s: tr.round_to(rng.standard_normal(s), "bf16")
    q, k, v = r16(B, T, Hq, D), r16(B, T, Hk, D), r16(B, T, Hk, D)
    seqlens = np.array([Smax - T - 9, [0, 1, 32, 17, 3, 40][case]], dtype=np.int32)
    lp = np.array([3, 0], dtype=np.int32) if case == 3 else None
    bidx = np.array([2, 0], dtype=np.int32) if case == 2 else None
    bt = None
    if paged:
        page = 16
        pps = Smax // page
        kc, vc = r16(B * pps + 1, page, Hk, D), r16(B * pps + 1, page, Hk, D)
        bt = rng.permutation(B * pps + 1)[: B * pps].reshape(B, pps).astype(np.int32)
    else:
        kc, vc = r16(3 if bidx is not None else B, Smax, Hk, D), r16(3 if bidx is not None else B, Smax, Hk, D)
    kd = vd = None
    if fp8:
        from oracle.kvcache import round_e4m3
        kd, vd = 0.05, 0.04
        kc, vc = round_e4m3(kc / kd), round_e4m3(vc / vd)
    cos = sin = None
    if rot:
        ang = np.arange(Smax + 8)[:, None] / (10000 ** (np.arange(0, 8, 2) / 8))[None, :]
        cos, sin = tr.round_to(np.cos(ang), "bf16"), tr.round_to(np.sin(ang), "bf16")
    kw = dict(rotary_cos=cos, rotary_sin=sin, cache_seqlens=seqlens, cache_batch_idx=bidx, cache_leftpad=lp, block_table=bt,
              softcap=softcap, rotary_interleaved=bool(case % 2), io_dtype="bf16", k_descale=kd, v_descale=vd)
    out_a, lse_a, kc_a, _ = tr.ref_tree(q, kc, vc, mask, k=k, v=v, depths=depths if rot else None, **kw)
    out_b, lse_b = tr.ref_tree_chains(q, kc, vc, mask, k, v, **kw)
    np.testing.assert_allclose(out_a, out_b, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lse_a, lse_b, rtol=2.0 ** -23, atol=2.0 ** -23)
    assert not np.array_equal(kc_a, kc)                              # (the append happened, on a copy)
    # (a) alone: an arbitrary mask with an empty row and no diagonal
    m2 = rng.random((B, T, T)) < 0.4
    m2[:, 0] = False
    sl0 = np.zeros(B, dtype=np.int32)
    out_c, lse_c, _, _ = tr.ref_tree(q, kc, vc, m2, k=k, v=v, depths=depths if rot else None, **{**kw, "cache_seqlens": sl0})
    assert np.all(out_c[:, 0] == 0) and np.all(np.isneginf(lse_c[:, :, 0])) and np.isfinite(out_c).all()
    sinks = rng.standard_normal(Hq)
    _, lse_s, _, _ = tr.ref_tree(q, kc, vc, m2, k=k, v=v, depths=depths if rot else None, sinks=sinks,
                                 **{**kw, "cache_seqlens": sl0})
    assert np.array_equal(lse_s[:, :, 0], np.broadcast_to(sinks, (B, Hq)))
