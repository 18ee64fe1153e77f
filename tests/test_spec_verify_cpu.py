"""CPU: the host side of fa_spec_accept / fa_spec_walk - the fp64 yardstick of tests/spec_verify_ref.py against its emulation of the
device's fp32 roundings on every case the GPU tests run (the margin is not vacuous), the losslessness of the rule on a grid of
uniform numbers, the walk reference against a brute-force enumeration of every tree with T <= 5, commit_slots against a Python
loop, the workspace query (which needs no device), the C ABI's argument checks on host pointers and the ctypes mirrors.  Nothing
here needs a GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import sample_ref as R
import spec_verify_ref as SR


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def spec():
    """(autouse: the reference tests, too, belong to the module they are the yardstick of)"""
    import __graft_entry__ as g
    g.build()
    import flash_attn_mi355.spec_decode as S
    return S


# the yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SR.ACCEPT_V)
def test_margin_reference_equals_the_emulation_on_every_gpu_case(V):
    """for every batch the GPU test runs (same V, same dtype pairs, same seeds): the builder reaches every child node, every
    recover margin is above 1.5, tau >= 1/4 wherever the residual is used, and the fp64 decision, the fp32-emulated decision and
    the builder's planted decision agree"""
    for tdtype, qdtype in SR.dtype_pairs(V):
        c = SR.batch_case(V, tdtype, qdtype)
        B, T, _ = c["target"].shape
        seen, accepts = set(), 0
        for b in range(B):
            par = c["parents"][b].numpy()
            for t in range(1, T):
                if not SR.valid_parent(par, t):
                    assert (int(c["accept"][b, t]), int(c["recovered"][b, t])) == (0, -1)
                    continue
                args = (c["target"][b, int(par[t])], c["draft"][b, t], int(c["draft_ids"][b, t]), float(c["temperature"][b]),
                        float(c["u_accept"][b, t]), float(c["u_recover"][b, t]))
                want = (int(c["accept"][b, t]), int(c["recovered"][b, t]))
                assert SR.accept_ref(*args) == want, (V, b, t)
                assert SR.accept_ref(*args, emulate=True) == want, (V, b, t)
                seen.add(want[1])
                accepts += want[0]
        assert seen >= set(SR.plants(V)) or V == 1                # the recovered token visits every plant
        assert 0 < accepts < 3 * (T - 1) - 1                      # both sides of the accept test


def test_margin_formula():
    assert SR.DELTA_P == 2.0 ** -13 and SR.margin_r(151936, 0.25) < 2.0 ** -9
    assert SR.margin_r(1 << 20, 0.25) == 8 * (2.0 ** -13 + 2.0 ** -20)
    row = SR.target_row(264, torch.float32, 3)
    q = SR.draft_row(row, 1.0, torch.float32, 0, 263, True)
    with pytest.raises(AssertionError, match="range"):
        SR.build(row * 10, q, 263, 1.0, want_accept=True)
    with pytest.raises(AssertionError, match="tau"):              # q = 0.9 p: tau = 0.1
        SR.build(row, torch.from_numpy(0.9 * SR.probs(R.values(row), 1.0)[0]), 5, 1.0, want_accept=True)


def test_reference_rules_on_exact_cases():
    """the cases that need no margin"""
    t = torch.tensor([0.0, 1.0, 2.0, 1.0])
    p, _ = SR.probs(R.values(t), 1.0)
    onehot = torch.tensor([0.0, 0.0, 1.0, 0.0])                   # residual = p with d = 2 removed
    for u, want in ((0.0, 0), (1 - 2.0 ** -24, 3), (1.0, 3), (float("nan"), 0), (-1.0, 0)):
        assert SR.accept_ref(t, onehot, 2, 1.0, 0.999, u) == (0, want)
    assert SR.accept_ref(t, onehot, 2, 1.0, float(p[2]) * 0.99, 0.5)[0] == 1
    ones = torch.ones(4)                                          # R == 0: the fallback draw over the target's own masses
    assert SR.accept_ref(t, ones, 2, 1.0, 0.9, 0.0) == (0, 0) and SR.accept_ref(t, ones, 2, 1.0, 0.9, 1.0) == (0, 3)
    assert SR.accept_ref(t, ones, 2, 1.0, 0.0, 0.5)[0] == 1       # uu = 0: 0 < p_d
    assert SR.accept_ref(t, ones, 2, 1.0, float("nan"), 0.5)[0] == 1
    for d in (-1, 4):
        assert SR.accept_ref(t, onehot, d, 1.0, 0.0, 0.0)[0] == 0
    for T in (0.0, -1.0, float("nan")):                           # greedy: the first maximum, q and u are not read
        assert SR.accept_ref(t, ones * float("nan"), 2, T, float("nan"), float("nan")) == (1, 2)
        assert SR.accept_ref(t, ones, 1, T, 0.0, 0.0) == (0, 2)
    assert SR.accept_ref(torch.full((4,), float("-inf")), ones, 0, 1.0, 0.0, 0.0) == (0, -1)
    inf = torch.tensor([0.0, float("inf"), 1.0, float("inf")])
    assert SR.accept_ref(inf, ones, 1, 1.0, 0.9, 0.9) == (1, 1) and SR.accept_ref(inf, ones, 3, 1.0, 0.0, 0.0) == (0, 1)
    filt = torch.tensor([float("-inf"), 1.0, float("-inf"), 1.0])  # a filtered row: p = (0, 1/2, 0, 1/2)
    assert SR.accept_ref(filt, onehot, 2, 1.0, 0.0, 0.6) == (0, 3)  # p_d = 0: 0 < 0 is a reject even at u = 0
    nanq = torch.tensor([float("nan"), 0.0, 0.0, 0.0])
    assert SR.accept_ref(t, nanq, 0, 1.0, 0.5, 0.0) == (0, 1)     # a NaN q_d rejects and its residual counts as 0


def test_the_rule_is_lossless_on_a_grid():
    """one V = 8 row pair, a G x G midpoint grid of (u_accept, u_recover), every d weighted by q_d: the emitted-token frequencies
    reproduce p.  The tolerance, from the grid geometry: per d the accept boundary min(1, p_d / q_d) falls between two grid lines
    and moves the accepted share by at most one line of G cells (1 / G for token d, and the same 1 / G taken from the recovered
    tokens); on a rejected line every token's residual interval has two boundaries, each between two cells (2 cells of G^2 per
    line, at most G lines: 2 / G).  Weighted by q_d (which sums to 1): |frequency - p_j| <= 4 / G."""
    G = 1024
    trow = R.randn_row(8, torch.float32, seed=21, spread=1.5)
    q = torch.softmax(R.randn_row(8, torch.float32, seed=22, spread=1.5), 0)
    p, _ = SR.probs(R.values(trow), 0.9)
    grid = (np.arange(G) + 0.5) / G
    freq = np.zeros(8)
    rec = np.array([SR.accept_ref(trow, q, 0, 0.9, 0.5, u)[1] for u in grid])
    rec_share = np.bincount(rec, minlength=8) / G                 # (the recovered token does not depend on d)
    for d in range(8):
        assert all(SR.accept_ref(trow, q, d, 0.9, 0.5, u)[1] == r for u, r in zip(grid[::97], rec[::97]))
        acc = np.array([SR.accept_ref(trow, q, d, 0.9, u, 0.5)[0] for u in grid]).mean()
        freq[d] += float(q[d]) * acc
        freq += float(q[d]) * (1.0 - acc) * rec_share
    tol = 4.0 / G
    print("max |frequency - p| =", np.abs(freq - p).max(), "tolerance", tol)
    assert np.abs(freq - p).max() <= tol


# the walk ----------------------------------------------------------------------------------------------------------------------
def _brute_walk(par, draft, target, accept, recovered):
    """every root path of the tree, filtered by the rules: exactly one survives"""
    T = len(draft)
    ok = lambda t: t >= 1 and 0 <= par[t] < t                    # noqa: E731
    kids = lambda c: [t for t in range(1, T) if ok(t) and par[t] == c]   # noqa: E731
    paths = [[0]]
    for path in paths:
        paths += [path + [t] for t in kids(path[-1])]
    good = []
    for path in paths:
        toks, fine = [], True
        for a, b in zip(path, path[1:]):
            if accept is None:
                match = [t for t in kids(a) if draft[t] == target[a]]
                fine &= target[a] != -1 and bool(match) and match[0] == b
                toks.append(target[a])
            else:
                fine &= kids(a)[0] == b and accept[b] != 0
                toks.append(draft[b])
        last = path[-1]
        if accept is None:
            fine &= target[last] == -1 or not [t for t in kids(last) if draft[t] == target[last]]
            toks.append(target[last])
        elif kids(last):
            fine &= accept[kids(last)[0]] == 0
            toks.append(recovered[kids(last)[0]])
        else:
            toks.append(target[last])
        if fine:
            good.append((toks, path))
    assert len(good) == 1
    return good[0]


def test_walk_reference_against_brute_force_on_all_small_trees():
    """every parent array with T <= 5 (values from -1 to T - 1: padding and out-of-order entries included), random ids from a small
    alphabet (so that siblings repeat and -1 occurs), both modes"""
    rng = np.random.default_rng(0)
    n = 0
    for T in range(1, 6):
        for tail in itertools.product(*[range(-1, T) for _ in range(1, T)]):
            par = [-1] + list(tail)
            for _ in range(4):
                draft = [int(x) for x in rng.integers(0, 3, T)]
                target = [int(x) for x in rng.integers(-1, 3, T)]
                accept = [int(x) for x in rng.integers(0, 2, T)]
                recovered = [int(x) for x in rng.integers(-1, 3, T)]
                for mode in (None, accept):
                    toks, path = _brute_walk(par, draft, target, mode, recovered)
                    out, num, nodes = SR.walk_ref(par, draft, target, mode, None if mode is None else recovered)
                    assert out == toks + [-1] * (T - len(toks)) and num == len(toks) and nodes == path + [-1] * (T - len(path))
                    n += 1
    assert n == 2 * 4 * (1 + 3 + 16 + 125 + 1296)
    # the chain: parents None, one bonus id for every node
    assert SR.walk_ref(None, [9, 5, 6, 7], 42, [0, 1, 1, 1], [-1, 1, 2, 3]) == ([5, 6, 7, 42], 4, [0, 1, 2, 3])
    assert SR.walk_ref(None, [9, 5, 6, 7], 42, [0, 1, 0, 1], [-1, 1, 2, 3]) == ([5, 2, -1, -1], 2, [0, 1, -1, -1])
    assert SR.walk_ref(None, [9, 5, 6, 7], 42, [0, 0, 1, 1], [-1, 1, 2, 3]) == ([1, -1, -1, -1], 1, [0, -1, -1, -1])


# commit_slots --------------------------------------------------------------------------------------------------------------------
def test_commit_slots_against_a_python_loop(spec):
    path = torch.tensor([[0, 2, 5, -1, -1, -1], [0, -1, -1, -1, -1, -1], [0, 1, 2, 3, 4, 5]], dtype=torch.int32)
    lens = torch.tensor([13, 0, 30], dtype=torch.int32)
    page = 16
    bt = torch.tensor([[4, 1, 7], [0, 9, 9], [3, 6, 2]], dtype=torch.int32)
    src, dst = spec.commit_slots(path, lens, block_table=bt, page_block_size=page)
    want = SR.commit_ref(path.tolist(), lens.tolist(), block_table=bt.tolist(), page_block_size=page)
    assert src.dtype == dst.dtype == torch.int64 and src.shape == dst.shape == (18,)
    assert (src.tolist(), dst.tolist()) == want
    assert src[1].item() == 4 * 16 + 15 and dst[1].item() == 4 * 16 + 14 and src[2].item() == 1 * 16 + 2   # (across a page boundary)
    for idx in (None, torch.tensor([2, 0, 5], dtype=torch.int32)):
        src, dst = spec.commit_slots(path, lens, seqlen_cache=64, cache_batch_idx=idx)
        want = SR.commit_ref(path.tolist(), lens.tolist(), seqlen_cache=64, cache_batch_idx=None if idx is None else idx.tolist())
        assert (src.tolist(), dst.tolist()) == want
    with pytest.raises(RuntimeError, match="block_table with page_block_size"):
        spec.commit_slots(path, lens)
    with pytest.raises(RuntimeError, match="block_table with page_block_size"):
        spec.commit_slots(path, lens, block_table=bt, seqlen_cache=64, page_block_size=16)


# the C ABI -------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_struct_sizes(lib):
    for name in ("fa_spec_accept", "fa_spec_accept_workspace_bytes", "fa_spec_accept_params_size", "fa_spec_walk",
                 "fa_spec_walk_params_size"):
        assert hasattr(lib.lib, name) and name in lib.EXPORTS
    assert lib.lib.fa_spec_accept_params_size() == ctypes.sizeof(lib.FaSpecAcceptParams)
    assert lib.lib.fa_spec_walk_params_size() == ctypes.sizeof(lib.FaSpecWalkParams)
    assert lib.FA_ABI_VERSION == 4 and lib.lib.fa_abi_version() == 4
    rows = {e: (s, q) for e, s, q in lib.ROW_OPS}
    assert rows["fa_spec_accept"] == (lib.FaSpecAcceptParams, "fa_spec_accept_workspace_bytes")
    assert rows["fa_spec_walk"] == (lib.FaSpecWalkParams, None)
    import build
    assert "fa_spec_verify.hip" in build.SOURCES


def _header_fields(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "fa_mi355.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        if stmt.strip():
            names = stmt.strip().split(",")
            fields.append(names[0].split()[-1].lstrip("*"))
            fields += [n.strip().lstrip("*") for n in names[1:]]
    return [f.split("[")[0] for f in fields]


def test_ctypes_mirrors_match_the_header(lib):
    for name, struct in (("fa_spec_accept_params", lib.FaSpecAcceptParams), ("fa_spec_walk_params", lib.FaSpecWalkParams)):
        fields = _header_fields(name)
        assert [f[0] for f in struct._fields_] == fields
        assert fields[0] == "struct_size" and fields[-1] == "reserved"
        assert ctypes.sizeof(struct) % 8 == 0 and ctypes.sizeof(dict(struct._fields_)["reserved"]) == 32


def test_the_not_covered_lists_name_what_remains():
    """the header, the README and sample.py no longer list verification as missing; spec_decode names what remains uncovered"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import flash_attn_mi355.sample as S
    import flash_attn_mi355.spec_decode as D
    gone = "rejection sampling and draft-tree verification for speculative decoding;"
    for text in (open(os.path.join(root, "include", "fa_mi355.h")).read(), open(os.path.join(root, "README.md")).read(), S.__doc__):
        assert gone not in re.sub(r"\s+\*?\s*", " ", text)
    for what in ("multi-child trees with draft probabilities", "typical acceptance", "in-kernel RNG", "fused commit"):
        assert what in re.sub(r"\s+", " ", D.__doc__)


# host buffers behind valid blocks: B = 2 requests of T = 4 nodes over V = 64
_B, _T, _V = 2, 4, 64
_ROWS = _B * _T
_OFF = {}
_o = 0
for _n, _sz in (("target_logits", _ROWS * 96 * 4), ("draft_probs", _ROWS * 96 * 4), ("draft_ids", _ROWS * 4), ("parents", _ROWS * 4),
                ("u_accept", _ROWS * 4), ("u_recover", _ROWS * 4), ("temperature", _B * 4), ("target_ids", _ROWS * 4),
                ("accept", _ROWS * 4), ("recovered", _ROWS * 4), ("out_tokens", _ROWS * 4), ("num_out", _B * 4),
                ("path_nodes", _ROWS * 4), ("workspace", 4096)):
    _OFF[_n] = _o
    _o += _sz
_TOTAL = _o + 64
_at = lambda name, add=0: (lambda b: b + _OFF[name] + add)      # noqa: E731
_ACCEPT_PTRS = ("target_logits", "draft_probs", "draft_ids", "parents", "u_accept", "u_recover", "temperature", "accept", "recovered",
                "workspace")
_WALK_PTRS = ("parents", "draft_ids", "target_ids", "accept", "recovered", "out_tokens", "num_out", "path_nodes")
_FORMS = ("bf16", "fp32", "mixed", "chain", "scalar")


def _accept_block(lib, buf, form="bf16"):
    """a valid fa_spec_accept block over host memory.  form: 'bf16' / 'fp32' (both tensors), 'mixed' (bf16 logits with row stride
    96, fp32 probs with row stride 80), 'chain' (parents NULL), 'scalar' (no temperature array)"""
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaSpecAcceptParams()
    s.struct_size = ctypes.sizeof(lib.FaSpecAcceptParams)
    for name in _ACCEPT_PTRS:
        setattr(s, name, base + _OFF[name])
    s.workspace_bytes = 4096
    s.batch, s.nodes, s.vocab = _B, _T, _V
    s.logits_row_stride = s.probs_row_stride = _V
    s.parents_batch_stride = _T
    s.dtype = s.probs_dtype = lib.FA_FP32 if form == "fp32" else lib.FA_BF16
    s.temperature_value = 1.0
    if form == "mixed":
        s.probs_dtype, s.logits_row_stride, s.probs_row_stride = lib.FA_FP32, 96, 80
    if form == "chain":
        s.parents, s.parents_batch_stride = None, 0
    if form == "scalar":
        s.temperature = None
    return s, base


def _walk_block(lib, buf, mode_b=True):
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaSpecWalkParams()
    s.struct_size = ctypes.sizeof(lib.FaSpecWalkParams)
    for name in _WALK_PTRS:
        setattr(s, name, base + _OFF[name])
    s.batch, s.nodes = _B, _T
    s.parents_batch_stride = s.target_ids_batch_stride = _T
    s.target_ids_node_stride = 1
    if not mode_b:
        s.accept = s.recovered = None
    return s, base


def test_accept_argument_errors_without_gpu(lib):
    """every FA_ERR_INVALID_ARGUMENT case of fa_spec_accept fires before any device work, and the workspace query answers 0 for a
    block the call rejects"""
    buf = (ctypes.c_char * _TOTAL)()

    def bad(match, form="bf16", code="(-1)", place=False, **kw):
        """place: the block is wrong only in where its tensors or its workspace lie, which the query does not look at"""
        s, base = _accept_block(lib, buf, form)
        for k, v in kw.items():
            setattr(s, k, v(base) if callable(v) else v)
        with pytest.raises(RuntimeError, match=match) as e:
            lib.call_spec_accept(s, 0)
        assert code in str(e.value) and "spec_accept" in str(e.value)
        assert lib.spec_accept_workspace_bytes(s) == (SR.workspace_bytes(_ROWS, _V) if place else 0)
    for form in _FORMS:
        bad("struct_size", form, struct_size=ctypes.sizeof(lib.FaSpecAcceptParams) - 8)
        for name in ("target_logits", "draft_probs", "draft_ids", "accept", "recovered"):
            bad("must not be NULL", form, **{name: None})
        bad("reserved", form, reserved=(ctypes.c_int64 * 4)(0, 0, 1, 0))
        bad("reserved", form, reserved0=1)
        bad("dtype must be fp16, bf16 or fp32", form, dtype=lib.FA_FP8_E4M3)
        bad("probs_dtype must be fp16, bf16 or fp32", form, probs_dtype=7)
        bad("nodes must be in 1 .. 64", form, nodes=0)
        bad("nodes must be in 1 .. 64", form, nodes=65)
        bad("vocab must be at least 1", form, vocab=0)
        bad("batch must be non-negative", form, batch=-1)
        bad("row strides", form, logits_row_stride=-64)
        bad("row strides", form, logits_row_stride=63)
        bad("row strides", form, probs_row_stride=40)
        bad("parents_batch_stride", form, parents_batch_stride=-1)
        bad("aligned", form, target_logits=_at("target_logits", 1))
        bad("aligned", form, draft_probs=_at("draft_probs", 1))
        for name in ("draft_ids", "u_accept", "u_recover", "accept", "recovered"):
            bad("aligned", form, **{name: _at(name, 2)})
        bad("workspace must be 16-byte aligned", form, place=True, workspace=_at("workspace", 8))
        bad("the workspace holds", form, place=True, workspace_bytes=lib.spec_accept_workspace_bytes(_accept_block(lib, buf, form)[0]) - 1)
        bad("the workspace holds", form, place=True, workspace=None)
        bad("accept overlaps target_logits", form, place=True, accept=_at("target_logits", 64))
        bad("accept overlaps draft_probs", form, place=True, accept=_at("draft_probs", 0))
        bad("recovered overlaps draft_ids", form, place=True, recovered=_at("draft_ids", 4))
        bad("accept overlaps u_accept", form, place=True, accept=_at("u_accept", 0))
        bad("recovered overlaps u_recover", form, place=True, recovered=_at("u_recover", 8))
        bad("accept overlaps recovered", form, place=True, recovered=_at("accept", 4))
        bad("accept overlaps workspace", form, place=True, accept=_at("workspace", 16))
        bad("u_accept and u_recover are needed", form, u_accept=None)
        bad("u_accept and u_recover are needed", form, u_recover=None)
    bad("aligned", "fp32", target_logits=_at("target_logits", 2))
    bad("aligned", "mixed", draft_probs=_at("draft_probs", 2))
    bad("aligned", "bf16", parents=_at("parents", 2))
    bad("aligned", "bf16", temperature=_at("temperature", 1))
    bad("accept overlaps parents", "bf16", place=True, accept=_at("parents", 0))
    bad("recovered overlaps temperature", "bf16", place=True, recovered=_at("temperature", 0))
    bad("u_accept and u_recover are needed", "scalar", u_accept=None, u_recover=None, temperature_value=1e-30)
    # FA_ERR_UNSUPPORTED
    bad(r"2\^20", code="(-2)", vocab=2 ** 20 + 1, logits_row_stride=2 ** 20 + 1, probs_row_stride=2 ** 20 + 1, batch=1, nodes=1)
    bad(r"2\^31", code="(-2)", batch=2 ** 31, vocab=1, logits_row_stride=1, probs_row_stride=1)
    bad(r"2\^31", code="(-2)", batch=2 ** 26, nodes=8, vocab=2 ** 16, logits_row_stride=2 ** 16, probs_row_stride=2 ** 16)


def test_walk_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * _TOTAL)()

    def bad(match, mode_b=True, code="(-1)", **kw):
        s, base = _walk_block(lib, buf, mode_b)
        for k, v in kw.items():
            setattr(s, k, v(base) if callable(v) else v)
        with pytest.raises(RuntimeError, match=match) as e:
            lib.call_spec_walk(s, 0)
        assert code in str(e.value) and "spec_walk" in str(e.value)
    for mode_b in (True, False):
        bad("struct_size", mode_b, struct_size=ctypes.sizeof(lib.FaSpecWalkParams) - 8)
        for name in ("draft_ids", "target_ids", "out_tokens", "num_out", "path_nodes"):
            bad("must not be NULL", mode_b, **{name: None})
        bad("reserved", mode_b, reserved=(ctypes.c_int64 * 4)(0, 0, 0, 5))
        bad("reserved", mode_b, reserved0=-1)
        bad("nodes must be in 1 .. 64", mode_b, nodes=0)
        bad("nodes must be in 1 .. 64", mode_b, nodes=65)
        bad("batch must be non-negative", mode_b, batch=-2)
        for name in ("parents_batch_stride", "target_ids_batch_stride", "target_ids_node_stride"):
            bad("strides must be non-negative", mode_b, **{name: -1})
        for name in ("parents", "draft_ids", "target_ids", "out_tokens", "num_out", "path_nodes"):
            bad("4-byte aligned", mode_b, **{name: _at(name, 2)})
        bad("out_tokens overlaps draft_ids", mode_b, out_tokens=_at("draft_ids", 0))
        bad("out_tokens overlaps target_ids", mode_b, out_tokens=_at("target_ids", 4))
        bad("path_nodes overlaps parents", mode_b, path_nodes=_at("parents", 0))
        bad("out_tokens overlaps path_nodes", mode_b, path_nodes=_at("out_tokens", 8))
        bad("num_out overlaps path_nodes", mode_b, num_out=_at("path_nodes", 0))
        bad(r"2\^31", mode_b, code="(-2)", batch=2 ** 31)
    bad("accept and recovered go together", True, accept=None)
    bad("accept and recovered go together", True, recovered=None)
    bad("4-byte aligned", True, accept=_at("accept", 2))
    bad("num_out overlaps accept", True, num_out=_at("accept", 0))
    bad("out_tokens overlaps recovered", True, out_tokens=_at("recovered", 0))


def test_valid_blocks_pass_the_checks(lib):
    """batch == 0 is FA_OK without a launch; non-finite host temperatures are rules, not errors; the uniform numbers may be missing
    where the host temperature is not above 0; a valid block reaches the launch (which fails here: there is no device)"""
    buf = (ctypes.c_char * _TOTAL)()
    for form in _FORMS:
        s, _ = _accept_block(lib, buf, form)
        s.batch = 0
        lib.call_spec_accept(s, 0)
    for t in (0.0, -1.0, float("nan")):
        s, _ = _accept_block(lib, buf, "scalar")
        s.batch, s.temperature_value, s.u_accept, s.u_recover = 0, t, None, None
        lib.call_spec_accept(s, 0)
    for mode_b in (True, False):
        s, _ = _walk_block(lib, buf, mode_b)
        s.batch = 0
        lib.call_spec_walk(s, 0)
    if not torch.cuda.is_available():
        s, _ = _accept_block(lib, buf, "mixed")
        with pytest.raises(RuntimeError, match=r"\(-3\)|launch"):
            lib.call_spec_accept(s, 0)


def test_workspace_query_is_a_function_of_shapes(lib):
    """fa_spec_accept_workspace_bytes needs no device, looks at neither the pointers' places nor the workspace fields, and is
    batch x nodes x (48 x chunks rounded up to 64)"""
    buf = (ctypes.c_char * _TOTAL)()
    for B, T, V in ((1, 1, 1), (2, 4, 64), (3, 5, 16384), (3, 5, 16385), (7, 64, 151936), (1, 9, 1 << 20)):
        for form in _FORMS:
            s, base = _accept_block(lib, buf, form)
            s.batch, s.nodes, s.vocab = B, T, V
            s.logits_row_stride = s.probs_row_stride = V + 8
            want = SR.workspace_bytes(B * T, V)
            assert lib.spec_accept_workspace_bytes(s) == want == B * T * ((48 * -(-V // 16384) + 63) // 64 * 64)
            s.workspace, s.workspace_bytes = None, 0
            assert lib.spec_accept_workspace_bytes(s) == want
            s.workspace, s.accept = base + 8, base + _OFF["target_logits"]      # misplaced: not the query's business
            assert lib.spec_accept_workspace_bytes(s) == want
    s, _ = _accept_block(lib, buf)
    s.batch = 0
    assert lib.spec_accept_workspace_bytes(s) == 0
    assert lib.lib.fa_spec_accept_workspace_bytes(None) == 0


def test_wrapper_argument_errors(spec):
    """the Python surface rejects bad shapes and dtypes before it looks for a device"""
    x = torch.zeros(2, 4, 16)
    ids = torch.zeros(2, 4, dtype=torch.int32)
    u = torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="fp16, bf16 or fp32"):
        spec.verify(x.double(), ids)
    with pytest.raises(RuntimeError, match=r"\[B, T, V\]"):
        spec.verify(x[0], ids)
    with pytest.raises(RuntimeError, match="T must be in 1 .. 64"):
        spec.verify(torch.zeros(1, 65, 4), torch.zeros(1, 65, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="draft_ids must be an int32 or int64"):
        spec.verify(x, ids.float())
    with pytest.raises(RuntimeError, match="draft_ids must be an int32 or int64"):
        spec.verify(x, ids[:, :3])
    with pytest.raises(RuntimeError, match="u_accept / u_recover go with draft_probs"):
        spec.verify(x, ids, u_accept=u)
    with pytest.raises(RuntimeError, match="draft_probs must be"):
        spec.accept_forward(x, x[:, :, :8], ids, u, u)
    with pytest.raises(RuntimeError, match="parents must be an int32"):
        spec.accept_forward(x, x, ids, u, u, parents=torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="u_accept must be a float32"):
        spec.accept_forward(x, x, ids, u.double(), u)
    with pytest.raises(RuntimeError, match="are needed unless temperature"):
        spec.accept_forward(x, x, ids, None, None)
    with pytest.raises(RuntimeError, match="temperature must be a number or a tensor of one value per row"):
        spec.accept_forward(x, x, ids, u, u, temperature=torch.ones(3))
    with pytest.raises(RuntimeError, match="target_ids must be an int32"):
        spec.walk(ids, ids.long())
    with pytest.raises(RuntimeError, match="accept and recovered go together"):
        spec.walk(ids, ids, accept=ids)
    import flash_attn_mi355.torch_ops as ops
    assert not {"spec_accept", "spec_walk", "spec_verify"} & set(ops.__all__)
    for name in ("spec_accept", "spec_walk", "spec_verify"):
        assert hasattr(torch.ops.flash_attn_mi355, name)
