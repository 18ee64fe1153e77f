"""CPU: the host side of the fa_moe_* ops - the fp64 / exact-integer yardstick of the GPU tests (moe_ref.py) against torch's own
topk / softmax / sigmoid / argsort and their autograd, the wrong variants it must be told apart from, the decisiveness of the
sigmoid + bias inputs the GPU tests use, the tie cases, the C ABI's blocks, argument checks and workspace query on host pointers,
the torch.library ops' schemas and fake implementations, and the Python wrappers' argument errors.  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import moe_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


COMBOS = [("softmax", True), ("softmax", False), ("sigmoid", True), ("sigmoid", False)]


def _torch_route(logits, k, scoring, renormalize, bias, scale):
    """the eager float64 composition a caller writes today"""
    if scoring == "softmax":
        p = torch.softmax(logits, dim=-1)
        _, ids = torch.topk(logits, k, dim=-1)
        w = p.gather(1, ids)
    else:
        s = torch.sigmoid(logits)
        _, ids = torch.topk(s if bias is None else s + bias, k, dim=-1)
        w = s.gather(1, ids)
    if renormalize:
        w = w / w.sum(-1, keepdim=True)
    return w * scale, ids


# the yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring,renormalize", COMBOS)
def test_reference_equals_torch_and_its_autograd(scoring, renormalize):
    g = torch.Generator().manual_seed(5)
    for T, E, k in ((5, 8, 2), (9, 60, 6), (4, 384, 8), (3, 16, 16)):
        logits = torch.randn(T, E, generator=g, dtype=torch.float64, requires_grad=True)          # (tie-free)
        bias = torch.randn(E, generator=g, dtype=torch.float64) * 0.3 if scoring == "sigmoid" else None
        dw = torch.randn(T, k, generator=g, dtype=torch.float64)
        w_t, ids_t = _torch_route(logits, k, scoring, renormalize, bias, 2.5)
        nb = None if bias is None else bias.numpy()
        w, ids, gap = R.route_ref(logits.detach().numpy(), k, scoring=scoring, renormalize=renormalize, bias=nb, scale=2.5)
        assert (ids == ids_t.numpy()).all() and (gap > 0).all()
        assert np.abs(w - w_t.detach().numpy()).max() < 1e-12
        (dl_t,) = torch.autograd.grad(w_t, logits, dw)
        dl = R.route_bwd_ref(dw.numpy(), logits.detach().numpy(), ids, scoring=scoring, renormalize=renormalize, bias=nb, scale=2.5)
        assert np.abs(dl - dl_t.numpy()).max() < 1e-12
        if not (scoring == "softmax" and not renormalize):
            sel = np.zeros((T, E), dtype=bool)
            sel[np.arange(T)[:, None], ids] = True
            assert (dl[~sel] == 0).all() and not np.signbit(dl[~sel]).any()


def test_reference_sort_equals_stable_argsort():
    rng = np.random.default_rng(3)
    for T, K, E, align in ((1, 1, 2, 1), (67, 2, 8, 1), (67, 6, 60, 16), (300, 8, 128, 128), (0, 4, 8, 16)):
        ids = rng.integers(0, E, size=(T, K)).astype(np.int32)
        sorted_slot, pos, offsets = R.sort_ref(ids, E, align=align)
        order = torch.argsort(torch.from_numpy(ids.reshape(-1).astype(np.int64)), stable=True).numpy()
        counts = np.bincount(ids.reshape(-1), minlength=E)
        assert (sorted_slot[sorted_slot >= 0] == order).all()
        assert len(sorted_slot) == T * K + E * (align - 1)
        assert (offsets[:-1] % align == 0).all() and (np.diff(offsets) == (counts + align - 1) // align * align).all()
        for e in range(E):
            seg = sorted_slot[offsets[e]:offsets[e + 1]]
            assert (seg[:counts[e]] >= 0).all() and (seg[counts[e]:] == -1).all() and (np.diff(seg[:counts[e]]) > 0).all()
        assert (sorted_slot[offsets[E]:] == -1).all()
        assert (sorted_slot[pos.reshape(-1)] == np.arange(T * K)).all()
    # dropped ids are compared, never used
    ids = np.array([[0, -1], [8, 1], [2 ** 31 - 1, 1]], dtype=np.int32)
    sorted_slot, pos, offsets = R.sort_ref(ids, 8, align=4)
    assert pos.tolist() == [[0, -1], [-1, 4], [-1, 5]] and offsets.tolist() == [0, 4, 8, 8, 8, 8, 8, 8, 8]


def test_reference_permute_and_combine_equal_torch_and_its_autograd():
    g = torch.Generator().manual_seed(7)
    T, K, E, N, align = 13, 3, 8, 16, 4
    ids = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(T)]).to(torch.int32)
    ids[2, 1] = -1                                                                                # a dropped slot
    sorted_slot, pos, offsets = R.sort_ref(ids.numpy(), E, align=align)
    x = torch.randn(T, N, generator=g, dtype=torch.float64)
    xp = R.permute_ref(x.numpy(), sorted_slot, K)
    live = sorted_slot >= 0
    assert (xp[live] == x.numpy()[sorted_slot[live] // K]).all() and (xp[~live] == 0).all()
    y = torch.randn(len(sorted_slot), N, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.rand(T, K, generator=g, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(T, N, generator=g, dtype=torch.float64)
    pt = torch.from_numpy(pos.astype(np.int64))
    out_t = ((w * (pt >= 0))[:, :, None] * y[pt.clamp(min=0)]).sum(1)
    out, mag = R.combine_ref(y.detach().numpy(), w.detach().numpy(), pos)
    assert np.abs(out - out_t.detach().numpy()).max() < 1e-12 and (mag >= np.abs(out) - 1e-12).all()
    dy_t, dw_t = torch.autograd.grad(out_t, (y, w), dout)
    dy, dw, _ = R.combine_bwd_ref(dout.numpy(), y.detach().numpy(), w.detach().numpy(), pos)
    assert np.abs(dy - dy_t.numpy()).max() < 1e-12 and np.abs(dw - dw_t.numpy()).max() < 1e-12
    assert (dy[~live] == 0).all() and dw[2, 1] == 0
    # dy is the scaled permute
    assert (dy == R.permute_ref(dout.numpy(), sorted_slot, K, scale=w.detach().numpy())).all()


def test_reference_tie_cases_and_special_values():
    inf, nan = np.inf, np.nan
    rows = np.array([[1., 1., 1., 1., 1., 1., 1., 1.],                 # all equal: the lowest indices
                     [0., 3., 3., 1., 3., 2., 2., -1.],                # ties inside the selection and across its boundary
                     [-inf] * 8,                                       # all -inf: ids 0 .. K - 1, NaN weights
                     [nan, 2., nan, -inf, 2., nan, 0., -0.],           # NaN counts as -inf; +0 == -0: the lower index
                     [0., inf, 1., inf, 2., 3., 4., 5.]])              # +inf: selected first, NaN weights
    w, ids, _ = R.route_ref(rows, 4, scoring="softmax", renormalize=True)
    assert ids.tolist() == [[0, 1, 2, 3], [1, 2, 4, 5], [0, 1, 2, 3], [1, 4, 6, 7], [1, 3, 7, 6]]
    assert np.allclose(w[0], 0.25) and np.isnan(w[2]).all() and np.isnan(w[4]).all() and np.isfinite(w[[0, 1, 3]]).all()
    w, ids, _ = R.route_ref(rows[3:4], 6, scoring="softmax", renormalize=True)
    assert ids.tolist() == [[1, 4, 6, 7, 0, 2]] and (w[0, 4:] == 0).all()     # a selected NaN / -inf logit weighs 0
    w, ids, _ = R.route_ref(rows[3:4], 6, scoring="sigmoid", renormalize=False)
    assert ids.tolist() == [[1, 4, 6, 7, 3, 0]] and np.isnan(w[0, 5]) and w[0, 4] == 0 and w[0, 2] == 0.5
    for r in range(len(rows)):
        for k in (1, 4, 8):
            _, ids, _ = R.route_ref(rows[r:r + 1], k, scoring="softmax")
            assert len(set(ids[0].tolist())) == k and ids.min() >= 0 and ids.max() < 8


def test_wrong_variants_are_told_apart_and_the_bounds_are_not_vacuous():
    rows = np.array([[0., 3., 3., 1., 3., 2., 2., -1.]])
    assert R.route_ref(rows, 2)[1].tolist() == [[1, 2]] and R.route_ref(rows, 2, variant="tie_high")[1].tolist() == [[4, 2]]
    for (T, E, K) in R.ROUTE_SHAPES:
        logits, bias = R.decisive_logits(T, E, K, R.route_seed(T, E, K))
        for renorm in (True, False):
            w, ids, _ = R.route_ref(logits, K, scoring="sigmoid", renormalize=renorm, bias=bias, scale=2.5)
            wb, idsb, _ = R.route_ref(logits, K, scoring="sigmoid", renormalize=renorm, bias=bias, scale=2.5, variant="bias_in_weight")
            bound = R.route_weight_bound(logits, w, ids, scoring="sigmoid", renormalize=renorm, bias=bias)
            assert (idsb == ids).all() and (bound < 1e-4 * np.abs(w) + 1e-30).all()
            if not (renorm and K == 1):                       # (one renormalised weight is 1 whatever it was)
                assert (np.abs(wb - w) > bound).any()
            # the unbiased selection differs: the bias decides who wins
            if K < E:
                assert (R.route_ref(logits, K, scoring="sigmoid", bias=None)[1] != ids).any() or T < 3
    rng = np.random.default_rng(11)
    ids = rng.integers(0, 8, size=(67, 2)).astype(np.int32)
    good = R.sort_ref(ids, 8, align=16)
    assert (R.sort_ref(ids, 8, align=16, variant="unstable")[0] != good[0]).any()
    assert (R.sort_ref(ids, 8, align=16, variant="pad_in_pos")[1] != good[1]).any()
    y, w, dout = rng.standard_normal((len(good[0]), 264)), rng.random((67, 2)), rng.standard_normal((67, 264))
    _, dw, mag = R.combine_bwd_ref(dout, y, w, good[1])
    _, dw_bad, _ = R.combine_bwd_ref(dout, y, w, good[1], variant="dw_from_w")
    assert (np.abs(dw_bad - dw) > R.DW_DEPTH * R.U * mag * R.SLACK).all()
    out, mag = R.combine_ref(y, w, good[1])
    assert (2 * R.U * mag < 1e-5).all()                        # K 2^-24 mag: far below the 16-bit rounding it is added to


def test_sigmoid_inputs_of_the_gpu_tests_are_decisive():
    """every row of every (seed, shape) the GPU tests route with sigmoid + bias: the first K + 1 scores are more than 1e-4 apart,
    so no rounding of the hardware exp2 / rcp (about 1e-7) can select another expert or another order.  No row is left out."""
    for (T, E, K) in R.ROUTE_SHAPES:
        logits, bias = R.decisive_logits(T, E, K, R.route_seed(T, E, K))
        assert logits.shape == (T, E) and bias.shape == (E,)
        for dt in (torch.bfloat16, torch.float16):
            assert (torch.from_numpy(logits).to(dt).float().numpy() == logits).all()             # exact in every io dtype
        for b in (bias, None):
            _, _, gap = R.route_ref(logits, K, scoring="sigmoid", bias=b)
            assert gap.shape == (T,) and (gap > R.DECISIVE_GAP).all(), (T, E, K, gap.min())


# the C ABI -------------------------------------------------------------------------------------------------------------------
_BLOCKS = [("fa_moe_route", "FaMoeRouteParams"), ("fa_moe_route_bwd", "FaMoeRouteBwdParams"), ("fa_moe_sort", "FaMoeSortParams"),
           ("fa_moe_permute", "FaMoePermuteParams"), ("fa_moe_combine", "FaMoeCombineParams"),
           ("fa_moe_combine_bwd", "FaMoeCombineBwdParams")]


def test_library_exports_and_struct_sizes(lib):
    rows = {e: (s, q) for e, s, q in lib.ROW_OPS}
    for entry, mirror in _BLOCKS:
        for name in (entry, entry + "_params_size"):
            assert hasattr(lib.lib, name) and name in lib.EXPORTS
        assert getattr(lib.lib, entry + "_params_size")() == ctypes.sizeof(getattr(lib, mirror))
        assert rows[entry][0] is getattr(lib, mirror)
        assert callable(getattr(lib, "call_" + entry[3:]))
    assert rows["fa_moe_sort"][1] == "fa_moe_sort_workspace_bytes" and all(rows[e][1] is None for e, _ in _BLOCKS if e != "fa_moe_sort")
    assert "fa_moe_sort_plan" in lib.EXPORTS and "fa_moe_sort_workspace_bytes" in lib.EXPORTS
    assert lib.FA_ABI_VERSION == 4 and lib.lib.fa_abi_version() == 4
    import build
    assert "fa_moe.hip" in build.SOURCES


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "fa_mi355.h")).read(), flags=re.S)


def _header_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        if stmt.strip():
            names = stmt.strip().split(",")
            fields.append(names[0].split()[-1].lstrip("*"))
            fields += [n.strip().lstrip("*") for n in names[1:]]
    return [f.split("[")[0] for f in fields]


def test_ctypes_mirrors_match_the_header(lib):
    for entry, mirror in _BLOCKS:
        m = getattr(lib, mirror)
        fields = _header_fields(entry + "_params")
        assert [f[0] for f in m._fields_] == fields, entry
        assert fields[0] == "struct_size" and fields[-1] == "reserved"
        assert ctypes.sizeof(m) % 8 == 0 and ctypes.sizeof(dict(m._fields_)["reserved"]) == 32
    body = re.search(r"typedef enum fa_moe_scoring \{(.*?)\} fa_moe_scoring;", _header(), flags=re.S).group(1)
    assert {k: int(v) for k, v in re.findall(r"(FA_MOE_\w+)\s*=\s*(\d+)", body)} == {"FA_MOE_SOFTMAX": 0, "FA_MOE_SIGMOID": 1}
    from flash_attn_mi355 import moe
    assert moe.SCORINGS == {"softmax": lib.FA_MOE_SOFTMAX, "sigmoid": lib.FA_MOE_SIGMOID}
    # fa_params is untouched
    assert ctypes.sizeof(lib.FaParams) == lib.lib.fa_params_size()


def _plan(slots, E):
    """csrc/fa_moe.h's moe_sort_plan restated"""
    per = (slots + 1023) // 1024
    chunk = max(256, (per + 63) // 64 * 64)
    chunks = max(1, (slots + chunk - 1) // chunk)
    return chunk, chunks, 4 * chunks * E


def test_sort_plan_and_workspace_depend_on_the_shapes_alone(lib):
    for slots in (0, 1, 255, 256, 257, 300 * 8, 2 ** 18, 2 ** 18 + 1, 65536 * 8, 2 ** 31 - 1):
        for E in (2, 8, 60, 384, 512):
            assert lib.moe_sort_plan(slots, E) == _plan(slots, E), (slots, E)
            assert _plan(slots, E)[1] <= 1024 and _plan(slots, E)[0] % 64 == 0
    assert lib.moe_sort_plan(300 * 8, 128)[1] > 1                 # T = 300, K = 8: more than one wave sorts
    s = lib.FaMoeSortParams()
    s.struct_size = ctypes.sizeof(lib.FaMoeSortParams)
    for T, K, E, align in ((0, 2, 8, 1), (67, 2, 8, 16), (300, 8, 128, 128), (65536, 8, 256, 1)):
        s.tokens, s.top_k, s.num_experts, s.align = T, K, E, align
        assert lib.moe_sort_workspace_bytes(s) == _plan(T * K, E)[2]          # no pointers set: the query reads sizes only
    s.num_experts = 513
    assert lib.moe_sort_workspace_bytes(s) == 0
    with pytest.raises(RuntimeError, match=r"\(-2\).*num_experts"):
        lib.moe_sort_plan(8, 1)
    with pytest.raises(RuntimeError, match=r"\(-1\).*slots"):
        lib.moe_sort_plan(-1, 8)


def _host(nbytes=1 << 16):
    buf = (ctypes.c_char * (nbytes + 64))()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _route_block(lib, base, bwd=False):
    s = (lib.FaMoeRouteBwdParams if bwd else lib.FaMoeRouteParams)()
    s.struct_size = ctypes.sizeof(s)
    s.logits, s.logits_row_stride = base, 64
    if bwd:
        s.dweights, s.ids, s.dlogits, s.dlogits_row_stride = base + 4096, base + 8192, base + 12288, 64
    else:
        s.weights, s.ids = base + 4096, base + 8192
    s.tokens, s.num_experts, s.top_k, s.dtype, s.scoring, s.renormalize, s.scale = 8, 64, 4, lib.FA_BF16, lib.FA_MOE_SOFTMAX, 1, 1.0
    return s


def _piece_block(lib, base, kind):
    s = {"permute": lib.FaMoePermuteParams, "combine": lib.FaMoeCombineParams, "combine_bwd": lib.FaMoeCombineBwdParams}[kind]()
    s.struct_size = ctypes.sizeof(s)
    s.rows, s.tokens, s.top_k, s.n, s.dtype = 16, 4, 2, 64, lib.FA_FP16
    if kind == "permute":
        s.x, s.sorted_slot, s.out, s.x_row_stride, s.out_row_stride = base, base + 4096, base + 8192, 64, 64
    elif kind == "combine":
        s.y, s.weights, s.pos, s.out, s.y_row_stride, s.out_row_stride = base, base + 4096, base + 5120, base + 8192, 64, 64
    else:
        s.dout, s.y, s.weights, s.pos, s.dy, s.dw = base, base + 4096, base + 8192, base + 9216, base + 12288, base + 16384
        s.dout_row_stride = s.y_row_stride = s.dy_row_stride = 64
    return s


def _raises(call, s, match, code="(-1)"):
    with pytest.raises(RuntimeError, match=match) as e:
        call(s, 0)
    assert code in str(e.value), str(e.value)


def _reaches_the_device(call, s, empty):
    """a block that passes every check gets as far as the launch - FA_ERR_LAUNCH (-3) / no device (-4), never an argument error.
    Host pointers: where there is a device the kernels must not run on them, so only the empty problem is called there."""
    if torch.cuda.is_available():
        for k, v in empty.items():
            setattr(s, k, v)
        call(s, 0)
        return
    try:
        call(s, 0)
    except RuntimeError as e:
        assert "(-3)" in str(e) or "(-4)" in str(e), str(e)


def test_argument_errors_without_gpu(lib):
    """the limits (FA_ERR_UNSUPPORTED, -2) and the argument rules (FA_ERR_INVALID_ARGUMENT, -1) fire before any device work"""
    buf, base = _host()
    for bwd, call in ((False, lib.call_moe_route), (True, lib.call_moe_route_bwd)):
        def bad(match, code="(-1)", **kw):
            s = _route_block(lib, base, bwd)
            for k, v in kw.items():
                setattr(s, k, v)
            _raises(call, s, match, code)
        bad("struct_size", struct_size=8)
        bad("reserved", reserved=(ctypes.c_int64 * 4)(0, 1, 0, 0))
        bad("num_experts", "(-2)", num_experts=1)
        bad("num_experts", "(-2)", num_experts=513)
        bad("top_k", "(-2)", top_k=0)
        bad("top_k", "(-2)", top_k=17)
        bad("top_k", "(-2)", num_experts=8, top_k=9)
        bad("2\\^31", "(-2)", tokens=2 ** 31 // 4 + 1)
        bad("tokens", tokens=-1)
        bad("dtype", dtype=lib.FA_FP8_E4M3)
        bad("scoring", scoring=2)
        bad("renormalize", renormalize=2)
        bad("scale", scale=float("inf"))
        bad("must not be NULL", logits=None)
        bad("must not be NULL", ids=None)
        bad("stride", logits_row_stride=63)
        bad("aligned", logits=base + 1)
        bad("overlaps", **({"dlogits": base + 64} if bwd else {"ids": base + 64}))
        _reaches_the_device(call, _route_block(lib, base, bwd), {"tokens": 0})
    s = _route_block(lib, base)
    s.bias = base + 16384
    _raises(lib.call_moe_route, s, "bias goes with sigmoid")

    def sort_block(**kw):
        s = lib.FaMoeSortParams()
        s.struct_size = ctypes.sizeof(s)
        s.ids, s.sorted_slot, s.pos, s.expert_offsets, s.workspace = base, base + 4096, base + 8192, base + 12288, base + 16384
        s.tokens, s.top_k, s.num_experts, s.align, s.workspace_bytes = 8, 2, 8, 16, 4 * 8
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    _raises(lib.call_moe_sort, sort_block(align=0), "align", "(-2)")
    _raises(lib.call_moe_sort, sort_block(align=257), "align", "(-2)")
    _raises(lib.call_moe_sort, sort_block(num_experts=1), "num_experts", "(-2)")
    _raises(lib.call_moe_sort, sort_block(top_k=17), "top_k", "(-2)")
    _raises(lib.call_moe_sort, sort_block(tokens=2 ** 30, align=256), "2\\^31", "(-2)")
    _raises(lib.call_moe_sort, sort_block(workspace_bytes=31), "workspace too small")
    _raises(lib.call_moe_sort, sort_block(workspace=None), "workspace too small")
    _raises(lib.call_moe_sort, sort_block(pos=None), "must not be NULL")
    _raises(lib.call_moe_sort, sort_block(pos=base + 2), "4-byte aligned")
    _raises(lib.call_moe_sort, sort_block(sorted_slot=base), "overlaps")
    _raises(lib.call_moe_sort, sort_block(reserved0=1), "reserved")
    if not torch.cuda.is_available():
        _reaches_the_device(lib.call_moe_sort, sort_block(), {})

    for kind, call, out in (("permute", lib.call_moe_permute, "out"), ("combine", lib.call_moe_combine, "out"),
                            ("combine_bwd", lib.call_moe_combine_bwd, "dy")):
        def bad(match, code="(-1)", **kw):
            s = _piece_block(lib, base, kind)
            for k, v in kw.items():
                setattr(s, k, v)
            _raises(call, s, match, code)
        bad("struct_size", struct_size=16)
        bad("n must be", "(-2)", n=60)
        bad("n must be", "(-2)", n=16392)
        bad("n must be", "(-2)", n=0)
        bad("top_k", "(-2)", top_k=17)
        bad("fp16 or bf16", dtype=lib.FA_FP32)
        bad("non-negative", rows=-1)
        bad("reserved", reserved0=3)
        bad("16-byte aligned", **{out: base + 8192 + 8})
        bad("16-byte aligned", **{out + "_row_stride": 68})
        bad("overlaps", **{out: base + 64})
        _reaches_the_device(call, _piece_block(lib, base, kind), {"rows": 0, "tokens": 0})
    del buf


# Python ----------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors_on_cpu_tensors():
    from flash_attn_mi355 import moe
    lg = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="scoring must be one of"):
        moe.moe_route(lg, 2, scoring="tanh")
    with pytest.raises(RuntimeError, match="num_experts must be in"):
        moe.moe_route(torch.zeros(4, 1), 1)
    with pytest.raises(RuntimeError, match="num_experts must be in"):
        moe.moe_route_forward(torch.zeros(4, 513), 1)
    with pytest.raises(RuntimeError, match="k must be in"):
        moe.moe_route(lg, 17)
    with pytest.raises(RuntimeError, match="k must be in"):
        moe.moe_route(lg[:, :8], 9)
    with pytest.raises(RuntimeError, match="logits must be fp16, bf16 or fp32"):
        moe.moe_route(lg.double(), 2)
    with pytest.raises(RuntimeError, match="bias goes with"):
        moe.moe_route(lg, 2, bias=torch.zeros(64))
    with pytest.raises(RuntimeError, match="bias must be an fp32"):
        moe.moe_route(lg, 2, scoring="sigmoid", bias=torch.zeros(63))
    with pytest.raises(RuntimeError, match="scale must be finite"):
        moe.moe_route(lg, 2, scale=float("nan"))
    ids = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ids must be an int32"):
        moe.moe_sort(ids.long(), 8)
    with pytest.raises(RuntimeError, match="align must be in"):
        moe.moe_sort(ids, 8, align=512)
    with pytest.raises(RuntimeError, match="num_experts must be in"):
        moe.moe_sort(ids, 1024)
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    ss = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="hidden size N"):
        moe.moe_permute(x[:, :60], ss, 2)
    with pytest.raises(RuntimeError, match="hidden size N"):
        moe.moe_permute(torch.zeros(1, 16392, dtype=torch.bfloat16), ss, 2)
    with pytest.raises(RuntimeError, match="x must be fp16 or bf16"):
        moe.moe_permute(x.float(), ss, 2)
    with pytest.raises(RuntimeError, match="k must be in"):
        moe.moe_permute(x, ss, 32)
    with pytest.raises(RuntimeError, match="weights must be fp32"):
        moe.moe_combine(torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(4, 2, dtype=torch.bfloat16), ids)
    with pytest.raises(RuntimeError, match="pos must be an int32"):
        moe.moe_combine(torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(4, 2), ids.long())
    with pytest.raises(RuntimeError, match="dout must have pos'"):
        moe.moe_combine_backward(x[:3], torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(4, 2), ids)
    # everything else in order: the CPU tensor itself is the error - there is no torch fallback
    y, w = torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(4, 2)
    for call in (lambda: moe.moe_route(lg, 2), lambda: moe.moe_route_forward(lg, 2, scoring="sigmoid", bias=torch.zeros(64)),
                 lambda: moe.moe_route_backward(w, lg, ids), lambda: moe.moe_sort(ids, 8, align=16),
                 lambda: moe.moe_permute(x, ss, 2), lambda: moe.moe_permute_forward(x, ss, 2, scale=w),
                 lambda: moe.moe_combine(y, w, ids), lambda: moe.moe_combine_forward(y, None, ids),
                 lambda: moe.moe_combine_backward(x, y, w, ids)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()


def test_torch_op_schemas_and_fake_implementations():
    """all six ops are functional; the fake implementations give the shapes - M_max = T K + E (align - 1) included - dtypes and
    contiguous strides"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    import flash_attn_mi355.torch_ops as T
    ns = torch.ops.flash_attn_mi355
    names = ("moe_route", "moe_route_bwd", "moe_sort", "moe_permute", "moe_combine", "moe_combine_bwd")
    sch = {n: getattr(ns, n).default._schema for n in names}
    for n in names:
        assert not [a.name for a in sch[n].arguments if a.alias_info is not None], n
        assert n not in T.__all__                            # reached through torch.ops only
    assert [a.name for a in sch["moe_route"].arguments] == ["logits", "k", "scoring", "renormalize", "bias", "scale"]
    assert [a.name for a in sch["moe_sort"].arguments] == ["ids", "num_experts", "align"]
    assert [len(sch[n].returns) for n in names] == [2, 1, 3, 1, 1, 2]
    with FakeTensorMode():
        for dt in (torch.float16, torch.bfloat16):
            Tn, E, K, N, align = 67, 60, 6, 264, 16
            logits = torch.empty(Tn, 64, dtype=dt, device="cuda")[:, :E]
            w, ids = ns.moe_route(logits, K, "softmax", True, None, 1.0)
            assert w.shape == (Tn, K) and w.dtype == torch.float32 and ids.shape == (Tn, K) and ids.dtype == torch.int32
            dl = ns.moe_route_bwd(w, logits, ids, "softmax", True, None, 1.0)
            assert dl.shape == (Tn, E) and dl.dtype == dt and dl.is_contiguous()
            sorted_slot, pos, offsets = ns.moe_sort(ids, E, align)
            M = Tn * K + E * (align - 1)
            assert sorted_slot.shape == (M,) and pos.shape == (Tn, K) and offsets.shape == (E + 1,)
            assert sorted_slot.dtype == pos.dtype == offsets.dtype == torch.int32
            x = torch.empty(Tn, N, dtype=dt, device="cuda")
            xp = ns.moe_permute(x, sorted_slot, K, None, pos)
            assert xp.shape == (M, N) and xp.dtype == dt and xp.is_contiguous()
            out = ns.moe_combine(xp, w, pos)
            assert out.shape == (Tn, N) and out.dtype == dt
            dy, dw = ns.moe_combine_bwd(out, xp, w, pos, True, True)
            assert dy.shape == (M, N) and dy.dtype == dt and dw.shape == (Tn, K) and dw.dtype == torch.float32
            dy, dw = ns.moe_combine_bwd(out, xp, w, pos, False, True)
            assert tuple(dy.shape) == (0,) and dw.shape == (Tn, K)


def test_public_name_lists_are_unchanged():
    import flash_attn
    import flash_attn_mi355
    import flash_attn_mi355.torch_ops as T
    for name in ("moe", "moe_route", "moe_sort", "moe_permute", "moe_combine", "moe_route_forward", "moe_combine_forward"):
        assert name not in flash_attn.__all__ and name not in flash_attn_mi355.__all__ and name not in T.__all__
    assert T.__all__ == ["fwd", "bwd", "varlen_fwd", "varlen_bwd", "fwd_kvcache", "fwd_kvcache_tree", "fwd_out", "varlen_fwd_out",
                         "bwd_out", "merge_states", "rotary", "rotary_", "kv_store"]
    from flash_attn_mi355 import moe
    for name in ("moe_route", "moe_route_forward", "moe_route_backward", "moe_sort", "moe_permute", "moe_permute_forward",
                 "moe_combine", "moe_combine_forward", "moe_combine_backward"):
        assert callable(getattr(moe, name))
