"""GPU: fa_merge_states (csrc/fa_merge.hip) against the fp64 merge rule of merge_ref.py on the same 16-bit inputs.

Gate (merge_ref.merge_gate; derived, not fitted): the rounding of the result to the output dtype - 2^-8 |ref| for bf16,
2^-10 |ref| + 2^-24 for fp16, the output-rounding terms of fp8_gate.OUT_ROUND - plus n 2^-22 max_s |out_s| for the fp32 weights
and sums; the LSE is held to util.LSE_ATOL."""
import ctypes

import numpy as np
import pytest
import torch

import guard
from merge_ref import merge_gate, merge_ref
from util import DT, LSE_ATOL, assert_lse_close, f64

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 3, 8), (2, 33, 3, 72), (1, 5, 2, 256), (3, 2, 8, 128)]


def _lib():
    from flash_attn_mi355 import _lib
    return _lib


def _slab8(shape, dtype):
    """a guard slab (NaN-filled bands and gaps, like guard.slab) whose base address and strides are multiples of 8 bytes and NOT
    of 16: the 8-byte path of the kernel"""
    B, S, H, D = shape
    hs = D + 4
    rs = H * hs + 4
    bs = S * rs + 4
    band = guard._up(max(guard.MAX_TILE_ROWS * rs, guard.MIN_BAND_BYTES // 2), 16)
    span = (B - 1) * bs + (S - 1) * rs + (H - 1) * hs + D
    buf = guard.fill_nan(torch.empty(band + 4 + span + band, dtype=dtype, device="cuda"))
    view = buf.as_strided(shape, (bs, rs, hs, 1), band + 4)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8
    return buf, view


def _o_slab(shape, dtype, layout):
    """(flat buf, view) of an o tensor: 'contig' (buf is the tensor), 'gaps' (guard.slab with gaps: 16-byte strides), 'align8'"""
    if layout == "contig":
        t = guard.fill_nan(torch.empty(shape, dtype=dtype, device="cuda"))
        return t.view(-1), t
    if layout == "gaps":
        return guard.slab(shape, dtype, gaps=True, device="cuda", check_prep=False)
    return _slab8(shape, dtype)


def _lse_slab(B, H, S, layout):
    """(buf, [B, H, S] view) of an fp32 LSE: 'bhs' contiguous, '1hbs' the dense op's [1, H, B S] read through strides,
    'gaps' a guard slab with gaps between rows, heads and batch entries"""
    if layout == "bhs":
        t = guard.fill_nan(torch.empty((B, H, S), dtype=torch.float32, device="cuda"))
        return t.view(-1), t
    if layout == "1hbs":
        t = guard.fill_nan(torch.empty((1, H, B * S), dtype=torch.float32, device="cuda"))
        return t.view(-1), t[0].view(H, B, S).permute(1, 0, 2)
    buf, v = guard.slab((B, H, S, 1), torch.float32, gaps=True, device="cuda", check_prep=False)
    return buf, v[..., 0]


def _call(parts, out, lse, dtype):
    lib = _lib()
    B, S, H, D = out.shape
    m = lib.FaMergeParams()
    m.struct_size = ctypes.sizeof(lib.FaMergeParams)
    m.n_parts, m.batch, m.seqlen, m.nheads, m.head_dim = len(parts), B, S, H, D
    m.dtype = lib.FA_BF16 if dtype == "bf16" else lib.FA_FP16
    for st, (o, l) in zip(m.parts, parts):
        lib.merge_state(st, o, l)
    lib.merge_state(m.out, out, lse)
    lib.call_merge(m, torch.cuda.current_stream().cuda_stream)


def _inputs(n, shape, dtype, seed):
    B, S, H, D = shape
    g = torch.Generator().manual_seed(seed)
    outs = [torch.randn(shape, generator=g).to(DT[dtype]) for _ in range(n)]
    lses = [torch.randn((B, H, S), generator=g) * 3.0 for _ in range(n)]
    return outs, lses


def _check(got_o, got_l, outs, lses, dtype, name):
    """got_o [B, S, H, D], got_l [B, H, S] against merge_ref on the same inputs (CPU tensors outs / lses)"""
    o_t = [f64(o).swapaxes(1, 2) for o in outs]
    l_t = [f64(l) for l in lses]
    ref_o, ref_l = merge_ref(o_t, l_t)
    got = f64(got_o).swapaxes(1, 2)
    assert np.isfinite(got).all(), f"{name}: non-finite (or unwritten) output"
    err, tol = np.abs(got - ref_o), merge_gate(ref_o, o_t, l_t, dtype)
    ratio = float((err / np.maximum(tol, 1e-300)).max())
    print(f"{name}: max |err| {err.max():.3e}, max err / gate {ratio:.3f}")
    assert (err <= tol).all(), f"{name}: error {ratio:.3f} x the gate"
    assert_lse_close(f64(got_l), ref_l, name + " lse", atol=LSE_ATOL)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("n", [2, 3, 8])
def test_merge_vs_reference_in_every_layout(n, shape, dtype):
    B, S, H, D = shape
    outs, lses = _inputs(n, shape, dtype, 100 * n + D)
    for o_layout, lse_in, lse_out in (("contig", "bhs", "bhs"), ("contig", "1hbs", "bhs"), ("gaps", "1hbs", "gaps"),
                                      ("gaps", "bhs", "1hbs"), ("align8", "bhs", "gaps"), ("align8", "1hbs", "bhs")):
        name = f"n{n} {shape} {dtype} o:{o_layout} lse:{lse_in}->{lse_out}"
        parts = []
        for i, (o, l) in enumerate(zip(outs, lses)):
            ob, ov = _o_slab(shape, DT[dtype], o_layout)
            ov.copy_(o)
            # (mixed LSE layouts in one call: the even parts take `lse_in`, the odd ones [B, H, S])
            lb, lv = _lse_slab(B, H, S, lse_in if i % 2 == 0 else "bhs")
            lv.copy_(l)
            parts.append((ov, lv))
        ob, ov = _o_slab(shape, DT[dtype], o_layout)
        lb, lv = _lse_slab(B, H, S, lse_out)
        snap_o, snap_l = guard.snapshot(ob), guard.snapshot(lb)
        _call(parts, ov, lv, dtype)
        torch.cuda.synchronize()
        guard.assert_untouched(ob, ov, snap_o, name + " out")
        guard.assert_untouched(lb, lv, snap_l, name + " lse")
        _check(ov, lv, outs, lses, dtype, name)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_minus_inf_parts_nan_and_bit_identity(n, dtype):
    """row r of every (batch, head): r % 4 == 0 all parts live, 1 one part -inf, 2 all but one -inf, 3 all -inf; the out of every
    -inf part holds NaN.  Rows with exactly one live part are that part's rows bit for bit (signed zeros included)."""
    shape = (2, 33, 3, 72)
    B, S, H, D = shape
    outs, lses = _inputs(n, shape, dtype, 7 + n)
    live = torch.ones((n, B, H, S), dtype=torch.bool)
    for r in range(S):
        if r % 4 == 1:
            live[r % n, :, :, r] = False
        elif r % 4 == 2:
            live[:, :, :, r] = False
            live[(r // 4) % n, :, :, r] = True
        elif r % 4 == 3:
            live[:, :, :, r] = False
    for s in range(n):
        lses[s][~live[s]] = float("-inf")
        outs[s][..., 0:D:9] = outs[s][..., 0:D:9] * 0.0                        # +0.0 and -0.0 among the values
        outs[s][(~live[s]).permute(0, 2, 1)] = float("nan")
    dev_o, dev_l = [o.cuda() for o in outs], [l.cuda() for l in lses]
    out = guard.fill_nan(torch.empty(shape, dtype=DT[dtype], device="cuda"))
    lse = guard.fill_nan(torch.empty((B, H, S), dtype=torch.float32, device="cuda"))
    _call(list(zip(dev_o, dev_l)), out, lse, dtype)
    torch.cuda.synchronize()
    _check(out, lse, outs, lses, dtype, f"n{n} {dtype} -inf patterns")
    out_c, lse_c = out.cpu(), lse.cpu()
    assert bool((outs[0].view(torch.int16) == -32768).any())                  # (the -0.0 pattern is really there)
    n_live = live.sum(0)                                                       # [B, H, S]
    for r in range(S):
        if r % 4 == 2:
            s = (r // 4) % n
            assert (n_live[:, :, r] == 1).all()
            assert torch.equal(out_c[:, r].view(torch.int16), outs[s][:, r].view(torch.int16)), f"row {r}: not part {s} bit for bit"
            assert torch.equal(lse_c[:, :, r].view(torch.int32), lses[s][:, :, r].view(torch.int32)), f"row {r}: LSE bits"
        elif r % 4 == 3:
            assert (out_c[:, r].view(torch.int16) == 0).all() and torch.isneginf(lse_c[:, :, r]).all(), f"row {r}"
    if n == 2:                                                                 # (one part -inf of two = exactly one live part)
        for r in range(1, S, 4):
            s = 1 - r % n
            assert torch.equal(out_c[:, r].view(torch.int16), outs[s][:, r].view(torch.int16)), f"row {r}"
    # the same through the Python function
    from flash_attn_mi355 import cascade
    out2, lse2 = cascade.merge_attention_states(dev_o, dev_l)
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16)) and torch.equal(lse2.view(torch.int32), lse.view(torch.int32))


def test_two_calls_are_bit_identical_and_the_python_function_takes_views():
    from flash_attn_mi355 import cascade
    shape, dtype, n = (3, 2, 8, 128), "bf16", 3
    B, S, H, D = shape
    outs, lses = _inputs(n, shape, dtype, 31)
    dev_o = [o.cuda() for o in outs]
    dev_l = [l.cuda() for l in lses]
    dev_l[0] = dev_l[0].permute(1, 0, 2).contiguous().view(1, H, B * S)[0].view(H, B, S).permute(1, 0, 2)   # [1, H, B S] storage
    wide = torch.zeros((B, S, H, 2 * D), dtype=DT[dtype], device="cuda")                                  # a column slice
    wide[..., D:] = dev_o[1]
    dev_o[1] = wide[..., D:]
    a = cascade.merge_attention_states(dev_o, dev_l)
    b = cascade.merge_attention_states(dev_o, dev_l)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _check(a[0], a[1], outs, lses, dtype, "python function on views")
    with pytest.raises(RuntimeError, match="2 .. 8"):
        cascade.merge_attention_states(dev_o[:1], dev_l[:1])
    with pytest.raises(RuntimeError, match="shape"):
        cascade.merge_attention_states(dev_o, [dev_l[0], dev_l[1], dev_l[2][:, :, :1]])
    with pytest.raises(RuntimeError, match="alias"):
        _call([(dev_o[0], dev_l[0]), (dev_o[2], dev_l[2])], dev_o[0], torch.empty_like(dev_l[2]), dtype)


def test_opcheck_on_the_merge_op():
    import flash_attn_mi355.torch_ops  # noqa: F401
    from flash_attn_mi355 import cascade
    outs, lses = _inputs(2, (2, 5, 4, 64), "fp16", 3)
    dev_o, dev_l = [o.cuda() for o in outs], [l.cuda() for l in lses]
    torch.library.opcheck(torch.ops.flash_attn_mi355.merge_states.default, (dev_o, dev_l),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    out, lse = torch.ops.flash_attn_mi355.merge_states(dev_o, dev_l)
    ref = cascade.merge_attention_states(dev_o, dev_l)
    assert torch.equal(out, ref[0]) and torch.equal(lse, ref[1])
