"""GPU: the standalone rotary embedding (csrc/fa_rotary.hip behind flash_attn.layers.rotary) against the fp64 reference of
rotary_ref.py on the same 16-bit inputs, and bit for bit against the kv-cache op's in-kernel RoPE, against itself (in place /
out of place, fast form / general form, dense / packed, one launch / two halves) and inside guard bands.

Bound (rotary_ref.bound; derived, not fitted): |y - y64| <= u |y64| + 2^-22 (|x0 c| + |x1 s|) + f per element - one rounding to the
io type, the fp32 evaluation of two products and one fused add, half of fp16's subnormal spacing."""
import numpy as np
import pytest
import torch

import guard
import rotary_ref as rr
from util import DT, assert_close, f64, rand16

pytestmark = pytest.mark.gpu

# (B, S, H, D, rotary_dim): the smallest shapes at which each path can go wrong
SHAPES = [(2, 5, 3, 64, 64), (2, 70, 3, 64, 32), (2, 70, 3, 64, 16), (1, 33, 2, 128, 128), (2, 9, 2, 80, 32),
          (2, 9, 2, 96, 24), (1, 17, 1, 256, 256)]
DTYPES = ["fp16", "bf16"]
# the kernel's own launch constants (csrc/fa_rotary.hip)
ROT_MAX_GROUP_ROWS, ROT_GRID_CAP = 16, 256 * 16


def R():
    from flash_attn.layers import rotary
    return rotary


def tables(seqlen_ro, rd, dtype, seed=5, device="cuda"):
    """cos / sin [seqlen_ro, rd / 2] of random angles, rounded to the io dtype"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ang = torch.rand(seqlen_ro, rd // 2, generator=g, dtype=torch.float64) * (2 * np.pi)
    return torch.cos(ang).to(DT[dtype]).to(device), torch.sin(ang).to(DT[dtype]).to(device)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(guard.bits(a.contiguous()), guard.bits(b.contiguous()))


def check_bound(y, x, cos, sin, pos, interleaved, dtype, name, conjugate=False):
    y64, mag = rr.rotary_ref(x, cos, sin, pos, interleaved, conjugate)
    ratio = rr.worst_ratio(y, y64, mag, DT[dtype])
    print(f"{name}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: error is {ratio:.3f} x the derived bound"
    return ratio


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 7])
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_against_fp64_reference(dtype, shape, interleaved, offset):
    B, S, H, D, rd = shape
    x = rand16((B, S, H, D), dtype, 11)
    cos, sin = tables(S + 7, rd, dtype)
    y = R().apply_rotary_emb(x, cos, sin, interleaved=interleaved, seqlen_offsets=offset)
    assert y.data_ptr() != x.data_ptr() and y.shape == x.shape and y.dtype == x.dtype
    check_bound(y, x, cos, sin, rr.positions(B, S, offset), interleaved, dtype, f"{dtype} {shape} il={interleaved} off={offset}")
    assert same_bits(y[..., rd:], x[..., rd:])


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("D,rd", [(64, 64), (128, 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_exact_against_the_kvcache_ops_rope(dtype, D, rd, interleaved):
    from flash_attn import flash_attn_with_kvcache
    B, T, H, cap = 2, 4, 2, 32
    q, k, v = (rand16((B, T, H, D), dtype, s) for s in (21, 22, 23))
    kc0, vc0 = rand16((B, cap, H, D), dtype, 24), rand16((B, cap, H, D), dtype, 25)
    cos, sin = tables(cap, rd, dtype)
    lens = torch.tensor([3, 11], dtype=torch.int32, device="cuda")
    kc, vc = kc0.clone(), vc0.clone()
    out = flash_attn_with_kvcache(q, kc, vc, k=k, v=v, rotary_cos=cos, rotary_sin=sin, cache_seqlens=lens, causal=True,
                                  rotary_interleaved=interleaved)
    k_rot = R().apply_rotary_emb(k, cos, sin, interleaved=interleaved, seqlen_offsets=lens)
    q_rot = R().apply_rotary_emb(q, cos, sin, interleaved=interleaved, seqlen_offsets=lens)
    for b, L in enumerate([3, 11]):
        assert same_bits(kc[b, L:L + T], k_rot[b]), f"appended k rows of batch {b}"
    kc2, vc2 = kc0.clone(), vc0.clone()
    out2 = flash_attn_with_kvcache(q_rot, kc2, vc2, k=k_rot, v=v, cache_seqlens=lens, causal=True)
    assert same_bits(kc, kc2) and same_bits(vc, vc2)
    assert same_bits(out, out2)


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_inplace_equals_out_of_place(dtype, shape, interleaved):
    B, S, H, D, rd = shape
    x = rand16((B, S, H, D), dtype, 31)
    cos, sin = tables(S + 3, rd, dtype)
    y = R().apply_rotary_emb(x, cos, sin, interleaved=interleaved, seqlen_offsets=3)
    xi = x.clone()
    yi = R().apply_rotary_emb(xi, cos, sin, interleaved=interleaved, inplace=True, seqlen_offsets=3)
    assert yi.data_ptr() == xi.data_ptr()
    assert same_bits(yi, y)
    assert same_bits(yi[..., rd:], x[..., rd:])


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[4] % 16 == 0], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_fast_form_equals_general_form(dtype, shape, interleaved, inplace):
    B, S, H, D, rd = shape
    x = rand16((B, S, H, D), dtype, 41)
    cos, sin = tables(S, rd, dtype)
    y = R().apply_rotary_emb(x.clone(), cos, sin, interleaved=interleaved, inplace=inplace)
    # the same problem one element further: a 2-byte aligned base
    buf = torch.zeros(x.numel() + 8, dtype=x.dtype, device="cuda")
    xs = buf[1:1 + x.numel()].view(x.shape)
    xs.copy_(x)
    assert xs.data_ptr() % 16 == 2
    ys = R().apply_rotary_emb(xs, cos, sin, interleaved=interleaved, inplace=inplace)
    assert same_bits(ys, y)
    assert int(guard.bits(buf)[0]) == 0 and not guard.bits(buf)[1 + x.numel():].any()
    # 16-bit cos / sin against their exact fp32 upcasts
    y32 = R().apply_rotary_emb(x.clone(), cos.float(), sin.float(), interleaved=interleaved, inplace=inplace)
    assert same_bits(y32, y)


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("rd,fp32_tables", [(64, False), (24, False), (64, True)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_offsets_and_the_table_edge(dtype, rd, fp32_tables, interleaved):
    B, S, H, D, ro = 2, 12, 2, 64 if rd == 64 else 96, 20
    x = rand16((B, S, H, D), dtype, 51)
    c, s = tables(ro, rd, dtype)
    tdt = torch.float32 if fp32_tables else DT[dtype]
    # cos / sin between NaN bands: a read past the table poisons the result
    _, cos = guard.slab((ro, rd // 2), tdt, gaps=False, device="cuda", check_prep=False)
    _, sin = guard.slab((ro, rd // 2), tdt, gaps=False, device="cuda", check_prep=False)
    cos.copy_(c)
    sin.copy_(s)
    offs = torch.tensor([0, 13], dtype=torch.int32, device="cuda")
    for inplace in (False, True):
        y = R().apply_rotary_emb(x.clone(), cos, sin, interleaved=interleaved, inplace=inplace, seqlen_offsets=offs)
        assert torch.isfinite(y.float()).all()
        assert same_bits(y[1, ro - 13:], x[1, ro - 13:]), "rows at positions >= seqlen_ro must come back unrotated"
        check_bound(y, x, c, s, rr.positions(B, S, [0, 13]), interleaved, dtype, f"{dtype} rd={rd} edge inplace={inplace}")


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_offsets", [False, True])
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("D,rd", [(64, 64), (96, 24)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_varlen_equals_per_sequence_dense_calls(dtype, D, rd, interleaved, with_offsets):
    cu_l, max_seqlen, H = [0, 3, 3, 40, 41], 37, 2
    offs_l = [2, 0, 5, 1] if with_offsets else [0, 0, 0, 0]
    x = rand16((cu_l[-1], H, D), dtype, 61)
    cos, sin = tables(64, rd, dtype)
    cu = torch.tensor(cu_l, dtype=torch.int32, device="cuda")
    offs = torch.tensor(offs_l, dtype=torch.int32, device="cuda") if with_offsets else 0
    y = R().apply_rotary_emb(x, cos, sin, interleaved=interleaved, seqlen_offsets=offs, cu_seqlens=cu, max_seqlen=max_seqlen)
    parts = [R().apply_rotary_emb(x[cu_l[b]:cu_l[b + 1]][None], cos, sin, interleaved=interleaved, seqlen_offsets=offs_l[b])[0]
             for b in range(4)]
    assert same_bits(y, torch.cat(parts))
    check_bound(y, x, cos, sin, rr.positions(4, 0, offs_l, cu_l), interleaved, dtype, f"{dtype} varlen D={D}")
    xi = x.clone()
    R().apply_rotary_emb(xi, cos, sin, interleaved=interleaved, inplace=True, seqlen_offsets=offs, cu_seqlens=cu, max_seqlen=max_seqlen)
    assert same_bits(xi, y)


# 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_entry_points(dtype, interleaved):
    rot = R()
    cos, sin = tables(16, 64, dtype)
    cos_k, sin_k = tables(16, 32, dtype, seed=6)
    one = lambda t, c=cos, s=sin: rot.apply_rotary_emb(t, c, s, interleaved=interleaved, seqlen_offsets=2)
    qkv = rand16((2, 9, 3, 4, 64), dtype, 71)
    for ck, sk in ((None, None), (cos_k, sin_k)):
        got = rot.apply_rotary_emb_qkv_(qkv.clone(), cos, sin, cos_k=ck, sin_k=sk, interleaved=interleaved, seqlen_offsets=2)
        assert same_bits(got[:, :, 0], one(qkv[:, :, 0]))
        assert same_bits(got[:, :, 1], one(qkv[:, :, 1]) if ck is None else one(qkv[:, :, 1], ck, sk))
        assert same_bits(got[:, :, 2], qkv[:, :, 2])
    gqa = rand16((2, 9, 4 + 2 * 2, 64), dtype, 72)
    got = rot.apply_rotary_emb_qkv_(gqa.clone(), cos, sin, interleaved=interleaved, seqlen_offsets=2, num_heads_q=4)
    assert same_bits(got[:, :, :6], one(gqa[:, :, :6])) and same_bits(got[:, :, 6:], gqa[:, :, 6:])
    got = rot.apply_rotary_emb_qkv_(gqa.clone(), cos, sin, cos_k=cos_k, sin_k=sin_k, interleaved=interleaved, seqlen_offsets=2,
                                    num_heads_q=4)
    assert same_bits(got[:, :, :4], one(gqa[:, :, :4])) and same_bits(got[:, :, 4:6], one(gqa[:, :, 4:6], cos_k, sin_k))
    assert same_bits(got[:, :, 6:], gqa[:, :, 6:])
    kv = rand16((2, 9, 2, 2, 64), dtype, 73)
    got = rot.apply_rotary_emb_kv_(kv.clone(), cos, sin, interleaved=interleaved, seqlen_offsets=2)
    assert same_bits(got[:, :, 0], one(kv[:, :, 0])) and same_bits(got[:, :, 1], kv[:, :, 1])


# 8 ------------------------------------------------------------------------------------------------------------------------
def _pair_sum(a, rd, interleaved):
    """per element: its own value plus its rotation partner's (columns behind rd: its own)"""
    out = a.copy()
    if interleaved:
        s = a[..., 0:rd:2] + a[..., 1:rd:2]
        out[..., 0:rd:2], out[..., 1:rd:2] = s, s
    else:
        s = a[..., :rd // 2] + a[..., rd // 2:rd]
        out[..., :rd // 2], out[..., rd // 2:rd] = s, s
    return out


@pytest.mark.parametrize("varlen", [False, True])
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients(dtype, interleaved, varlen):
    """dx is the conjugate rotation of dout: held to case 1's bound on dout against the fp64 reference; the fp32 torch
    restatement's autograd gradient is held to its own fp32 error (three roundings: 2^-22 of the magnitude) against the same
    reference, so kernel and restatement are compared through the exact value."""
    H, D, rd = 2, 64, 32
    cos, sin = tables(64, rd, dtype)
    if varlen:
        cu_l = [0, 3, 3, 40, 41]
        shape, pos = (cu_l[-1], H, D), rr.positions(4, 0, 5, cu_l)
        kw = dict(cu_seqlens=torch.tensor(cu_l, dtype=torch.int32, device="cuda"), max_seqlen=37, seqlen_offsets=5)
    else:
        shape, pos = (2, 9, H, D), rr.positions(2, 9, 5)
        kw = dict(seqlen_offsets=5)
    x = rand16(shape, dtype, 81).requires_grad_()
    dout = rand16(shape, dtype, 82)
    y = R().apply_rotary_emb(x, cos, sin, interleaved=interleaved, **kw)
    (dx,) = torch.autograd.grad(y, x, dout)
    assert dx.data_ptr() != dout.data_ptr()
    check_bound(dx, dout, cos, sin, pos, interleaved, dtype, f"{dtype} dx varlen={varlen}", conjugate=True)
    x32 = x.detach().float().requires_grad_()
    (dx32,) = torch.autograd.grad(rr.rotate_torch(x32, cos, sin, torch.from_numpy(pos).cuda(), interleaved), x32, dout.float())
    g64, mag = rr.rotary_ref(dout, cos, sin, pos, interleaved, conjugate=True)
    assert np.all(np.abs(f64(dx32) - g64) <= 2.0 ** -22 * mag)
    # rotate, then conjugate: x again.  Each step contributes its bound once ("twice the bound"): the first step's error
    # reaches an element through the second rotation, |c| e0 + |s| e1 <= e0 + e1 over its pair.  The tables themselves are
    # rounded to 16 bits, so the two exact rotations compose to (c^2 + s^2) x: that defect of the INPUT tables, exact in fp64,
    # is the reference's own distance from x and joins the bound
    z = R().apply_rotary(y.detach(), cos, sin, interleaved=interleaved, conjugate=True, **kw)
    y64, mag_y = rr.rotary_ref(x, cos, sin, pos, interleaved)
    b1 = _pair_sum(rr.bound(y64, mag_y, DT[dtype]), rd, interleaved)
    z64, mag_z = rr.rotary_ref(y, cos, sin, pos, interleaved, conjugate=True)
    b2 = rr.bound(z64, mag_z, DT[dtype])
    err = np.abs(f64(z) - f64(x))
    b3 = rr.table_defect(cos, sin, pos, interleaved, D) * np.abs(f64(x))
    ratio = float(np.max(err[..., :rd] / (b1 + b2 + b3)[..., :rd]))
    print(f"{dtype} rotate-then-conjugate: worst |err| / (bound + bound) = {ratio:.3f}")
    assert ratio <= 1.0 and same_bits(z[..., rd:], x[..., rd:])


def test_torch_library_op_autograd_and_opcheck():
    import flash_attn_mi355.torch_ops  # noqa: F401  (registers the ops)
    op = torch.ops.flash_attn_mi355.rotary
    x = rand16((2, 9, 2, 64), "bf16", 91).requires_grad_()
    dout = rand16((2, 9, 2, 64), "bf16", 92)
    cos, sin = tables(16, 32, "bf16")
    offs = torch.tensor([1, 4], dtype=torch.int32, device="cuda")
    y = op(x, cos, sin, offs, None, 0, 0, False, False)
    assert same_bits(y, R().apply_rotary_emb(x.detach(), cos, sin, seqlen_offsets=offs))
    (dx,) = torch.autograd.grad(y, x, dout)
    assert same_bits(dx, R().apply_rotary(dout, cos, sin, seqlen_offsets=offs, conjugate=True))
    xi = x.detach().clone()
    torch.ops.flash_attn_mi355.rotary_(xi, cos, sin, offs, None, 0, 0, False, False)
    assert same_bits(xi, y)
    torch.library.opcheck(op, (x.detach(), cos, sin, offs, None, 0, 0, False, False))
    torch.library.opcheck(op, (x.detach().requires_grad_(), cos, sin, None, None, 3, 0, True, False),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    torch.library.opcheck(torch.ops.flash_attn_mi355.rotary_, (x.detach().clone(), cos, sin, offs, None, 0, 0, False, False))


# 9 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("case", ["dense", "varlen", "qkv", "gqa", "kv"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_guard_bands(dtype, case, interleaved):
    rot = R()
    cos, sin = tables(48, 32, dtype)
    if case in ("dense", "varlen"):
        cu_l = [0, 3, 3, 40, 41]
        kw = {} if case == "dense" else dict(cu_seqlens=torch.tensor(cu_l, dtype=torch.int32, device="cuda"), max_seqlen=37)
        data = rand16((2, 9, 3, 64) if case == "dense" else (41, 3, 64), dtype, 95)
        want = rot.apply_rotary_emb(data, cos, sin, interleaved=interleaved, seqlen_offsets=2, **kw)
        xbuf, x, xsnap = guard.guarded(data)
        obuf, o, osnap = guard.guarded(shape=data.shape, dtype=DT[dtype], device="cuda")
        # out of place into a NaN-filled slab: every logical element is written, nothing else
        from flash_attn_mi355 import rotary as impl
        impl._launch(x, o, cos, sin, interleaved, False, 2, kw.get("cu_seqlens"), kw.get("max_seqlen"))
        torch.cuda.synchronize()
        assert torch.equal(guard.bits(xbuf), xsnap)
        guard.assert_untouched(obuf, o, osnap, "out")
        assert same_bits(o, want)
        # in place
        rot.apply_rotary_emb(x, cos, sin, interleaved=interleaved, inplace=True, seqlen_offsets=2, **kw)
        torch.cuda.synchronize()
        guard.assert_untouched(xbuf, x, xsnap, "x in place")
        assert same_bits(x, want)
        return
    shape, row_dim = {"qkv": ((2, 9, 3, 4, 64), 1), "gqa": ((2, 9, 8, 64), 1), "kv": ((2, 9, 2, 2, 64), 1)}[case]
    data = rand16(shape, dtype, 96)
    buf, view = guard.slab(shape, DT[dtype], gaps=True, device="cuda", check_prep=False, row_dim=row_dim)
    view.copy_(data)
    snap = guard.snapshot(buf)
    if case == "kv":
        want = rot.apply_rotary_emb_kv_(data.clone(), cos, sin, interleaved=interleaved, seqlen_offsets=2)
        rot.apply_rotary_emb_kv_(view, cos, sin, interleaved=interleaved, seqlen_offsets=2)
    else:
        nq = 4 if case == "gqa" else None
        want = rot.apply_rotary_emb_qkv_(data.clone(), cos, sin, interleaved=interleaved, seqlen_offsets=2, num_heads_q=nq)
        rot.apply_rotary_emb_qkv_(view, cos, sin, interleaved=interleaved, seqlen_offsets=2, num_heads_q=nq)
    torch.cuda.synchronize()
    guard.assert_untouched(buf, view, snap, case)
    assert same_bits(view, want)


# 10 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True])
def test_grid_stride(inplace):
    """H 1, D 64 NeoX: 4 items per row, so a workgroup step takes ROT_MAX_GROUP_ROWS = 16 rows and the grid is capped at
    ROT_GRID_CAP = 4096 steps = 65536 rows.  2 x 33000 rows (8.4 MB) are 4125 steps: the last 29 are reached by the grid stride
    only; each half (2063 steps) fits the grid."""
    B, S = 2, 33000
    assert B * S > ROT_MAX_GROUP_ROWS * ROT_GRID_CAP > S
    x = rand16((B, S, 1, 64), "bf16", 101)
    cos, sin = tables(S, 64, "bf16")
    y = R().apply_rotary_emb(x.clone(), cos, sin, inplace=inplace)
    halves = [R().apply_rotary_emb(x[b:b + 1].clone(), cos, sin, inplace=inplace) for b in range(B)]
    assert same_bits(y, torch.cat(halves))
    assert not same_bits(y[1, -16:], x[1, -16:])


# 11 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rotary_embedding_then_attention(dtype):
    import oracle
    from flash_attn import flash_attn_qkvpacked_func
    B, S, H, D = 2, 33, 2, 64
    qkv = rand16((B, S, 3, H, D), dtype, 111)
    m = R().RotaryEmbedding(D, device="cuda")
    rot = m(qkv.clone())
    assert same_bits(rot[:, :, 2], qkv[:, :, 2])
    out = flash_attn_qkvpacked_func(rot, causal=True)
    pos = rr.positions(B, S)
    q64 = rr.rotary_ref(qkv[:, :, 0], m._cos_cached, m._sin_cached, pos, False)[0]
    k64 = rr.rotary_ref(qkv[:, :, 1], m._cos_cached, m._sin_cached, pos, False)[0]
    t = lambda a: np.asarray(a).transpose(0, 2, 1, 3)
    ref = oracle.attn_fwd(t(q64), t(k64), t(f64(qkv[:, :, 2])), D ** -0.5, causal=True)[0]
    assert_close(t(f64(out)), ref, dtype, "RotaryEmbedding -> flash_attn_qkvpacked_func")
