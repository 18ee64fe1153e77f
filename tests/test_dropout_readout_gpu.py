"""The dropout keep mask read back from every kernel that replays it (tests/dropout_readout.py), bit by bit.

Each case runs call A (dQ and dK carry the dQ kernel's and the dK/dV kernel's dS-side mask) and call B (O and dV carry the
forward's and the dK/dV kernel's P-side mask) through flash_attn_func / flash_attn_varlen_func with autograd, in fp16 and
bf16, with (seed, offset) read from the default generator before each call, and asserts
  (i)   the four decoded masks and the sign pattern of `dmask` equal oracle.dropout_keep_mask AND visible - bitwise, on
        every visible element (dmask: +1 kept, -1 dropped, never 0 there);
  (ii)  worst |got - ref| / gate <= 1, the gate a quarter of what the element's own bit does to it (a wrong bit: 4.0);
  (iii) the full tensors inside util.assert_close at the dropout multipliers (out 1.5, gradients 3);
  (iv)  the LSE (pre-dropout: log n, or the ALiBi profile's) inside assert_lse_close at LSE_ATOL.
tests/test_dropout_readout_cpu.py proves the data on the oracle: 16-bit rounding alone stays below 0.025 of a gate.

Case -> kernels, read from launch_fwd_td (csrc/fa_fwd.hip) and plan_bwd / launch_bwd_td (csrc/fa_bwd.hip).  With dropout
neither the hand-scheduled forward, dQ and dK/dV kernels nor the dS hand-off apply (fwd_asm_applicable,
bwd_dq_asm_applicable, bwd_asm_applicable and bwd_ds_workspace_bytes all refuse p_dropout > 0), no dK/dV launch is
split, and the kernel width is the head dim padded to 64 / 128 / 256 with DV = 96 (width 128, head dim <= 96) or 192
(width 256, head dim <= 192) columns of V / dO / O in the forward and dQ:
  head dim  bias   forward                        dQ                               dK/dV
  32, 64    no     fa_fwd<64,0,false,true>        fa_bwd_dq<64,0,1,true>           fa_bwd_dkdv2<64,0,true>
  96        no     fa_fwd<128,0,false,true,96>    fa_bwd_dq<128,0,1,true,96>       fa_bwd_dkdv2<128,0,true,96>
  128       no     fa_fwd<128,0,false,true>       fa_bwd_dq<128,0,1,true>          fa_bwd_dkdv2<128,0,true>
  160, 192  no     fa_fwd<256,0,false,true,192>   fa_bwd_dq<256,0,1,true,192>      fa_bwd_dkdv<256,0,true>
  256       no     fa_fwd<256,0,false,true>       fa_bwd_dq<256,0,1,true>          fa_bwd_dkdv<256,0,true>
  64        ALiBi  fa_fwd<64,1,false,true>        fa_bwd_dq<64,1,1,true>           fa_bwd_dkdv<64,1,true>
  96        ALiBi  fa_fwd<128,1,false,true,96>    fa_bwd_dq<128,1,1,true,96>       fa_bwd_dkdv<128,1,true>
  128       ALiBi  fa_fwd<128,1,false,true>       fa_bwd_dq<128,1,1,true>          fa_bwd_dkdv<128,1,true>
  160       ALiBi  fa_fwd<256,1,false,true,192>   fa_bwd_dq<256,1,1,true,192>      fa_bwd_dkdv<256,1,true>
  256       ALiBi  fa_fwd<256,1,false,true>       fa_bwd_dq<256,1,1,true>          fa_bwd_dkdv<256,1,true>
(names without the _kernel suffix and the io type; the dense, GQA, carry and varlen families are the "no" rows of their
head dim, the alibi family and varlen_alibi_d128_causal the "ALiBi" rows; causal, window and full masks share a kernel.)

Worst |got - ref| / gate per family and channel on the MI355X (printed when the module finishes; 1.0 is the gate, a
wrong bit is 4.0), fp16 and bf16 together, all 86 tests passing, then the largest fraction used of the assert_close
gates of (iii) per io type and of LSE_ATOL:
  family                                               o      dq     dk     dv     close fp16 / bf16   lse
  dense   (12 shapes, head dims 32 .. 256)             0.016  0.031  0.031  0.026  0.468 / 0.512       0.010
  alibi   (D 64 / 96 / 128 / 160 / 256, [H], [B, H])   0.029  0.032  0.032  0.023  0.398 / 0.536       0.010
  gqa     (4 : 1 and 8 : 1, D 64 and 128)              0.014  0.031  0.031  0.026  0.468 / 0.512       0.010
  carry   (offset 2^32 - 64, D 64 and 128)             0.014  0.019  0.019  0.014  0.296 / 0.331       0.010
  varlen  (q 70 0 5 130, k 33 7 131 64; max_k + 6, 29) 0.023  0.029  0.029  0.023  0.346 / 0.434       0.010
  entry   (qkvpacked, kvpacked, torch.ops fwd / bwd)   0.014  0.023  0.023  0.022  0.398 / 0.462       0.010
No kernel read a bit differently from the oracle, so no kernel changed.  What the channels show is rounding: the saved
16-bit O (D_i is its row sum here, so its last bit moves every dS of the row by 2^-9 .. 2^-8 of the level) and the 16-bit
P and dS operands of the matrix pipe; on the oracle the io rounding alone gives 0.016 / 0.025 (o / dq) and 0.42 of the bf16
assert_close gate.  tests/test_dropout_gpu.py's dense LSE check now uses assert_lse_close at LSE_ATOL (5e-5) instead of
2e-3: the dropout forward passes it (here it lands 5e-7 from log n).

Wall time on the MI355X (pytest's own totals, references included): this file 6.6 s for its 86 tests (the slowest 1.1 s,
the first to touch the GPU).  The GPU suite with it: 2496 tests in 381 s, run as two halves of 190.5 s and 190.9 s;
before it 2405 tests in about 371 s (the rest is the fuzz kind `dropout`, 24 cases in 3.9 s).
"""
import functools

import numpy as np
import pytest
import torch

import dropout_readout as dr
from util import DT, LSE_ATOL, TOL_FRO, TOL_MAXREL, assert_close, assert_lse_close, errs, f64

pytestmark = pytest.mark.gpu

WORST = {}                                                        # family -> {quantity: (ratio, case)}


def _fa():
    import flash_attn
    return flash_attn


def _gen():
    dev = torch.cuda.current_device()                              # (initialises the runtime: the tuple below is empty before)
    return torch.cuda.default_generators[dev]


def _record(fam, what, r, cid):
    d = WORST.setdefault(fam, {})
    if r > d.get(what, (-1.0, ""))[0]:
        d[what] = (r, cid)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam, d in WORST.items():
        print(f"\nreadout {fam}: worst  " + "  ".join(f"{k} {r:.3f} [{c}]" for k, (r, c) in sorted(d.items())))


@functools.lru_cache(maxsize=None)
def _ref(name, call, seed, offset):
    """the oracle's outputs and the expected mask: computed once, shared by both io types and the entry-point tests"""
    c = dr.BY_NAME[name]
    ref = c.reference(call, seed, offset)
    for a in ref.values():
        a.setflags(write=False)
    return ref, c.expected(seed, offset)


def _dev(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DT[dt]).cuda()


def _launch(c, call, dt, entry):
    """One forward + backward on the GPU: dict o, lse, dq, dk, dv (fp64 numpy, the op's layout) and dmask"""
    x = {k: _dev(a, dt) for k, a in c.build(call).items()}
    s = c.slopes(call)
    slopes = None if s is None else torch.from_numpy(s).cuda()
    kw = dict(dropout_p=c.p, causal=c.causal, window_size=c.window, alibi_slopes=slopes)
    q, k, v, do = x["q"], x["k"], x["v"], x["do"]
    if entry == "torch_ops":
        import flash_attn_mi355.torch_ops  # noqa: F401  (registers the ops)
        ops = torch.ops.flash_attn_mi355
        seed, offset = _gen().initial_seed(), _gen().get_offset()
        out, lse, dmask, rng_state = ops.fwd(q, k, v, slopes, c.p, c.scale, c.causal, c.window[0], c.window[1], 0.0, True)
        assert rng_state.tolist() == [seed, offset], "the forward op returns the (seed, offset) it drew"
        # (the generator has moved on: a backward that drew from it instead of rng_state would replay another mask)
        dq, dk, dv, _ = ops.bwd(do, q, k, v, out, lse, slopes, c.p, c.scale, c.causal, c.window[0], c.window[1], 0.0, False,
                                rng_state)
    elif entry == "qkvpacked":
        qkv = torch.stack([q, k, v], dim=2).requires_grad_(True)
        out, lse, dmask = _fa().flash_attn_qkvpacked_func(qkv, return_attn_probs=True, **kw)
        dq, dk, dv = torch.autograd.grad(out, qkv, do)[0].unbind(dim=2)
    elif entry == "kvpacked":
        q.requires_grad_(True)
        kv = torch.stack([k, v], dim=2).requires_grad_(True)
        out, lse, dmask = _fa().flash_attn_kvpacked_func(q, kv, return_attn_probs=True, **kw)
        dq, dkv = torch.autograd.grad(out, (q, kv), do)
        dk, dv = dkv.unbind(dim=2)
    else:
        for t in (q, k, v):
            t.requires_grad_(True)
        if c.varlen:
            cu_q, cu_k = torch.from_numpy(c.cu_q).cuda(), torch.from_numpy(c.cu_k).cuda()
            out, lse, dmask = _fa().flash_attn_varlen_func(q, k, v, cu_q, cu_k, c.max_q, c.max_k, return_attn_probs=True, **kw)
        else:
            out, lse, dmask = _fa().flash_attn_func(q, k, v, return_attn_probs=True, **kw)
        dq, dk, dv = torch.autograd.grad(out, (q, k, v), do)
    torch.cuda.synchronize()
    return {"o": f64(out), "lse": f64(lse), "dq": f64(dq), "dk": f64(dk), "dv": f64(dv)}, f64(dmask)


def _dmask_blocks(c, dm):
    """dmask as [Hq, sq, sk] per sequence: dense [B, Hq, Sq, Sk] (every batch entry is a reading), varlen
    [T_q, Hq, max_seqlen_k]"""
    if not c.varlen:
        return [dm.reshape(-1, c.Sq, c.Sk)]
    assert dm.shape[2] == c.max_k
    return [dm[q0:q0 + sq, :, :sk].transpose(1, 0, 2) for q0, sq, _, sk in c.seqs()]


def _check(c, dt, entry="func", fam=None):
    fam = fam or dr.FAMILY[c.name]
    cid = f"{c.name} {dt}" + ("" if entry == "func" else f" {entry}")
    gen = _gen()
    saved = gen.get_state()
    try:
        torch.manual_seed(dr.SEED)
        for call, want in zip("AB", dr.offsets(c)):
            if c.offset is not None:
                gen.set_offset(c.offset)
            seed, offset = gen.initial_seed(), gen.get_offset()
            assert (seed, offset) == (dr.SEED, want), "the generator is not where the shared reference expects it"
            got, dm = _launch(c, call, dt, entry)
            B, Hq, _ = c.dims(call)
            assert gen.get_offset() == offset + B * Hq * 32        # what a call consumes (fused_mha_forward.cu:382-383)
            ref, keep = _ref(c.name, call, seed, offset)
            vis = c.visible()
            # (i) dmask, then the four channels
            assert dm.shape == ((B, Hq, c.Sq, c.Sk) if not c.varlen else (int(c.cu_q[-1]), Hq, c.max_k)), dm.shape
            assert set(np.unique(dm)).issubset({-1.0, 0.0, 1.0})
            for b, (blk, k, v) in enumerate(zip(_dmask_blocks(c, dm), keep, vis)):
                bad = np.argwhere(((blk > 0) != k[None]) & v[None])
                assert bad.size == 0, f"dmask differs from the oracle's mask at (reading, i, j) {bad[:4].tolist()} of " \
                                      f"sequence {b} [{cid} call {call}]"
                assert (blk != 0)[np.broadcast_to(v[None], blk.shape)].all(), f"dmask has unvisited visible elements [{cid}]"
            res = c.decode(call, ref, got, keep)
            for ch, (implied, worst, at) in res.items():
                print(f"{cid} call {call} {ch}: worst {worst:.4f} of the gate at (sequence, reading, i, j) {at}")
                _record(fam, ch, worst, cid)
            for ch, (implied, worst, at) in res.items():
                wrong = dr.wrong_bits(implied, keep)
                assert not wrong, f"{ch} reads {len(wrong)} keep bits differently from the oracle, first (sequence, reading, " \
                                  f"i, j) {wrong[:4]} [{cid} call {call}]"
                assert worst <= 1.0, f"{ch}: {worst:.3f} of the gate at (sequence, reading, i, j) {at} [{cid} call {call}]"   # (ii)
            # (iii) the whole tensors, (iv) the LSE
            for name, mult in (("o", 1.5), ("dq", 3.0), ("dk", 3.0), ("dv", 3.0)):
                mr, fro, _ = errs(got[name], ref[name])
                r = max(mr / (TOL_MAXREL[dt] * mult), fro / (TOL_FRO[dt] * mult))
                print(f"{cid} call {call} {name}: max-rel {mr:.2e} fro {fro:.2e} = {r:.3f} of the assert_close gate")
                _record(fam, f"close_{dt}", r, f"{cid} {call} {name}")
            for name, mult in (("o", 1.5), ("dq", 3.0), ("dk", 3.0), ("dv", 3.0)):
                assert_close(got[name], ref[name], dt, f"{name} [{cid} call {call}]", mult=mult)
            d = assert_lse_close(got["lse"], ref["lse"], f"lse [{cid} call {call}]", atol=LSE_ATOL)
            _record(fam, "lse", d / LSE_ATOL, cid)
    finally:
        gen.set_state(saved)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in dr.CASES])
def test_every_kernel_replays_the_oracles_mask(name, dt):
    _check(dr.BY_NAME[name], dt)


# one read-out case each through the packed entry points (self-attention shape; Sq != Sk) and the torch.ops pair, whose
# backward must take the mask from the forward's returned rng_state
@pytest.mark.parametrize("entry,name,dt", [("qkvpacked", "d64_200x200_causal", "bf16"),
                                           ("kvpacked", "d64_130x203_full", "fp16"),
                                           ("torch_ops", "d128_96x130_causal", "bf16"),
                                           ("torch_ops", "alibi_d64_130x131_full", "fp16")])
def test_entry_points_replay_the_oracles_mask(entry, name, dt):
    _check(dr.BY_NAME[name], dt, entry=entry, fam="entry")
