"""CPU: the fp8-e4m3 q / k / v forward (csrc/fa_fwd_fp8.hip) - ABI 4 fields, its argument checks through the C ABI (no device
work happens before them), the compiled code (block-scaled K = 64 MFMAs only, no spill, no scratch) and the fake op."""
import ctypes
import json
import os
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


def test_abi_4_appends_q_descale_and_o_dtype(lib):
    assert lib.lib.fa_abi_version() == 4 == lib.FA_ABI_VERSION
    assert lib.lib.fa_params_size() == ctypes.sizeof(lib.FaParams)
    names = [f[0] for f in lib.FaParams._fields_]
    assert names[-3:] == ["workspace_bytes", "q_descale", "o_dtype"]
    # appended: every ABI 3 field keeps its offset
    assert lib.FaParams.q_descale.offset >= lib.FaParams.workspace_bytes.offset + ctypes.sizeof(ctypes.c_size_t)


def _fp8_params(lib, buf):
    p = lib.FaParams()
    addr = (ctypes.addressof(buf) + 15) & ~15
    p.q = p.k = p.v = p.o = p.lse = addr
    p.batch, p.nheads_q, p.nheads_k, p.head_dim, p.seqlen_q, p.seqlen_k = 1, 2, 2, 128, 4, 4
    p.q_row_stride = p.k_row_stride = p.v_row_stride = p.o_row_stride = 256
    p.q_head_stride = p.k_head_stride = p.v_head_stride = p.o_head_stride = 128
    p.dtype = p.kv_dtype = lib.FA_FP8_E4M3
    p.o_dtype = lib.FA_BF16
    p.softmax_scale = 0.125
    p.window_left = p.window_right = -1
    return p


def test_fp8_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * 65536)()
    addr = (ctypes.addressof(buf) + 15) & ~15

    def fails(p, match, op="fa_fwd"):
        with pytest.raises(RuntimeError, match=match):
            lib.call(op, p, 0)

    p = _fp8_params(lib, buf)
    p.kv_dtype = lib.FA_FP16
    fails(p, "fp8-e4m3 k and v")
    p = _fp8_params(lib, buf)
    p.alibi_slopes = addr
    fails(p, r"failed \(-2\).*ALiBi")
    p = _fp8_params(lib, buf)
    p.softcap = 30.0
    fails(p, r"failed \(-2\).*softcap")
    p = _fp8_params(lib, buf)
    p.p_dropout = 0.1
    fails(p, r"failed \(-2\).*dropout")
    p = _fp8_params(lib, buf)
    p.head_dim = 256
    fails(p, r"failed \(-2\).*head dimension 256")
    p = _fp8_params(lib, buf)
    p.o_dtype = lib.FA_FP8_E4M3
    fails(p, r"failed \(-1\).*o_dtype")
    for name in ("q_descale", "k_descale", "v_descale"):
        for bad in (-1.0, float("inf"), float("nan")):
            p = _fp8_params(lib, buf)
            setattr(p, name, bad)
            fails(p, r"failed \(-1\).*descale")
    p = _fp8_params(lib, buf)
    p.head_dim_v = 72
    fails(p, "multiple of 16")
    # varlen: paged K/V with fp8 q
    cu = (ctypes.c_int32 * 2)(0, 4)
    p = _fp8_params(lib, buf)
    p.cu_seqlens_q = p.cu_seqlens_k = ctypes.addressof(cu)
    p.total_q, p.total_k = 4, 4
    p.block_table, p.page_block_size = addr, 16
    fails(p, r"failed \(-2\).*paged", op="fa_varlen_fwd")
    # the other ops reject fp8 q exactly as before (the 16-bit message)
    p = _fp8_params(lib, buf)
    p.dout = p.softmax_d = addr
    fails(p, "q must be fp16 or bf16", op="fa_bwd")
    p = _fp8_params(lib, buf)
    fails(p, "q must be fp16 or bf16", op="fa_fwd_kvcache")
    # an unknown dtype still names the 16-bit types on the forward ops too
    p = _fp8_params(lib, buf)
    p.dtype = 7
    fails(p, "fp16 or bf16")


def test_fp8_needs_no_workspace(lib):
    buf = (ctypes.c_char * 65536)()
    p = _fp8_params(lib, buf)
    p.is_causal = 1
    p.flags = lib.FA_FLAG_FWD_KEY_SPLIT
    assert lib.lib.fa_fwd_workspace_bytes(ctypes.byref(p)) == 0


def _disassemble(obj, wd):
    llvm = "/opt/rocm/lib/llvm/bin"
    fat, co = os.path.join(wd, "f.fat"), os.path.join(wd, "f.co")
    subprocess.run([f"{llvm}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj], check=True)
    subprocess.run([f"{llvm}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fat}", f"--output={co}", "--unbundle"], check=True)
    return subprocess.run([f"{llvm}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout


def test_fp8_kernel_runs_on_the_block_scaled_mfma(lib):
    import build
    obj = os.path.join(build.CSRC, "build", "fa_fwd_fp8.o")
    assert "fa_fwd_fp8.hip" in build.SOURCES and os.path.exists(obj)
    with tempfile.TemporaryDirectory() as wd:
        txt = _disassemble(obj, wd)
    assert txt.count("v_mfma_scale_f32_32x32x64_f8f6f4") >= 4 * 2 * 6        # four kernels, two unrolled stages, >= 6 each
    for other in ("v_mfma_f32_32x32x16_bf16", "v_mfma_f32_32x32x16_f16", "v_mfma_f32_32x32x16_fp8_fp8"):
        assert other not in txt, other


def test_fp8_kernels_do_not_spill(lib):
    import build
    res = json.load(open(build.RESOURCES))
    fp8 = {n: r for n, r in res.items() if "fa_fwd_fp8_kernel" in n}
    assert len(fp8) == 4, sorted(fp8)                                        # {bf16, fp16 out} x {64, 128}
    for n, r in fp8.items():
        assert r.get("spill", 0) == 0 and r.get("scratch", 0) == 0, (n, r)
    budget = json.load(open(os.path.join(build.CSRC, "spill_budget.json")))["spill"]
    assert not [n for n in budget if "fa_fwd_fp8_kernel" in n]


def test_fake_ops_give_bf16_out_for_fp8_q():
    import flash_attn_mi355.torch_ops  # noqa: F401
    B, S, H, Hk, D = 2, 96, 4, 2, 128
    q = torch.empty(B, S, H, D, dtype=torch.float8_e4m3fn, device="meta")
    k = torch.empty(B, S + 32, Hk, D, dtype=torch.float8_e4m3fn, device="meta")
    out, lse, dmask, rng = torch.ops.flash_attn_mi355.fwd(q, k, k.clone(), None, 0.0, 0.125, True, -1, -1, 0.0, False)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert lse.shape == (B, H, S) and lse.dtype == torch.float32
    T = 300
    q = torch.empty(T, H, D, dtype=torch.float8_e4m3fn, device="meta")
    cu = torch.empty(4, dtype=torch.int32, device="meta")
    out, lse, _, _ = torch.ops.flash_attn_mi355.varlen_fwd(q, q, q, cu, cu, None, None, 128, 128, 0.0, 0.1, True,
                                                           -1, -1, 0.0, False)
    assert out.shape == (T, H, D) and out.dtype == torch.bfloat16 and lse.shape == (H, T)


def test_python_rejections_before_launch():
    """mixed dtypes and the uncovered options raise in Python, before any tensor reaches the device (CPU tensors here:
    the device check would fire only after them)"""
    import flash_attn_mi355 as fa
    q8 = torch.zeros(1, 16, 2, 64, dtype=torch.float8_e4m3fn)
    q16 = torch.zeros(1, 16, 2, 64, dtype=torch.bfloat16)
    from flash_attn_mi355 import flash_attn_interface as fi
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        fi._is_fp8_qkv(q8, q16, q16)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        fi._is_fp8_qkv(q16, q8, q8)
    assert fi._is_fp8_qkv(q8, q8, q8) and not fi._is_fp8_qkv(q16, q16, q16)
    for kw, match in ((dict(head_size_og=256), "head dimension"), (dict(dropout_p=0.1), "dropout"),
                      (dict(softcap=5.0), "softcap"), (dict(alibi_slopes=torch.zeros(2)), "ALiBi"),
                      (dict(paged=True), "paged")):
        args = dict(head_size_og=64, dropout_p=0.0, softcap=0.0, alibi_slopes=None)
        args.update(kw)
        with pytest.raises(RuntimeError, match=match):
            fi._check_fp8_options(**args)
    assert "q_descale" in __import__("inspect").signature(fa.flash_attn_varlen_func).parameters


def test_packed_entry_points_reject_fp8_with_grad_before_launch():
    """the packed autograd Functions refuse fp8 inputs that require grad at forward time (the check comes before the device
    check, so CPU tensors reach it), as flash_attn_func does"""
    import flash_attn_mi355 as fa
    qkv = torch.zeros(1, 16, 3, 2, 64, dtype=torch.float8_e4m3fn).requires_grad_()
    with pytest.raises(RuntimeError, match="forward-only"):
        fa.flash_attn_qkvpacked_func(qkv)
    q = torch.zeros(1, 16, 2, 64, dtype=torch.float8_e4m3fn)
    kv = torch.zeros(1, 16, 2, 2, 64, dtype=torch.float8_e4m3fn).requires_grad_()
    with pytest.raises(RuntimeError, match="forward-only"):
        fa.flash_attn_kvpacked_func(q, kv)
    with pytest.raises(RuntimeError, match="forward-only"):
        fa.flash_attn_kvpacked_func(q.clone().requires_grad_(), kv.detach())


# ---------------------------------------------------------------------------------------------------------------------
# the shared fp8 gate (tests/fp8_gate.py) against an emulation of the kernel's arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _emulate(q8, k8, v8, scale, causal, wl, wr, qd=1.0, kd=1.0, vd=1.0, o_dtype=torch.bfloat16, mutate=None):
    """fa_fwd_fp8.hip on one head, in torch: scores in fp32 from the e4m3 codes, 64-key tiles, waves of 32 rows with the
    deferred rescale (a wave keeps its maxima unless one row would exceed its own by more than 2^8), P = exp2(s c - m) in
    fp32, l from the fp32 P, P quantised through float8_e4m3fn for O += P V in fp32, out = O v_descale / l.
    mutate: 'drop' - the P of each row's highest-scoring visible key is left out of O; 'swap' - the P of keys 2t and 2t + 1 trade
    places in O."""
    from oracle.attention import visible_mask
    sq, sk = q8.shape[0], k8.shape[0]
    s = q8.float() @ k8.float().T
    vis = torch.from_numpy(visible_mask(sq, sk, causal, wl, wr))
    c = torch.tensor(scale * 1.4426950408889634, dtype=torch.float32) * torch.tensor(qd * kd, dtype=torch.float32)
    m_run = torch.full((sq,), -torch.inf)
    l_run = torch.zeros(sq)
    o = torch.zeros(sq, v8.shape[1])
    heavy = torch.where(vis.any(1), torch.where(vis, s, -torch.inf).argmax(1), -1)
    for n0 in range(0, sk, 64):
        st = torch.where(vis[:, n0:n0 + 64], s[:, n0:n0 + 64], -torch.inf)
        mx = st.max(dim=1).values * c
        for w0 in range(0, sq, 32):
            w = slice(w0, w0 + 32)
            if not bool(((mx[w] - m_run[w]) <= 8.0).all()):
                m_new = torch.maximum(m_run[w], mx[w])
                alpha = torch.exp2(m_run[w] - torch.where(m_new == -torch.inf, 0.0, m_new))
                m_run[w], l_run[w] = m_new, l_run[w] * alpha
                o[w] *= alpha[:, None]
        m_use = torch.where(m_run == -torch.inf, 0.0, m_run)
        p = torch.exp2(st * c - m_use[:, None])
        assert float(p.max()) <= 256.0
        l_run += p.sum(dim=1)
        pq = p.to(torch.float8_e4m3fn).float()
        if mutate == "drop":
            j = heavy - n0
            rows = torch.nonzero((j >= 0) & (j < pq.shape[1]))[:, 0]
            pq[rows, j[rows]] = 0.0
        elif mutate == "swap":
            n = pq.shape[1] // 2 * 2
            pq[:, 0:n] = pq[:, 0:n].reshape(sq, -1, 2).flip(2).reshape(sq, n)
        o += pq @ v8[n0:n0 + 64].float()
    inv = torch.where(l_run > 0, torch.tensor(vd, dtype=torch.float32) / l_run, 0.0)
    out = (o * inv[:, None]).to(o_dtype)
    lse = torch.where(l_run > 0, (m_run + torch.log2(l_run)) * 0.6931471805599453, -torch.inf)
    return out, lse


def _e4m3(shape, seed, mag):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * mag).clamp(-448, 448).to(torch.float8_e4m3fn)


EMULATED = [
    # (Sq, Sk, D, causal, window, magnitude, descales (q, k, v), out dtype)
    (130, 200, 64, True, (-1, -1), 1.0, (1.0, 1.0, 1.0), "bf16"),
    (96, 300, 128, False, (-1, -1), 8.0, (1.0, 1.0, 1.0), "bf16"),     # P up to 2^8, both rescale paths
    (100, 100, 16, False, (20, 5), 1.0, (0.5, 0.25, 2.0), "fp16"),
    (65, 257, 80, False, (-1, -1), 32.0, (1.0, 1.0, 1.0), "bf16"),     # large scores: the accumulation term
    (200, 70, 48, True, (-1, -1), 0.125, (0.013, 3.0, 0.013), "fp16"),  # Sq > Sk: rows without keys
]


@pytest.mark.parametrize("Sq,Sk,D,causal,window,mag,ds,odt", EMULATED)
def test_fp8_gate_holds_for_the_emulated_kernel(Sq, Sk, D, causal, window, mag, ds, odt):
    import fp8_gate
    import oracle
    from oracle.attention import normalize_flags
    q8, k8, v8 = _e4m3((Sq, D), Sq + D, mag), _e4m3((Sk, D), Sk + 1, mag), _e4m3((Sk, D), Sk + 2, mag)
    scale = D ** -0.5
    c, wl, wr = normalize_flags(Sq, Sk, causal, window[0], window[1], False)
    out, lse = _emulate(q8, k8, v8, scale, c, wl, wr, *ds, o_dtype=fp8_gate.DTYPE_OF[odt])
    q, k, v = (t.double().numpy() * d for t, d in zip((q8, k8, v8), ds))
    o_ref, lse_ref, _ = oracle.attn_fwd(q[None, None], k[None, None], v[None, None], scale, causal=causal, window=window)
    bnd, delta = fp8_gate.bound(q, k, v, scale, causal, window)
    r = fp8_gate.check_out(out.double().numpy(), o_ref[0, 0], bnd, "emulated out", o_dtype=odt)
    rl = fp8_gate.check_lse(lse.double().numpy(), lse_ref[0, 0], delta, "emulated lse")
    print(f"Sq{Sq} Sk{Sk} D{D} mag {mag}: out {r:.3f}, lse {rl:.3f} of the gate")


@pytest.mark.parametrize("mutate", ["drop", "swap"])
def test_fp8_gate_rejects_a_wrong_emulation(mutate):
    """each case of EMULATED with one visible key dropped or two adjacent keys' P swapped lands outside the gate"""
    import fp8_gate
    import oracle
    from oracle.attention import normalize_flags
    for Sq, Sk, D, causal, window, mag, ds, odt in EMULATED:
        q8, k8, v8 = _e4m3((Sq, D), Sq + D, mag), _e4m3((Sk, D), Sk + 1, mag), _e4m3((Sk, D), Sk + 2, mag)
        scale = D ** -0.5
        c, wl, wr = normalize_flags(Sq, Sk, causal, window[0], window[1], False)
        out, _ = _emulate(q8, k8, v8, scale, c, wl, wr, *ds, o_dtype=fp8_gate.DTYPE_OF[odt], mutate=mutate)
        q, k, v = (t.double().numpy() * d for t, d in zip((q8, k8, v8), ds))
        o_ref, _, _ = oracle.attn_fwd(q[None, None], k[None, None], v[None, None], scale, causal=causal, window=window)
        bnd, _ = fp8_gate.bound(q, k, v, scale, causal, window)
        with pytest.raises(AssertionError, match="fp8 gate"):
            fp8_gate.check_out(out.double().numpy(), o_ref[0, 0], bnd, f"{mutate} Sq{Sq} Sk{Sk} D{D}", o_dtype=odt)
