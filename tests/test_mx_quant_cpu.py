"""CPU: the host side of fa_mx_quant / fa_mx_dequant - structs against the header, exports, the build list, the kernels'
registers, and every argument error of the C ABI and of the wrappers, all before any device work.  Nothing here needs a GPU."""
import ctypes
import json
import os
import re

import pytest
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flash_attn_mi355 import _lib
    return _lib


@pytest.mark.parametrize("name,cls", [("fa_mx_quant", "FaMxQuantParams"), ("fa_mx_dequant", "FaMxDequantParams")])
def test_struct_matches_the_header(lib, name, cls):
    hdr = open(os.path.join(ROOT, "include", "fa_mi355.h")).read()
    body = re.search(r"typedef struct %s_params \{(.*?)\} %s_params;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    struct = getattr(lib, cls)
    assert names == [f[0] for f in struct._fields_]
    assert getattr(lib.lib, name + "_params_size")() == ctypes.sizeof(struct) and lib.lib.fa_abi_version() == 4
    assert {name, name + "_params_size"} <= set(lib.EXPORTS) and hasattr(lib, "call_" + name[3:])


def test_build_list_registers_and_names(lib):
    import build
    import flash_attn
    import flash_attn_mi355
    from flash_attn_mi355 import torch_ops
    assert "fa_mx_quant.hip" in build.SOURCES
    res = json.load(open(os.path.join(os.path.dirname(lib.__file__), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if "mx_quant_" in k or "mx_dequant_" in k}
    assert len(mine) == 6                                   # quant: nk / kn x bf16 / fp16; dequant: nk / kn
    assert all(v["spill"] == 0 and v["scratch"] == 0 for v in mine.values()), mine
    for pkg in (flash_attn, flash_attn_mi355, torch_ops):
        assert not {"quant_mxfp4", "dequant_mxfp4"} & set(pkg.__all__)
    assert torch.ops.flash_attn_mi355.quant_mxfp4 and torch.ops.flash_attn_mi355.dequant_mxfp4


def _block(lib, op, **kw):
    """a valid block of 4 experts [32, 64] over host memory, then `kw` (pointers: offsets into the buffer)"""
    buf = (ctypes.c_char * 0x40040)()
    base = (ctypes.addressof(buf) + 15) & ~15
    s = lib.FaMxQuantParams() if op == "mx_quant" else lib.FaMxDequantParams()
    s.struct_size = ctypes.sizeof(s)
    ptrs = dict(blocks=0x20000, scales=0x30000, **({"w": 0} if op == "mx_quant" else {"out": 0}))
    stride = "w_expert_stride" if op == "mx_quant" else "out_expert_stride"
    vals = dict(ptrs, blocks_expert_stride=1024, scales_expert_stride=64, num_experts=4, n=32, k=64, dtype=lib.FA_BF16,
                layout=lib.FA_MOE_W_NK, elem_format=lib.FA_MX_ELEM_E2M1, **{stride: 2048})
    vals.update(kw)
    for k, v in vals.items():
        setattr(s, k, base + v if k in ptrs else v)
    return s, buf


@pytest.mark.parametrize("op", ["mx_quant", "mx_dequant"])
@pytest.mark.parametrize("match,code,kw", [
    ("struct_size", "(-1)", dict(struct_size=8)), ("reserved", "(-1)", dict(reserved=(0, 0, 1, 0))),
    ("k must be a multiple of 32", "(-2)", dict(k=48)), ("n must be a multiple of 8", "(-2)", dict(n=12)),
    ("65535 experts", "(-2)", dict(num_experts=65536)), ("non-negative", "(-1)", dict(num_experts=-1)),
    ("dtype", "(-1)", dict(dtype=3)), ("unknown layout", "(-1)", dict(layout=2)), ("elem_format", "(-2)", dict(elem_format=1)),
    ("blocks must be 16-byte aligned", "(-2)", dict(blocks=0x20008)),
    ("scales' expert stride", "(-2)", dict(scales_expert_stride=63)), ("overlaps scales", "(-1)", dict(scales=0x20100)),
    ("overlaps blocks", "(-1)", dict(blocks=0x1000))])
def test_c_abi_rejects_before_any_device_work(lib, op, match, code, kw):
    s, buf = _block(lib, op, **kw)
    with pytest.raises(RuntimeError, match=match) as e:
        getattr(lib, "call_" + op)(s, 0)
    assert code in str(e.value), str(e.value)


def test_c_abi_quant_only_fields_and_empty_tensors(lib):
    for match, kw in (("unknown scale_rule", dict(scale_rule=2)), ("reserved", dict(reserved0=1)), ("must be 16-byte aligned", dict(w=8)),
                      ("w must be", dict(w_expert_stride=2044))):
        with pytest.raises(RuntimeError, match=match):
            lib.call_mx_quant(_block(lib, "mx_quant", **kw)[0], 0)
    for op in ("mx_quant", "mx_dequant"):                   # empty: FA_OK without a launch, whatever the pointers
        for kw in (dict(num_experts=0), dict(n=0), dict(k=0)):
            getattr(lib, "call_" + op)(_block(lib, op, **kw)[0], 0)


def test_wrappers_reject_by_name_without_a_device(lib):
    from flash_attn_mi355 import quant
    w, b, s = torch.zeros(2, 16, 64, dtype=torch.bfloat16), torch.zeros(2, 16, 32, dtype=torch.uint8), torch.zeros(2, 16, 2, dtype=torch.uint8)

    def bad(match, fn, *a, **kw):
        with pytest.raises(RuntimeError, match=match):
            fn(*a, **kw)
    q, d = quant.quant_mxfp4, quant.dequant_mxfp4
    bad("K must be a multiple of 32", q, w[:, :, :48].contiguous())
    bad("N must be a multiple of 8", q, w[:, :12].contiguous())
    bad("w must be a tensor of dtype", q, w.float())
    bad("w_layout must be one of", q, w, w_layout="nn")
    bad("scale_rule must be one of", q, w, scale_rule="ceil")
    bad("w needs a contiguous last dimension", q, w.transpose(1, 2))
    buf = torch.zeros(2048, dtype=torch.uint8)
    bad(r"out\[0\] overlaps out\[1\]", q, w, out=(buf[:1024].view(2, 16, 32), buf[1000:1064].view(2, 16, 2)))
    bad(r"out\[0\] must be 16-byte aligned", q, w, out=(buf[8:1032].view(2, 16, 32), s))
    bad("w must be 16-byte aligned with an expert stride", q, torch.zeros(2, 1028, dtype=torch.bfloat16)[:, :1024].view(2, 16, 64))
    big = torch.zeros(8192, dtype=torch.uint8)
    bad("blocks overlaps out", d, big[:1024].view(2, 16, 32), s, out=big[512:4608].view(torch.bfloat16).view(2, 16, 64))
    bad(r"out\[0\] must have shape", q, w, out=(b[:, :, :16].contiguous(), s))
    bad(r"out\[1\] must be a tensor of dtype", q, w, out=(b, s.to(torch.int8)))
    bad("w requires grad", q, w.clone().requires_grad_())
    bad("scales must have shape", d, b, s[:, :, :1].contiguous())
    bad("blocks must be a tensor of dtype", d, b.to(torch.int8), s)
    bad("out must be a tensor of dtype", d, b, s, out=w.half())
    bad("out must have shape", d, b, s, w_layout="kn", out=w)
    bad("no CPU fallback", q, w)
    bad("no CPU fallback", d, b, s)
