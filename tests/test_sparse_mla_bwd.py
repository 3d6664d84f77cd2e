"""CPU: sparse_mla_bwd's entry declared, exported and in the ctypes table, every refusal of the C entry and of the wrapper before a launch,
and the bounds of tests/sparse_mla_bwd_ref.py holding for the design's own roundings on the inputs of the GPU bound test."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import sparse_mla_bwd_ref as B
import sparse_mla_ref as R
from sparse_mla_support import _aligned, _args, _refused

ROOT = Path(__file__).resolve().parent.parent


def test_symbol_is_declared_exported_and_in_the_table(dga):
    from deepgemm_ascend_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dga_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+dga_sparse_mla_bwd\s*\(", text) and re.search(r"#define\s+DGA_SPARSE_MLA_BWD_HEADS\s+32\b", text)
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "dga_sparse_mla_bwd")
    restype, argtypes = _lib.SIGNATURES["dga_sparse_mla_bwd"]
    assert restype is ctypes.c_int and len(argtypes) == 19 and callable(dga.sparse_mla_bwd) and "sparse_mla_bwd" in dga.__all__


def test_c_entry_checks_before_any_launch(dga):
    """the forward's refusals in the forward's order, then this entry's own; M == 0 accepted; none touches a device"""
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf, p = _aligned()

    def call(q=p, kv=p, idx=p, off=None, m=1, heads=16, s=4, kv_stride=576, topk=2, idx_stride=2, flags=0, out=p, d_out=p, lse=p, dq=p, dkv=p,
             dkv_stride=576):
        return L.dga_sparse_mla_bwd(q, kv, idx, off, m, heads, s, kv_stride, topk, idx_stride, 0.1, flags, out, d_out, lse, dq, dkv, dkv_stride, None)

    shape = call(m=-1)
    assert shape != 0 and {shape} == {call(heads=8), call(heads=144), call(s=0), call(topk=0), call(kv_stride=575), call(idx_stride=1), call(dkv_stride=575)}
    assert call(m=0) == 0 and call(m=0, q=None, dq=None, dkv=None, dkv_stride=0) == 0
    null = call(q=None)
    assert null not in (0, shape) and {null} == {call(out=None), call(d_out=None), call(lse=None), call(dq=None), call(dkv=None)}
    align = call(kv=p + 8)
    assert align not in (0, shape, null) and {align} == {call(out=p + 8), call(d_out=p + 4), call(lse=p + 2), call(dq=p + 2), call(dkv=p + 4), call(dkv_stride=578)}
    rng = call(flags=2)
    assert rng not in (0, shape, null, align) and rng == call(s=1 << 31) == call(s=1 << 30, dkv_stride=1 << 62) == call(flags=2, m=-1)
    assert call(q=None, dkv_stride=575) == null and call(kv=p + 8, dkv=None) == align     # the common clauses come first


def test_every_refusal_comes_from_the_wrapper(dga):
    q, kv, idx = _args()
    z = lambda shape, dtype=torch.bfloat16: torch.zeros(shape, dtype=dtype)
    good = dict(out=z((2, 16, 512)), d_out=z((2, 16, 512)), lse=z((2, 16), torch.float32))
    call = lambda q=q, kv=kv, idx=idx, **kw: (lambda a: dga.sparse_mla_bwd(q, kv, a.pop("out"), a.pop("d_out"), idx, a.pop("lse"), 0.1, **a))({**good, **kw})
    odd = lambda n, dtype: torch.zeros(n + 1, dtype=dtype)[1:]                           # a base 2 or 4 bytes off 16
    bad = {
        "q dtype": lambda: call(q=q.float()), "Hq = 24": lambda: call(q=_args(h=24)[0]), "kv stride 580": lambda: call(kv=z((8, 580))[:, :576]),
        "indices dtype": lambda: call(idx=idx.long()), "d_v": lambda: call(d_v=576),
        "out dtype": lambda: call(out=z((2, 16, 512), torch.float32)), "out shape": lambda: call(out=z((2, 16, 576))),
        "out strided": lambda: call(out=z((2, 16, 1024))[:, :, ::2]), "out misaligned": lambda: call(out=odd(2 * 16 * 512, torch.bfloat16).view(2, 16, 512)),
        "d_out dtype": lambda: call(d_out=z((2, 16, 512), torch.float16)), "d_out shape": lambda: call(d_out=z((2, 8, 512))),
        "d_out strided": lambda: call(d_out=z((2, 32, 512))[:, ::2]), "d_out misaligned": lambda: call(d_out=odd(2 * 16 * 512, torch.bfloat16).view(2, 16, 512)),
        "lse dtype": lambda: call(lse=z((2, 16))), "lse shape": lambda: call(lse=z((2, 16, 1), torch.float32)),
        "lse strided": lambda: call(lse=z((2, 32), torch.float32)[:, ::2]),
        "dq dtype": lambda: call(dq=z((2, 16, 576), torch.float32)), "dq shape": lambda: call(dq=z((2, 16, 512))),
        "dq strided": lambda: call(dq=z((2, 16, 1152))[:, :, ::2]), "dq misaligned": lambda: call(dq=odd(2 * 16 * 576, torch.bfloat16).view(2, 16, 576)),
        "dkv dtype": lambda: call(dkv=z((8, 576))), "dkv rows": lambda: call(dkv=z((7, 576), torch.float32)), "dkv columns": lambda: call(dkv=z((8, 512), torch.float32)),
        "dkv last dimension strided": lambda: call(dkv=z((8, 1152), torch.float32)[:, ::2]), "dkv stride 578": lambda: call(dkv=z((8, 578), torch.float32)[:, :576]),
        "dkv misaligned": lambda: call(dkv=odd(8 * 576, torch.float32).view(8, 576)),
    }
    _refused(dga, bad, (call, lambda: call(dkv=z((8, 640), torch.float32)[:, :576], dq=z((2, 16, 576)), index_offsets=z((2,), torch.int32))))


@pytest.mark.parametrize("h", (16, 32, 48, 128))
def test_the_bounds_leave_room_for_the_designs_roundings(h):
    """the reference with p, dS and dq rounded to bf16 as the kernel rounds them stays inside the bounds on the GPU bound test's inputs"""
    q, kv, idx, out, lse, d_out, scale = B.operands(h)
    ref, got = B.expected(h), B.reference(q, kv, out, d_out, idx, lse, scale, rounded=True)
    assert (np.abs(got["dq"] - ref["dq"]) <= B.bound_dq(ref, R.TOPK4)).all() and (np.abs(got["dkv"] - ref["dkv"]) <= B.bound_dkv(ref, h)).all()
    assert ref["count"].max() > 1 and (ref["count"] == 0).any() and np.abs(ref["dq"]).min() > 0
