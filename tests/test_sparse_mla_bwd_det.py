"""CPU: the deterministic form of sparse_mla_bwd -- both C symbols declared, exported and in the ctypes table, the C entry's refusals before
any launch in the documented order, the workspace rule, and the wrapper's refusal of a deterministic= that is no bool."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from sparse_mla_support import _aligned, _args

ROOT = Path(__file__).resolve().parent.parent
STAGING = 1 << 31


def test_symbols_are_declared_exported_and_in_the_table(dga):
    from deepgemm_ascend_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dga_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+dga_sparse_mla_bwd_det\s*\(", text) and re.search(r"\bint64_t\s+dga_sparse_mla_bwd_det_workspace_bytes\s*\(", text)
    assert re.search(r"#define\s+DGA_SPARSE_MLA_BWD_DET_STAGING_BYTES\s+%dll\b" % STAGING, text)
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(so, "dga_sparse_mla_bwd_det") and hasattr(so, "dga_sparse_mla_bwd_det_workspace_bytes")
    assert len(_lib.SIGNATURES["dga_sparse_mla_bwd_det"][1]) == 22 and _lib.SIGNATURES["dga_sparse_mla_bwd_det_workspace_bytes"][0] is ctypes.c_int64
    assert _lib.lib().dga_abi_version() == 7


def test_c_entry_checks_before_any_launch(dga):
    """dga_sparse_mla_bwd's refusals in its order, then chunk_tokens, the null workspace, its alignment, its size; M == 0 accepted"""
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf, p = _aligned()
    need = L.dga_sparse_mla_bwd_det_workspace_bytes(1, 16, 2, 4)
    assert need >= 2 * 2304 + 3 * 5 * 4 + 2 * 2 * 4

    def call(q=p, m=1, heads=16, s=4, topk=2, idx_stride=2, flags=0, dkv=p, dkv_stride=576, chunk=0, ws=p, ws_bytes=need):
        return L.dga_sparse_mla_bwd_det(q, p, p, None, m, heads, s, 576, topk, idx_stride, 0.1, flags, p, p, p, p, dkv, dkv_stride, chunk, ws, ws_bytes, None)

    shape = call(m=-1)
    assert shape != 0 and {shape} == {call(heads=8), call(topk=0), call(dkv_stride=575), call(chunk=-1)}
    assert call(m=0) == 0 and call(m=0, q=None, dkv=None, ws=None, ws_bytes=0, chunk=-1) == 0
    null = call(q=None)
    assert null not in (0, shape) and null == call(dkv=None) == call(ws=None)
    align = call(dkv=p + 4)
    assert align not in (0, shape, null) and align == call(ws=p + 8)
    rng = call(flags=2)
    assert rng not in (0, shape, null, align) and rng == call(s=1 << 30, dkv_stride=1 << 62)
    small = call(ws_bytes=need - 1)
    assert small not in (0, shape, null, align, rng)
    # the order: the backward's clauses, then shape, null, alignment, workspace
    assert call(dkv=None, chunk=-1) == null and call(flags=2, chunk=-1) == rng and call(chunk=-1, ws=None) == shape
    assert call(ws=None, ws_bytes=0) == null and call(ws=p + 8, ws_bytes=0) == align


def test_workspace_grows_with_m_up_to_the_chunk_cap(dga):
    from deepgemm_ascend_amd import _lib
    ws = _lib.lib().dga_sparse_mla_bwd_det_workspace_bytes
    cap = STAGING // (2048 * 2304)
    assert cap == 455
    sizes = [ws(m, 128, 2048, 32768) for m in (1, 2, 100, cap - 1, cap, cap + 1, 4096, 1 << 20)]
    assert all(a < b for a, b in zip(sizes[:4], sizes[1:5])) and len(set(sizes[4:])) == 1
    assert sizes[4] == cap * 2048 * 2304 + 3 * 32769 * 4 + 4 + 2 * cap * 2048 * 4       # (the three int32 arrays padded to 16 bytes)
    assert ws(0, 128, 2048, 32768) == 0 and ws(4, 24, 2048, 32768) == 0 and ws(4, 128, 0, 32768) == 0 and ws(4, 128, 2048, 0) == 0
    assert ws(8, 16, 1 << 20, 64) == (1 << 20) * 2304 + 3 * 65 * 4 + 4 + 2 * (1 << 20) * 4                # (topk beyond the cap: one token a chunk)


def test_the_wrapper_refuses_a_deterministic_that_is_no_bool(dga):
    q, kv, idx = _args()
    z = lambda shape, dtype=torch.bfloat16: torch.zeros(shape, dtype=dtype)
    for bad in ("yes", 1, None):
        with pytest.raises(Exception, match="deterministic must be a bool"):
            dga.sparse_mla_bwd(q, kv, z((2, 16, 512)), z((2, 16, 512)), idx, z((2, 16), torch.float32), 0.1, deterministic=bad)
    with pytest.raises(Exception, match="out"):                                          # (after the existing checks)
        dga.sparse_mla_bwd(q, kv, z((2, 16, 576)), z((2, 16, 512)), idx, z((2, 16), torch.float32), 0.1, deterministic="yes")
