"""CPU: gather_per_token_cast_to_fp8_transposed's exports, the C entry's refusals (nothing is launched), the Python argument checks, and the
unit's compile-time guards (dga_gather_cast_transposed.hip)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import deepgemm_ascend_amd as dga
from deepgemm_ascend_amd import _lib
from test_build import _ship_flags

OK, E_NULL, E_SHAPE, E_DTYPE, E_RANGE = 0, -1, -2, -3, -9   # include/dga_hip.h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepgemm_ascend_amd", "csrc")
UNIT = "dga_gather_cast_transposed.hip"


def test_the_symbols_are_exported():
    assert "gather_per_token_cast_to_fp8_transposed" in dga.__all__
    assert "dga_gather_cast_to_fp8_1x128_transposed" in _lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "dga_hip.h")).read()
    assert re.search(r"\bint\s+dga_gather_cast_to_fp8_1x128_transposed\s*\(", text)
    assert "#define DGA_ABI_VERSION 7" in text                              # an added symbol: the ABI version stays
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert UNIT in mk.split("SRCS =")[1].split("HDRS =")[0]
    dep = [l for l in mk.splitlines() if l.rstrip().endswith(": dga_cast_device.hpp")]
    assert len(dep) == 1 and "$(OBJ)/dga_gather_cast_transposed.o" in dep[0].split()     # the shared device text rebuilds it
    assert callable(_lib.lib().dga_gather_cast_to_fp8_1x128_transposed)     # ... and the built library has it
    cpp = open(os.path.join(CSRC, "python_api_amd.cpp")).read()
    assert 'm.def("gather_per_token_cast_to_fp8_transposed"' in cpp


def _c_call(src=1, dt=_lib.DT_BF16, s=8, h=128, index=4, div=1, scale=None, g=1, rows=4, masked_m=None, qt=2, ldqt=None, sft=3, q=None,
            sf=None, flags=0):
    ptr = lambda v: None if v is None else ctypes.c_void_p(0x1000 * v)   # (never dereferenced: every case returns before a launch)
    ldqt = g * rows if ldqt is None else ldqt
    return _lib.lib().dga_gather_cast_to_fp8_1x128_transposed(ptr(src), dt, s, h, ptr(index), div, ptr(scale), g, rows, ptr(masked_m), ptr(qt),
                                                              ldqt, ptr(sft), ptr(q), ptr(sf), flags, None)


def test_c_abi_refuses_without_launching():
    # DGA_E_RANGE: an unknown flag, before everything else
    assert _c_call(flags=2) == E_RANGE and _c_call(flags=_lib.CAST_UE8M0 | 4) == E_RANGE
    assert _c_call(flags=2, rows=-1) == E_RANGE and _c_call(flags=2, src=None) == E_RANGE and _c_call(flags=2, div=0) == E_RANGE
    # DGA_E_SHAPE: negative sizes, index_div < 1, S * index_div beyond int64, groups != 1 without masked_m, the ldqt rule, one of q_row / sf_row
    assert _c_call(rows=-1, ldqt=0) == E_SHAPE and _c_call(h=-128) == E_SHAPE and _c_call(g=-3, ldqt=0) == E_SHAPE and _c_call(s=-1) == E_SHAPE
    assert _c_call(g=0, ldqt=0) == E_SHAPE
    assert _c_call(div=0) == E_SHAPE and _c_call(div=-3) == E_SHAPE
    assert _c_call(s=1 << 40, div=1 << 40) == E_SHAPE
    assert _c_call(g=2) == E_SHAPE and _c_call(g=2, rows=2, ldqt=4) == E_SHAPE
    assert _c_call(rows=300, ldqt=299) == E_SHAPE and _c_call(rows=300, ldqt=385) == E_SHAPE
    assert _c_call(rows=256, ldqt=257) == E_SHAPE and _c_call(g=2, rows=100, ldqt=100, masked_m=5) == E_SHAPE
    assert _c_call(g=1 << 40, rows=1 << 40, ldqt=0, masked_m=5) == E_SHAPE
    assert _c_call(q=7) == E_SHAPE and _c_call(sf=8) == E_SHAPE
    assert _c_call(rows=0, ldqt=5) == E_SHAPE and _c_call(div=0, rows=0) == E_SHAPE and _c_call(q=7, src=None) == E_SHAPE   # before nothing-to-do and the pointers
    # DGA_OK: T == 0 or H == 0, whatever the pointers
    assert _c_call(rows=0) == OK and _c_call(h=0) == OK
    assert _c_call(rows=0, src=None, index=None, qt=None, sft=None) == OK and _c_call(h=0, src=None, index=None, qt=None, sft=None, q=7, sf=8) == OK
    assert _c_call(g=3, rows=0, masked_m=5) == OK
    # DGA_E_NULL: a required pointer, before the dtype
    assert _c_call(src=None) == E_NULL and _c_call(index=None) == E_NULL and _c_call(qt=None) == E_NULL and _c_call(sft=None) == E_NULL
    assert _c_call(index=None, dt=99) == E_NULL
    assert _c_call(src=None, s=0, dt=99) == E_DTYPE                          # a source without rows needs no pointer: every index excludes
    # DGA_E_DTYPE
    assert _c_call(dt=_lib.DT_FP8_E4M3FN) == E_DTYPE and _c_call(dt=99) == E_DTYPE
    # DGA_E_RANGE: more tiles than a grid holds, element indices of src beyond int64
    assert _c_call(rows=1 << 40, h=1 << 20) == E_RANGE and _c_call(rows=1, h=1 << 40) == E_RANGE
    assert _c_call(s=1 << 40, h=1 << 24, rows=1) == E_RANGE
    # every ldqt of the range gets past the shape check (a bad dtype is met next); so do the table's other forms
    for ldqt in (300, 301, 383, 384):
        assert _c_call(rows=300, ldqt=ldqt, dt=99) == E_DTYPE, ldqt
    assert _c_call(g=3, rows=100, ldqt=384, dt=99, masked_m=5) == E_DTYPE
    assert _c_call(q=7, sf=8, dt=99, scale=9, div=3) == E_DTYPE and _c_call(g=1, masked_m=5, dt=99) == E_DTYPE


def _x(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


def _ix(*shape):
    return torch.zeros(*shape, dtype=torch.int64)


# (case, the message of the check it exercises): every check runs before the device guard, so a CPU call reaches the check itself
ARG_CASES = [
    ("src_rank", r"src must be a contiguous \[S, H\]"), ("src_strided", r"src must be a contiguous \[S, H\]"),
    ("src_dtype", "float32, bfloat16 or float16"), ("div_zero", "index_div must be an integer >= 1"), ("div_float", "index_div must be an integer >= 1"),
    ("index_dtype", r"index must be a contiguous int64 \[T\]"), ("index_rank", r"index must be a contiguous int64 \[T\]"),
    ("index_rank_masked", r"index must be a contiguous int64 \[G, Mmax\]"), ("index_strided", r"index must be a contiguous int64 \[T\]"),
    ("masked_dtype", r"masked_m must be a contiguous int32 \[4\]"), ("masked_shape", r"masked_m must be a contiguous int32 \[4\]"),
    ("scale_dtype", "row_scale must be contiguous float32 with 24 elements"), ("scale_size", "row_scale must be contiguous float32 with 24 elements"),
    ("out_len", r"out must be \(qt, sft\)"), ("out_nesting", r"out must hold \(qt, sft\)"), ("out_len_rowwise", r"out must be \(\(qt, sft\), \(q, sf\)\)"),
    ("out_qt_shape", r"out qt must be \[200, 8\]"), ("out_qt_stride", "rows 128 bytes apart"),
    ("out_sft_shape", r"out sft must be contiguous float32 \[200, 1\]"), ("out_q_shape", "out q must be contiguous"),
    ("out_q_shape_masked", r"out q must be contiguous \[4, 2, 200\]"), ("out_sf_shape", "out sf must be contiguous float32"),
]


@pytest.mark.parametrize("case,msg", ARG_CASES, ids=[c[0] for c in ARG_CASES])
def test_argument_errors_raise(case, msg):
    src, index, kw = _x(8, 200), _ix(8), {}
    qt, sft = torch.zeros(200, 8, dtype=torch.uint8), torch.zeros(200, 1)
    q, sf = torch.zeros(8, 200, dtype=torch.uint8), torch.zeros(8, 2)
    if case == "src_rank":
        src = _x(2, 4, 200)
    elif case == "src_strided":
        src = _x(8, 400)[:, :200]
    elif case == "src_dtype":
        src = _x(8, 200, dtype=torch.float64)
    elif case == "div_zero":
        kw["index_div"] = 0
    elif case == "div_float":
        kw["index_div"] = 2.0
    elif case == "index_dtype":
        index = index.int()
    elif case == "index_rank":
        index = _ix(4, 2)
    elif case == "index_rank_masked":
        kw["masked_m"] = torch.zeros(4, dtype=torch.int32)
    elif case == "index_strided":
        index = _ix(16)[::2]
    elif case == "masked_dtype":
        index = _ix(4, 2); kw["masked_m"] = torch.zeros(4, dtype=torch.int64)
    elif case == "masked_shape":
        index = _ix(4, 2); kw["masked_m"] = torch.zeros(5, dtype=torch.int32)
    elif case == "scale_dtype":
        kw.update(index_div=3, row_scale=torch.zeros(24, dtype=torch.float64))
    elif case == "scale_size":
        kw.update(index_div=3, row_scale=torch.zeros(8))
    elif case == "out_len":
        kw["out"] = (qt,)
    elif case == "out_nesting":
        kw.update(rowwise=True, out=(qt, sft))
    elif case == "out_len_rowwise":
        kw.update(rowwise=True, out=((qt, sft),))
    elif case == "out_qt_shape":
        kw["out"] = (torch.zeros(200, 16, dtype=torch.uint8), sft)
    elif case == "out_qt_stride":
        kw.update(aligned_rows=True, out=(qt, sft))
    elif case == "out_sft_shape":
        kw["out"] = (qt, torch.zeros(200, 2))
    elif case == "out_q_shape":
        kw.update(rowwise=True, out=((qt, sft), (torch.zeros(8, 256, dtype=torch.uint8), sf)))
    elif case == "out_q_shape_masked":
        index = _ix(4, 2); kw.update(masked_m=torch.zeros(4, dtype=torch.int32), rowwise=True, out=((qt, sft), (q, sf)))
    elif case == "out_sf_shape":
        kw.update(rowwise=True, out=((qt, sft), (q, torch.zeros(8, 1))))
    with pytest.raises(dga.DGAError, match=msg):
        dga.gather_per_token_cast_to_fp8_transposed(src, index, **kw)


@pytest.mark.parametrize("layout", ["flat", "div", "scaled", "masked", "out", "out_aligned", "rowwise", "rowwise_out_masked", "odd"])
def test_a_valid_cpu_call_gets_past_every_argument_check(layout):
    """The same arguments without a fault reach the device guard (so each case above is refused by its own check): CPU tensors raise there."""
    src, index, kw = _x(8, 200), _ix(8), {}
    if layout == "div":
        kw["index_div"] = 3
    elif layout == "scaled":
        kw.update(index_div=3, row_scale=torch.zeros(8, 3))
    elif layout == "masked":
        index = _ix(4, 2); kw["masked_m"] = torch.zeros(4, dtype=torch.int32)
    elif layout == "out":
        kw["out"] = (torch.zeros(200, 8, dtype=torch.float8_e4m3fn), torch.zeros(200, 1))
    elif layout == "out_aligned":
        kw.update(aligned_rows=True, out=(torch.zeros(200, 128, dtype=torch.uint8)[:, :8], torch.zeros(200, 1)))
    elif layout == "rowwise":
        kw["rowwise"] = True
    elif layout == "rowwise_out_masked":
        index = _ix(4, 2)
        kw.update(masked_m=torch.zeros(4, dtype=torch.int32), rowwise=True,
                  out=((torch.zeros(200, 8, dtype=torch.uint8), torch.zeros(200, 1)), (torch.zeros(4, 2, 200, dtype=torch.uint8), torch.zeros(4, 2, 2))))
    elif layout == "odd":
        src, index = _x(3, 77, dtype=torch.float32), _ix(5)
    with pytest.raises(dga.DGAError, match="no CPU path"):
        dga.gather_per_token_cast_to_fp8_transposed(src, index, **kw)


def test_the_unit_compiles_without_spills_or_scratch():
    """tests/test_build.py's method on dga_gather_cast_transposed.hip, with the Makefile's flags: the tile holds 64 values per lane and this
    kernel 8 more addresses, and none of its 12 builds (3 types x row-wise output x row scale) may spill."""
    flags = _ship_flags(UNIT)
    assert "--offload-arch=gfx950" in flags and "-O3" in flags
    cmd = ["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-S", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage",
           os.path.join(CSRC, UNIT)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen = None, set()
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen.add(name)
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m:
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
        m = re.search(r"VGPRs: (\d+)", line)
        if m:
            assert int(m.group(1)) <= 256, name
    assert len(seen) == 12 and all("gather_cast_1x128_transposed_kernel" in n for n in seen), seen
