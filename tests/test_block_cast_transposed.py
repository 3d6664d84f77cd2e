"""CPU: per_block_cast_to_fp8_transposed's exports, the C entry's refusals (nothing is launched), the Python argument checks
(dga_cast_transposed_block.hip), and the oracle identity tests/test_block_cast_transposed_gpu.py leans on: the 128x128 quantiser of a
transpose is the 128x128 quantiser transposed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import block_cast_cases as B
import deepgemm_ascend_amd as dga
from deepgemm_ascend_amd import _lib

OK, E_NULL, E_SHAPE, E_DTYPE, E_RANGE = 0, -1, -2, -3, -9   # include/dga_hip.h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepgemm_ascend_amd", "csrc")
UNIT = "dga_cast_transposed_block.hip"
SYMBOL = "dga_cast_to_fp8_128x128_transposed"


def test_the_symbols_are_exported():
    assert "per_block_cast_to_fp8_transposed" in dga.__all__
    assert SYMBOL in _lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "dga_hip.h")).read()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text)
    assert "#define DGA_ABI_VERSION 7" in text                              # an added symbol: the ABI version stays
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert UNIT in mk.split("SRCS =")[1].split("HDRS =")[0]
    dep = [l for l in mk.splitlines() if l.rstrip().endswith(": dga_cast_device.hpp")]
    assert len(dep) == 1 and "$(OBJ)/dga_cast_transposed_block.o" in dep[0].split()     # the shared device text rebuilds it
    assert callable(getattr(_lib.lib(), SYMBOL))                            # ... and the built library has it
    cpp = open(os.path.join(CSRC, "python_api_amd.cpp")).read()
    assert 'm.def("per_block_cast_to_fp8_transposed"' in cpp


def test_the_built_library_exports_the_symbol():
    """A handle of its own on the file the build left in the tree (dlsym sees exported symbols only), not what _lib resolved."""
    dga.build()
    so = ctypes.CDLL(os.path.join(ROOT, "deepgemm_ascend_amd", "libdga_hip.so"))
    fn = getattr(so, SYMBOL)
    assert ctypes.cast(fn, ctypes.c_void_p).value
    assert so.dga_abi_version() == 7


def _c_call(w=1, dt=_lib.DT_BF16, g=2, n=4, k=128, qt=2, sft=3, q=None, sf=None, flags=0):
    ptr = lambda v: None if v is None else ctypes.c_void_p(0x1000 * v)   # (never dereferenced: every case returns before a launch)
    return getattr(_lib.lib(), SYMBOL)(ptr(w), dt, g, n, k, ptr(qt), ptr(sft), ptr(q), ptr(sf), flags, None)


def test_c_abi_refuses_without_launching():
    # DGA_E_RANGE: an unknown flag, before everything else
    assert _c_call(flags=2) == E_RANGE and _c_call(flags=_lib.CAST_UE8M0 | 4) == E_RANGE
    assert _c_call(flags=2, n=-1) == E_RANGE and _c_call(flags=2, w=None) == E_RANGE and _c_call(flags=2, g=0) == E_RANGE
    # DGA_E_SHAPE: a negative size, exactly one of q_row / sf_row
    assert _c_call(g=-1) == E_SHAPE and _c_call(n=-1) == E_SHAPE and _c_call(k=-128) == E_SHAPE
    assert _c_call(q=7) == E_SHAPE and _c_call(sf=8) == E_SHAPE
    assert _c_call(n=0, q=7) == E_SHAPE and _c_call(q=7, w=None) == E_SHAPE and _c_call(n=-1, g=0) == E_SHAPE   # ... before nothing-to-do and the pointers
    # DGA_OK: groups, n or k zero, whatever the pointers
    assert _c_call(g=0) == OK and _c_call(n=0) == OK and _c_call(k=0) == OK
    assert _c_call(g=0, w=None, qt=None, sft=None) == OK and _c_call(k=0, w=None, qt=None, sft=None, q=7, sf=8) == OK
    assert _c_call(n=0, dt=99) == OK
    # DGA_E_NULL: a required pointer, before the dtype
    assert _c_call(w=None) == E_NULL and _c_call(qt=None) == E_NULL and _c_call(sft=None) == E_NULL
    assert _c_call(w=None, dt=99) == E_NULL and _c_call(sft=None, q=7, sf=8) == E_NULL
    # DGA_E_DTYPE
    assert _c_call(dt=_lib.DT_FP8_E4M3FN) == E_DTYPE and _c_call(dt=99) == E_DTYPE and _c_call(q=7, sf=8, dt=99) == E_DTYPE
    # DGA_E_RANGE: more tiles than a grid holds -- the tile count, not the element count, and over the groups too
    assert _c_call(g=1, n=1 << 40, k=1 << 20) == E_RANGE
    assert _c_call(g=1, n=1, k=1 << 40) == E_RANGE and _c_call(g=1, n=1 << 40, k=1) == E_RANGE       # 2^33 tiles of one row or column
    assert _c_call(g=1 << 31, n=1, k=1) == E_RANGE and _c_call(g=1 << 16, n=1 << 15, k=1 << 15) == E_RANGE   # 2^31; 2^16 groups of 2^16 tiles
    assert _c_call(g=(1 << 63) - 1, n=(1 << 63) - 1, k=(1 << 63) - 1) == E_RANGE                     # no product overflows on the way
    assert _c_call(g=(1 << 31) - 1, n=1, k=1, dt=99) == E_DTYPE                                      # (2^31 - 1 tiles get past: dtype comes first)


def _w(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


def _outs(g=(3,), n=200, k=136):
    nb, kb = (n + 127) // 128, (k + 127) // 128
    return ((torch.zeros(g + (k, n), dtype=torch.uint8), torch.zeros(g + (kb, nb))),
            (torch.zeros(g + (n, k), dtype=torch.uint8), torch.zeros(g + (nb, kb))))


# (case, the message of the check it exercises): every check runs before the device guard, so a CPU call reaches the check itself
ARG_CASES = [
    ("rank_1", r"\[N, K\] or \[G, N, K\]"), ("rank_4", r"\[N, K\] or \[G, N, K\]"), ("non_contiguous", "contiguous"),
    ("transposed_view", "contiguous"), ("int_dtype", "float32, bfloat16 or float16"), ("float64", "float32, bfloat16 or float16"),
    ("out_len", r"out must be \(qt, sft\)"), ("out_not_a_tuple", r"out must be \(qt, sft\)"), ("out_len_rowwise", r"out must be \(\(qt, sft\), \(q, sf\)\)"),
    ("out_nesting", r"out must hold \(qt, sft\)"), ("out_nesting_flat", r"out must hold \(qt, sft\)"), ("out_inner_len", r"out must hold \(q, sf\)"),
    ("out_qt_dtype", "float8_e4m3fn or uint8"), ("out_qt_shape", r"out qt must be contiguous \[3, 136, 200\]"),
    ("out_qt_untransposed", r"out qt must be contiguous \[3, 136, 200\]"), ("out_qt_2d_for_3d", r"out qt must be contiguous \[3, 136, 200\]"),
    ("out_qt_stride", r"out qt must be contiguous \[3, 136, 200\]"),
    ("out_sft_dtype", r"out sft must be contiguous float32 \[3, 2, 2\]"), ("out_sft_shape", r"out sft must be contiguous float32 \[3, 2, 2\]"),
    ("out_sft_untransposed", r"out sft must be contiguous float32 \[2, 3\]"),
    ("out_q_shape", r"out q must be contiguous \[3, 200, 136\]"), ("out_q_dtype", "float8_e4m3fn or uint8"),
    ("out_sf_shape", r"out sf must be contiguous float32 \[3, 2, 2\]"), ("out_sf_stride", r"out sf must be contiguous float32 \[3, 2, 2\]"),
]


@pytest.mark.parametrize("case,msg", ARG_CASES, ids=[c[0] for c in ARG_CASES])
def test_argument_errors_raise(case, msg):
    w, kw = _w(3, 200, 136), {}
    (qt, sft), (q, sf) = _outs()
    if case == "rank_1":
        w = _w(200)
    elif case == "rank_4":
        w = _w(1, 3, 200, 136)
    elif case == "non_contiguous":
        w = _w(3, 200, 272)[:, :, :136]
    elif case == "transposed_view":
        w = _w(3, 136, 200).transpose(1, 2)
    elif case == "int_dtype":
        w = _w(3, 200, 136, dtype=torch.int32)
    elif case == "float64":
        w = _w(3, 200, 136, dtype=torch.float64)
    elif case == "out_len":
        kw["out"] = (qt,)
    elif case == "out_not_a_tuple":
        kw["out"] = qt
    elif case == "out_len_rowwise":
        kw.update(rowwise=True, out=((qt, sft),))
    elif case == "out_nesting":
        kw.update(rowwise=True, out=(qt, sft))
    elif case == "out_nesting_flat":
        kw["out"] = ((qt, sft), (q, sf))
    elif case == "out_inner_len":
        kw.update(rowwise=True, out=((qt, sft), (q, sf, sf)))
    elif case == "out_qt_dtype":
        kw["out"] = (qt.view(torch.int8), sft)
    elif case == "out_qt_shape":
        kw["out"] = (torch.zeros(3, 136, 208, dtype=torch.uint8), sft)
    elif case == "out_qt_untransposed":
        kw["out"] = (q, sft)
    elif case == "out_qt_2d_for_3d":
        kw["out"] = (torch.zeros(3 * 136, 200, dtype=torch.uint8), sft)
    elif case == "out_qt_stride":
        kw["out"] = (torch.zeros(3, 136, 256, dtype=torch.uint8)[:, :, :200], sft)
    elif case == "out_sft_dtype":
        kw["out"] = (qt, sft.double())
    elif case == "out_sft_shape":
        kw["out"] = (qt, torch.zeros(3, 2, 1))
    elif case == "out_sft_untransposed":
        w = _w(300, 136)                                                # sft is [ceil(K/128), ceil(N/128)] = [2, 3], sf [3, 2]
        kw["out"] = (torch.zeros(136, 300, dtype=torch.uint8), torch.zeros(3, 2))
    elif case == "out_q_shape":
        kw.update(rowwise=True, out=((qt, sft), (qt.clone(), sf)))
    elif case == "out_q_dtype":
        kw.update(rowwise=True, out=((qt, sft), (q.to(torch.int16), sf)))
    elif case == "out_sf_shape":
        kw.update(rowwise=True, out=((qt, sft), (q, torch.zeros(3, 2, 3))))
    elif case == "out_sf_stride":
        kw.update(rowwise=True, out=((qt, sft), (q, torch.zeros(3, 2, 4)[:, :, ::2])))
    with pytest.raises(dga.DGAError, match=msg):
        dga.per_block_cast_to_fp8_transposed(w, **kw)


@pytest.mark.parametrize("layout", ["grouped", "flat", "out", "out_fp8", "rowwise", "rowwise_out", "flat_rowwise_out", "odd", "fp16"])
def test_a_valid_cpu_call_gets_past_every_argument_check(layout):
    """The same arguments without a fault reach the device guard (so each case above is refused by its own check): CPU tensors raise there."""
    w, kw = _w(3, 200, 136), {}
    (qt, sft), (q, sf) = _outs()
    if layout == "flat":
        w = _w(200, 136)
    elif layout == "out":
        kw["out"] = (qt, sft)
    elif layout == "out_fp8":
        kw["out"] = [qt.view(torch.float8_e4m3fn), sft]
    elif layout == "rowwise":
        kw["rowwise"] = True
    elif layout == "rowwise_out":
        kw.update(rowwise=True, use_ue8m0=True, out=((qt, sft), (q.view(torch.float8_e4m3fn), sf)))
    elif layout == "flat_rowwise_out":
        w = _w(200, 136)
        kw.update(rowwise=True, out=_outs(g=()))
    elif layout == "odd":
        w = _w(2, 3, 77, dtype=torch.float32)
    elif layout == "fp16":
        w = _w(1, 1, 1, dtype=torch.float16)
    with pytest.raises(dga.DGAError, match="no CPU path"):
        dga.per_block_cast_to_fp8_transposed(w, **kw)


# ---- the identity the GPU tests lean on

@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
@pytest.mark.parametrize("shape", B.SHAPES + [B.SHAPE_2D], ids=lambda s: "x".join(map(str, s)))
def test_the_oracle_commutes_with_transposition_on_every_shape(oracle, shape, ue8m0):
    w = B.random_weights(*((1,) + shape if len(shape) == 2 else shape), seed=sum(shape))
    B.assert_transposition_identity(oracle, w.reshape(shape), ue8m0)


@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
def test_the_oracle_commutes_with_transposition_on_special_values(oracle, ue8m0):
    w = B.special_values()
    B.assert_transposition_identity(oracle, w, ue8m0)
    (qt, sft), (q, sf) = B.reference(oracle, w, ue8m0)
    # what the cases are there for: infinite scales, scale 1 for the all-zero and the NaN-only tile, fp32 max as 448 (ue8m0: 256, under the scale 2^120), NaN codes
    assert np.isinf(sf[1, 0, 0]) and np.isinf(sf[1, 0, 1]) and np.isinf(sf[1, 1, 1]) and np.isfinite(sf[1, 1, 0])
    assert sf[2, 0, 0] == 1.0 and sf[2, 0, 1] == 1.0 and q[2, 131, 66] == (0x78 if ue8m0 else 0x7E) and q[2, 100, 133] == 0xFF
    assert (q[2, 7:40, 9:50] == 0x80).all() and np.count_nonzero(q[2, :128, :128] & 0x7F) == 0
    assert np.isfinite(sf[0]).all() and np.isfinite(sf[3]).all() and q[0, 0, 0] == 0x7F and q[0, 5, 77] == 0x7F and q[0, 64, 130] == 0x7F
    assert q[3, 7, 7] == 0x7F and q[3, 63, 127] == 0x7F and q[3, 135, 15] == 0x7F and q[3, 64, 0] == 0x7F
    assert q[0, 1, 1] == 0x80 and q[1, 3, 4] == 0x7F and q[1, 199, 135] == 0xFF


def test_the_oracle_commutes_with_transposition_on_amax_positions_and_ties(oracle):
    w = B.amax_positions()
    lanes = set()
    for i in range(256):
        r, c = np.unravel_index(np.argmax(np.abs(w[i])), (128, 128))
        lanes.add((16 * (r // 8) + c // 8, 8 * (r % 8) + c % 8))
    assert {t for t, _ in lanes} == set(range(256)) and {s for _, s in lanes} == set(range(64))       # every lane, every (pass, slot)
    B.assert_transposition_identity(oracle, w[::5])
    B.assert_transposition_identity(oracle, B.tie_matrix())
