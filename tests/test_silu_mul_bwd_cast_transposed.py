"""CPU: silu_and_mul_backward_per_token_cast_to_fp8_transposed's exports, the C entry's refusals (nothing is launched), the Python argument
checks, and the resource usage of its kernels (dga_silu_mul_bwd_cast_transposed.hip)."""
import ctypes
import os
import re

import pytest
import torch

import deepgemm_ascend_amd as dga
from deepgemm_ascend_amd import _lib
from test_silu_mul_cast import _resource_usage

OK, E_NULL, E_SHAPE, E_DTYPE, E_RANGE = 0, -1, -2, -3, -9   # include/dga_hip.h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepgemm_ascend_amd", "csrc")
UNIT = "dga_silu_mul_bwd_cast_transposed.hip"


def test_the_symbols_are_exported():
    assert "silu_and_mul_backward_per_token_cast_to_fp8_transposed" in dga.__all__
    assert "dga_silu_mul_bwd_cast_to_fp8_1x128_transposed" in _lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "dga_hip.h")).read()
    assert re.search(r"\bint\s+dga_silu_mul_bwd_cast_to_fp8_1x128_transposed\s*\(", text)
    assert "#define DGA_ABI_VERSION 7" in text                              # an added symbol: the ABI version stays
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert UNIT in mk.split("SRCS =")[1].split("HDRS =")[0].split()
    dep = [l for l in mk.splitlines() if l.rstrip().endswith(": dga_cast_device.hpp")]
    assert len(dep) == 1 and "$(OBJ)/dga_silu_mul_bwd_cast_transposed.o" in dep[0].split()     # the shared device text rebuilds it
    assert callable(_lib.lib().dga_silu_mul_bwd_cast_to_fp8_1x128_transposed)   # ... and the built library has it


def test_the_backward_device_text_is_shared():
    """silu_mul_bwd and the two fp64-rounded maxima are defined once, in dga_cast_device.hpp, and both backward units use them from there."""
    hpp = open(os.path.join(CSRC, "dga_cast_device.hpp")).read()
    for fn in ("silu_mul_bwd", "dgate_abs_rounded", "dup_abs_rounded"):
        define = re.compile(r"__device__ __forceinline__ \w+ " + fn + r"\(")
        assert len(define.findall(hpp)) == 1, fn
        for unit in ("dga_silu_mul_bwd_cast.hip", UNIT):
            text = open(os.path.join(CSRC, unit)).read()
            assert not define.search(text) and re.search(r"\b" + fn + r"\(", text), (unit, fn)


def _c_call(x=1, grad=9, dt=_lib.DT_BF16, g=1, rows=4, h=128, masked_m=None, m_indices=None, qt=2, ldqt=None, sft=3, q=None, sf=None,
            flags=0):
    ptr = lambda v: None if v is None else ctypes.c_void_p(0x1000 * v)   # (never dereferenced: every case returns before a launch)
    ldqt = g * rows if ldqt is None else ldqt
    return _lib.lib().dga_silu_mul_bwd_cast_to_fp8_1x128_transposed(ptr(x), ptr(grad), dt, g, rows, h, ptr(masked_m), ptr(m_indices), ptr(qt),
                                                                    ldqt, ptr(sft), ptr(q), ptr(sf), flags, None)


def test_c_abi_refuses_without_launching():
    """The cases of tests/test_silu_mul_cast_transposed.py test_c_abi_refuses_without_launching, with its codes and its order, plus grad_h and
    h % 128 (h: half the width of x)."""
    # DGA_E_RANGE: an unknown flag, before everything else
    assert _c_call(flags=2) == E_RANGE and _c_call(flags=_lib.CAST_UE8M0 | 4) == E_RANGE
    assert _c_call(flags=2, rows=-1) == E_RANGE and _c_call(flags=2, x=None) == E_RANGE and _c_call(flags=2, h=64) == E_RANGE
    # DGA_E_SHAPE: negative sizes, h % 128 != 0, both masks, m_indices with groups != 1, ldqt out of range, exactly one of q_row / sf_row
    assert _c_call(rows=-1, ldqt=0) == E_SHAPE and _c_call(h=-128) == E_SHAPE and _c_call(g=-3, ldqt=0) == E_SHAPE
    assert _c_call(g=0, ldqt=0) == E_SHAPE                                  # (groups < 1, as in the fused entries)
    assert _c_call(h=64) == E_SHAPE and _c_call(h=200) == E_SHAPE and _c_call(h=129) == E_SHAPE
    assert _c_call(h=64, x=None) == E_SHAPE and _c_call(h=64, rows=0) == E_SHAPE     # ... before nothing-to-do and the pointers
    assert _c_call(masked_m=4, m_indices=5) == E_SHAPE
    assert _c_call(g=2, m_indices=5) == E_SHAPE
    assert _c_call(rows=300, ldqt=299) == E_SHAPE and _c_call(rows=300, ldqt=385) == E_SHAPE
    assert _c_call(rows=256, ldqt=257) == E_SHAPE and _c_call(rows=256, ldqt=384) == E_SHAPE     # round_up(256, 128) = 256
    assert _c_call(g=2, rows=100, ldqt=100) == E_SHAPE                      # T = groups * rows
    assert _c_call(g=1 << 40, rows=1 << 40, ldqt=0) == E_SHAPE              # a T beyond int64 has no ldqt
    assert _c_call(q=7) == E_SHAPE and _c_call(sf=8) == E_SHAPE
    assert _c_call(rows=0, ldqt=5) == E_SHAPE and _c_call(q=7, x=None) == E_SHAPE     # ... before nothing-to-do and the pointers
    # DGA_OK: T == 0 or h == 0, whatever the pointers
    assert _c_call(rows=0) == OK and _c_call(h=0) == OK
    assert _c_call(rows=0, x=None, grad=None, qt=None, sft=None) == OK and _c_call(h=0, x=None, grad=None, qt=None, sft=None, q=7, sf=8) == OK
    assert _c_call(g=3, rows=0, masked_m=4) == OK
    # DGA_E_NULL: a required pointer, before the dtype
    assert _c_call(x=None) == E_NULL and _c_call(grad=None) == E_NULL and _c_call(qt=None) == E_NULL and _c_call(sft=None) == E_NULL
    assert _c_call(x=None, dt=99) == E_NULL and _c_call(grad=None, dt=99) == E_NULL
    # DGA_E_DTYPE
    assert _c_call(dt=_lib.DT_FP8_E4M3FN) == E_DTYPE and _c_call(dt=99) == E_DTYPE
    # DGA_E_RANGE: more tile halves than a grid holds
    assert _c_call(rows=1 << 40, h=1 << 20) == E_RANGE
    assert _c_call(rows=1, h=1 << 40) == E_RANGE                            # 2^34 tile halves of one token: the tile count, not the element count
    assert _c_call(rows=1, h=128 << 30) == E_RANGE                          # 2^30 tiles fit a grid, their 2^31 halves do not
    # every ldqt of the range gets past the shape check (a bad dtype is met next)
    for ldqt in (300, 301, 383, 384):
        assert _c_call(rows=300, ldqt=ldqt, dt=99) == E_DTYPE, ldqt
    assert _c_call(g=3, rows=100, ldqt=384, dt=99, masked_m=4) == E_DTYPE
    assert _c_call(q=7, sf=8, dt=99) == E_DTYPE


def _x(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


# (case, the message of the check it exercises): every check runs before the device guard, so a CPU call reaches the check itself.
# x is [8, 512], grad_h [8, 256]: H = 256, T = 8, 2H = 512 channels in the result -- the family's cases and messages on the output side.
ARG_CASES = [
    ("not_256", "H a multiple of 128"), ("odd", "H a multiple of 128"), ("non_contiguous", "contiguous"), ("rank_flat", r"\[rows, 2H\]"),
    ("rank_masked", r"\[G, Mmax, 2H\]"), ("rank_contiguous", r"\[rows, 2H\]"), ("x_dtype", "float32, bfloat16 or float16"),
    ("both", "exclude each other"),
    ("masked_dtype", r"masked_m must be a contiguous int32 \[4\]"), ("masked_shape", r"masked_m must be a contiguous int32 \[4\]"),
    ("indices_dtype", r"m_indices must be a contiguous int32 \[8\]"), ("indices_shape", r"m_indices must be a contiguous int32 \[8\]"),
    ("grad_dtype", "grad_h must have x's dtype"), ("grad_shape", r"grad_h must be contiguous \[8, 256\]"),
    ("grad_full_width", r"grad_h must be contiguous \[8, 256\]"), ("grad_rank", r"grad_h must be contiguous \[4, 2, 256\]"),
    ("grad_non_contiguous", r"grad_h must be contiguous \[8, 256\]"),
    ("out_len", r"out must be \(qt, sft\)"), ("out_nesting", r"out must hold \(qt, sft\)"), ("out_len_rowwise", r"out must be \(\(qt, sft\), \(q, sf\)\)"),
    ("out_qt_dtype", "float8_e4m3fn or uint8"), ("out_qt_shape", r"out qt must be \[512, 8\]"), ("out_qt_untransposed", r"out qt must be \[512, 8\]"),
    ("out_qt_half_width", r"out qt must be \[512, 8\]"),
    ("out_qt_stride", "rows 128 bytes apart"), ("out_qt_stride_unaligned", "rows 8 bytes apart"),
    ("out_sft_dtype", r"out sft must be contiguous float32 \[512, 1\]"), ("out_sft_shape", r"out sft must be contiguous float32 \[512, 1\]"),
    ("out_q_shape", "out q must be contiguous"), ("out_sf_shape", "out sf must be contiguous float32"),
]


@pytest.mark.parametrize("case,msg", ARG_CASES, ids=[c[0] for c in ARG_CASES])
def test_argument_errors_raise(case, msg):
    x, grad, kw = _x(8, 512), _x(8, 256), {}
    qt, sft = torch.zeros(512, 8, dtype=torch.uint8), torch.zeros(512, 1)
    q, sf = torch.zeros(8, 512, dtype=torch.uint8), torch.zeros(8, 4)
    if case == "not_256":
        x, grad = _x(8, 384), _x(8, 192)
    elif case == "odd":
        x = _x(8, 511)
    elif case == "non_contiguous":
        x = _x(8, 1024)[:, :512]
    elif case == "rank_flat":
        x, grad = _x(2, 4, 512), _x(2, 4, 256)
    elif case == "rank_masked":
        kw["masked_m"] = torch.zeros(4, dtype=torch.int32)
    elif case == "rank_contiguous":
        x, grad = _x(2, 4, 512), _x(2, 4, 256); kw["m_indices"] = torch.zeros(8, dtype=torch.int32)
    elif case == "x_dtype":
        x, grad = _x(8, 512, dtype=torch.float64), _x(8, 256, dtype=torch.float64)
    elif case == "both":
        kw.update(masked_m=torch.zeros(4, dtype=torch.int32), m_indices=torch.zeros(8, dtype=torch.int32))
    elif case == "masked_dtype":
        x, grad = _x(4, 2, 512), _x(4, 2, 256); kw["masked_m"] = torch.zeros(4, dtype=torch.int64)
    elif case == "masked_shape":
        x, grad = _x(4, 2, 512), _x(4, 2, 256); kw["masked_m"] = torch.zeros(5, dtype=torch.int32)
    elif case == "indices_dtype":
        kw["m_indices"] = torch.zeros(8, dtype=torch.int64)
    elif case == "indices_shape":
        kw["m_indices"] = torch.zeros(16, dtype=torch.int32)[::2][:7]
    elif case == "grad_dtype":
        grad = _x(8, 256, dtype=torch.float16)
    elif case == "grad_shape":
        grad = _x(7, 256)
    elif case == "grad_full_width":
        grad = _x(8, 512)
    elif case == "grad_rank":
        x = _x(4, 2, 512); kw["masked_m"] = torch.zeros(4, dtype=torch.int32)       # grad_h [8, 256] beside x [4, 2, 512]
    elif case == "grad_non_contiguous":
        grad = _x(8, 512)[:, :256]
    elif case == "out_len":
        kw["out"] = (qt,)
    elif case == "out_nesting":
        kw.update(rowwise=True, out=(qt, sft))
    elif case == "out_len_rowwise":
        kw.update(rowwise=True, out=((qt, sft),))
    elif case == "out_qt_dtype":
        kw["out"] = (torch.zeros(512, 8, dtype=torch.int8), sft)
    elif case == "out_qt_shape":
        kw["out"] = (torch.zeros(512, 16, dtype=torch.uint8), sft)
    elif case == "out_qt_untransposed":
        kw["out"] = (torch.zeros(8, 512, dtype=torch.uint8), sft)
    elif case == "out_qt_half_width":
        kw["out"] = (torch.zeros(256, 8, dtype=torch.uint8), sft)      # the channels of the result are 2H, not H
    elif case == "out_qt_stride":
        kw.update(aligned_rows=True, out=(qt, sft))
    elif case == "out_qt_stride_unaligned":
        kw["out"] = (torch.zeros(512, 128, dtype=torch.uint8)[:, :8], sft)
    elif case == "out_sft_dtype":
        kw["out"] = (qt, sft.double())
    elif case == "out_sft_shape":
        kw["out"] = (qt, torch.zeros(512, 2))
    elif case == "out_q_shape":
        kw.update(rowwise=True, out=((qt, sft), (torch.zeros(8, 256, dtype=torch.uint8), sf)))
    elif case == "out_sf_shape":
        kw.update(rowwise=True, out=((qt, sft), (q, torch.zeros(8, 2))))
    with pytest.raises(dga.DGAError, match=msg):
        dga.silu_and_mul_backward_per_token_cast_to_fp8_transposed(x, grad, **kw)


def test_there_is_no_grad_x_out():
    with pytest.raises(TypeError):
        dga.silu_and_mul_backward_per_token_cast_to_fp8_transposed(_x(8, 512), _x(8, 256), grad_x_out=_x(8, 512))


@pytest.mark.parametrize("layout", ["flat", "masked", "contiguous", "out", "out_aligned", "rowwise", "rowwise_out", "fp32", "fp16"])
def test_a_valid_cpu_call_gets_past_every_argument_check(layout):
    """The same arguments without a fault reach the device guard (so each case above is refused by its own check): CPU tensors raise there."""
    x, grad, kw = _x(8, 512), _x(8, 256), {}
    if layout == "masked":
        x, grad = _x(4, 2, 512), _x(4, 2, 256); kw["masked_m"] = torch.zeros(4, dtype=torch.int32)
    elif layout == "contiguous":
        kw["m_indices"] = torch.zeros(8, dtype=torch.int32)
    elif layout == "out":
        kw["out"] = (torch.zeros(512, 8, dtype=torch.float8_e4m3fn), torch.zeros(512, 1))
    elif layout == "out_aligned":
        kw.update(aligned_rows=True, out=(torch.zeros(512, 128, dtype=torch.uint8)[:, :8], torch.zeros(512, 1)))
    elif layout == "rowwise":
        kw["rowwise"] = True
    elif layout == "rowwise_out":
        kw.update(rowwise=True, out=((torch.zeros(512, 8, dtype=torch.uint8), torch.zeros(512, 1)),
                                     (torch.zeros(8, 512, dtype=torch.uint8), torch.zeros(8, 4))))
    elif layout == "fp32":
        x, grad = _x(3, 256, dtype=torch.float32), _x(3, 128, dtype=torch.float32)
    elif layout == "fp16":
        x, grad = _x(3, 256, dtype=torch.float16), _x(3, 128, dtype=torch.float16)
    with pytest.raises(dga.DGAError, match="no CPU path"):
        dga.silu_and_mul_backward_per_token_cast_to_fp8_transposed(x, grad, **kw)


def test_the_kernels_do_not_spill():
    """Three input types x with and without the row-wise output (each holds both halves' text behind a uniform branch); each keeps everything
    in registers -- no scratch, no VGPR or SGPR spills -- in at most 128 VGPRs, what __launch_bounds__(256, 4) declares: 16 waves per CU
    keep four per SIMD, and with 18 KB of LDS four workgroups share a CU."""
    unit = open(os.path.join(CSRC, UNIT)).read()
    assert unit.count("__launch_bounds__(256, 4)") == 2 and unit.count("__launch_bounds__(") == 2      # the kernel and its comment
    ks = _resource_usage(UNIT)
    assert len(ks) == 6 and all("silu_mul_bwd_cast_1x128_transposed_kernel" in k[0] for k in ks), [k[0] for k in ks]
    for name, vgprs, vspill, sspill, scratch in ks:
        assert vgprs <= 128 and vspill == 0 and sspill == 0 and scratch == 0, (name, vgprs, vspill, sspill, scratch)
