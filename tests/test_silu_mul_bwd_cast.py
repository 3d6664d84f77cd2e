"""CPU: silu_and_mul_backward_per_token_cast_to_fp8's exports, the C entry's refusals (nothing is launched), the Python argument checks,
and the resource usage of its kernels (dga_silu_mul_bwd_cast.hip)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import deepgemm_ascend_amd as dga
from deepgemm_ascend_amd import _lib

OK, E_NULL, E_SHAPE, E_DTYPE, E_RANGE = 0, -1, -2, -3, -9   # include/dga_hip.h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepgemm_ascend_amd", "csrc")
UNIT = "dga_silu_mul_bwd_cast.hip"


def test_the_symbols_are_exported():
    assert "silu_and_mul_backward_per_token_cast_to_fp8" in dga.__all__
    assert "dga_silu_mul_bwd_cast_to_fp8_1x128" in _lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "dga_hip.h")).read()
    assert re.search(r"\bint\s+dga_silu_mul_bwd_cast_to_fp8_1x128\s*\(", text)
    assert "#define DGA_ABI_VERSION 7" in text                              # an added symbol: the ABI version stays
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert UNIT in mk.split("SRCS =")[1].split("HDRS =")[0]
    assert callable(_lib.lib().dga_silu_mul_bwd_cast_to_fp8_1x128)          # ... and the built library has it
    cpp = open(os.path.join(CSRC, "python_api_amd.cpp")).read()
    assert 'm.def("silu_and_mul_backward_per_token_cast_to_fp8"' in cpp


def _c_call(x=1, grad=6, dt=_lib.DT_BF16, g=1, rows=4, h=128, masked_m=None, m_indices=None, q=2, sf=3, gx=None, flags=0):
    ptr = lambda v: None if v is None else ctypes.c_void_p(0x1000 * v)   # (never dereferenced: every case returns before a launch)
    return _lib.lib().dga_silu_mul_bwd_cast_to_fp8_1x128(ptr(x), ptr(grad), dt, g, rows, h, ptr(masked_m), ptr(m_indices), ptr(q), ptr(sf),
                                                         ptr(gx), flags, None)


def test_c_abi_refuses_without_launching():
    assert _c_call(x=None) == E_NULL and _c_call(grad=None) == E_NULL and _c_call(q=None) == E_NULL and _c_call(sf=None) == E_NULL
    assert _c_call(rows=0) == OK and _c_call(h=0) == OK
    assert _c_call(rows=0, x=None, grad=None, q=None, sf=None) == OK       # nothing to do comes before the pointers
    assert _c_call(rows=0, gx=7) == OK
    assert _c_call(dt=_lib.DT_FP8_E4M3FN) == E_DTYPE and _c_call(dt=99) == E_DTYPE
    assert _c_call(flags=2) == E_RANGE and _c_call(flags=_lib.CAST_UE8M0 | 4) == E_RANGE
    assert _c_call(flags=2, h=100) == E_RANGE                              # the flags come before the shape
    for h in (1, 64, 127, 129, 192, 1000):                                 # H % 128: a block would straddle gate | up
        assert _c_call(h=h) == E_SHAPE, h
    assert _c_call(h=100, x=None) == E_SHAPE and _c_call(h=100, rows=0) == E_SHAPE   # ... before nothing-to-do and the pointers
    assert _c_call(masked_m=4, m_indices=5) == E_SHAPE                     # both masks
    assert _c_call(g=2, m_indices=5) == E_SHAPE                            # the contiguous layout has one group
    assert _c_call(rows=-1) == E_SHAPE and _c_call(h=-128) == E_SHAPE and _c_call(g=0) == E_SHAPE and _c_call(g=-3) == E_SHAPE
    assert _c_call(rows=1 << 40, h=1 << 20) == E_RANGE                     # 2^53 blocks: no grid holds them
    assert _c_call(g=1 << 40, rows=1 << 40, h=128) == E_RANGE
    assert _c_call(x=None, dt=99) == E_NULL                                # the pointers come before the dtype


def _x(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


# (case, the message of the check it exercises): every check runs before the device guard, so a CPU call reaches the check itself
ARG_CASES = [
    ("h_mod_128", "H a multiple of 128"), ("h_odd", "H a multiple of 128"), ("non_contiguous", "contiguous"), ("rank_flat", r"\[rows, 2H\]"),
    ("rank_masked", r"\[G, Mmax, 2H\]"), ("rank_contiguous", r"\[rows, 2H\]"), ("x_dtype", "float32, bfloat16 or float16"),
    ("both", "exclude each other"),
    ("grad_shape", r"grad_h must be contiguous \[8, 256\]"), ("grad_rank", r"grad_h must be contiguous \[8, 256\]"),
    ("grad_strided", r"grad_h must be contiguous \[8, 256\]"), ("grad_dtype", "grad_h must have x's dtype"),
    ("masked_dtype", r"masked_m must be a contiguous int32 \[4\]"), ("masked_shape", r"masked_m must be a contiguous int32 \[4\]"),
    ("indices_dtype", r"m_indices must be a contiguous int32 \[8\]"), ("indices_shape", r"m_indices must be a contiguous int32 \[8\]"),
    ("out_len", r"out must be \(dq, dsf\)"), ("out_q_dtype", "float8_e4m3fn or uint8"), ("out_q_shape", "out dq must be contiguous"),
    ("out_q_strided", "out dq must be contiguous"), ("out_sf_dtype", "out dsf must be contiguous float32"),
    ("out_sf_shape", "out dsf must be contiguous float32"),
    ("gx_shape", r"grad_x_out must be contiguous \[8, 512\]"), ("gx_strided", r"grad_x_out must be contiguous \[8, 512\]"),
    ("gx_dtype", "grad_x_out must have x's dtype"),
]


@pytest.mark.parametrize("case,msg", ARG_CASES, ids=[c[0] for c in ARG_CASES])
def test_argument_errors_raise(case, msg):
    x, d, kw = _x(8, 512), _x(8, 256), {}
    q, sf = torch.zeros(8, 512, dtype=torch.uint8), torch.zeros(8, 4)
    if case == "h_mod_128":
        x, d = _x(8, 384), _x(8, 192)
    elif case == "h_odd":
        x, d = _x(8, 511), _x(8, 255)
    elif case == "non_contiguous":
        x = _x(8, 1024)[:, :512]
    elif case == "rank_flat":
        x, d = _x(2, 4, 512), _x(2, 4, 256)
    elif case == "rank_masked":
        kw["masked_m"] = torch.zeros(4, dtype=torch.int32)
    elif case == "rank_contiguous":
        x, d = _x(2, 4, 512), _x(2, 4, 256); kw["m_indices"] = torch.zeros(8, dtype=torch.int32)
    elif case == "x_dtype":
        x, d = _x(8, 512, dtype=torch.float64), _x(8, 256, dtype=torch.float64)
    elif case == "both":
        kw.update(masked_m=torch.zeros(4, dtype=torch.int32), m_indices=torch.zeros(8, dtype=torch.int32))
    elif case == "grad_shape":
        d = _x(8, 512)
    elif case == "grad_rank":
        d = _x(2, 4, 256)
    elif case == "grad_strided":
        d = _x(8, 512)[:, :256]
    elif case == "grad_dtype":
        d = _x(8, 256, dtype=torch.float16)
    elif case == "masked_dtype":
        x, d = _x(4, 2, 512), _x(4, 2, 256); kw["masked_m"] = torch.zeros(4, dtype=torch.int64)
    elif case == "masked_shape":
        x, d = _x(4, 2, 512), _x(4, 2, 256); kw["masked_m"] = torch.zeros(5, dtype=torch.int32)
    elif case == "indices_dtype":
        kw["m_indices"] = torch.zeros(8, dtype=torch.int64)
    elif case == "indices_shape":
        kw["m_indices"] = torch.zeros(16, dtype=torch.int32)[::2][:7]
    elif case == "out_len":
        kw["out"] = (q,)
    elif case == "out_q_dtype":
        kw["out"] = (torch.zeros(8, 512, dtype=torch.int8), sf)
    elif case == "out_q_shape":
        kw["out"] = (torch.zeros(8, 256, dtype=torch.uint8), sf)
    elif case == "out_q_strided":
        kw["out"] = (torch.zeros(8, 1024, dtype=torch.uint8)[:, :512], sf)
    elif case == "out_sf_dtype":
        kw["out"] = (q, sf.double())
    elif case == "out_sf_shape":
        kw["out"] = (q, torch.zeros(8, 2))
    elif case == "gx_shape":
        kw["grad_x_out"] = _x(8, 256)
    elif case == "gx_strided":
        kw["grad_x_out"] = _x(8, 1024)[:, :512]
    elif case == "gx_dtype":
        kw["grad_x_out"] = _x(8, 512, dtype=torch.float32)
    with pytest.raises(dga.DGAError, match=msg):
        dga.silu_and_mul_backward_per_token_cast_to_fp8(x, d, **kw)


@pytest.mark.parametrize("layout", ["flat", "masked", "contiguous", "out", "grad_x_out"])
def test_a_valid_cpu_call_gets_past_every_argument_check(layout):
    """The same arguments without a fault reach the device guard (so each case above is refused by its own check)."""
    x, d, kw = _x(8, 512), _x(8, 256), {}
    if layout == "masked":
        x, d = _x(4, 2, 512), _x(4, 2, 256); kw["masked_m"] = torch.zeros(4, dtype=torch.int32)
    elif layout == "contiguous":
        kw["m_indices"] = torch.zeros(8, dtype=torch.int32)
    elif layout == "out":
        kw["out"] = (torch.zeros(8, 512, dtype=torch.float8_e4m3fn), torch.zeros(8, 4))
    elif layout == "grad_x_out":
        kw["grad_x_out"] = _x(8, 512)
    with pytest.raises(dga.DGAError, match="no CPU path"):
        dga.silu_and_mul_backward_per_token_cast_to_fp8(x, d, **kw)


def _resource_usage(unit):
    """(kernel, VGPRs, VGPR spills, SGPR spills, scratch bytes) of every kernel of a unit, compiled with the flags `make -n` gives it
    (as tests/test_silu_mul_cast.py reads them)."""
    obj = f"../../build/csrc/{os.path.splitext(unit)[0]}.o"
    r = subprocess.run(["make", "-n", "-B", "-C", CSRC, obj], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-1000:]
    line = [l for l in r.stdout.splitlines() if "hipcc" in l and f" {unit} " in l + " "][-1].split()
    flags = [w for i, w in enumerate(line[1:], 1) if w not in ("-c", unit) and line[i - 1] != "-o" and w != "-o"]
    cmd = ["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-S", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", unit]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = [], None
    for l in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = [m.group(1), 0, 0, 0, 0]
            out.append(cur)
        for i, key in ((1, r"VGPRs"), (2, r"VGPRs Spill"), (3, r"SGPRs Spill"), (4, r"ScratchSize \[bytes/lane\]")):
            m = re.search(r"remark:\s+" + key + r": (\d+)", l)
            if m and cur:
                cur[i] = int(m.group(1))
    return out


def test_the_kernels_do_not_spill():
    """One instantiation per input type; each keeps everything in registers: no scratch, no VGPR or SGPR spills.  The VGPR counts are
    printed (DESIGN.md records them: 53 / 55 / 57 for fp32 / bf16 / fp16, eight waves per SIMD); measured with this compiler, so the
    assertion is the occupancy they stand for, <= 64, as for the forward kernel."""
    ks = _resource_usage(UNIT)
    assert len(ks) == 3 and all("silu_mul_bwd_cast_1x128_kernel" in k[0] for k in ks), [k[0] for k in ks]
    for name, vgprs, vspill, sspill, scratch in ks:
        print(f"{name}: {vgprs} VGPRs, {vspill} VGPR spills, {sspill} SGPR spills, {scratch} scratch bytes")
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vgprs, vspill, sspill, scratch)
        assert vgprs <= 64, (name, vgprs)
