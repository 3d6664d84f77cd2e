"""CPU: silu_and_mul_per_token_cast_to_fp8's exports, the C entry's refusals (nothing is launched), the Python argument checks, and
the resource usage of its kernels (dga_silu_mul_cast.hip)."""
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
UNIT = "dga_silu_mul_cast.hip"


def test_the_status_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "dga_hip.h")).read()
    for name, val in (("DGA_OK", OK), ("DGA_E_NULL", E_NULL), ("DGA_E_SHAPE", E_SHAPE), ("DGA_E_DTYPE", E_DTYPE), ("DGA_E_RANGE", E_RANGE)):
        assert re.search(rf"\b{name}\s*=\s*{val}\b", text), name


def test_the_symbols_are_exported():
    assert "silu_and_mul_per_token_cast_to_fp8" in dga.__all__
    assert "dga_silu_mul_cast_to_fp8_1x128" in _lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "dga_hip.h")).read()
    assert re.search(r"\bint\s+dga_silu_mul_cast_to_fp8_1x128\s*\(", text)
    assert "#define DGA_ABI_VERSION 7" in text                              # an added symbol: the ABI version stays
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert UNIT in mk.split("SRCS =")[1].split("HDRS =")[0]


def _c_call(x=1, dt=_lib.DT_BF16, g=1, rows=4, h=128, masked_m=None, m_indices=None, q=2, sf=3, flags=0):
    ptr = lambda v: None if v is None else ctypes.c_void_p(0x1000 * v)   # (never dereferenced: every case returns before a launch)
    return _lib.lib().dga_silu_mul_cast_to_fp8_1x128(ptr(x), dt, g, rows, h, ptr(masked_m), ptr(m_indices), ptr(q), ptr(sf), flags, None)


def test_c_abi_refuses_without_launching():
    assert _c_call(x=None) == E_NULL and _c_call(q=None) == E_NULL and _c_call(sf=None) == E_NULL
    assert _c_call(rows=0) == OK and _c_call(h=0) == OK
    assert _c_call(rows=0, x=None, q=None, sf=None) == OK                  # nothing to do comes before the pointers
    assert _c_call(dt=_lib.DT_FP8_E4M3FN) == E_DTYPE and _c_call(dt=99) == E_DTYPE
    assert _c_call(flags=2) == E_RANGE and _c_call(flags=_lib.CAST_UE8M0 | 4) == E_RANGE
    assert _c_call(masked_m=4, m_indices=5) == E_SHAPE                     # both masks
    assert _c_call(g=2, m_indices=5) == E_SHAPE                            # the contiguous layout has one group
    assert _c_call(rows=-1) == E_SHAPE and _c_call(h=-1) == E_SHAPE and _c_call(g=0) == E_SHAPE and _c_call(g=-3) == E_SHAPE
    assert _c_call(rows=1 << 40, h=1 << 20) == E_RANGE                     # 2^53 blocks: no grid holds them
    assert _c_call(g=1 << 40, rows=1 << 40, h=128) == E_RANGE


def _x(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


# (case, the message of the check it exercises): every check runs before the device guard, so a CPU call reaches the check itself
ARG_CASES = [
    ("odd", "must be even"), ("non_contiguous", "contiguous"), ("rank_flat", r"\[rows, 2H\]"), ("rank_masked", r"\[G, Mmax, 2H\]"),
    ("rank_contiguous", r"\[rows, 2H\]"), ("x_dtype", "float32, bfloat16 or float16"), ("both", "exclude each other"),
    ("masked_dtype", r"masked_m must be a contiguous int32 \[4\]"), ("masked_shape", r"masked_m must be a contiguous int32 \[4\]"),
    ("indices_dtype", r"m_indices must be a contiguous int32 \[8\]"), ("indices_shape", r"m_indices must be a contiguous int32 \[8\]"),
    ("out_len", r"out must be \(q, sf\)"), ("out_q_dtype", "float8_e4m3fn or uint8"), ("out_q_shape", "out q must be contiguous"),
    ("out_q_strided", "out q must be contiguous"), ("out_sf_dtype", "out sf must be contiguous float32"),
    ("out_sf_shape", "out sf must be contiguous float32"),
]


@pytest.mark.parametrize("case,msg", ARG_CASES, ids=[c[0] for c in ARG_CASES])
def test_argument_errors_raise(case, msg):
    x, kw = _x(8, 512), {}
    q, sf = torch.zeros(8, 256, dtype=torch.uint8), torch.zeros(8, 2)
    if case == "odd":
        x = _x(8, 511)
    elif case == "non_contiguous":
        x = _x(8, 1024)[:, :512]
    elif case == "rank_flat":
        x = _x(2, 4, 512)
    elif case == "rank_masked":
        kw["masked_m"] = torch.zeros(4, dtype=torch.int32)
    elif case == "rank_contiguous":
        x = _x(2, 4, 512); kw["m_indices"] = torch.zeros(8, dtype=torch.int32)
    elif case == "x_dtype":
        x = _x(8, 512, dtype=torch.float64)
    elif case == "both":
        kw.update(masked_m=torch.zeros(4, dtype=torch.int32), m_indices=torch.zeros(8, dtype=torch.int32))
    elif case == "masked_dtype":
        x = _x(4, 2, 512); kw["masked_m"] = torch.zeros(4, dtype=torch.int64)
    elif case == "masked_shape":
        x = _x(4, 2, 512); kw["masked_m"] = torch.zeros(5, dtype=torch.int32)
    elif case == "indices_dtype":
        kw["m_indices"] = torch.zeros(8, dtype=torch.int64)
    elif case == "indices_shape":
        kw["m_indices"] = torch.zeros(16, dtype=torch.int32)[::2][:7]
    elif case == "out_len":
        kw["out"] = (q,)
    elif case == "out_q_dtype":
        kw["out"] = (torch.zeros(8, 256, dtype=torch.int8), sf)
    elif case == "out_q_shape":
        kw["out"] = (torch.zeros(8, 512, dtype=torch.uint8), sf)
    elif case == "out_q_strided":
        kw["out"] = (torch.zeros(8, 512, dtype=torch.uint8)[:, :256], sf)
    elif case == "out_sf_dtype":
        kw["out"] = (q, sf.double())
    elif case == "out_sf_shape":
        kw["out"] = (q, torch.zeros(8, 3))
    with pytest.raises(dga.DGAError, match=msg):
        dga.silu_and_mul_per_token_cast_to_fp8(x, **kw)


@pytest.mark.parametrize("layout", ["flat", "masked", "contiguous", "out"])
def test_a_valid_cpu_call_gets_past_every_argument_check(layout):
    """The same arguments without a fault reach the device guard (so each case above is refused by its own check)."""
    x, kw = _x(8, 512), {}
    if layout == "masked":
        x = _x(4, 2, 512); kw["masked_m"] = torch.zeros(4, dtype=torch.int32)
    elif layout == "contiguous":
        kw["m_indices"] = torch.zeros(8, dtype=torch.int32)
    elif layout == "out":
        kw["out"] = (torch.zeros(8, 256, dtype=torch.float8_e4m3fn), torch.zeros(8, 2))
    with pytest.raises(dga.DGAError, match="no CPU path"):
        dga.silu_and_mul_per_token_cast_to_fp8(x, **kw)


def _resource_usage(unit):
    """(kernel, VGPRs, VGPR spills, SGPR spills, scratch bytes) of every kernel of a unit, compiled with the flags `make -n` gives it
    (as tests/test_k_grouped_wgrad.py reads them)."""
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
    """One instantiation per input type; each keeps everything in registers: no scratch, no VGPR or SGPR spills, and few enough
    VGPRs (<= 64) for eight waves per SIMD -- the kernel hides its load latency by occupancy alone."""
    ks = _resource_usage(UNIT)
    assert len(ks) == 3 and all("silu_mul_cast_1x128_kernel" in k[0] for k in ks), [k[0] for k in ks]
    for name, vgprs, vspill, sspill, scratch in ks:
        assert vgprs <= 64 and vspill == 0 and sspill == 0 and scratch == 0, (name, vgprs, vspill, sspill, scratch)
