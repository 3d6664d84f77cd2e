"""CPU: k_grouped_wgrad_gemm_fp8_fp8_fp32_nt's exports, default tilings, refusals and argument checks (nothing is launched), and the
resource usage of its builds (dga_launch_menu_p.hip)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import deepgemm_ascend_amd as dga
from deepgemm_ascend_amd import _lib

E_NULL, E_SHAPE, E_ALIGN, E_TILING = -1, -2, -4, -6   # include/dga_hip.h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepgemm_ascend_amd", "csrc")


def test_the_symbols_are_exported():
    for name in ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", "tiling_k_grouped_wgrad", "tiling_check_k_grouped_wgrad"):
        assert name in dga.__all__


@pytest.mark.parametrize("g,m,n,k", [(1, 128, 128, 128), (8, 4096, 7168, 32768), (32, 7168, 2048, 32768), (4, 300, 257, 0),
                                     (64, 16, 16, 8192), (2, 1, 1, 256)])
def test_default_tilings_pass_their_own_check(g, m, n, k):
    t = dga.tiling_k_grouped_wgrad(m, n, k, g)
    assert dga.tiling_check_k_grouped_wgrad(t) == 0
    assert t.dispatchPolicyTag == 7 and t.splitkFactor == 1 and t.kernelSerial == 0
    assert _lib.lib().dga_workspace_bytes(ctypes.byref(t)) == 0


def test_large_rasters_take_the_persistent_build():
    assert dga.tiling_k_grouped_wgrad(4096, 7168, 32768, 8).build == 7
    assert dga.tiling_k_grouped_wgrad(128, 256, 1024, 2).build == 8


def test_groups_of_fewer_than_eight_tiles_take_a_one_tile_build():
    """The persistent list gives XCD x chunk x of every group: with 2 tiles per group six XCDs would idle."""
    t = dga.tiling_k_grouped_wgrad(256, 256, 32768, 128)
    assert t.build == 8 and dga.tiling_check_k_grouped_wgrad(t) == 0


def test_a_strict_process_default_gives_tag_3():
    code = ("import deepgemm_ascend_amd as d; t = d.tiling_k_grouped_wgrad(512, 512, 4096, 4); "
            "print(t.dispatchPolicyTag, d.tiling_check_k_grouped_wgrad(t))")
    env = dict(os.environ, DGA_DEFAULT_POLICY="strict")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["3", "0"]


def _base():
    return dga.tiling_k_grouped_wgrad(1024, 1024, 4096, 4)


REFUSED = {
    "split_k": dict(splitkFactor=4, kernelSerial=4),
    "split_k_strict": dict(splitkFactor=2, dispatchPolicyTag=3),
    "two_launch_split_k": dict(kernelSerial=4),
    "tail_pair": dict(kernelSerial=5, m1=128, n1=256),
    "workgroup_split_k": dict(kernelSerial=6),
    "stream_k": dict(kernelSerial=7, m1=128, n1=256),
    "decode": dict(kernelSerial=6, build=10, m1=64, n1=128),
    "register": dict(kernelSerial=6, build=1),
    "image": dict(build=5),
    "aimage": dict(build=4),
    "grouped": dict(build=9),
    "fast": dict(dispatchPolicyTag=0),
    "fast_persistent": dict(dispatchPolicyTag=5),
    "ue8m0": dict(dispatchPolicyTag=7 | 16),
    "persistent_off_128x256": dict(build=7, m1=64, n1=128),
    "tile_off_the_menu": dict(m1=96, n1=192),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_tilings(name):
    t = _base()
    for k, v in REFUSED[name].items():
        setattr(t, k, v)
    assert dga.tiling_check_k_grouped_wgrad(t) == E_TILING


def _c_call(a=1, lda=256, sfa=1, b=1, ldb=256, sfb=1, c=None, out=1, ks=1, g=2, m=8, n=8, k=256, flags=0, t=None):
    tt = _base() if t is None else t
    ptr = lambda v: None if v is None else ctypes.c_void_p(0x1000 * v)   # (never dereferenced: every case is refused first)
    return _lib.lib().dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(ptr(a), lda, ptr(sfa), ptr(b), ldb, ptr(sfb), ptr(c), ptr(out), ptr(ks),
                                                                g, m, n, k, flags, ctypes.byref(tt), None, 0, None)


def test_c_abi_refuses_without_launching():
    assert _c_call(m=-1) == E_SHAPE
    assert _c_call(g=-1) == E_SHAPE
    assert _c_call(k=200, lda=256, ldb=256) == E_SHAPE
    assert _c_call(lda=128) == E_SHAPE
    assert _c_call(lda=264) == E_ALIGN
    assert _c_call(ks=None) == E_NULL
    assert _c_call(a=None) == E_NULL
    assert _c_call(out=None) == E_NULL
    assert _c_call(c=1, out=2, m=64, n=64) == E_SHAPE   # c overlaps out by part
    t = _base(); t.splitkFactor = 2
    assert _c_call(t=t) == E_TILING
    assert _c_call(g=0) == 0 and _c_call(m=0) == 0          # nothing to do


def _args(g=3, m=64, n=32, k=512):
    a = torch.zeros(m, k, dtype=torch.uint8)
    b = torch.zeros(n, k, dtype=torch.uint8)
    return (a, torch.ones(m, k // 128)), (b, torch.ones(n, k // 128)), torch.zeros(g, m, n)


# (case, the message of the check it exercises): every check runs before the device guard, so a CPU call reaches the check itself
ARG_CASES = [("len", "ks must hold 3 counts"), ("mult", "multiple of 128"), ("neg", "multiple of 128"), ("sum", "exceeds K_total"),
             ("block_sfb", r"sfb must be \[32,4\]"), ("ks_dtype", "ks_tensor must be a contiguous int32"),
             ("ks_shape", "ks_tensor must be a contiguous int32"), ("out_shape", r"B \[33, K_total\]"),
             ("out_dtype", "out must be a contiguous float32"), ("k_total", "K_total must be a multiple of 128"),
             ("c_shape", "c must be a contiguous float32"), ("c_overlap", "c must be out itself or not overlap it"),
             ("policy", "policy must be one of"), ("sfa_shape", r"sfa must be \[64,4\]"), ("stride", "multiples of 16 bytes")]


@pytest.mark.parametrize("case,msg", ARG_CASES, ids=[c[0] for c in ARG_CASES])
def test_argument_errors_raise(case, msg):
    lhs, rhs, out = _args()
    ks = [128, 256, 128]
    kw = {}
    if case == "len":
        ks = [128, 256]
    elif case == "mult":
        ks = [100, 256, 128]
    elif case == "neg":
        ks = [-128, 256, 128]
    elif case == "sum":
        ks = [256, 256, 128]
    elif case == "block_sfb":
        rhs = (rhs[0], torch.ones(1, 4))
    elif case == "ks_dtype":
        kw["ks_tensor"] = torch.tensor(ks, dtype=torch.int64)
    elif case == "ks_shape":
        kw["ks_tensor"] = torch.tensor(ks + [0], dtype=torch.int32)
    elif case == "out_shape":
        out = torch.zeros(3, 64, 33)
    elif case == "out_dtype":
        out = torch.zeros(3, 64, 32, dtype=torch.bfloat16)
    elif case == "k_total":
        lhs = (torch.zeros(64, 500, dtype=torch.uint8), torch.ones(64, 4))
        rhs = (torch.zeros(32, 500, dtype=torch.uint8), torch.ones(32, 4))
    elif case == "c_shape":
        kw["c"] = torch.zeros(3, 64, 31)
    elif case == "c_overlap":
        big = torch.zeros(2 * 3 * 64 * 32)
        out = big[:3 * 64 * 32].view(3, 64, 32)
        kw["c"] = big[64:64 + 3 * 64 * 32].view(3, 64, 32)
    elif case == "policy":
        kw["policy"] = "fast"
    elif case == "sfa_shape":
        lhs = (lhs[0], torch.ones(64, 3))
    elif case == "stride":
        lhs = (torch.zeros(64, 520, dtype=torch.uint8)[:, :512], lhs[1])
    with pytest.raises(dga.DGAError, match=msg):
        dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, out, ks, **kw)


def test_a_valid_cpu_call_gets_past_every_argument_check():
    """The same arguments without a fault reach the device guard (so each case above is refused by its own check)."""
    lhs, rhs, out = _args()
    with pytest.raises(dga.DGAError, match="no CPU path"):
        dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, out, [128, 256, 128])


def _resource_usage(unit):
    """(kernel, VGPRs, VGPR spills, SGPR spills, scratch bytes) of every kernel of a unit, compiled with the Makefile's flags (as
    tests/test_wgrad.py reads them)."""
    obj = f"../../build/csrc/{os.path.splitext(unit)[0]}.o"
    r = subprocess.run(["make", "-n", "-B", "-C", CSRC, obj], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-1000:]
    line = [l for l in r.stdout.splitlines() if "hipcc" in l and f" {unit} " in l + " "][-1].split()
    flags = [w for i, w in enumerate(line[1:], 1) if w not in ("-c", unit) and line[i - 1] != "-o" and w != "-o"]
    cmd = ["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-S", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", unit]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, cwd=CSRC)
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


def test_the_k_grouped_builds_do_not_spill():
    """The eight k-grouped builds fit 256 VGPRs with nothing in scratch; the one-tile and strict builds spill no SGPRs either, the
    persistent one no more than the 50 SGPR lanes it keeps in VGPRs now (the existing persistent builds keep 19-38)."""
    ks = _resource_usage("dga_launch_menu_p.hip")
    assert len(ks) == 8, [k[0] for k in ks]
    for name, vgprs, vspill, sspill, scratch in ks:
        assert vgprs <= 256 and vspill == 0 and scratch == 0, name
        assert sspill <= (50 if "persistent" in name else 0), (name, sspill)
