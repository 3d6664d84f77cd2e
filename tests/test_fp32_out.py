"""CPU: the fp32-output entry (dga_gemm_fp8_fp8_fp32_nt, api.gemm_fp8_fp8_fp32_nt) -- exports, its default tiling, the tilings it
refuses, and the argument checks that raise before anything is launched.  Its GPU results: tests/test_fp32_out_gpu.py."""
import ctypes

import pytest
import torch

import deepgemm_ascend_amd as dga
from deepgemm_ascend_amd import _lib

E_TILING = -6
# DGA_BUILD_* without an fp32 epilogue: the bf16 image builds and the masked grouped kernel
NO_F32_BUILDS = (4, 5, 6, 9)


def test_the_three_symbols_are_exported():
    L = _lib.lib()
    for name in ("dga_gemm_fp8_fp8_fp32_nt", "dga_tiling_fp32_out", "dga_tiling_check_fp32_out"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert dga.gemm_fp8_fp8_fp32_nt is dga.api.gemm_fp8_fp8_fp32_nt


# M across the workgroup split-K (<= 32), the one-launch split-K (17..512 rows), the one-tile and persistent builds, the quarter-tile tail
# and Stream-K ranges; K % 128 != 0 and K % 16 != 0 among them
SHAPES = [(m, n, k) for m in (1, 8, 16, 24, 32, 48, 64, 100, 128, 192, 256, 512, 1000, 1024, 2304, 3511, 4096, 8192)
          for (n, k) in ((4096, 7168), (2048, 7168), (6151, 8191), (18432, 7168), (4096, 4096), (7168, 2048), (257, 1000), (4096, 4100))]


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_default_tiling_is_the_bf16_exact_pick_and_passes_its_check(m, n, k):
    t = dga.tiling_fp32_out(m, n, k)
    tb = dga.tiling(m, n, k, policy="bf16_exact")
    assert dga.tiling_check_fp32_out(t) == 0
    if tb.build in NO_F32_BUILDS or tb.dispatchPolicyTag != 7:
        assert (t.build, t.dispatchPolicyTag) == (0, 7)
        tb.build, tb.dispatchPolicyTag = 0, 7
    assert bytes(t) == bytes(tb)


CSV_HEAD = ("m,n,k,m1,n1,k1,kernelSerial,paddingTagA,paddingTagB,paddingTagC,blockDim,splitkFactor,stages,swizzleOffset,wavesM,wavesN,"
            "dispatchPolicyTag,groups,contiguous,build\n")


@pytest.mark.parametrize("tag,build", [(7, 4), (7, 5), (7, 6)])
def test_a_cache_row_without_an_fp32_build_is_mapped(tmp_path, tag, build):
    m, n, k = 300, 520, 1024
    path = tmp_path / "rows.csv"
    path.write_text(CSV_HEAD + f"{m},{n},{k},128,256,128,0,0,0,0,6,1,3,1,0,0,{tag},1,0,{build}\n")
    try:
        dga.tiling_cache_open(str(path))
        tb = dga.tiling(m, n, k, policy="bf16_exact")
        assert (tb.m1, tb.n1, tb.build, tb.dispatchPolicyTag) == (128, 256, build, tag)   # the row itself
        t = dga.tiling_fp32_out(m, n, k)
        assert (t.m1, t.n1, t.kernelSerial, t.build, t.dispatchPolicyTag) == (128, 256, tb.kernelSerial, 0, 7)
        assert dga.tiling_check_fp32_out(t) == 0
        tb.build, tb.dispatchPolicyTag = 0, 7
        assert bytes(t) == bytes(tb)
    finally:
        dga.tiling_cache_open(None)
        dga.tiling_cache_clear()
        dga.api._PLANS.clear()


@pytest.mark.parametrize("build", [0, 8])
def test_a_ue8m0_cache_row_comes_back_on_tag_7(tmp_path, build):
    """A bf16-exact row with the power-of-two-scales flag (tag 23): the bf16-exact entry keeps the row's tile and build but not the
    flag -- only the caller's policy or process default adds it -- and the fp32 entry runs the same tiling, the one-tile build (8)
    included, since it has an fp32 epilogue."""
    m, n, k = 300, 520, 1024
    path = tmp_path / "rows.csv"
    path.write_text(CSV_HEAD + f"{m},{n},{k},128,256,128,0,0,0,0,6,1,3,1,0,0,23,1,0,{build}\n")
    try:
        dga.tiling_cache_open(str(path))
        tb = dga.tiling(m, n, k, policy="bf16_exact")
        assert (tb.m1, tb.n1, tb.build, tb.dispatchPolicyTag) == (128, 256, build, 7)
        assert dga.tiling_check(tb) == 0
        t = dga.tiling_fp32_out(m, n, k)
        assert (t.m1, t.n1, t.kernelSerial, t.build, t.dispatchPolicyTag) == (128, 256, tb.kernelSerial, build, 7)
        assert dga.tiling_check_fp32_out(t) == 0
        assert bytes(t) == bytes(tb)
    finally:
        dga.tiling_cache_open(None)
        dga.tiling_cache_clear()
        dga.api._PLANS.clear()


def _bx(build=0, tag=7, serial=0, m1=128, n1=256):
    t = dga.tiling(4096, 4096, 4096, policy="bf16_exact")
    t.m1, t.n1, t.kernelSerial, t.build, t.dispatchPolicyTag, t.splitkFactor = m1, n1, serial, build, tag, 1
    return t


@pytest.mark.parametrize("build", NO_F32_BUILDS)
def test_builds_without_an_fp32_epilogue_are_refused(build):
    t = _bx(build=build)
    assert dga.tiling_check(t) == 0   # (a tiling the bf16 entry runs)
    assert dga.tiling_check_fp32_out(t) == E_TILING


@pytest.mark.parametrize("tag", [0, 1, 2, 4, 5, 6, 7 | 16, 2 | 16])
def test_fast_and_ue8m0_tags_are_refused(tag):
    t = dga.tiling(4096, 4096, 4096)
    t.dispatchPolicyTag = tag
    assert dga.tiling_check_fp32_out(t) == E_TILING


@pytest.mark.parametrize("t", [_bx(), _bx(tag=3), _bx(build=7), _bx(build=8), _bx(serial=5), _bx(serial=7),
                               _bx(serial=6, build=10, m1=64, n1=128)])
def test_builds_with_an_fp32_path_pass(t):
    assert dga.tiling_check_fp32_out(t) == 0


def test_the_check_keeps_the_general_refusals():
    t = _bx()
    t.reserved0 = 1
    assert dga.tiling_check_fp32_out(t) == E_TILING


def _args(m=64, n=128, k=256, dev="cpu"):
    a = torch.zeros((m, k), dtype=torch.uint8, device=dev)
    b = torch.zeros((n, k), dtype=torch.uint8, device=dev)
    sfa = torch.ones((m, (k + 127) // 128), dtype=torch.float32, device=dev)
    sfb = torch.ones(((n + 127) // 128, (k + 127) // 128), dtype=torch.float32, device=dev)
    return (a, sfa), (b, sfb), torch.zeros((m, n), dtype=torch.float32, device=dev)


def test_cpu_tensors_raise():
    lhs, rhs, out = _args()
    with pytest.raises(dga.DGAError):
        dga.gemm_fp8_fp8_fp32_nt(lhs, rhs, out)


def test_bf16_out_raises():
    lhs, rhs, out = _args()
    with pytest.raises(dga.DGAError, match="float32"):
        dga.gemm_fp8_fp8_fp32_nt(lhs, rhs, out.to(torch.bfloat16))


@pytest.mark.parametrize("bad", ["shape", "dtype", "strided"])
def test_a_bad_c_raises(bad):
    lhs, rhs, out = _args()
    c = {"shape": torch.zeros((64, 127)), "dtype": torch.zeros((64, 128), dtype=torch.bfloat16),
         "strided": torch.zeros((128, 64)).t()}[bad]
    with pytest.raises(dga.DGAError):
        dga.gemm_fp8_fp8_fp32_nt(lhs, rhs, out, c=c)


def test_a_c_that_partially_overlaps_out_raises():
    lhs, rhs, _ = _args()
    buf = torch.zeros(64 * 128 + 4)
    out, c = buf[:64 * 128].view(64, 128), buf[4:].view(64, 128)
    with pytest.raises(dga.DGAError, match="overlap"):
        dga.gemm_fp8_fp8_fp32_nt(lhs, rhs, out, c=c)


@pytest.mark.parametrize("policy", ["fast", "auto", "fast_ue8m0", "bf16_exact_ue8m0"])
def test_policies_without_an_fp32_epilogue_raise(policy):
    lhs, rhs, out = _args()
    with pytest.raises(dga.DGAError, match="policy"):
        dga.gemm_fp8_fp8_fp32_nt(lhs, rhs, out, policy=policy)


def test_the_c_abi_refuses_a_partial_overlap_and_an_image_tiling_before_any_launch():
    """Host-side refusals: no device pointer is dereferenced (the pointers below are never valid device memory)."""
    L = _lib.lib()
    m, n, k = 64, 128, 256
    fake = ctypes.c_void_p(1 << 40)
    out = (1 << 40) + 4096
    t = _bx(build=4)
    assert L.dga_gemm_fp8_fp8_fp32_nt(fake, k, fake, fake, k, fake, out + 4, out, m, n, k, 0, None, None, 0, None) == -2
    assert L.dga_gemm_fp8_fp8_fp32_nt(fake, k, fake, fake, k, fake, None, out, m, n, k, 0, ctypes.byref(t), None, 0, None) == E_TILING
    assert L.dga_gemm_fp8_fp8_fp32_nt(fake, k, fake, fake, k, fake, None, out, 0, n, k, 0, None, None, 0, None) == 0
