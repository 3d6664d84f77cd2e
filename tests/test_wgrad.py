"""CPU: the weight-gradient entry (dga_wgrad_gemm_fp8_fp8_fp32_nt, api.wgrad_gemm_fp8_fp8_fp32_nt: per-1x128 scales on both operands,
sfb [N, KB]) -- exports, its default tiling and the builds it maps away, the tilings it refuses, the argument checks that raise before
anything is launched, and the register budget of its builds.  Its GPU results: tests/test_wgrad_gpu.py."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest
import torch

import deepgemm_ascend_amd as dga
from deepgemm_ascend_amd import _lib

E_TILING = -6
CSRC = Path(__file__).resolve().parent.parent / "deepgemm_ascend_amd" / "csrc"
# kernelSerial 6 (workgroup split-K) / 7 (one-launch Stream-K), DGA_BUILD_WSK_REGISTER / _BX_DECODE: no per-row-sfb form
NO_ROWS_SERIALS = (6, 7)
NO_ROWS_BUILDS = (1, 10)


def test_the_three_symbols_are_exported():
    L = _lib.lib()
    for name in ("dga_wgrad_gemm_fp8_fp8_fp32_nt", "dga_tiling_wgrad", "dga_tiling_check_wgrad"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert dga.wgrad_gemm_fp8_fp8_fp32_nt is dga.api.wgrad_gemm_fp8_fp8_fp32_nt
    assert dga.tiling_wgrad is dga.api.tiling_wgrad and dga.tiling_check_wgrad is dga.api.tiling_check_wgrad
    assert L.dga_abi_version() == 7


# the weight-gradient shapes (M, N, K = out_features, in_features, tokens), 4096^3, decode-like M (the workgroup split-K and its decode
# build under the bf16 policies), ragged M / N, K % 128 != 0, K % 16 != 0, K = 0
WGRAD = [(4096, 4096, 4096), (7168, 2048, 4096), (2048, 7168, 4096), (7168, 2112, 8192), (4096, 7168, 8192), (1536, 7168, 4096)]
SHAPES = WGRAD + [(m, n, k) for m in (1, 16, 32, 48, 64, 100, 256, 1000, 3511)
                  for (n, k) in ((4096, 7168), (6151, 8191), (18432, 7168), (257, 1000), (4096, 4100), (7168, 2048), (2112, 0))]


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_default_tiling_is_the_fp32_pick_mapped_and_passes_its_check(m, n, k):
    t = dga.tiling_wgrad(m, n, k)
    tf = dga.tiling_fp32_out(m, n, k)
    assert dga.tiling_check_wgrad(t) == 0
    assert t.kernelSerial not in NO_ROWS_SERIALS and t.build not in NO_ROWS_BUILDS
    assert (t.m1, t.n1, t.dispatchPolicyTag) == (tf.m1, tf.n1, tf.dispatchPolicyTag)   # the same tile and arithmetic
    if tf.kernelSerial in NO_ROWS_SERIALS:
        assert t.kernelSerial == (4 if tf.splitkFactor > 1 else 0) and t.splitkFactor == tf.splitkFactor
        assert t.build == 0
    else:
        assert bytes(t) == bytes(tf)


def test_the_default_tiling_maps_the_decode_and_workgroup_builds():
    """Shapes whose fp32 pick is a build without a per-row-sfb form: they exist in the list above (otherwise the mapping is untested)."""
    picks = {(dga.tiling_fp32_out(m, n, k).kernelSerial, dga.tiling_fp32_out(m, n, k).build) for m, n, k in SHAPES}
    assert (6, 10) in picks and (6, 0) in picks


def test_strict_process_default_gives_the_strict_tag():
    r = subprocess.run(["python3", "-c", "import deepgemm_ascend_amd as d; t = d.tiling_wgrad(48, 4096, 7168); "
                        "print(t.dispatchPolicyTag, d.tiling_check_wgrad(t))"],
                       capture_output=True, text=True, timeout=120, cwd=str(CSRC.parent.parent),
                       env={**__import__("os").environ, "DGA_DEFAULT_POLICY": "strict"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["3", "0"]


CSV_HEAD = ("m,n,k,m1,n1,k1,kernelSerial,paddingTagA,paddingTagB,paddingTagC,blockDim,splitkFactor,stages,swizzleOffset,wavesM,wavesN,"
            "dispatchPolicyTag,groups,contiguous,build\n")


# cache rows naming every build or tag without a per-row-sfb path: the workgroup split-K (LDS-DMA build, register build, decode build
# with its split factor), the one-launch Stream-K, the bf16 image builds, the grouped build, the fast tags, the UE8M0 flag
@pytest.mark.parametrize("m1,n1,serial,splitk,tag,build,want_serial", [
    (32, 128, 6, 1, 7, 0, 0), (32, 128, 6, 1, 7, 1, 0), (64, 128, 6, 6, 7, 10, 4), (128, 256, 7, 1, 7, 0, 0),
    (128, 256, 0, 1, 7, 4, 0), (128, 256, 0, 1, 7, 5, 0), (128, 256, 0, 1, 7, 6, 0), (128, 256, 0, 1, 7, 9, 0),
    (128, 256, 0, 1, 0, 0, 0), (128, 256, 0, 1, 5, 0, 0), (128, 256, 0, 1, 7 | 16, 0, 0), (128, 256, 0, 1, 2 | 16, 0, 0)])
def test_a_cache_row_without_a_rows_build_is_mapped(tmp_path, m1, n1, serial, splitk, tag, build, want_serial):
    m, n, k = 300, 520, 4096
    path = tmp_path / "rows.csv"
    path.write_text(CSV_HEAD + f"{m},{n},{k},{m1},{n1},128,{serial},0,0,0,6,{splitk},3,1,0,0,{tag},1,0,{build}\n")
    try:
        dga.tiling_cache_open(str(path))
        t = dga.tiling_wgrad(m, n, k)
        assert dga.tiling_check_wgrad(t) == 0
        if (tag & 7) != 7:   # (a fast-path row is not the bf16-exact selector's: its own pick, on a rows build)
            assert (t.build, t.dispatchPolicyTag) == (0, 7) and t.kernelSerial not in NO_ROWS_SERIALS
            return
        assert (t.m1, t.n1, t.kernelSerial, t.splitkFactor, t.build, t.dispatchPolicyTag) == (m1, n1, want_serial, splitk, 0, 7)
    finally:
        dga.tiling_cache_open(None)
        dga.tiling_cache_clear()
        dga.api._PLANS.clear()


def _bx(build=0, tag=7, serial=0, m1=128, n1=256, splitk=1):
    t = dga.tiling(4096, 4096, 4096, policy="bf16_exact")
    t.m1, t.n1, t.kernelSerial, t.build, t.dispatchPolicyTag, t.splitkFactor = m1, n1, serial, build, tag, splitk
    return t


@pytest.mark.parametrize("t", [_bx(serial=6, m1=32, n1=128), _bx(serial=6, build=1, m1=32, n1=128), _bx(serial=6, build=10, m1=64, n1=128, splitk=6),
                               _bx(serial=7), _bx(build=4), _bx(build=5), _bx(build=6), _bx(build=9), _bx(tag=0), _bx(tag=5), _bx(tag=7 | 16)],
                         ids=["wsk", "wsk_register", "decode", "streamk", "aimage", "image8", "image4", "grouped", "fast0", "fast5", "ue8m0"])
def test_builds_without_a_rows_path_are_refused(t):
    assert dga.tiling_check_wgrad(t) == E_TILING


@pytest.mark.parametrize("t", [_bx(), _bx(tag=3), _bx(tag=3, serial=7), _bx(build=7), _bx(build=8), _bx(serial=5), _bx(serial=4, splitk=4),
                               _bx(m1=64, n1=128), _bx(m1=32, n1=128), _bx(m1=64, n1=256), _bx(m1=128, n1=128)])
def test_builds_with_a_rows_path_pass(t):
    assert dga.tiling_check_wgrad(t) == 0


def _args(m=300, n=520, k=256, dev="cpu", sfb_rows=None):
    a = torch.zeros((m, k), dtype=torch.uint8, device=dev)
    b = torch.zeros((n, k), dtype=torch.uint8, device=dev)
    sfa = torch.ones((m, (k + 127) // 128), dtype=torch.float32, device=dev)
    sfb = torch.ones((n if sfb_rows is None else sfb_rows, (k + 127) // 128), dtype=torch.float32, device=dev)
    return (a, sfa), (b, sfb), torch.zeros((m, n), dtype=torch.float32, device=dev)


def test_a_block_shaped_sfb_raises():
    lhs, rhs, out = _args(sfb_rows=(520 + 127) // 128)   # [ceil(N/128), KB]: the 1D2D layout
    with pytest.raises(dga.DGAError, match=r"sfb must be \[520,2\]"):
        dga.wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, out)


@pytest.mark.parametrize("which", ["sfa", "sfb"])
def test_non_float32_scales_raise(which):
    (a, sfa), (b, sfb), out = _args()
    if which == "sfa":
        sfa = sfa.to(torch.bfloat16)
    else:
        sfb = sfb.double()
    with pytest.raises(dga.DGAError, match="float32"):
        dga.wgrad_gemm_fp8_fp8_fp32_nt((a, sfa), (b, sfb), out)


def test_bf16_out_raises():
    lhs, rhs, out = _args()
    with pytest.raises(dga.DGAError, match="float32"):
        dga.wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, out.to(torch.bfloat16))


def test_cpu_tensors_raise():
    lhs, rhs, out = _args()
    with pytest.raises(dga.DGAError):
        dga.wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, out)


def test_a_c_that_partially_overlaps_out_raises():
    lhs, rhs, _ = _args()
    buf = torch.zeros(300 * 520 + 4)
    out, c = buf[:300 * 520].view(300, 520), buf[4:].view(300, 520)
    with pytest.raises(dga.DGAError, match="overlap"):
        dga.wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, out, c=c)


@pytest.mark.parametrize("policy", ["fast", "auto", "fast_ue8m0", "bf16_exact_ue8m0"])
def test_policies_without_a_rows_path_raise(policy):
    lhs, rhs, out = _args()
    with pytest.raises(dga.DGAError, match="policy"):
        dga.wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, out, policy=policy)


def test_the_c_abi_refuses_unsupported_tilings_and_a_partial_overlap_before_any_launch():
    """Host-side refusals: no device pointer is dereferenced (the pointers below are never valid device memory)."""
    L = _lib.lib()
    m, n, k = 64, 128, 256
    fake = ctypes.c_void_p(1 << 40)
    out = (1 << 40) + 4096
    for t in (_bx(serial=7), _bx(serial=6, build=10, m1=64, n1=128, splitk=6), _bx(serial=6, m1=32, n1=128), _bx(build=4), _bx(tag=0)):
        assert L.dga_wgrad_gemm_fp8_fp8_fp32_nt(fake, k, fake, fake, k, fake, None, out, m, n, k, 0, ctypes.byref(t), None, 0, None) == E_TILING
    assert L.dga_wgrad_gemm_fp8_fp8_fp32_nt(fake, k, fake, fake, k, fake, out + 4, out, m, n, k, 0, None, None, 0, None) == -2
    assert L.dga_wgrad_gemm_fp8_fp8_fp32_nt(fake, k, fake, fake, k, fake, None, out, 0, n, k, 0, None, None, 0, None) == 0
    # (the fp32 entry takes a Stream-K tiling: the refusal above is the weight-gradient entry's own)
    assert L.dga_tiling_check_fp32_out(ctypes.byref(_bx(serial=7))) == 0


def _resource_usage(unit, extra=()):
    """(kernel, VGPRs, VGPR spills, SGPR spills, scratch bytes) of every kernel of a unit, compiled with the Makefile's flags."""
    obj = f"../../build/csrc/{Path(unit).stem}.o"
    r = subprocess.run(["make", "-n", "-B", "-C", str(CSRC), obj], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-1000:]
    line = [l for l in r.stdout.splitlines() if "hipcc" in l and f" {unit} " in l + " "][-1].split()
    flags = [w for i, w in enumerate(line[1:], 1) if w not in ("-c", unit) and line[i - 1] != "-o" and w != "-o"]
    cmd = ["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-S", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage", unit]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(CSRC))
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


def test_the_rows_tile_builds_do_not_spill():
    """The ten one-tile builds with per-row sfb (5 tiles x k-tail) keep every register array in registers (a k-block body that is not
    fully unrolled sends them to scratch) and fit 256 VGPRs."""
    ks = [k for k in _resource_usage("dga_launch_menu_o.hip") if "gemm_fp8_blockscaled_nt_kernel" in k[0]]
    assert len(ks) == 10
    for name, vgprs, vspill, sspill, scratch in ks:
        assert vgprs <= 256 and vspill == 0 and sspill == 0 and scratch == 0, name
