"""CPU: the register budget of the paired body of the bf16-exact dense persistent kernel (csrc/gemm_fp8_bf16x_pair_kernel.hpp, unit
dga_launch_menu_q.hip).  128 accumulators per lane at two waves per SIMD leave 128 registers for everything else; the body exists only
as long as it fits: at most 256 vector registers, none of them AGPRs (the promotion reads the accumulators with vector instructions), no
spill, no scratch -- under the flags the Makefile ships the unit with."""
import re
import subprocess

from test_build import CSRC, _ship_flags


def test_the_paired_body_fits_two_waves_per_simd():
    unit = "dga_launch_menu_q.hip"
    flags = _ship_flags(unit)
    assert "--offload-arch=gfx950" in flags and "-O3" in flags
    cmd = ["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-S", "-o", "/dev/null",
           "-Rpass-analysis=kernel-resource-usage", str(CSRC / unit)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(CSRC))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    mine = [b for b in blocks if "gemm_fp8_bf16x_pair_kernel" in b.split()[0]]
    assert len(mine) == 1, [b.split()[0] for b in blocks]
    usage = {k: int(v) for k, v in re.findall(r"(VGPRs|AGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", mine[0])}
    assert usage["VGPRs"] <= 256 and usage["AGPRs"] == 0, usage
    assert usage["VGPRs Spill"] == 0 and usage["SGPRs Spill"] == 0 and usage["ScratchSize [bytes/lane]"] == 0, usage
    assert usage["Occupancy [waves/SIMD]"] == 2, usage
