"""The paired body of the bf16-exact policy's dense persistent kernel (csrc/gemm_fp8_bf16x_pair_kernel.hpp: one workgroup computes two
stacked 128 x 256 raster tiles at once, 64 x 128 wave tiles) against the one-tile build (tiling.build = 8) on the same inputs: the same
arithmetic in the same order per output element, so the bar is BIT IDENTITY; against the oracle it is the policy's bar
(tests/test_bf16_exact_gpu.py).  The body is forced through the library's diagnostic switch (dga_diag_bf16x_pair_force), the launcher's
own rule is read through dga_diag_bf16x_pair_rule and what a launch took through dga_diag_bf16x_pair_last."""
import numpy as np
import pytest
import torch

from test_bf16_exact_gpu import _assert_bar, _bits, _dev, EPS

pytestmark = pytest.mark.gpu


def _tiling(dga, m, n, k, build):
    t = dga.tiling(m, n, k, policy="bf16_exact")
    t.m1, t.n1, t.splitkFactor, t.kernelSerial, t.dispatchPolicyTag = 128, 256, 1, 0, 7
    t.stages, t.build, t.wavesM, t.wavesN, t.swizzleOffset = 3, build, 2, 4, 4
    return t


def _run(dga, a, sfa, b, sfb, t):
    out = torch.full((a.shape[0], b.shape[0]), float("nan"), dtype=torch.bfloat16, device="cuda")
    dga.gemm_fp8_fp8_bf16_nt((_dev(a), _dev(sfa)), (_dev(b), _dev(sfb)), out, policy="bf16_exact", sync=True, tiling_=t)
    return _bits(out)


@pytest.fixture
def pair(dga):
    """force(grid): the next launches of build 7 take the paired body, on `grid` workgroups (0: one per CU); the rule is back afterwards."""
    L = dga.lib()
    yield lambda grid=0: L.dga_diag_bf16x_pair_force(1, grid)
    L.dga_diag_bf16x_pair_force(-1, 0)


@pytest.mark.parametrize("m,n,k,grid,bar", [
    (256, 256, 256, 0, True),     # one pair, two k blocks
    (512, 512, 384, 1, True),     # four pairs on one workgroup: the ring across three boundaries, an odd block count
    (257, 256, 256, 0, False),    # the lower tile of the second pair holds one row
    (129, 520, 256, 0, False),    # the lower tile nearly empty, ragged N (three pair columns, the last 8 columns wide)
    (384, 256, 512, 0, False),    # an odd number of m-tiles: the last pair has no lower tile
    (256, 256, 256, 5, False),    # more workgroups than pairs: the ones without work exit
])
def test_paired_body_is_bit_identical_to_the_one_tile_build(dga, oracle, pair, m, n, k, grid, bar):
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=m * 3 + n + 7 * k)
    ref = _run(dga, a, sfa, b, sfb, _tiling(dga, m, n, k, 8))
    pair(grid)
    got = _run(dga, a, sfa, b, sfb, _tiling(dga, m, n, k, 7))
    assert dga.lib().dga_diag_bf16x_pair_last() == 1, "the launch did not take the paired body"
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {got.size} outputs differ"
    if bar:
        want = oracle.gemm_fp8_fp8_bf16_nt(a, sfa, b, sfb, threads=8)
        _assert_bar(oracle, got, want, a, sfa, b, sfb, eps=EPS)


def test_the_launcher_rule_pairs_only_where_no_round_is_added(dga):
    L = dga.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip("the shapes below are stated for 256 CUs")
    assert L.dga_diag_bf16x_pair_rule(4096, 4096) == 1      # 256 pairs, one per CU
    assert L.dga_diag_bf16x_pair_rule(8192, 8192) == 1      # 1024 pairs, four rounds against eight
    assert L.dga_diag_bf16x_pair_rule(4096, 2048) == 0      # 4096 x 2048 x 7168: 128 pairs would idle half the CUs
    assert L.dga_diag_bf16x_pair_rule(256, 256) == 0        # one round either way


def test_a_launch_under_the_rule_reports_its_body(dga, oracle):
    """2304 x 4096: 288 tiles are two rounds, 144 pairs one -- the rule pairs; 256 x 256 is one round of tiles: it does not."""
    L = dga.lib()
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the shapes below are stated for 256 CUs")
    for (m, n, k), want in (((2304, 4096, 256), 1), ((256, 256, 256), 0)):
        a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=5)
        got = _run(dga, a, sfa, b, sfb, _tiling(dga, m, n, k, 7))
        assert L.dga_diag_bf16x_pair_last() == want
        assert np.array_equal(got, _run(dga, a, sfa, b, sfb, _tiling(dga, m, n, k, 8)))
