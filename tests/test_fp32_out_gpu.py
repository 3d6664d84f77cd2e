"""GPU: gemm_fp8_fp8_fp32_nt -- fp32 rows with an optional addend C (dga_gemm_fp8_fp8_fp32_nt).  The bf16-exact builds finish with the
same fp32 accumulator the bf16 entry rounds, so round-to-nearest-even of the fp32 output must equal the bf16 output BIT FOR BIT on the
same tiling -- on every build of the kernels table, the one-launch decode split-K, Stream-K and workgroup split-K included; the
strict kernel's fp32 output is the oracle's fp32 result bit for bit (the reference's golden is that fp32 matmul:
deep_gemm_ascend/scripts/gen_golden.py:14-15)."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _f32(dga, a, sfa, b, sfb, t=None, c=None, out=None, **kw):
    m, n = a.shape[0], b.shape[0]
    if out is None:
        out = torch.full((m, n), float("nan"), dtype=torch.float32, device="cuda")
    lhs = (a if isinstance(a, torch.Tensor) else _dev(a), _dev(sfa))
    rhs = (b if isinstance(b, torch.Tensor) else _dev(b), _dev(sfb))
    dga.gemm_fp8_fp8_fp32_nt(lhs, rhs, out, c=c, tiling_=t, sync=True, **kw)
    return out.cpu().numpy()


def _bf16(dga, a, sfa, b, sfb, t=None):
    out = torch.full((a.shape[0], b.shape[0]), float("nan"), dtype=torch.bfloat16, device="cuda")
    lhs = (a if isinstance(a, torch.Tensor) else _dev(a), _dev(sfa))
    rhs = (b if isinstance(b, torch.Tensor) else _dev(b), _dev(sfb))
    dga.gemm_fp8_fp8_bf16_nt(lhs, rhs, out, policy="bf16_exact", tiling_=t, sync=True)
    return out.view(torch.int16).cpu().numpy().view(np.uint16)


def _assert_rounds_to(oracle, f32, bf16_bits):
    nan = np.isnan(f32)
    bnan = (bf16_bits & 0x7FFF) > 0x7F80
    assert np.array_equal(nan, bnan), "NaN positions differ"
    got = oracle.f32_to_bf16_bits(np.where(nan, 0, f32).astype(np.float32))
    bad = (got != bf16_bits) & ~nan
    assert not bad.any(), f"{int(bad.sum())} of {f32.size} outputs round to other bf16 bits"


def _tile(dga, m, n, k, m1, n1, serial=0, build=8, sk=1):
    t = dga.tiling(m, n, k, policy="bf16_exact")
    t.m1, t.n1, t.kernelSerial, t.build, t.splitkFactor, t.dispatchPolicyTag = m1, n1, serial, build, sk, 7
    t.stages, t.wavesM, t.wavesN = 3, 0, 0
    return t


# (name, m, n, k, tiling maker): each a build of the kernels table, on ragged M / N and K % 128 != 0 / K % 16 != 0
CASES = [
    ("one_tile_128x256", 300, 257, 1000, lambda d, m, n, k: _tile(d, m, n, k, 128, 256)),
    ("one_tile_128x128", 129, 127, 640, lambda d, m, n, k: _tile(d, m, n, k, 128, 128)),
    ("one_tile_64x256", 100, 520, 1003, lambda d, m, n, k: _tile(d, m, n, k, 64, 256)),
    ("one_tile_64x128", 65, 300, 256, lambda d, m, n, k: _tile(d, m, n, k, 64, 128)),
    ("one_tile_32x128", 33, 1000, 2048 + 8, lambda d, m, n, k: _tile(d, m, n, k, 32, 128)),
    ("persistent", 2400, 4200, 400, lambda d, m, n, k: _tile(d, m, n, k, 128, 256, build=7)),
    ("persistent_ragged", 1000, 9001, 384 + 16, lambda d, m, n, k: _tile(d, m, n, k, 128, 256, build=7)),
    ("tail_pair", 2304, 4096, 384, lambda d, m, n, k: _tile(d, m, n, k, 128, 256, serial=5, build=0)),
    ("split_k", 100, 300, 128 * 9 + 5, lambda d, m, n, k: _tile(d, m, n, k, 64, 128, serial=4, build=0, sk=4)),
    ("split_k_ragged", 64, 257, 128 * 16, lambda d, m, n, k: _tile(d, m, n, k, 32, 128, serial=4, build=0, sk=8)),
    ("default", 200, 300, 1000 + 3, None),
]


@pytest.mark.parametrize("name,m,n,k,mk", CASES, ids=[c[0] for c in CASES])
def test_fp32_rounds_to_the_bf16_output(dga, oracle, name, m, n, k, mk):
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=m + 3 * n + k)
    t = mk(dga, m, n, k) if mk else None
    _assert_rounds_to(oracle, _f32(dga, a, sfa, b, sfb, t), _bf16(dga, a, sfa, b, sfb, t))


# the one-launch builds the default tiling names for decode rows and rasters with a partial last round: decode split-K (kernelSerial 6,
# DGA_BUILD_BX_DECODE), Stream-K (kernelSerial 7), the LDS-DMA workgroup split-K (kernelSerial 6, M <= 32; both of its forms: pass by
# pass and the continuous ring).  The forced tiling is the same for both entries; K % 128 != 0 and ragged N too.
ONE_LAUNCH = [
    ("dsk", 128, 4096, 7168, None),
    ("dsk_ragged", 100, 3000 + 7, 4096 + 32, lambda d, m, n, k: _tile(d, m, n, k, 64, 128, serial=6, build=10, sk=4)),
    ("streamk", 3511, 6151, 8191, None),
    ("streamk_forced", 2000, 9000, 6144 + 64, lambda d, m, n, k: _tile(d, m, n, k, 128, 256, serial=7, build=0)),
    ("wsk_pass", 8, 4096, 7168, None),
    ("wsk_ring", 8, 18432, 7168, None),
    ("wsk_32_rows", 30, 2048 + 5, 3072 + 16, lambda d, m, n, k: _tile(d, m, n, k, 32, 128, serial=6, build=0)),
]


@pytest.mark.parametrize("name,m,n,k,mk", ONE_LAUNCH, ids=[c[0] for c in ONE_LAUNCH])
def test_one_launch_builds_round_to_the_bf16_output(dga, oracle, name, m, n, k, mk):
    t = mk(dga, m, n, k) if mk else dga.tiling_fp32_out(m, n, k)
    assert t.kernelSerial in (6, 7)
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=m + n + k)
    got = _f32(dga, a, sfa, b, sfb, t)
    _assert_rounds_to(oracle, got, _bf16(dga, a, sfa, b, sfb, t))
    c = np.random.default_rng(7).standard_normal((m, n)).astype(np.float32)
    _assert_same_bits(_f32(dga, a, sfa, b, sfb, t, c=_dev(c)), (got + c).astype(np.float32), name + " + c")
    _assert_same_bits(_f32(dga, a, sfa, b, sfb, t), got, name + " again")   # the flags and epochs: two calls, the same bits


def test_row_strided_views(dga, oracle):
    m, n, k = 200, 300, 1000
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=9)
    pa = torch.zeros((m, 1024), dtype=torch.uint8, device="cuda")
    pb = torch.zeros((n, 1152), dtype=torch.uint8, device="cuda")
    pa[:, :k] = _dev(a.view(np.uint8) if a.dtype != np.uint8 else a)
    pb[:, :k] = _dev(b.view(np.uint8) if b.dtype != np.uint8 else b)
    va, vb = pa[:, :k], pb[:, :k]
    for zp in (None, (True, True)):
        f32 = _f32(dga, va, sfa, vb, sfb, zero_padded=zp)
        _assert_rounds_to(oracle, f32, _bf16(dga, a, sfa, b, sfb))


def _strict_cases(oracle):
    g = np.load(GOLDEN / "c1_unit_128.npz")
    yield "configs0_golden", g["a"], g["sfa"], g["b"], g["sfb"]
    a, sfa, b, sfb = oracle.make_inputs(100, 300, 1000, seed=3)
    sfa = sfa.copy()
    sfa[7, 2] = np.float32(1e-40)   # a subnormal scale
    sfb = sfb.copy()
    sfb[1, 0] = np.float32("nan")   # NaN reaches a block of columns
    yield "nan_subnormal", a, sfa, b, sfb


def _assert_same_bits(got, want, what):
    """Bit-exact: NaN positions equal, every other element's bits equal (so +0 / -0 differ)."""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    g, w = np.where(gn, 0, got).astype(np.float32), np.where(wn, 0, want).astype(np.float32)
    bad = g.view(np.uint32) != w.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} outputs differ in their bits"


def test_strict_is_the_oracle_in_fp32(dga, oracle):
    for name, a, sfa, b, sfb in _strict_cases(oracle):
        want = oracle.gemm_fp8_fp8_bf16_nt(a, sfa, b, sfb, threads=8, want_f32=True)[1]
        _assert_same_bits(_f32(dga, a, sfa, b, sfb, strict=True), want, name)
        c = np.random.default_rng(1).standard_normal(want.shape).astype(np.float32)
        c[1, :] = np.float32(-0.0)     # a zero product plus -0 must come out as the IEEE sum's sign
        got_c = _f32(dga, a, sfa, b, sfb, strict=True, c=_dev(c))
        _assert_same_bits(got_c, (want + c).astype(np.float32), name + " + c")


@pytest.mark.parametrize("m,n,k", [(300, 520, 1024), (64, 1024, 7168), (128, 2048, 4096), (8, 2048, 7168)])
def test_bf16_exact_within_the_bar_of_the_exact_result(dga, oracle, m, n, k):
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=m + n)
    c = np.random.default_rng(2).standard_normal((m, n)).astype(np.float32)
    ref = oracle.gemm_fp8_fp8_f64_nt(a, sfa, b, sfb).astype(np.float64) + c.astype(np.float64)
    S = np.asarray(oracle.abs_term_sum(a, sfa, b, sfb), np.float64)
    got = _f32(dga, a, sfa, b, sfb, c=_dev(c)).astype(np.float64)
    excess = np.abs(got - ref) - (2.0 ** -22 * S + 2.0 ** -24 * np.abs(ref))
    assert (excess <= 0).all(), f"{int((excess > 0).sum())} outputs beyond the bar"


@pytest.mark.parametrize("m,n,k", [(300, 257, 1000), (2400, 4200, 400), (128, 4096, 7168), (100, 300, 128 * 9 + 5)])
def test_c_semantics(dga, oracle, m, n, k):
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=11)
    plain = _f32(dga, a, sfa, b, sfb)                      # out prefilled with NaN: every element written
    assert not np.isnan(plain).any()
    c = np.random.default_rng(3).standard_normal((m, n)).astype(np.float32)
    c[0, 0] = np.float32("nan")
    sep = _f32(dga, a, sfa, b, sfb, c=_dev(c))
    assert np.array_equal(sep.view(np.uint32)[1:], (plain + c).astype(np.float32).view(np.uint32)[1:])
    assert np.isnan(sep[0, 0])                              # NaN in c propagates
    buf = _dev(c)
    inplace = _f32(dga, a, sfa, b, sfb, c=buf, out=buf)    # c is out
    assert np.array_equal(np.nan_to_num(inplace).view(np.uint32), np.nan_to_num(sep).view(np.uint32))
    again = _f32(dga, a, sfa, b, sfb, c=_dev(c))
    assert np.array_equal(np.nan_to_num(again).view(np.uint32), np.nan_to_num(sep).view(np.uint32))


def test_k_zero_gives_c(dga):
    m, n = 40, 70
    a = torch.zeros((m, 0), dtype=torch.uint8, device="cuda")
    b = torch.zeros((n, 0), dtype=torch.uint8, device="cuda")
    sfa = torch.zeros((m, 0), dtype=torch.float32, device="cuda")
    sfb = torch.zeros(((n + 127) // 128, 0), dtype=torch.float32, device="cuda")
    c = torch.randn((m, n), device="cuda")
    c[0, 0] = -0.0
    out = torch.full((m, n), float("nan"), device="cuda")
    dga.gemm_fp8_fp8_fp32_nt((a, sfa), (b, sfb), out, c=c, sync=True)
    assert torch.equal(out.view(torch.int32), c.view(torch.int32))
    dga.gemm_fp8_fp8_fp32_nt((a, sfa), (b, sfb), out, sync=True)
    assert torch.equal(out, torch.zeros_like(out))


def test_refusals_never_launch(dga, oracle):
    m, n, k = 128, 256, 512
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=1)
    out = torch.full((m, n), 7.0, device="cuda")
    t = _tile(dga, m, n, k, 128, 256, build=4)    # an image build
    with pytest.raises(dga.DGAError):
        dga.gemm_fp8_fp8_fp32_nt((_dev(a), _dev(sfa)), (_dev(b), _dev(sfb)), out, tiling_=t, sync=True)
    with pytest.raises(dga.DGAError):
        dga.gemm_fp8_fp8_fp32_nt((_dev(a), _dev(sfa)), (_dev(b), _dev(sfb)), out, policy="fast", sync=True)
    tf = dga.tiling(m, n, k)
    tf.dispatchPolicyTag = 2
    with pytest.raises(dga.DGAError):
        dga.gemm_fp8_fp8_fp32_nt((_dev(a), _dev(sfa)), (_dev(b), _dev(sfb)), out, tiling_=tf, sync=True)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_graph_capture_of_an_accumulating_call(dga, oracle):
    m, n, k = 100, 300, 1000
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=4)
    da, dsa, db, dsb = _dev(a), _dev(sfa), _dev(b), _dev(sfb)
    want1 = oracle.gemm_fp8_fp8_bf16_nt(a, sfa, b, sfb, threads=8, want_f32=True)[1]
    c0 = np.random.default_rng(5).standard_normal((m, n)).astype(np.float32)
    buf = _dev(c0)
    dga.gemm_fp8_fp8_fp32_nt((da, dsa), (db, dsb), torch.empty_like(buf), strict=True, sync=True)   # plan + workspace outside the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dga.gemm_fp8_fp8_fp32_nt((da, dsa), (db, dsb), buf, c=buf, strict=True)
    torch.cuda.synchronize()
    buf.copy_(_dev(c0))
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    want = c0
    for _ in range(3):
        want = (want1 + want).astype(np.float32)
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_deep_gemm_cpp_matches_the_python_api(dga, oracle):
    from deepgemm_ascend_amd import deep_gemm_cpp
    m, n, k = 300, 257, 1000
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=8)
    c = _dev(np.random.default_rng(6).standard_normal((m, n)).astype(np.float32))
    want = _f32(dga, a, sfa, b, sfb, c=c)
    out = torch.full((m, n), float("nan"), device="cuda")
    deep_gemm_cpp.gemm_fp8_fp8_fp32_nt(_dev(a), _dev(sfa), _dev(b), _dev(sfb), out, c)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    out2 = torch.full((m, n), float("nan"), device="cuda")
    deep_gemm_cpp.gemm_fp8_fp8_fp32_nt(_dev(a), _dev(sfa), _dev(b), _dev(sfb), out2)
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy().view(np.uint32), _f32(dga, a, sfa, b, sfb).view(np.uint32))
