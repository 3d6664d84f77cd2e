"""GPU: wgrad_gemm_fp8_fp8_fp32_nt -- per-1x128 scales on both operands (sfb [N, KB], dga_wgrad_gemm_fp8_fp8_fp32_nt).  The strict kernel
is the oracle's definition with each column's own sfb, bit for bit (the oracle called one column at a time); every bf16-exact build
with a per-row-sfb form equals gemm_fp8_fp8_fp32_nt on the same tiling bit for bit when the rows of each 128-row block of B share one
scale, and stays within that entry's bar of the exact result when they do not."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _wgrad(dga, a, sfa, b, sfb, t=None, c=None, out=None, **kw):
    m, n = a.shape[0], b.shape[0]
    if out is None:
        out = torch.full((m, n), float("nan"), dtype=torch.float32, device="cuda")
    lhs = (a if isinstance(a, torch.Tensor) else _dev(a), _dev(sfa))
    rhs = (b if isinstance(b, torch.Tensor) else _dev(b), _dev(sfb))
    dga.wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, out, c=c, tiling_=t, sync=True, **kw)
    return out.cpu().numpy()


def _f32(dga, a, sfa, b, sfb, t=None):
    out = torch.full((a.shape[0], b.shape[0]), float("nan"), dtype=torch.float32, device="cuda")
    dga.gemm_fp8_fp8_fp32_nt((_dev(a), _dev(sfa)), (_dev(b), _dev(sfb)), out, tiling_=t, sync=True)
    return out.cpu().numpy()


def _assert_same_bits(got, want, what):
    """Bit-exact: NaN positions equal, every other element's bits equal (so +0 / -0 differ)."""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    g, w = np.where(gn, 0, got).astype(np.float32), np.where(wn, 0, want).astype(np.float32)
    bad = g.view(np.uint32) != w.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} outputs differ in their bits"


def _rows(sfb2d, n):
    """The 1x128 layout of a 128x128 sfb: every row of a block on the block's scale."""
    return np.ascontiguousarray(np.repeat(sfb2d, 128, axis=0)[:n])


def _per_row(oracle, sfb2d, n, seed):
    """Scales that genuinely differ per row: the block's scale times a power of two (2^-3 .. 2^3) times an arbitrary factor in [0.5, 2)."""
    rng = np.random.default_rng(seed)
    f = np.exp2(rng.integers(-3, 4, size=(n, 1))) * rng.uniform(0.5, 2.0, size=(n, 1))
    return (_rows(sfb2d, n) * f).astype(np.float32)


def _oracle_cols(oracle, a, sfa, b, sfb):
    """The oracle's fp32 result with per-row sfb: its definition applied to one column (one row of B and its scales) at a time."""
    return np.concatenate([oracle.gemm_fp8_fp8_bf16_nt(a, sfa, b[j:j + 1], sfb[j:j + 1], threads=8, want_f32=True)[1]
                           for j in range(b.shape[0])], axis=1)


def _exact(oracle, a, sfa, b, sfb):
    """(ref, S): the float64 product of the dequantised operands and the sum of its terms' magnitudes, per-row sfb -- the definition
    of oracle.gemm_fp8_fp8_f64_nt / abs_term_sum restated with sfb[n]."""
    tab = oracle.e4m3fn_table().astype(np.float64)
    k = a.shape[1]
    da = tab[np.asarray(a, np.uint8)] * np.repeat(sfa.astype(np.float64), 128, axis=1)[:, :k]
    db = tab[np.asarray(b, np.uint8)] * np.repeat(sfb.astype(np.float64), 128, axis=1)[:, :k]
    return da @ db.T, np.abs(da) @ np.abs(db).T


def _tile(dga, m, n, k, m1, n1, serial=0, build=8, sk=1):
    t = dga.tiling(m, n, k, policy="bf16_exact")
    t.m1, t.n1, t.kernelSerial, t.build, t.splitkFactor, t.dispatchPolicyTag = m1, n1, serial, build, sk, 7
    t.stages, t.wavesM, t.wavesN = 3, 0, 0
    return t


# (name, m, n, k, tiling maker): each build with a per-row-sfb form, on ragged M / N and K % 128 != 0 / K % 16 != 0
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
def test_block_uniform_row_scales_give_the_fp32_entry_bits(dga, oracle, name, m, n, k, mk):
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=m + 3 * n + k)
    t = mk(dga, m, n, k) if mk else None
    _assert_same_bits(_wgrad(dga, a, sfa, b, _rows(sfb, n), t), _f32(dga, a, sfa, b, sfb, t), name)


@pytest.mark.parametrize("name,m,n,k,mk", CASES, ids=[c[0] for c in CASES])
def test_bf16_exact_within_the_bar_with_per_row_scales(dga, oracle, name, m, n, k, mk):
    """The bar of test_fp32_out_gpu.py::test_bf16_exact_within_the_bar_of_the_exact_result, with scales that differ from row to row."""
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=m + 5 * n + k)
    sfb1 = _per_row(oracle, sfb, n, seed=n)
    t = mk(dga, m, n, k) if mk else None
    got = _wgrad(dga, a, sfa, b, sfb1, t).astype(np.float64)
    ref, S = _exact(oracle, a, sfa, b, sfb1)
    excess = np.abs(got - ref) - (2.0 ** -22 * S + 2.0 ** -24 * np.abs(ref))
    assert (excess <= 0).all(), f"{name}: {int((excess > 0).sum())} outputs beyond the bar"


@pytest.mark.parametrize("m,n,k", [(100, 300, 1000), (33, 130, 128 * 3 + 8), (70, 257, 1003), (200, 140, 256)])
def test_strict_is_the_per_column_oracle(dga, oracle, m, n, k):
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=k)
    sfb1 = _per_row(oracle, sfb, n, seed=m)
    want = _oracle_cols(oracle, a, sfa, b, sfb1)
    _assert_same_bits(_wgrad(dga, a, sfa, b, sfb1, strict=True), want, "strict")
    c = np.random.default_rng(1).standard_normal(want.shape).astype(np.float32)
    c[1, :] = np.float32(-0.0)     # a zero product plus -0 must come out as the IEEE sum's sign
    _assert_same_bits(_wgrad(dga, a, sfa, b, sfb1, strict=True, c=_dev(c)), (want + c).astype(np.float32), "strict + c")


def test_strict_takes_the_128_row_tile(dga, oracle):
    """The strict kernel's 128-row build runs where the raster has two 128 x 128 tiles per CU: its per-row sfb slots are all 256 threads'."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m, n, k = 128 * 8, 128 * (2 * cus // 8 + 1), 256
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=21)
    sfb1 = _per_row(oracle, sfb, n, seed=22)
    got = _wgrad(dga, a, sfa, b, sfb1, strict=True)
    cols = [0, 1, 127, 128, 129, 255, n // 2, n - 1]
    want = np.concatenate([oracle.gemm_fp8_fp8_bf16_nt(a, sfa, b[j:j + 1], sfb1[j:j + 1], threads=8, want_f32=True)[1] for j in cols], axis=1)
    _assert_same_bits(got[:, cols], want, "strict 128-row tile")


def test_end_to_end_weight_gradient_through_the_quantiser(dga):
    """dW = dY^T . X over two micro-batches, both operands quantised per token with per_token_cast_to_fp8, accumulated in place."""
    torch.manual_seed(0)
    T, out_f, in_f = 1000, 300, 520      # (T: K % 128 != 0)
    out = torch.full((out_f, in_f), float("nan"), dtype=torch.float32, device="cuda")
    ref = np.zeros((out_f, in_f), np.float64)
    S = np.zeros((out_f, in_f), np.float64)
    for mb in range(2):
        dy = torch.randn((T, out_f), device="cuda").to(torch.bfloat16)
        x = (torch.randn((T, in_f), device="cuda") * (1 + torch.arange(in_f, device="cuda") / 64)).to(torch.bfloat16)
        qa, sa = dga.per_token_cast_to_fp8(dy.t().contiguous())
        qb, sb = dga.per_token_cast_to_fp8(x.t().contiguous())
        assert tuple(sb.shape) == (in_f, (T + 127) // 128)
        dga.wgrad_gemm_fp8_fp8_fp32_nt((qa, sa), (qb, sb), out, c=None if mb == 0 else out, sync=True)
        # the float64 product of the dequantised operands
        da = qa.float().double() * sa.double().repeat_interleave(128, dim=1)[:, :T]
        db = qb.float().double() * sb.double().repeat_interleave(128, dim=1)[:, :T]
        ref += (da @ db.t()).cpu().numpy()
        S += (da.abs() @ db.abs().t()).cpu().numpy()
    got = out.double().cpu().numpy()
    excess = np.abs(got - ref) - (2.0 ** -22 * S + 2.0 ** -24 * np.abs(ref) + 2.0 ** -24 * S)
    assert (excess <= 0).all(), f"{int((excess > 0).sum())} outputs beyond the bar"
    assert np.isfinite(got).all()


@pytest.mark.parametrize("m,n,k", [(300, 257, 1000), (2400, 4200, 400), (100, 300, 128 * 9 + 5)])
def test_c_semantics(dga, oracle, m, n, k):
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=11)
    sfb1 = _per_row(oracle, sfb, n, seed=12)
    plain = _wgrad(dga, a, sfa, b, sfb1)                   # out prefilled with NaN: every element written, never read
    assert not np.isnan(plain).any()
    c = np.random.default_rng(3).standard_normal((m, n)).astype(np.float32)
    sep = _wgrad(dga, a, sfa, b, sfb1, c=_dev(c))
    assert np.array_equal(sep.view(np.uint32), (plain + c).astype(np.float32).view(np.uint32))
    buf = _dev(c)
    inplace = _wgrad(dga, a, sfa, b, sfb1, c=buf, out=buf)   # c is out
    assert np.array_equal(inplace.view(np.uint32), sep.view(np.uint32))


def test_k_zero_gives_c(dga):
    m, n = 40, 70
    a = torch.zeros((m, 0), dtype=torch.uint8, device="cuda")
    b = torch.zeros((n, 0), dtype=torch.uint8, device="cuda")
    sfa = torch.zeros((m, 0), dtype=torch.float32, device="cuda")
    sfb = torch.zeros((n, 0), dtype=torch.float32, device="cuda")
    c = torch.randn((m, n), device="cuda")
    c[0, 0] = -0.0
    out = torch.full((m, n), float("nan"), device="cuda")
    dga.wgrad_gemm_fp8_fp8_fp32_nt((a, sfa), (b, sfb), out, c=c, sync=True)
    assert torch.equal(out.view(torch.int32), c.view(torch.int32))
    dga.wgrad_gemm_fp8_fp8_fp32_nt((a, sfa), (b, sfb), out, sync=True)
    assert torch.equal(out, torch.zeros_like(out))


def test_row_strided_views(dga, oracle):
    m, n, k = 200, 300, 1000
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=9)
    sfb1 = _per_row(oracle, sfb, n, seed=10)
    pa = torch.zeros((m, 1024), dtype=torch.uint8, device="cuda")
    pb = torch.zeros((n, 1152), dtype=torch.uint8, device="cuda")
    pa[:, :k] = _dev(a)
    pb[:, :k] = _dev(b)
    want = _wgrad(dga, a, sfa, b, sfb1)
    for zp in (None, (True, True)):
        _assert_same_bits(_wgrad(dga, pa[:, :k], sfa, pb[:, :k], sfb1, zero_padded=zp), want, f"strided, zero_padded={zp}")


def test_graph_capture_of_an_accumulating_call(dga, oracle):
    m, n, k = 100, 300, 1000
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=4)
    sfb1 = _per_row(oracle, sfb, n, seed=5)
    da, dsa, db, dsb = _dev(a), _dev(sfa), _dev(b), _dev(sfb1)
    p = _wgrad(dga, a, sfa, b, sfb1)                      # plan + workspace outside the capture
    c0 = np.random.default_rng(5).standard_normal((m, n)).astype(np.float32)
    buf = _dev(c0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dga.wgrad_gemm_fp8_fp8_fp32_nt((da, dsa), (db, dsb), buf, c=buf)
    torch.cuda.synchronize()
    buf.copy_(_dev(c0))
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    want = c0
    for _ in range(2):
        want = (want + p).astype(np.float32)
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_deep_gemm_cpp_matches_the_python_api(dga, oracle):
    from deepgemm_ascend_amd import deep_gemm_cpp
    m, n, k = 300, 257, 1000
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=8)
    sfb1 = _per_row(oracle, sfb, n, seed=9)
    c = _dev(np.random.default_rng(6).standard_normal((m, n)).astype(np.float32))
    want = _wgrad(dga, a, sfa, b, sfb1, c=c)
    out = torch.full((m, n), float("nan"), device="cuda")
    deep_gemm_cpp.wgrad_gemm_fp8_fp8_fp32_nt(_dev(a), _dev(sfa), _dev(b), _dev(sfb1), out, c)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    out2 = torch.full((m, n), float("nan"), device="cuda")
    deep_gemm_cpp.wgrad_gemm_fp8_fp8_fp32_nt(_dev(a), _dev(sfa), _dev(b), _dev(sfb1), out2)
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy().view(np.uint32), _wgrad(dga, a, sfa, b, sfb1).view(np.uint32))


def test_refusals_never_launch(dga, oracle):
    m, n, k = 128, 256, 512
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=1)
    out = torch.full((m, n), 7.0, device="cuda")
    for t in (_tile(dga, m, n, k, 128, 256, serial=7, build=0), _tile(dga, m, n, k, 128, 256, build=4)):
        with pytest.raises(dga.DGAError):
            dga.wgrad_gemm_fp8_fp8_fp32_nt((_dev(a), _dev(sfa)), (_dev(b), _dev(_rows(sfb, n))), out, tiling_=t, sync=True)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
