"""GPU: per_token_cast_to_fp8_transposed against its one definition, oracle.quant_1x128 on the transpose of x with the rows a mask excludes
set to zero.  Scales are compared as uint32 and codes as bytes (tests/test_cast_gpu.py _check): there is no tolerance anywhere except in
the GEMM test, which has the k-grouped GEMM's own bar.  Every output tensor is pre-filled with a sentinel, so an element of (qt, sft) that
the kernel leaves unwritten shows, and so does a row of (q, sf) that it writes although a mask excludes it."""
import numpy as np
import pytest
import torch

import cast_cases as C

pytestmark = pytest.mark.gpu

SENTINEL_Q, SENTINEL_SF = 0xA5, 0x7FC0A5A5


def _same(gq, gsf, wq, wsf, x, what):
    gsf, wsf = np.ascontiguousarray(gsf, np.float32), np.ascontiguousarray(wsf, np.float32)
    assert gsf.shape == wsf.shape and gq.shape == wq.shape, (what, gsf.shape, wsf.shape, gq.shape, wq.shape)
    sbad = np.nonzero(gsf.view(np.uint32) != wsf.view(np.uint32))
    assert sbad[0].size == 0, f"{what}: {sbad[0].size} scales differ, first at {[int(i[0]) for i in sbad]}: " \
                              f"{gsf.view(np.uint32)[sbad][0]:#x} vs {wsf.view(np.uint32)[sbad][0]:#x}"
    bad = np.nonzero(gq != wq)
    assert bad[0].size == 0, f"{what}: {bad[0].size} of {gq.size} codes differ, first at {[int(i[0]) for i in bad]}: " \
                             f"{gq[bad][0]:#x} vs {wq[bad][0]:#x} for x={x[bad][0]!r}"


def _sentinels(shape_q, shape_sf):
    return (torch.full(shape_q, SENTINEL_Q, dtype=torch.uint8, device="cuda"),
            torch.full(shape_sf, SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32))


def _run(dga, oracle, x_t, valid=None, rowwise=False, aligned_rows=False, ue8m0=False, **masks):
    """One call into sentinel-filled out= tensors, compared with the definition.  valid: bool [T] (None: every row).  Returns the device
    outputs ((qt, sft), (q, sf) or None) and the expected (qt, sft)."""
    h = x_t.shape[-1]
    lead = tuple(x_t.shape[:-1])
    t_n = int(np.prod(lead))
    ldqt = (t_n + 127) // 128 * 128 if aligned_rows else t_n
    buf, sft = _sentinels((h, ldqt), (h, (t_n + 127) // 128))
    qt = buf[:, :t_n]
    out = (qt, sft)
    if rowwise:
        q, sf = _sentinels(lead + (h,), lead + ((h + 127) // 128,))
        out = (out, (q, sf))
    res = dga.per_token_cast_to_fp8_transposed(x_t, rowwise=rowwise, aligned_rows=aligned_rows, use_ue8m0=ue8m0, out=out, sync=True, **masks)
    rt = res[0] if rowwise else res
    assert rt[0].dtype == torch.float8_e4m3fn and rt[0].data_ptr() == buf.data_ptr() and rt[1].data_ptr() == sft.data_ptr()
    assert bool(getattr(rt[0], "_dga_zero_padded", False)) == (ldqt != t_n)
    x = x_t.float().cpu().numpy().reshape(t_n, h)
    valid = np.ones(t_n, bool) if valid is None else valid
    x0 = np.where(valid[:, None], x, np.float32(0.0))
    wq, wsf = oracle.quant_1x128(np.ascontiguousarray(x0.T), ue8m0=ue8m0)
    gbuf = buf.cpu().numpy()
    _same(gbuf[:, :t_n], sft.cpu().numpy(), wq, wsf, x0.T, "transposed")
    assert not gbuf[:, t_n:].any(), "the tails of the aligned rows are not zero"
    if rowwise:
        rq, rsf = dga.per_token_cast_to_fp8(x_t.reshape(t_n, h), use_ue8m0=ue8m0)
        gq, gsf = q.cpu().numpy().reshape(t_n, h), sf.cpu().numpy().reshape(t_n, -1)
        _same(gq[valid], gsf[valid], rq.view(torch.uint8).cpu().numpy()[valid], rsf.cpu().numpy()[valid], x[valid], "row-wise")
        oq, osf = oracle.quant_1x128(x[valid], ue8m0=ue8m0)
        _same(gq[valid], gsf[valid], oq, osf, x[valid], "row-wise against the oracle")
        assert (gq[~valid] == SENTINEL_Q).all() and (gsf[~valid].view(np.uint32) == SENTINEL_SF).all(), "an excluded row of (q, sf) was written"
    return res, (wq, wsf)


def _randn(t_n, h, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn((t_n, h), device="cuda", generator=g) * 3.0).to(dtype)


DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])


@DTYPES
@pytest.mark.parametrize("t_n,h", [(1, 8), (127, 77), (128, 128), (129, 136), (300, 384), (256, 1000)])
def test_shapes(dga, oracle, dtype, t_n, h):
    """Partial tiles in both directions, more than one tile in both directions, H and T that are no multiples of 8 (byte-wise stores)."""
    _run(dga, oracle, _randn(t_n, h, dtype, t_n * 7 + h))


@DTYPES
@pytest.mark.parametrize("t_n,h", [(129, 136), (300, 384)])
def test_aligned_rows(dga, oracle, dtype, t_n, h):
    """Rows of qt 256 and 384 bytes apart with zero tails; without out= the result is the same view."""
    x = _randn(t_n, h, dtype, t_n * 11 + h)
    (qt, sft), _ = _run(dga, oracle, x, aligned_rows=True)
    assert qt.stride(0) == (t_n + 127) // 128 * 128 and tuple(qt.shape) == (h, t_n)
    qt2, sft2 = dga.per_token_cast_to_fp8_transposed(x, aligned_rows=True, sync=True)
    assert qt2.stride() == qt.stride() and qt2._dga_zero_padded
    assert torch.equal(qt2.view(torch.uint8), qt.view(torch.uint8)) and torch.equal(sft2.view(torch.int32), sft.view(torch.int32))
    pad = torch.as_strided(qt2.view(torch.uint8), (h, qt.stride(0)), (qt.stride(0), 1))
    assert not pad[:, t_n:].any().item()
    qt3, sft3 = dga.per_token_cast_to_fp8_transposed(x, sync=True)               # ... and the plain form without out=
    assert qt3.is_contiguous() and not getattr(qt3, "_dga_zero_padded", False)
    assert torch.equal(qt3.view(torch.uint8), qt.view(torch.uint8)) and torch.equal(sft3.view(torch.int32), sft.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("t_n,h", [(129, 136), (300, 384)])
def test_rowwise(dga, oracle, dtype, t_n, h):
    """(q, sf) equals per_token_cast_to_fp8(x) bytes, and (qt, sft) is what it is without the row-wise output."""
    x = _randn(t_n, h, dtype, t_n * 13 + h)
    ((qt, sft), (q, sf)), _ = _run(dga, oracle, x, rowwise=True)
    (qt0, sft0), _ = _run(dga, oracle, x)
    assert torch.equal(qt.view(torch.uint8), qt0.view(torch.uint8)) and torch.equal(sft.view(torch.int32), sft0.view(torch.int32))
    (_, (q2, sf2)) = dga.per_token_cast_to_fp8_transposed(x, rowwise=True, sync=True)     # without out=
    assert q2.dtype == torch.float8_e4m3fn and torch.equal(q2.view(torch.uint8), q.view(torch.uint8)) and torch.equal(sf2, sf)


@DTYPES
def test_rowwise_bytewise(dga, oracle, dtype):
    """(127, 77): H % 8 != 0, so the row-wise codes, like the loads and the transposed codes, go element by element."""
    _run(dga, oracle, _randn(127, 77, dtype, 19), rowwise=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_misaligned_pointers(dga, oracle, dtype):
    """Shapes that allow the 16- and 8-byte accesses, (300, 384), on pointers that do not: x one element into a buffer, qt 3 bytes and q
    1 byte into theirs (out= as slices).  The same bytes as on aligned tensors."""
    t_n, h = 300, 384
    x0 = _randn(t_n, h, dtype, 23)
    xb = torch.empty(t_n * h + 8, dtype=dtype, device="cuda")
    x = xb[1:1 + t_n * h].view(t_n, h)
    x.copy_(x0)
    qtb = torch.full((h * t_n + 8,), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    qb = torch.full((h * t_n + 8,), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    qt, q = qtb[3:3 + h * t_n].view(h, t_n), qb[1:1 + h * t_n].view(t_n, h)
    assert x.data_ptr() % 16 and qt.data_ptr() % 8 and q.data_ptr() % 8
    _, sft = _sentinels((1,), (h, 3))
    _, sf = _sentinels((1,), (t_n, 3))
    dga.per_token_cast_to_fp8_transposed(x, rowwise=True, out=((qt, sft), (q, sf)), sync=True)
    xn = x0.float().cpu().numpy()
    wq, wsf = oracle.quant_1x128(np.ascontiguousarray(xn.T))
    _same(qt.cpu().numpy(), sft.cpu().numpy(), wq, wsf, xn.T, "transposed")
    oq, osf = oracle.quant_1x128(xn)
    _same(q.cpu().numpy(), sf.cpu().numpy(), oq, osf, xn, "row-wise")
    for b, lo in ((qtb, 3), (qb, 1)):
        assert (b[:lo] == SENTINEL_Q).all().item() and (b[lo + h * t_n:] == SENTINEL_Q).all().item(), "bytes outside the slice were written"


def test_ue8m0(dga, oracle):
    (_, sft), _ = _run(dga, oracle, _randn(300, 384, torch.bfloat16, 5), ue8m0=True)
    bits = sft.view(torch.int32)
    assert bool(((bits & 0x007FFFFF) == 0).all()) and bool((bits > 0).all()), "a scale is not a power of two"
    _run(dga, oracle, _randn(300, 384, torch.float32, 6), ue8m0=True, rowwise=True)


# ---- edge values

def _edge_matrix():
    """The 9 x 256 matrix of tests/test_cast_gpu.py test_cast_edge_values, row for row."""
    x = np.zeros((9, 256), np.float32)
    x[0, :128] = np.linspace(-1, 1, 128)           # ordinary
    x[1, 0] = 448.0; x[1, 1:9] = [2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 1e-3, -1e-3, 2.0 ** -6, 17.0, 19.0]
    x[2, :128] = 0.0                               # all-zero block -> scale 1, codes 0
    x[2, 128:] = -0.0
    x[3, :128] = np.float32(1e-38) * np.arange(128)  # tiny amax: the scale is subnormal-adjacent
    x[4, :128] = np.float32(3e38) * np.linspace(-1, 1, 128)
    x[5, :128] = np.arange(128) * 0.0625           # many exact ties after scaling
    x[6, 5] = np.nan; x[6, 6] = -np.nan; x[6, 7] = 1.0
    x[7, 128:] = np.float32(1e-45)                 # denormal inputs
    x[8, :10] = [np.inf, -np.inf, 1.0, -1.0, 0.0, -0.0, 3e38, -1e-45, np.nan, -np.nan]
    x[8, 128] = -np.inf; x[8, 129:133] = [5.0, -5.0, np.inf, -np.nan]      # -inf alone makes the maximum infinite too
    return x


@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
def test_edge_values(dga, oracle, ue8m0):
    """Fed as its transpose [256, 9]: the blocks lie along the tokens, and row 8's spelled-out codes appear in channel 8."""
    x = _edge_matrix()
    xt = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    (qt, sft), (wq, wsf) = _run(dga, oracle, xt, ue8m0=ue8m0)
    oq, osf = oracle.quant_1x128(x, ue8m0=ue8m0)
    assert (oq == wq).all() and (osf.view(np.uint32) == wsf.view(np.uint32)).all()
    q8 = qt.view(torch.uint8)
    assert q8[8, :10].tolist() == [0x7F, 0xFF, 0, 0x80, 0, 0x80, 0, 0x80, 0x7F, 0xFF]
    assert q8[8, 128:134].tolist() == [0xFF, 0, 0x80, 0x7F, 0xFF, 0] and sft[8].tolist() == [np.inf, np.inf]
    assert sft[2].tolist() == [1.0, 1.0] and not q8[2, :128].any().item() and (q8[2, 128:] == 0x80).all().item()
    # NaN of both signs beside the block's only number: amax = 1, which is 448 s (ue8m0: s = 2^-8, and 256 is code 0x78)
    assert q8[6, 5:8].tolist() == [0x7F, 0xFF, 0x78 if ue8m0 else 0x7E]
    assert sft[6, 0].item() == (2.0 ** -8 if ue8m0 else np.float32(1.0) / np.float32(448.0))


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_signalling_nan_and_nan_only_blocks(dga, oracle, kind):
    """16-bit signalling NaNs of both signs at every place of a lane's and a wave's reduction order (token 8 c + 7 and token 128 + c of
    channel c, among ordinary values), a block whose only non-zero is a quiet NaN and one whose only non-zero is a signalling NaN: the
    maximum ignores them all (scale 1 for the NaN-only blocks), the codes are sign | 0x7F."""
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[kind]
    snan, qnan = {"bf16": (0x7F81, 0x7FC0), "fp16": (0x7D01, 0x7E00)}[kind]
    t_n, h = 256, 24
    bits = _randn(t_n, h, dtype, 17).view(torch.int16).cpu().numpy().view(np.uint16).copy()
    for c in range(16):
        bits[8 * c + 7, c] = snan | (0x8000 if c % 2 else 0)
        bits[128 + c, c] = snan | (0 if c % 2 else 0x8000)
    bits[:, 16:20] = 0
    bits[37, 16] = qnan; bits[128 + 90, 16] = qnan | 0x8000
    bits[0, 17] = snan; bits[255, 17] = snan | 0x8000
    bits[127, 18] = snan | 0x8000                                       # (channel 19 stays an all-zero channel beside them)
    xt = torch.from_numpy(bits.view(np.int16)).cuda().view(dtype)
    ((qt, sft), _), _ = _run(dga, oracle, xt, rowwise=True)
    q8, s = qt.view(torch.uint8).cpu().numpy(), sft.cpu().numpy()
    assert (s[16:20] == 1.0).all() and np.isfinite(s).all() and (s > 0).all()
    assert q8[16, 37] == 0x7F and q8[16, 218] == 0xFF and q8[17, 0] == 0x7F and q8[17, 255] == 0xFF and q8[18, 127] == 0xFF
    assert np.count_nonzero(q8[16:20]) == 5
    for c in range(16):
        assert q8[c, 8 * c + 7] == (0xFF if c % 2 else 0x7F) and q8[c, 128 + c] == (0x7F if c % 2 else 0xFF), c


# ---- rounding ties

@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
def test_ties_along_the_tokens(dga, oracle, ue8m0):
    """64 tie blocks (cast_cases.tie_blocks, the scale exponents of tests/test_cast_rounding_gpu.py: inside, at both ends of and beyond
    quant8's fast path) laid along the token direction: channel c holds blocks 2 c and 2 c + 1, x is [256, 32] fp32."""
    blocks = C.tie_blocks(64, C.TIE_EXPS, 31)
    xt = torch.from_numpy(np.ascontiguousarray(blocks.reshape(32, 256).T)).cuda()
    _, (wq, wsf) = _run(dga, oracle, xt, ue8m0=ue8m0)
    oq, osf = oracle.quant_1x128(blocks, ue8m0=ue8m0)                   # block by block: the same bytes in another shape
    assert (wq.reshape(64, 128) == oq).all() and (wsf.reshape(64, 1).view(np.uint32) == osf.view(np.uint32)).all()


# ---- masks

def _poison(x, valid):
    """NaN and 3e38 (fp16: inf) in the rows the mask excludes."""
    bad = torch.from_numpy(np.nonzero(~valid)[0]).cuda()
    x[bad[0::2]] = float("nan")
    x[bad[1::2]] = 3e38
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rowwise", [False, True], ids=["transposed", "rowwise"])
def test_m_indices(dga, oracle, dtype, rowwise):
    """T = 512, H = 200; negative indices on a scattered set, on the whole 128-token block 1 and on the last 40 rows."""
    t_n, h = 512, 200
    rng = np.random.default_rng(3)
    idx = np.repeat(np.arange(4, dtype=np.int32), 128)
    idx[rng.choice(np.r_[0:128, 256:472], size=45, replace=False)] = -1
    idx[128:256] = -1
    idx[472:] = -7
    valid = idx >= 0
    x = _poison(_randn(t_n, h, dtype, 41), valid)
    res, (wq, wsf) = _run(dga, oracle, x, valid=valid, rowwise=rowwise, m_indices=torch.from_numpy(idx).cuda())
    qt, sft = res[0] if rowwise else res
    assert (wsf[:, 1] == 1.0).all() and not wq[:, 128:256].any() and not wq[:, 472:].any()       # (what the definition says there)
    assert (sft[:, 1] == 1.0).all().item() and not qt.view(torch.uint8)[:, 128:256].any().item()


@pytest.mark.parametrize("rowwise", [False, True], ids=["transposed", "rowwise"])
def test_masked_m(dga, oracle, rowwise):
    """x [3, 128, 256] with masked_m = [128, 0, 77]: T = 384, group 1 is a block without a valid token."""
    counts = [128, 0, 77]
    valid = np.concatenate([np.arange(128) < c for c in counts])
    x = _poison(_randn(384, 256, torch.bfloat16, 43), valid).view(3, 128, 256)
    res, (wq, wsf) = _run(dga, oracle, x, valid=valid, rowwise=rowwise, masked_m=torch.tensor(counts, dtype=torch.int32, device="cuda"))
    qt, sft = res[0] if rowwise else res
    assert (sft[:, 1] == 1.0).all().item() and not qt.view(torch.uint8)[:, 128:256].any().item()
    assert not qt.view(torch.uint8)[:, 256 + 77:].any().item()


def test_masked_m_groups_that_straddle_tiles(dga, oracle):
    """Mmax = 5 and 200: groups shorter than a lane's 8 tokens, and groups that no tile boundary respects."""
    for g_n, mmax, seed in ((61, 5, 47), (3, 200, 48)):
        counts = np.random.default_rng(seed).integers(0, mmax + 1, size=g_n).astype(np.int32)
        counts[0], counts[-1] = mmax, 0
        valid = np.concatenate([np.arange(mmax) < c for c in counts])
        x = _poison(_randn(g_n * mmax, 136, torch.bfloat16, seed), valid).view(g_n, mmax, 136)
        _run(dga, oracle, x, valid=valid, rowwise=True, masked_m=torch.from_numpy(counts).cuda())


# ---- in the pipeline

def test_graph_capture_follows_m_indices(dga, oracle):
    """One call with m_indices and out= is the whole graph (a single kernel node).  The contents of m_indices and x are changed in place,
    one replay gives the result of the new contents."""
    t_n, h = 300, 136
    x = _randn(t_n, h, torch.bfloat16, 51)
    idx = torch.zeros(t_n, dtype=torch.int32, device="cuda")
    idx[100:] = -1
    buf, sft = _sentinels((h, t_n), (h, 3))
    q, sf = _sentinels((t_n, h), (t_n, 2))
    call = lambda: dga.per_token_cast_to_fp8_transposed(x, m_indices=idx, rowwise=True, out=((buf, sft), (q, sf)))
    call(); torch.cuda.synchronize()                       # eager once: the library is loaded
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    torch.cuda.synchronize()
    new_idx = np.zeros(t_n, np.int32)
    new_idx[::3] = -1; new_idx[128:256] = 2; new_idx[290:] = -1
    valid = new_idx >= 0
    idx.copy_(torch.from_numpy(new_idx).cuda())
    x.copy_(_poison(_randn(t_n, h, torch.bfloat16, 52), valid))
    for t, s in ((buf, SENTINEL_Q), (q, SENTINEL_Q)):
        t.fill_(s)
    sft.view(torch.int32).fill_(SENTINEL_SF); sf.view(torch.int32).fill_(SENTINEL_SF)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    xn = x.float().cpu().numpy()
    wq, wsf = oracle.quant_1x128(np.ascontiguousarray(np.where(valid[:, None], xn, np.float32(0.0)).T))
    _same(buf.cpu().numpy(), sft.cpu().numpy(), wq, wsf, xn.T, "replay")
    oq, osf = oracle.quant_1x128(xn[valid])
    gq, gsf = q.cpu().numpy(), sf.cpu().numpy()
    _same(gq[valid], gsf[valid], oq, osf, xn[valid], "replay, row-wise")
    assert (gq[~valid] == SENTINEL_Q).all() and (gsf[~valid].view(np.uint32) == SENTINEL_SF).all()


def test_pybind_matches_the_python_entry(dga):
    from deepgemm_ascend_amd import deep_gemm_cpp
    t_n, h = 300, 384
    idx = torch.zeros(t_n, dtype=torch.int32, device="cuda")
    idx[5::7] = -1; idx[250:] = -1
    x = _poison(_randn(t_n, h, torch.bfloat16, 61), (idx >= 0).cpu().numpy())
    qt, sft = dga.per_token_cast_to_fp8_transposed(x, m_indices=idx, sync=True)
    pq, psf = deep_gemm_cpp.per_token_cast_to_fp8_transposed(x, idx)
    torch.cuda.synchronize()
    assert pq.dtype == torch.float8_e4m3fn and tuple(pq.shape) == (h, t_n) and tuple(psf.shape) == (h, 3)
    assert torch.equal(pq.view(torch.uint8), qt.view(torch.uint8)) and torch.equal(psf.view(torch.int32), sft.view(torch.int32))
    pq, psf = deep_gemm_cpp.per_token_cast_to_fp8_transposed(x[:250])                  # ... and without a mask
    qt, sft = dga.per_token_cast_to_fp8_transposed(x[:250], sync=True)
    assert torch.equal(pq.view(torch.uint8), qt.view(torch.uint8)) and torch.equal(psf.view(torch.int32), sft.view(torch.int32))


def test_into_the_k_grouped_wgrad_gemm(dga, oracle):
    """tests/test_k_grouped_wgrad_gpu.py test_end_to_end_from_the_contiguous_forward_layout without the torch transposes and without zeroed
    padding: dY [T, M] and X [T, N] in the contiguous layout, every expert's segment padded to 128 rows with NaN that m_indices marks.
    Each expert against the float64 dY_g^T X_g of the dequantised operands, under that test's bar."""
    torch.manual_seed(0)
    tokens = [200, 0, 77, 300]
    m, n = 256, 384
    seg = [(t + 127) // 128 * 128 for t in tokens]
    T = sum(seg) + 128
    dy = torch.full((T, m), float("nan"), dtype=torch.bfloat16)
    x = torch.full((T, n), float("nan"), dtype=torch.bfloat16)
    idx = torch.full((T,), -1, dtype=torch.int32)
    r = 0
    for g, (t, s) in enumerate(zip(tokens, seg)):
        dy[r:r + t] = torch.randn(t, m).to(torch.bfloat16)
        x[r:r + t] = torch.randn(t, n).to(torch.bfloat16)
        idx[r:r + t] = g
        r += s
    idx = idx.cuda()
    a, sfa = dga.per_token_cast_to_fp8_transposed(dy.cuda(), m_indices=idx)
    b, sfb = dga.per_token_cast_to_fp8_transposed(x.cuda(), m_indices=idx)
    out = torch.full((len(tokens), m, n), float("nan"), dtype=torch.float32, device="cuda")
    dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt((a, sfa), (b, sfb), out, seg, sync=True)
    valid = (idx >= 0).cpu().numpy()
    for q_, sf_, src in ((a, sfa, dy), (b, sfb, x)):                   # the operands are the definition's
        wq, wsf = oracle.quant_1x128(np.ascontiguousarray(np.where(valid[:, None], src.float().numpy(), np.float32(0.0)).T))
        _same(q_.view(torch.uint8).cpu().numpy(), sf_.cpu().numpy(), wq, wsf, src.float().numpy().T, "operand")
    tab = oracle.e4m3fn_table().astype(np.float64)
    da = tab[a.view(torch.uint8).cpu().numpy()] * np.repeat(sfa.cpu().numpy().astype(np.float64), 128, axis=1)
    db = tab[b.view(torch.uint8).cpu().numpy()] * np.repeat(sfb.cpu().numpy().astype(np.float64), 128, axis=1)
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    k0 = 0
    for g, s in enumerate(seg):
        ref = da[:, k0:k0 + s] @ db[:, k0:k0 + s].T
        S = np.abs(da[:, k0:k0 + s]) @ np.abs(db[:, k0:k0 + s]).T
        assert (np.abs(got[g] - ref) <= 2.0 ** -22 * S + 2.0 ** -24 * np.abs(ref)).all(), f"expert {g}"
        k0 += s
    assert not got[1].any() and np.abs(got[0]).max() > 1.0
