"""GPU: silu_and_mul_per_token_cast_to_fp8_transposed = per_token_cast_to_fp8 of (silu(gate) * up)^T with the product kept in fp32 and the
rows a mask excludes counted as +0.

Exact family (gate >= 20: the fp32 product is fl32(gate * up) exactly): (qt, sft) against oracle.quant_1x128 on the transpose of that
product, scales as uint32 and codes as bytes, in every layout.  Tolerance family (|gate| <= 16): the forward quantiser's scale and code
bounds and its cap on the share of elements off the oracle (tests/test_silu_mul_cast_gpu.py), with the blocks running along the tokens.
The row-wise output is the forward quantiser's bit for bit on any input.  Every output goes into sentinel-filled out= tensors, so an element
of (qt, sft) that the kernel leaves unwritten shows, and so does a row of (q, sf) that it writes although a mask excludes it."""
import numpy as np
import pytest
import torch

from test_silu_mul_cast_gpu import (SENTINEL_Q, SENTINEL_SF, _check_tolerance, _exact_inputs, _h_ref, _sentinels, _share_off_the_oracle,
                                    _tol_inputs, _u8)

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
UE8M0 = pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])


def _same(gq, gsf, wq, wsf, what):
    gsf, wsf = np.ascontiguousarray(gsf, np.float32), np.ascontiguousarray(wsf, np.float32)
    assert gsf.shape == wsf.shape and gq.shape == wq.shape, (what, gsf.shape, wsf.shape, gq.shape, wq.shape)
    sbad = np.nonzero(gsf.view(np.uint32) != wsf.view(np.uint32))
    assert sbad[0].size == 0, f"{what}: {sbad[0].size} scales differ, first at {[int(i[0]) for i in sbad]}: " \
                              f"{gsf.view(np.uint32)[sbad][0]:#x} vs {wsf.view(np.uint32)[sbad][0]:#x}"
    bad = np.nonzero(gq != wq)
    assert bad[0].size == 0, f"{what}: {bad[0].size} of {gq.size} codes differ, first at {[int(i[0]) for i in bad]}: " \
                             f"{gq[bad][0]:#x} vs {wq[bad][0]:#x}"


def _product(gate, up):
    """fl32(gate * up), rows flattened: the exact family's h."""
    gf = gate.float().cpu().numpy().reshape(-1, gate.shape[-1])
    uf = up.float().cpu().numpy().reshape(-1, up.shape[-1])
    return (gf * uf).astype(np.float32)


def _run(dga, oracle, x, want_h=None, valid=None, rowwise=False, aligned_rows=False, ue8m0=False, **masks):
    """One call into sentinel-filled out= tensors.  want_h [T, H] fp32 (None: the tolerance family, nothing to compare bytes with): (qt, sft)
    against oracle.quant_1x128(where(valid, want_h, 0)^T).  rowwise: (q, sf) against silu_and_mul_per_token_cast_to_fp8 with the same
    mask, bit for bit on the valid rows, the sentinel on the others.  valid: bool [T] (None: every row).  Returns the device outputs."""
    h = x.shape[-1] // 2
    lead = tuple(x.shape[:-1])
    t_n = int(np.prod(lead))
    ldqt = (t_n + 127) // 128 * 128 if aligned_rows else t_n
    buf, sft = _sentinels((h, ldqt), (h, (t_n + 127) // 128))
    qt = buf[:, :t_n]
    out = (qt, sft)
    if rowwise:
        q, sf = _sentinels(lead + (h,), lead + ((h + 127) // 128,))
        out = (out, (q, sf))
    res = dga.silu_and_mul_per_token_cast_to_fp8_transposed(x, rowwise=rowwise, aligned_rows=aligned_rows, use_ue8m0=ue8m0, out=out,
                                                            sync=True, **masks)
    rt = res[0] if rowwise else res
    assert rt[0].dtype == torch.float8_e4m3fn and rt[0].data_ptr() == buf.data_ptr() and rt[1].data_ptr() == sft.data_ptr()
    assert tuple(rt[0].shape) == (h, t_n) and rt[0].stride(0) == ldqt
    assert bool(getattr(rt[0], "_dga_zero_padded", False)) == (ldqt != t_n)
    valid = np.ones(t_n, bool) if valid is None else valid
    gbuf, gsft = buf.cpu().numpy(), sft.cpu().numpy()
    assert (gsft.view(np.uint32) != SENTINEL_SF).all(), "a scale of sft was not written"
    assert not gbuf[:, t_n:].any(), "the tails of the aligned rows are not zero"
    if want_h is not None:
        h0 = np.where(valid[:, None], want_h.reshape(t_n, h), np.float32(0.0))
        wq, wsf = oracle.quant_1x128(np.ascontiguousarray(h0.T), ue8m0=ue8m0)
        _same(gbuf[:, :t_n], gsft, wq, wsf, "transposed")
    if rowwise:
        fq, fsf = _sentinels(lead + (h,), lead + ((h + 127) // 128,))
        dga.silu_and_mul_per_token_cast_to_fp8(x, out=(fq, fsf), use_ue8m0=ue8m0, sync=True, **masks)
        gq, gsf = q.cpu().numpy().reshape(t_n, h), sf.cpu().numpy().reshape(t_n, -1)
        _same(gq[valid], gsf[valid], fq.cpu().numpy().reshape(t_n, h)[valid], fsf.cpu().numpy().reshape(t_n, -1)[valid], "row-wise")
        assert (gq[~valid] == SENTINEL_Q).all() and (gsf[~valid].view(np.uint32) == SENTINEL_SF).all(), "an excluded row of (q, sf) was written"
    return res


# ---- 1. the exact family, byte for byte

SHAPES = [(1, 8), (127, 77), (128, 128), (129, 136), (300, 384), (256, 1000)]


@UE8M0
@DTYPES
@pytest.mark.parametrize("t_n,h", SHAPES)
def test_exact_shapes(dga, oracle, dtype, t_n, h, ue8m0):
    """Partial tiles in both directions, more than one tile in both directions, H and T that are no multiples of 8 (byte-wise paths)."""
    x, gate, up = _exact_inputs((t_n,), h, dtype, seed=t_n * 7 + h)
    _run(dga, oracle, x, _product(gate, up), ue8m0=ue8m0)


@DTYPES
@pytest.mark.parametrize("t_n,h", [(129, 136), (300, 384)])
def test_aligned_rows(dga, oracle, dtype, t_n, h):
    """Rows of qt 256 and 384 bytes apart with zero tails; without out= the result is the same view."""
    x, gate, up = _exact_inputs((t_n,), h, dtype, seed=t_n * 11 + h)
    qt, sft = _run(dga, oracle, x, _product(gate, up), aligned_rows=True)
    assert qt.stride(0) == (t_n + 127) // 128 * 128 and tuple(qt.shape) == (h, t_n)
    qt2, sft2 = dga.silu_and_mul_per_token_cast_to_fp8_transposed(x, aligned_rows=True, sync=True)
    assert qt2.stride() == qt.stride() and qt2._dga_zero_padded
    assert torch.equal(qt2.view(torch.uint8), qt.view(torch.uint8)) and torch.equal(sft2.view(torch.int32), sft.view(torch.int32))
    pad = torch.as_strided(qt2.view(torch.uint8), (h, qt.stride(0)), (qt.stride(0), 1))
    assert not pad[:, t_n:].any().item()
    qt3, sft3 = dga.silu_and_mul_per_token_cast_to_fp8_transposed(x, sync=True)          # ... and the plain form without out=
    assert qt3.is_contiguous() and not getattr(qt3, "_dga_zero_padded", False)
    assert torch.equal(qt3.view(torch.uint8), qt.view(torch.uint8)) and torch.equal(sft3.view(torch.int32), sft.view(torch.int32))


# ---- 2. the row-wise output is the forward's, on any input

@UE8M0
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("family", ["exact", "tolerance"])
@pytest.mark.parametrize("t_n,h", [(129, 136), (300, 384), (127, 77)])
def test_rowwise_is_the_forward_quantisers(dga, oracle, family, dtype, t_n, h, ue8m0):
    """(q, sf) equals silu_and_mul_per_token_cast_to_fp8's bit for bit (_run), and (qt, sft) is what it is without the row-wise output."""
    x, gate, up = (_exact_inputs if family == "exact" else _tol_inputs)((t_n,), h, dtype, seed=t_n * 13 + h)
    want = _product(gate, up) if family == "exact" else None
    (qt, sft), (q, sf) = _run(dga, oracle, x, want, rowwise=True, ue8m0=ue8m0)
    qt0, sft0 = _run(dga, oracle, x, want, ue8m0=ue8m0)
    assert torch.equal(qt.view(torch.uint8), qt0.view(torch.uint8)) and torch.equal(sft.view(torch.int32), sft0.view(torch.int32))
    (_, (q2, sf2)) = dga.silu_and_mul_per_token_cast_to_fp8_transposed(x, rowwise=True, use_ue8m0=ue8m0, sync=True)     # without out=
    assert q2.dtype == torch.float8_e4m3fn and torch.equal(q2.view(torch.uint8), q.view(torch.uint8))
    assert torch.equal(sf2.view(torch.int32), sf.view(torch.int32))


# ---- 3. the tolerance family

TOL = [(torch.bfloat16, 256, 512), (torch.float32, 300, 1000), (torch.float16, 300, 1000), (torch.bfloat16, 127, 77)]


@UE8M0
@pytest.mark.parametrize("dtype,t_n,h", TOL, ids=[f"{str(d)[6:]}-{t}x{h}" for d, t, h in TOL])
def test_tolerance(dga, oracle, dtype, t_n, h, ue8m0):
    """The forward's checks with the blocks along the tokens: scales within 2^-18 + 2^-23 of amax / 448 of the float64 h, every code
    between RNE(y (1 - 2 eps)) and RNE(y (1 + 2 eps)); on the cases of >= 50 000 elements at most 1e-3 of the elements may differ from
    oracle.quant_1x128 on fl32 of the float64 h -- the forward's cap, which holds only while the amax of every 128-token block is the
    fp32 nearest to the real value (a scale one ULP off moves every element of its block): the channel amax is refined in fp64."""
    x, gate, up = _tol_inputs((t_n,), h, dtype, seed=t_n * 3 + h)
    qt, sft = _run(dga, oracle, x, ue8m0=ue8m0)
    href_t = np.ascontiguousarray(_h_ref(gate, up).T)
    gq, gsf = _u8(qt), sft.cpu().numpy()
    label = f"{dtype} {t_n}x{h} ue8m0={ue8m0}"
    _check_tolerance(oracle, gq, gsf, href_t, ue8m0, np.arange(h), label)
    if t_n * h >= 50000:
        assert _share_off_the_oracle(oracle, gq, gsf, href_t, ue8m0, label) <= 1e-3


def test_tolerance_masked(dga, oracle):
    """The same with m_indices: the excluded rows are zeros of the reference."""
    t_n, h = 300, 520
    x, gate, up = _tol_inputs((t_n,), h, torch.bfloat16, seed=29)
    idx = np.zeros(t_n, np.int32)
    idx[5::9] = -1; idx[128:170] = -1; idx[290:] = -1
    valid = idx >= 0
    qt, sft = _run(dga, oracle, _poison(x, valid), valid=valid, m_indices=torch.from_numpy(idx).cuda())
    href_t = np.ascontiguousarray(np.where(valid[:, None], _h_ref(gate, up), np.float32(0.0)).T)
    gq, gsf = _u8(qt), sft.cpu().numpy()
    _check_tolerance(oracle, gq, gsf, href_t, False, np.arange(h), "masked")
    assert _share_off_the_oracle(oracle, gq, gsf, href_t, False, "masked") <= 1e-3
    assert not gq[:, ~valid].any()


# ---- 4. edge values

@UE8M0
def test_edge_values(dga, oracle, ue8m0):
    """fp32, H = 8, T = 256 (two token blocks per channel).  Channel 0: up all zero -> scale 1, codes 0.  Channels 1, 3 and 4: NaN in gate
    at a lane's last token (8 c + 7) and NaN in up in the second token block -> codes with & 0x7F == 0x7F, the rest of each block
    quantised as if the NaN were absent.  Channel 2: gate = -120 and -1e4 decode to 0 and leave the rest alone."""
    t_n, h = 256, 8
    rng = np.random.default_rng(7)
    gate = rng.uniform(20.0, 60.0, (t_n, h)).astype(np.float32)
    up = (rng.standard_normal((t_n, h)) * 3.0).astype(np.float32)
    up[:, 0] = 0.0
    nans = [(8 * 1 + 7, 1), (128 + 37, 1), (8 * 3 + 7, 3), (8 * 15 + 7, 4), (255, 4)]
    gate[15, 1] = np.nan; up[165, 1] = np.nan; gate[31, 3] = -np.nan; up[127, 4] = np.nan; gate[255, 4] = np.nan
    zeros = [(3, 2), (200, 2)]
    gate[3, 2] = -120.0; gate[200, 2] = -1e4
    x = torch.from_numpy(np.concatenate([gate, up], axis=1)).cuda()
    qt, sft = _run(dga, oracle, x, ue8m0=ue8m0)
    want_h = (gate * up).astype(np.float32)
    for tok, c in nans + zeros:
        want_h[tok, c] = 0.0                          # "as if the NaN were absent"; silu(-120), silu(-1e4): below every e4m3 step here
    wq, wsf = oracle.quant_1x128(np.ascontiguousarray(want_h.T), ue8m0=ue8m0)
    gq, gsf = _u8(qt), sft.cpu().numpy()
    assert (gsf.view(np.uint32) == wsf.view(np.uint32)).all(), "scales differ"
    assert (gsf[0] == 1.0).all() and not gq[0].any()
    keep = np.ones((h, t_n), bool)
    for tok, c in nans:
        assert (gq[c, tok] & 0x7F) == 0x7F, (tok, c)
        keep[c, tok] = False
    for tok, c in zeros:
        assert (gq[c, tok] & 0x7F) == 0, (tok, c)
        keep[c, tok] = False
    assert (gq[keep] == wq[keep]).all()


# ---- 5. masks

def _poison(x, valid):
    """NaN and 3e38 (fp16: inf) in the rows the mask excludes, gate and up alike."""
    bad = torch.from_numpy(np.nonzero(~valid)[0]).cuda()
    flat = x.view(-1, x.shape[-1])
    flat[bad[0::2]] = float("nan")
    flat[bad[1::2]] = 3e38
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
    x, gate, up = _exact_inputs((t_n,), h, dtype, seed=41)
    res = _run(dga, oracle, _poison(x, valid), _product(gate, up), valid=valid, rowwise=rowwise, m_indices=torch.from_numpy(idx).cuda())
    qt, sft = res[0] if rowwise else res
    assert (sft[:, 1] == 1.0).all().item() and not qt.view(torch.uint8)[:, 128:256].any().item()
    assert not qt.view(torch.uint8)[:, 472:].any().item()


@pytest.mark.parametrize("rowwise", [False, True], ids=["transposed", "rowwise"])
def test_masked_m(dga, oracle, rowwise):
    """x [3, 128, 2 * 256] with masked_m = [128, 0, 77]: T = 384, group 1 is a block without a valid token."""
    counts = [128, 0, 77]
    valid = np.concatenate([np.arange(128) < c for c in counts])
    x, gate, up = _exact_inputs((3, 128), 256, torch.bfloat16, seed=43)
    res = _run(dga, oracle, _poison(x, valid), _product(gate, up), valid=valid, rowwise=rowwise,
               masked_m=torch.tensor(counts, dtype=torch.int32, device="cuda"))
    qt, sft = res[0] if rowwise else res
    assert (sft[:, 1] == 1.0).all().item() and not qt.view(torch.uint8)[:, 128:256].any().item()
    assert not qt.view(torch.uint8)[:, 256 + 77:].any().item()


@pytest.mark.parametrize("g_n,mmax,seed", [(61, 5, 47), (3, 200, 48)])
def test_masked_m_groups_that_straddle_tiles(dga, oracle, g_n, mmax, seed):
    """Mmax = 5 and 200: groups shorter than a lane's 8 tokens, and groups that no tile boundary respects."""
    counts = np.random.default_rng(seed).integers(0, mmax + 1, size=g_n).astype(np.int32)
    counts[0], counts[-1] = mmax, 0
    valid = np.concatenate([np.arange(mmax) < c for c in counts])
    x, gate, up = _exact_inputs((g_n, mmax), 136, torch.bfloat16, seed=seed)
    _run(dga, oracle, _poison(x, valid), _product(gate, up), valid=valid, rowwise=True, masked_m=torch.from_numpy(counts).cuda())


# ---- 6. misaligned pointers

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_misaligned_pointers(dga, oracle, dtype):
    """Shapes that allow the 16- and 8-byte accesses, (300, 384), on pointers that do not: x one element into a buffer, qt 3 bytes and q
    1 byte into theirs (out= as slices).  The same bytes as on aligned tensors, and nothing outside the slices is written."""
    t_n, h = 300, 384
    x0, gate, up = _exact_inputs((t_n,), h, dtype, seed=23)
    xb = torch.empty(t_n * 2 * h + 8, dtype=dtype, device="cuda")
    x = xb[1:1 + t_n * 2 * h].view(t_n, 2 * h)
    x.copy_(x0)
    qtb = torch.full((h * t_n + 8,), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    qb = torch.full((h * t_n + 8,), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    qt, q = qtb[3:3 + h * t_n].view(h, t_n), qb[1:1 + h * t_n].view(t_n, h)
    assert x.data_ptr() % 16 and qt.data_ptr() % 8 and q.data_ptr() % 8
    _, sft = _sentinels((1,), (h, 3))
    _, sf = _sentinels((1,), (t_n, 3))
    dga.silu_and_mul_per_token_cast_to_fp8_transposed(x, rowwise=True, out=((qt, sft), (q, sf)), sync=True)
    want = _product(gate, up)
    wq, wsf = oracle.quant_1x128(np.ascontiguousarray(want.T))
    _same(qt.cpu().numpy(), sft.cpu().numpy(), wq, wsf, "transposed")
    oq, osf = oracle.quant_1x128(want)
    _same(q.cpu().numpy(), sf.cpu().numpy(), oq, osf, "row-wise")
    (aqt, asft), (aq, asf) = dga.silu_and_mul_per_token_cast_to_fp8_transposed(x0, rowwise=True, sync=True)      # the aligned call
    assert torch.equal(aqt.view(torch.uint8), qt) and torch.equal(aq.view(torch.uint8), q)
    assert torch.equal(asft.view(torch.int32), sft.view(torch.int32)) and torch.equal(asf.view(torch.int32), sf.view(torch.int32))
    for b, lo in ((qtb, 3), (qb, 1)):
        assert (b[:lo] == SENTINEL_Q).all().item() and (b[lo + h * t_n:] == SENTINEL_Q).all().item(), "bytes outside the slice were written"


# ---- in the pipeline

def test_graph_capture_follows_m_indices(dga, oracle):
    """One call with m_indices, rowwise and out= is the whole graph.  The contents of m_indices and x are changed in place, one replay
    gives the result of the new contents."""
    t_n, h = 300, 136
    x, _, _ = _exact_inputs((t_n,), h, torch.bfloat16, seed=51)
    idx = torch.zeros(t_n, dtype=torch.int32, device="cuda")
    idx[100:] = -1
    buf, sft = _sentinels((h, t_n), (h, 3))
    q, sf = _sentinels((t_n, h), (t_n, 2))
    call = lambda: dga.silu_and_mul_per_token_cast_to_fp8_transposed(x, m_indices=idx, rowwise=True, out=((buf, sft), (q, sf)))
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
    x2, gate, up = _exact_inputs((t_n,), h, torch.bfloat16, seed=52)
    x.copy_(_poison(x2, valid))
    for t in (buf, q):
        t.fill_(SENTINEL_Q)
    sft.view(torch.int32).fill_(SENTINEL_SF); sf.view(torch.int32).fill_(SENTINEL_SF)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = _product(gate, up)
    wq, wsf = oracle.quant_1x128(np.ascontiguousarray(np.where(valid[:, None], want, np.float32(0.0)).T))
    _same(buf.cpu().numpy(), sft.cpu().numpy(), wq, wsf, "replay")
    oq, osf = oracle.quant_1x128(want[valid])
    gq, gsf = q.cpu().numpy(), sf.cpu().numpy()
    _same(gq[valid], gsf[valid], oq, osf, "replay, row-wise")
    assert (gq[~valid] == SENTINEL_Q).all() and (gsf[~valid].view(np.uint32) == SENTINEL_SF).all()


def test_pybind_matches_the_python_entry(dga):
    from deepgemm_ascend_amd import deep_gemm_cpp
    t_n, h = 300, 384
    idx = torch.zeros(t_n, dtype=torch.int32, device="cuda")
    idx[5::7] = -1; idx[250:] = -1
    x, _, _ = _tol_inputs((t_n,), h, torch.bfloat16, seed=61)
    x = _poison(x, (idx >= 0).cpu().numpy())
    qt, sft = dga.silu_and_mul_per_token_cast_to_fp8_transposed(x, m_indices=idx, sync=True)
    pq, psf = deep_gemm_cpp.silu_and_mul_per_token_cast_to_fp8_transposed(x, idx)
    torch.cuda.synchronize()
    assert pq.dtype == torch.float8_e4m3fn and tuple(pq.shape) == (h, t_n) and tuple(psf.shape) == (h, 3)
    assert torch.equal(pq.view(torch.uint8), qt.view(torch.uint8)) and torch.equal(psf.view(torch.int32), sft.view(torch.int32))
    pq, psf = deep_gemm_cpp.silu_and_mul_per_token_cast_to_fp8_transposed(x[:250])     # ... and without a mask
    qt, sft = dga.silu_and_mul_per_token_cast_to_fp8_transposed(x[:250], sync=True)
    assert torch.equal(pq.view(torch.uint8), qt.view(torch.uint8)) and torch.equal(psf.view(torch.int32), sft.view(torch.int32))


def test_into_the_k_grouped_wgrad_gemm(dga, oracle):
    """dW2[g] = dout_g^T . h_g in the contiguous layout of tests/test_cast_transposed_gpu.py test_into_the_k_grouped_wgrad_gemm: dout [T, M]
    and gate_up [T, 2 H], every expert's segment padded to 128 rows with NaN that m_indices marks.  The operand made from gate_up is the
    definition's bytes; each expert against the float64 product of the dequantised operands, under that test's bar."""
    torch.manual_seed(0)
    tokens = [200, 0, 77, 300]
    m, n = 256, 384
    seg = [(t + 127) // 128 * 128 for t in tokens]
    T = sum(seg) + 128
    dy = torch.full((T, m), float("nan"), dtype=torch.bfloat16)
    gate_up = torch.full((T, 2 * n), float("nan"), dtype=torch.bfloat16)
    idx = torch.full((T,), -1, dtype=torch.int32)
    r = 0
    for g, (t, s) in enumerate(zip(tokens, seg)):
        dy[r:r + t] = torch.randn(t, m).to(torch.bfloat16)
        gate_up[r:r + t, :n] = (torch.rand(t, n) * 40.0 + 20.0).to(torch.bfloat16).clamp(20.0, 60.0)
        gate_up[r:r + t, n:] = (torch.randn(t, n) * 3.0).to(torch.bfloat16)
        idx[r:r + t] = g
        r += s
    idx = idx.cuda()
    a, sfa = dga.per_token_cast_to_fp8_transposed(dy.cuda(), m_indices=idx)
    b, sfb = dga.silu_and_mul_per_token_cast_to_fp8_transposed(gate_up.cuda(), m_indices=idx)
    out = torch.full((len(tokens), m, n), float("nan"), dtype=torch.float32, device="cuda")
    dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt((a, sfa), (b, sfb), out, seg, sync=True)
    valid = (idx >= 0).cpu().numpy()
    hprod = _product(gate_up[:, :n], gate_up[:, n:])
    wq, wsf = oracle.quant_1x128(np.ascontiguousarray(np.where(valid[:, None], hprod, np.float32(0.0)).T))
    _same(_u8(b), sfb.cpu().numpy(), wq, wsf, "operand")
    tab = oracle.e4m3fn_table().astype(np.float64)
    da = tab[_u8(a)] * np.repeat(sfa.cpu().numpy().astype(np.float64), 128, axis=1)
    db = tab[_u8(b)] * np.repeat(sfb.cpu().numpy().astype(np.float64), 128, axis=1)
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    k0 = 0
    for g, s in enumerate(seg):
        ref = da[:, k0:k0 + s] @ db[:, k0:k0 + s].T
        S = np.abs(da[:, k0:k0 + s]) @ np.abs(db[:, k0:k0 + s]).T
        assert (np.abs(got[g] - ref) <= 2.0 ** -22 * S + 2.0 ** -24 * np.abs(ref)).all(), f"expert {g}"
        k0 += s
    assert not got[1].any() and np.abs(got[0]).max() > 1.0
