"""GPU: silu_and_mul_backward_per_token_cast_to_fp8_transposed = per_token_cast_to_fp8_transposed of the fp32 [dgate | dup], with the
gradient kept in registers and the rows a mask excludes counted as zeros.

The contract is by composition, exact, on every input: with G the float32 grad_x_out that silu_and_mul_backward_per_token_cast_to_fp8 writes
for (x.float(), grad_h.float()) under the same mask, (dqt, dsft) = per_token_cast_to_fp8_transposed(G, same mask) byte for byte and bit for
bit, and with rowwise=True (dq, dsf) is silu_and_mul_backward_per_token_cast_to_fp8's on the original dtype.  G is prefilled with NaN, so a
row that entry left unwritten would show; every output of the new entry goes into sentinel-filled out= tensors, so an element of
(dqt, dsft) that is not written shows, and so does a row of (dq, dsf) that is written although a mask excludes it.  The exact family
(gate >= 20) is compared with the oracle alone."""
import numpy as np
import pytest
import torch

from fused_bounds import _reference
from test_silu_mul_bwd_cast_gpu import M_INDICES, MASKS, SENTINEL_Q, SENTINEL_SF, _exact_case, _tol_case, _u8
from test_silu_mul_cast_transposed_gpu import _same, _sentinels

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
UE8M0 = pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
NAN16 = 0x7FC1


def _composed(dga, x, grad, aligned_rows=False, ue8m0=False, **masks):
    """(per_token_cast_to_fp8_transposed(G), G): G the existing entry's unrounded fp32 gradient of the up-converted inputs, NaN where that
    entry wrote nothing."""
    big_g = torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda")
    dga.silu_and_mul_backward_per_token_cast_to_fp8(x.float(), grad.float(), grad_x_out=big_g, use_ue8m0=ue8m0, **masks)
    return dga.per_token_cast_to_fp8_transposed(big_g, aligned_rows=aligned_rows, use_ue8m0=ue8m0, sync=True, **masks), big_g


def _run(dga, x, grad, valid=None, rowwise=False, aligned_rows=False, ue8m0=False, compose=True, **masks):
    """One call into sentinel-filled out= tensors: the shapes, strides and the zero-padding promise; every element of (dqt, dsft) written;
    (dqt, dsft) against the composition; with rowwise (dq, dsf) against the existing entry on the same tensors, bit for bit on the valid
    rows, the sentinels on the others.  valid: bool [T] (None: every row).  Returns the device outputs."""
    h = x.shape[-1] // 2
    lead = tuple(x.shape[:-1])
    t_n = int(np.prod(lead))
    ldqt = (t_n + 127) // 128 * 128 if aligned_rows else t_n
    buf, sft = _sentinels((2 * h, ldqt), (2 * h, (t_n + 127) // 128))
    out = (buf[:, :t_n], sft)
    if rowwise:
        q, sf = _sentinels(lead + (2 * h,), lead + (2 * h // 128,))
        out = (out, (q, sf))
    res = dga.silu_and_mul_backward_per_token_cast_to_fp8_transposed(x, grad, rowwise=rowwise, aligned_rows=aligned_rows, use_ue8m0=ue8m0,
                                                                     out=out, sync=True, **masks)
    rt = res[0] if rowwise else res
    assert rt[0].dtype == torch.float8_e4m3fn and rt[0].data_ptr() == buf.data_ptr() and rt[1].data_ptr() == sft.data_ptr()
    assert tuple(rt[0].shape) == (2 * h, t_n) and rt[0].stride(0) == ldqt
    assert bool(getattr(rt[0], "_dga_zero_padded", False)) == (ldqt != t_n)
    valid = np.ones(t_n, bool) if valid is None else valid
    gbuf, gsft = buf.cpu().numpy(), sft.cpu().numpy()
    assert (gsft.view(np.uint32) != SENTINEL_SF).all(), "a scale of dsft was not written"
    assert not gbuf[:, t_n:].any(), "the tails of the aligned rows are not zero"
    assert not gbuf[:, :t_n][:, ~valid].any(), "an excluded token's code is not 0"
    if compose:
        (wqt, wsft), _ = _composed(dga, x, grad, aligned_rows=aligned_rows, ue8m0=ue8m0, **masks)
        assert wqt.stride(0) == ldqt
        _same(gbuf[:, :t_n], gsft, wqt.view(torch.uint8).cpu().numpy(), wsft.cpu().numpy(), "transposed against the composition")
    if rowwise:
        fq, fsf = _sentinels(lead + (2 * h,), lead + (2 * h // 128,))
        dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, out=(fq, fsf), use_ue8m0=ue8m0, sync=True, **masks)
        gq, gsf = q.cpu().numpy().reshape(t_n, 2 * h), sf.cpu().numpy().reshape(t_n, -1)
        _same(gq[valid], gsf[valid], fq.cpu().numpy().reshape(t_n, 2 * h)[valid], fsf.cpu().numpy().reshape(t_n, -1)[valid], "row-wise")
        assert (gq[~valid] == SENTINEL_Q).all() and (gsf[~valid].view(np.uint32) == SENTINEL_SF).all(), "an excluded row of (dq, dsf) was written"
    return res


def _poisoned(t, valid):
    """A copy of t with NaN (bf16: the bits 0x7FC1) in the rows that are not valid."""
    t = t.clone()
    bad = torch.from_numpy(np.nonzero(~valid)[0]).cuda()
    if t.dtype == torch.bfloat16:
        t.view(torch.int16).view(-1, t.shape[-1])[bad] = NAN16
    else:
        t.view(-1, t.shape[-1])[bad] = float("nan")
    return t


# ---- 1. the composition

# a one-token tile; the token tail; several tiles on both axes; both halves everywhere
SHAPES = [(1, 128), (127, 128), (128, 256), (129, 128), (300, 384)]


@UE8M0
@DTYPES
@pytest.mark.parametrize("t_n,h", SHAPES)
def test_composition(dga, dtype, t_n, h, ue8m0):
    """The tolerance family's inputs (gate in [-16, 16]: the sigmoid path is live).  Both forms against the composition and the existing
    entry (_run), and (dqt, dsft) does not depend on rowwise."""
    x, grad, ref, bound = _tol_case(dtype, t_n, h, t_n * 3 + h)
    qt0, sft0 = _run(dga, x, grad, ue8m0=ue8m0)
    (qt, sft), (q, sf) = _run(dga, x, grad, rowwise=True, ue8m0=ue8m0)
    assert torch.equal(qt.view(torch.uint8), qt0.view(torch.uint8)) and torch.equal(sft.view(torch.int32), sft0.view(torch.int32))
    (_, (q2, sf2)) = dga.silu_and_mul_backward_per_token_cast_to_fp8_transposed(x, grad, rowwise=True, use_ue8m0=ue8m0, sync=True)    # without out=
    assert q2.dtype == torch.float8_e4m3fn and torch.equal(q2.view(torch.uint8), q.view(torch.uint8))
    assert torch.equal(sf2.view(torch.int32), sf.view(torch.int32))


def test_the_composed_gradient_is_the_existing_entrys(dga):
    """What the composition stands on: G is within the existing entry's element bounds of the float64 reference (fused_bounds._reference), and
    it has no NaN left on an unmasked input -- so the accuracy of the new entry is that entry's, and no new bound is introduced."""
    h = 384
    x, grad, _, _ = _tol_case(torch.bfloat16, 300, h, 300 * 3 + h)
    ref, bound = _reference(x[:, :h].cpu(), x[:, h:].cpu(), grad.cpu())
    _, big_g = _composed(dga, x, grad)
    got = big_g.cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any() and (np.abs(got - ref) <= bound).all()


# ---- 2. the exact family against the oracle alone

@UE8M0
@DTYPES
@pytest.mark.parametrize("t_n,h", [(130, 256), (300, 384)])
def test_exact_against_the_oracle(dga, oracle, dtype, t_n, h, ue8m0):
    """gate >= 20: the gradient is fl32([d u | d g]) exactly, so (dqt, dsft) is oracle.quant_1x128 of its transpose; no device code in the
    expectation."""
    x, grad, want, _ = _exact_case((t_n,), h, dtype, t_n * 7 + h)
    qt, sft = _run(dga, x, grad, ue8m0=ue8m0, compose=False)
    wq, wsf = oracle.quant_1x128(np.ascontiguousarray(want.T), ue8m0=ue8m0)
    _same(_u8(qt), sft.cpu().numpy(), wq, wsf, "transposed against the oracle")


# ---- 3. aligned_rows

@DTYPES
@pytest.mark.parametrize("t_n,h", [(129, 128), (300, 384)])
def test_aligned_rows(dga, dtype, t_n, h):
    """Rows of dqt 256 and 384 bytes apart with zero tails (the buffer is prefilled with 0xA5: _run); without out= the result is the same view
    and carries the promise."""
    x, grad, _, _ = _tol_case(dtype, t_n, h, t_n * 3 + h)
    qt, sft = _run(dga, x, grad, aligned_rows=True)
    ld = (t_n + 127) // 128 * 128
    assert qt.stride(0) == ld and tuple(qt.shape) == (2 * h, t_n)
    qt2, sft2 = dga.silu_and_mul_backward_per_token_cast_to_fp8_transposed(x, grad, aligned_rows=True, sync=True)
    assert qt2.stride() == qt.stride() and qt2._dga_zero_padded
    assert torch.equal(qt2.view(torch.uint8), qt.view(torch.uint8)) and torch.equal(sft2.view(torch.int32), sft.view(torch.int32))
    pad = torch.as_strided(qt2.view(torch.uint8), (2 * h, ld), (ld, 1))
    assert not pad[:, t_n:].any().item()
    qt3, sft3 = dga.silu_and_mul_backward_per_token_cast_to_fp8_transposed(x, grad, sync=True)          # ... and the plain form without out=
    assert qt3.is_contiguous() and not getattr(qt3, "_dga_zero_padded", False)
    assert torch.equal(qt3.view(torch.uint8), qt.view(torch.uint8)) and torch.equal(sft3.view(torch.int32), sft.view(torch.int32))


# ---- 4. masks

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rowwise", [False, True], ids=["transposed", "rowwise"])
def test_m_indices(dga, dtype, rowwise):
    """40 rows in three segments with -1 tails, H = 384; the excluded rows of x and grad_h hold NaN."""
    t_n, h = len(M_INDICES), 384
    valid = np.array(M_INDICES) >= 0
    x, grad, _, _ = _tol_case(dtype, t_n, h, 71)
    idx = torch.tensor(M_INDICES, dtype=torch.int32, device="cuda")
    _run(dga, _poisoned(x, valid), _poisoned(grad, valid), valid=valid, rowwise=rowwise, m_indices=idx)


@pytest.mark.parametrize("rowwise", [False, True], ids=["transposed", "rowwise"])
def test_m_indices_with_an_empty_block(dga, rowwise):
    """T = 300: the whole 128-token block 1 and the last 10 rows excluded -> scale 1 and codes 0 there."""
    t_n, h = 300, 128
    idx = np.zeros(t_n, np.int32)
    idx[5::9] = -1; idx[128:256] = -1; idx[290:] = -1
    valid = idx >= 0
    x, grad, _, _ = _tol_case(torch.bfloat16, t_n, h, 73)
    res = _run(dga, _poisoned(x, valid), _poisoned(grad, valid), valid=valid, rowwise=rowwise, m_indices=torch.from_numpy(idx).cuda())
    qt, sft = res[0] if rowwise else res
    assert (sft[:, 1] == 1.0).all().item() and not qt.view(torch.uint8)[:, 128:256].any().item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rowwise", [False, True], ids=["transposed", "rowwise"])
def test_masked_m(dga, dtype, rowwise):
    """x [4, 24, 2 * 256] with masked_m = [0, 24, 1, 17]."""
    g_n, mmax, h = len(MASKS), 24, 256
    valid = np.concatenate([np.arange(mmax) < c for c in MASKS])
    x, grad, _, _ = _tol_case(dtype, g_n * mmax, h, 79)
    x, grad = _poisoned(x, valid).view(g_n, mmax, 2 * h), _poisoned(grad, valid).view(g_n, mmax, h)
    _run(dga, x, grad, valid=valid, rowwise=rowwise, masked_m=torch.tensor(MASKS, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("g_n,mmax,seed", [(61, 5, 47), (3, 200, 48)])
def test_masked_m_groups_that_straddle_tiles(dga, g_n, mmax, seed):
    """Mmax = 5 and 200: groups shorter than a lane's 8 tokens, and groups that no tile boundary respects."""
    counts = np.random.default_rng(seed).integers(0, mmax + 1, size=g_n).astype(np.int32)
    counts[0], counts[-1] = mmax, 0
    valid = np.concatenate([np.arange(mmax) < c for c in counts])
    h = 128
    x, grad, _, _ = _tol_case(torch.bfloat16, g_n * mmax, h, seed)
    x, grad = _poisoned(x, valid).view(g_n, mmax, 2 * h), _poisoned(grad, valid).view(g_n, mmax, h)
    _run(dga, x, grad, valid=valid, rowwise=True, masked_m=torch.from_numpy(counts).cuda())


# ---- 5. edge values

@UE8M0
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_edge_values(dga, dtype, ue8m0):
    """(128, 128), one special value per element, through the composition (both forms: _run).  Channels 0 .. 2: NaN in gate, up and grad;
    3 .. 5: +-inf in gate, up and grad; 6: gate = -100 and +100; 7: a subnormal grad on every token; 8: grad all zero -> scale 1 and zero
    codes in both halves; 9: grad zero but for one NaN -> scale 1, that code sign | 0x7F, in both halves."""
    t_n = h = 128
    x0, grad0, _, _ = _tol_case(torch.float32, t_n, h, 83)
    x, grad = x0.clone(), grad0.clone()
    nan, inf = float("nan"), float("inf")
    x[5, 0] = nan; x[6, h + 1] = nan; grad[7, 2] = nan
    x[8, 3] = inf; x[9, 3] = -inf; x[10, h + 4] = inf; x[11, h + 4] = -inf; grad[12, 5] = -inf; grad[13, 5] = inf
    x[0:64:3, 6] = -100.0; x[1:64:3, 6] = 100.0
    grad[:, 7] = 1e-40
    grad[:, 8] = 0.0
    grad[:, 9] = 0.0; grad[3, 9] = nan
    x, grad = x.to(dtype), grad.to(dtype)
    g7 = grad[:, 7].float().cpu()
    assert (g7 != 0).all().item() and (g7.abs() < 1.2e-38).all().item()      # still subnormal in the input type
    (qt, sft), _ = _run(dga, x, grad, rowwise=True, ue8m0=ue8m0)
    _run(dga, x, grad, ue8m0=ue8m0)
    gq, gsf = _u8(qt), sft.cpu().numpy()
    for c in (8, h + 8, 9, h + 9):
        assert gsf[c, 0] == 1.0, c
    assert not (gq[8] & 0x7F).any() and not (gq[h + 8] & 0x7F).any()
    for c in (9, h + 9):
        assert (gq[c, 3] & 0x7F) == 0x7F and not (np.delete(gq[c], 3) & 0x7F).any(), c
    # NaN in gate or grad reaches both halves, NaN in up dgate alone
    for tok, c, both in ((5, 0, True), (6, 1, False), (7, 2, True)):
        assert (gq[c, tok] & 0x7F) == 0x7F and ((gq[h + c, tok] & 0x7F) == 0x7F) == both, (tok, c)
    # gate = -100: both gradients are below every e4m3 step of their block
    assert not (gq[6, 0:64:3] & 0x7F).any() and not (gq[h + 6, 0:64:3] & 0x7F).any()


# ---- 6. misaligned pointers

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_misaligned_pointers(dga, dtype):
    """A shape that allows the 16- and 8-byte accesses, (300, 384), on pointers that do not: x and grad_h one element, dqt 2 bytes and dq 1
    byte into their buffers.  The same bytes as on aligned tensors, and nothing outside the slices is written."""
    t_n, h = 300, 384
    x0, grad0, _, _ = _tol_case(dtype, t_n, h, 89)
    xb = torch.empty(t_n * 2 * h + 8, dtype=dtype, device="cuda")
    gb = torch.empty(t_n * h + 8, dtype=dtype, device="cuda")
    x, grad = xb[1:1 + t_n * 2 * h].view(t_n, 2 * h), gb[1:1 + t_n * h].view(t_n, h)
    x.copy_(x0); grad.copy_(grad0)
    n = 2 * h * t_n
    qtb = torch.full((n + 8,), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    qb = torch.full((n + 8,), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    qt, q = qtb[2:2 + n].view(2 * h, t_n), qb[1:1 + n].view(t_n, 2 * h)
    assert x.data_ptr() % 16 and grad.data_ptr() % 16 and qt.data_ptr() % 8 == 2 and q.data_ptr() % 8 == 1
    _, sft = _sentinels((1,), (2 * h, 3))
    _, sf = _sentinels((1,), (t_n, 2 * h // 128))
    dga.silu_and_mul_backward_per_token_cast_to_fp8_transposed(x, grad, rowwise=True, out=((qt, sft), (q, sf)), sync=True)
    (aqt, asft), (aq, asf) = _run(dga, x0, grad0, rowwise=True)                                    # the aligned call, itself checked
    assert torch.equal(aqt.view(torch.uint8), qt) and torch.equal(aq.view(torch.uint8), q)
    assert torch.equal(asft.view(torch.int32), sft.view(torch.int32)) and torch.equal(asf.view(torch.int32), sf.view(torch.int32))
    for b, lo in ((qtb, 2), (qb, 1)):
        assert (b[:lo] == SENTINEL_Q).all().item() and (b[lo + n:] == SENTINEL_Q).all().item(), "bytes outside the slice were written"


# ---- in the pipeline

def test_graph_capture_follows_masked_m(dga):
    """One call with masked_m, rowwise and out= is the whole graph.  masked_m is rewritten in place; one replay gives the composition under
    the new counts, and the row-wise output the existing entry's on the valid rows with the sentinels elsewhere."""
    g_n, mmax, h = 4, 40, 128
    x, grad, _, _ = _tol_case(torch.bfloat16, g_n * mmax, h, 97)
    x, grad = x.view(g_n, mmax, 2 * h), grad.view(g_n, mmax, h)
    masked = torch.tensor([40, 0, 3, 17], dtype=torch.int32, device="cuda")
    t_n = g_n * mmax
    buf, sft = _sentinels((2 * h, t_n), (2 * h, 2))
    q, sf = _sentinels((g_n, mmax, 2 * h), (g_n, mmax, 2))
    call = lambda: dga.silu_and_mul_backward_per_token_cast_to_fp8_transposed(x, grad, masked_m=masked, rowwise=True, out=((buf, sft), (q, sf)))
    call(); torch.cuda.synchronize()                       # eager once: the library is loaded
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    torch.cuda.synchronize()
    counts = [1, 40, 25, 0]
    valid = np.concatenate([np.arange(mmax) < c for c in counts])
    masked.copy_(torch.tensor(counts, dtype=torch.int32, device="cuda"))
    for t in (buf, q):
        t.fill_(SENTINEL_Q)
    sft.view(torch.int32).fill_(SENTINEL_SF); sf.view(torch.int32).fill_(SENTINEL_SF)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    (wqt, wsft), _ = _composed(dga, x, grad, masked_m=masked)
    _same(buf.cpu().numpy(), sft.cpu().numpy(), _u8(wqt), wsft.cpu().numpy(), "replay")
    fq, fsf = _sentinels((g_n, mmax, 2 * h), (g_n, mmax, 2))
    dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, masked_m=masked, out=(fq, fsf), sync=True)
    gq, gsf = q.cpu().numpy().reshape(t_n, -1), sf.cpu().numpy().reshape(t_n, -1)
    _same(gq[valid], gsf[valid], fq.cpu().numpy().reshape(t_n, -1)[valid], fsf.cpu().numpy().reshape(t_n, -1)[valid], "replay, row-wise")
    assert (gq[~valid] == SENTINEL_Q).all() and (gsf[~valid].view(np.uint32) == SENTINEL_SF).all()


def test_into_the_k_grouped_wgrad_gemm(dga, oracle):
    """The step test's geometry (tests/test_moe_mlp_step_gpu.py: D = 384, H = 256, experts with [200, 0, 77, 1] tokens, contiguous layout), on
    the Y1 and grad_h its step produced: k_grouped_wgrad_gemm_fp8_fp8_fp32_nt takes (dqt, dsft) as returned and gives the dW1 bits of the
    composed operand.  The relative Frobenius error of dW1 against the float64 step is printed, not asserted, for the fused operand and for
    the step's B3 + B6 pair (which quantises the bf16 dY1): the lines profiles/moe_mlp_step_error.txt holds."""
    import moe_mlp_ref as R
    from test_moe_mlp_step_gpu import _run as _step_run
    lay, case, inp, b, _, hb = _step_run(dga, "contiguous", False)
    mask = lay.mask(inp["counts"])
    dqt, dsft = dga.silu_and_mul_backward_per_token_cast_to_fp8_transposed(b["y1"], b["grad_h"], **mask)
    assert tuple(dqt.shape) == (2 * R.H, lay.t_n) and tuple(dsft.shape) == (2 * R.H, lay.t_n // 128)
    (wqt, wsft), _ = _composed(dga, b["y1"], b["grad_h"], **mask)
    _same(_u8(dqt), dsft.cpu().numpy(), _u8(wqt), wsft.cpu().numpy(), "operand")
    assert not _u8(dqt)[:, ~lay.valid].any()
    xt = (b["xt_q"], b["xt_sf"])
    dw1 = torch.full((R.G, 2 * R.H, R.D), float("nan"), dtype=torch.float32, device="cuda")
    dw1_c = torch.full_like(dw1, float("nan"))
    dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt((dqt, dsft), xt, dw1, lay.ks)
    dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt((wqt, wsft), xt, dw1_c, lay.ks, sync=True)
    assert torch.equal(dw1.view(torch.int32), dw1_c.view(torch.int32)) and bool(torch.isfinite(dw1).all())
    got = dw1.cpu().numpy()
    assert got[0].any() and not got[case["tokens"].index(0)].any()
    exact = R.step_exact(case)["dW1"]
    print(f"moe_mlp_step_error: dW1, fused silu_and_mul_backward_per_token_cast_to_fp8_transposed operand (fp32 dY1) "
          f"{R.rel_error(got.astype(np.float64), exact):12.7f}")
    print(f"moe_mlp_step_error: dW1, B3 grad_x_out + B6 per_token_cast_to_fp8_transposed pair (bf16 dY1)             "
          f"{R.rel_error(hb['dw1'].astype(np.float64), exact):12.7f}")
