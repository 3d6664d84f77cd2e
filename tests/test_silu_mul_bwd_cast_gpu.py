"""GPU: silu_and_mul_backward_per_token_cast_to_fp8 = per_token_cast_to_fp8([dgate | dup]) with both gradients kept in fp32,
dgate = d u silu'(g), dup = d silu(g) for g = x[..., :H], u = x[..., H:], d = grad_h.

Exact family: for gate >= 20 sigmoid and silu' are exactly 1 in fp32, so codes and scales equal the oracle's quantiser on
[fl32(d u) | fl32(d g)] byte for byte and grad_x_out is the RNE of those values, in every row layout; excluded rows keep their sentinels.
Tolerance family: for |gate| <= 16 the fp32 gradients are within the two element bounds of DESIGN.md ("Fused SiLU-and-multiply backward
quantiser") of a float64 reference; scales and codes are bounded from that.  Then the edges, the operator between two masked GEMMs under
graph capture, and the pybind module.

The worst error ratios (error over the bound's magnitude; the bounds are 2^-17 and 2^-18) are printed before they are asserted; an fp32
emulation with correctly rounded exponential and reciprocal gives 2^-22.1 for both."""
import functools

import numpy as np
import pytest
import torch

from fused_bounds import EPS_GATE, EPS_UP, _e4m3_rne_satfinite, _reference    # (moved there unchanged: the expert-MLP step test shares them)

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SENTINEL_Q = 0xA5
SENTINEL_SF = 0x7FC0A5A5            # a NaN pattern the kernel never writes (its scales are positive and finite)
MASKS = [0, 24, 1, 17]
M_INDICES = [0] * 10 + [-1] * 6 + [1] * 13 + [-1] * 3 + [2] * 7 + [-1] * 1      # 40 rows, three segments with -1 tails


def _u8(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _sentinels(lead, h, dtype):
    """(dq, dsf, grad_x_out) prefilled: 0xA5 bytes in dq and grad_x_out, SENTINEL_SF in dsf."""
    q = torch.full(lead + (2 * h,), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sf = torch.full(lead + (2 * h // 128,), SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    gx = torch.empty(lead + (2 * h,), dtype=dtype, device="cuda")
    gx.view(torch.uint8).fill_(SENTINEL_Q)
    return q, sf, gx


@functools.lru_cache(maxsize=None)
def _exact_case(lead, h, dtype, seed):
    """gate uniform in [20, 60], up N(0, 3^2), grad N(0, 0.5^2), each rounded to the input type; x = [gate | up].  Returns the device
    inputs and, on the host with the rows flattened, fl32([d u | d g]) and its RNE to the input type as bytes.  Computed once per case."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    gate = (torch.rand(lead + (h,), device="cuda", generator=g) * 40.0 + 20.0).to(dtype).clamp(20.0, 60.0)
    up = (torch.randn(lead + (h,), device="cuda", generator=g) * 3.0).to(dtype)
    grad = (torch.randn(lead + (h,), device="cuda", generator=g) * 0.5).to(dtype).contiguous()
    x = torch.cat([gate, up], dim=-1).contiguous()
    f = lambda t: t.float().cpu().numpy().reshape(-1, h)
    gf, uf, df = f(gate), f(up), f(grad)
    want = np.concatenate([df * uf, df * gf], axis=1).astype(np.float32)          # one fp32 rounding per product
    want.setflags(write=False)
    want_gx = _u8(torch.from_numpy(want.copy()).to(dtype))                        # torch's conversion rounds to nearest even
    return x, grad, want, want_gx


@functools.lru_cache(maxsize=None)
def _exact_want(oracle, lead, h, dtype, seed, ue8m0):
    return oracle.quant_1x128(_exact_case(lead, h, dtype, seed)[2], ue8m0=ue8m0)


def _assert_rows_exact(gq, gsf, wq, wsf, rows):
    assert (gsf[rows].view(np.uint32) == wsf[rows].view(np.uint32)).all(), "scales differ"
    bad = np.nonzero(gq[rows] != wq[rows])
    assert bad[0].size == 0, f"{bad[0].size} codes differ, first at row {rows[bad[0][0]]}, column {bad[1][0]}"


# (2048, 2048): the launcher has no size-dependent path (one kernel, one 16-lane group per column block); the issue's "large"
FLAT = [(3, 128), (64, 512), (130, 1024), (2048, 2048)]


@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("rows,h", FLAT)
def test_exact_flat(dga, oracle, rows, h, dtype, ue8m0):
    x, grad, _, want_gx = _exact_case((rows,), h, dtype, rows * 7 + h)
    gx = torch.empty_like(x)
    q, sf = dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, grad_x_out=gx, use_ue8m0=ue8m0, sync=True)
    assert q.dtype == torch.float8_e4m3fn and tuple(q.shape) == (rows, 2 * h) and tuple(sf.shape) == (rows, 2 * h // 128)
    wq, wsf = _exact_want(oracle, (rows,), h, dtype, rows * 7 + h, ue8m0)
    _assert_rows_exact(_u8(q), sf.cpu().numpy(), wq, wsf, np.arange(rows))
    assert (_u8(gx) == want_gx).all(), "grad_x_out is not the RNE of the fp32 gradient"
    q2, sf2 = dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, use_ue8m0=ue8m0, sync=True)     # without grad_x_out: the same bytes
    assert torch.equal(q2.view(torch.uint8), q.view(torch.uint8)) and torch.equal(sf2.view(torch.int32), sf.view(torch.int32))


def _assert_untouched(gq, gsf, ggx, rest):
    assert (gq[rest] == SENTINEL_Q).all(), "an excluded row of dq was written"
    assert (gsf[rest].view(np.uint32) == SENTINEL_SF).all(), "an excluded row of dsf was written"
    assert (ggx[rest] == SENTINEL_Q).all(), "an excluded row of grad_x_out was written"


@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_exact_masked(dga, oracle, dtype, ue8m0):
    """Valid rows exact; every masked row of dq, dsf and grad_x_out still holds the sentinel bytewise."""
    G, mmax, h = 4, 24, 256
    x, grad, _, want_gx = _exact_case((G, mmax), h, dtype, 11)
    masked = torch.tensor(MASKS, dtype=torch.int32, device="cuda")
    q, sf, gx = _sentinels((G, mmax), h, dtype)
    rq, rsf = dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, masked_m=masked, out=(q, sf), grad_x_out=gx, use_ue8m0=ue8m0,
                                                              sync=True)
    assert rq.dtype == torch.float8_e4m3fn and rq.data_ptr() == q.data_ptr() and rsf is sf
    wq, wsf = _exact_want(oracle, (G, mmax), h, dtype, 11, ue8m0)
    gq, gsf, ggx = _u8(q).reshape(G * mmax, -1), sf.cpu().numpy().reshape(G * mmax, -1), _u8(gx).reshape(G * mmax, -1)
    valid = np.concatenate([np.arange(MASKS[g]) + g * mmax for g in range(G)]).astype(np.int64)
    _assert_rows_exact(gq, gsf, wq, wsf, valid)
    assert (ggx[valid] == want_gx[valid]).all()
    rest = np.setdiff1d(np.arange(G * mmax), valid)
    assert rest.size == G * mmax - sum(MASKS)
    _assert_untouched(gq, gsf, ggx, rest)


@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_exact_contiguous(dga, oracle, dtype, ue8m0):
    rows, h = 40, 384
    assert len(M_INDICES) == rows
    x, grad, _, want_gx = _exact_case((rows,), h, dtype, 13)
    idx = torch.tensor(M_INDICES, dtype=torch.int32, device="cuda")
    q, sf, gx = _sentinels((rows,), h, dtype)
    dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, m_indices=idx, out=(q.view(torch.float8_e4m3fn), sf), grad_x_out=gx,
                                                    use_ue8m0=ue8m0, sync=True)
    wq, wsf = _exact_want(oracle, (rows,), h, dtype, 13, ue8m0)
    gq, gsf, ggx = _u8(q), sf.cpu().numpy(), _u8(gx)
    valid = np.nonzero(np.array(M_INDICES) >= 0)[0]
    rest = np.nonzero(np.array(M_INDICES) < 0)[0]
    _assert_rows_exact(gq, gsf, wq, wsf, valid)
    assert (ggx[valid] == want_gx[valid]).all()
    _assert_untouched(gq, gsf, ggx, rest)


def _carved(shape, dtype, like=None):
    """A contiguous tensor of `shape` that starts one element into a flat allocation of two elements more, every byte 0xA5 (or a copy of
    `like`), and that allocation."""
    n = int(np.prod(shape))
    flat = torch.empty(n + 2, dtype=dtype, device="cuda")
    flat.view(torch.uint8).fill_(SENTINEL_Q)
    t = flat[1:n + 1].view(shape)
    if like is not None:
        t.copy_(like)
    return t, flat


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("rows,h", [(3, 128), (17, 256)])
def test_misaligned_pointers(dga, oracle, rows, h, dtype):
    """x, grad_h and grad_x_out one element, dq one byte into their allocations: the kernel's element-by-element loads and stores.  dq, dsf
    and grad_x_out equal bit for bit what the same values give through aligned tensors (which are the oracle's, as in test_exact_flat), and
    the element in front of and behind each carved output keeps its bytes."""
    x, grad, _, want_gx = _exact_case((rows,), h, dtype, rows * 7 + h)
    gx = torch.empty_like(x)
    q, sf = dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, grad_x_out=gx, sync=True)
    wq, wsf = _exact_want(oracle, (rows,), h, dtype, rows * 7 + h, False)
    _assert_rows_exact(_u8(q), sf.cpu().numpy(), wq, wsf, np.arange(rows))
    assert (_u8(gx) == want_gx).all(), "grad_x_out is not the RNE of the fp32 gradient"
    (mx, _), (mgrad, _) = _carved(x.shape, dtype, x), _carved(grad.shape, dtype, grad)
    (mgx, gx_flat), (mq, q_flat) = _carved(x.shape, dtype), _carved((rows, 2 * h), torch.uint8)
    assert all(t.data_ptr() % 16 == t.element_size() for t in (mx, mgrad, mgx)) and mq.data_ptr() % 8 == 1
    msf = torch.empty((rows, 2 * h // 128), dtype=torch.float32, device="cuda")
    rq, rsf = dga.silu_and_mul_backward_per_token_cast_to_fp8(mx, mgrad, out=(mq, msf), grad_x_out=mgx, sync=True)
    assert rq.data_ptr() == mq.data_ptr() and rsf is msf
    assert torch.equal(mq, q.view(torch.uint8)), "dq differs from the aligned call's"
    assert torch.equal(msf.view(torch.int32), sf.view(torch.int32)), "dsf differs from the aligned call's"
    assert (_u8(mgx) == _u8(gx)).all(), "grad_x_out differs from the aligned call's"
    for flat in (gx_flat, q_flat):
        ends = _u8(flat[[0, -1]])
        assert (ends == SENTINEL_Q).all(), "an element outside the carved tensor was written"


def test_h_not_a_multiple_of_128_is_refused_on_the_device_too(dga):
    x = torch.zeros((4, 384), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(dga.DGAError, match="H a multiple of 128"):
        dga.silu_and_mul_backward_per_token_cast_to_fp8(x, torch.zeros((4, 192), dtype=torch.bfloat16, device="cuda"))


# ---- tolerance family

@functools.lru_cache(maxsize=None)
def _tol_host(dtype, rows, h, seed):
    """gate N(0, 3^2) clamped to +-16, up N(0, 3^2), grad N(0, 0.5^2), rounded to the input type, from a host generator (the case is the
    same on every machine).  Returns x = [gate | up] and grad on the host and, in float64, the reference [dgate | dup] with its element
    bounds."""
    g = torch.Generator().manual_seed(seed)
    gate = (torch.randn((rows, h), generator=g) * 3.0).clamp(-16.0, 16.0).to(dtype)
    up = (torch.randn((rows, h), generator=g) * 3.0).to(dtype)
    grad = (torch.randn((rows, h), generator=g) * 0.5).to(dtype)
    ref, bound = _reference(gate, up, grad)
    return torch.cat([gate, up], dim=1).contiguous(), grad.contiguous(), ref, bound


@functools.lru_cache(maxsize=None)
def _tol_case(dtype, rows, h, seed):
    x, grad, ref, bound = _tol_host(dtype, rows, h, seed)
    return x.cuda(), grad.cuda(), ref, bound


def _check_tolerance(oracle, label, got, gq, gsf, ref, bound):
    """The tolerance family's checks on the fp32 gradient `got` (as float64), the codes gq and the scales gsf of [rows, 2H] outputs against
    the float64 reference and its element bounds; prints each figure before it asserts."""
    rows, h = ref.shape[0], ref.shape[1] // 2
    # 0. the two element bounds
    err = np.abs(got - ref)
    for name, sl, eps in (("dgate", slice(0, h), EPS_GATE), ("dup", slice(h, 2 * h), EPS_UP)):
        m = bound[:, sl] / eps                                   # the magnitude the bound is relative to
        ratio = np.divide(err[:, sl], m, out=np.zeros_like(m), where=m > 0).max()
        print(f"[{label}] {name}: worst error / magnitude 2^{np.log2(max(ratio, 1e-300)):.2f} (bound 2^{np.log2(eps):.0f})")
    assert (err <= bound).all(), f"{int((err > bound).sum())} elements outside their bound"
    # 1. scales: bit-equal to the oracle's on fl32(reference) on every decided block
    nb = 2 * h // 128
    ref32 = ref.astype(np.float32)
    wq, wsf = oracle.quant_1x128(ref32)
    a, b = np.abs(ref).reshape(rows, nb, 128), bound.reshape(rows, nb, 128)
    top = a.argmax(axis=2)[..., None]
    a_top, b_top = np.take_along_axis(a, top, 2)[..., 0], np.take_along_axis(b, top, 2)[..., 0]
    others = a + b
    np.put_along_axis(others, top, -np.inf, 2)
    decided = a_top - b_top > others.max(axis=2)
    und = int((~decided).sum())
    print(f"[{label}] scales: {und} of {decided.size} blocks undecided by the reference; "
          f"{int((gsf.view(np.uint32) != wsf.view(np.uint32)).sum())} scales differ from the oracle's on the reference")
    assert und <= 1e-3 * decided.size
    assert (gsf.view(np.uint32)[decided] == wsf.view(np.uint32)[decided]).all(), "a decided block's scale differs"
    w64 = wsf.astype(np.float64)
    assert (np.abs(gsf.astype(np.float64) - w64)[~decided] <= EPS_GATE * w64[~decided]).all()
    # 2. codes, every element: between the RNE codes of (ref -+ bound) / the device's scale
    dec = oracle.e4m3fn_table()[gq].astype(np.float64)
    s = np.repeat(gsf.astype(np.float64), 128, axis=1)
    b0, b1 = _e4m3_rne_satfinite(oracle, (ref - bound) / s), _e4m3_rne_satfinite(oracle, (ref + bound) / s)
    lo, hi = np.minimum(b0, b1), np.maximum(b0, b1)
    outside = (dec < lo) | (dec > hi) | np.isnan(dec)
    print(f"[{label}] codes: {int(outside.sum())} of {dec.size} outside [RNE((ref - bound) / s), RNE((ref + bound) / s)]; "
          f"{int((lo != hi).sum())} elements have two admissible codes")
    assert not outside.any()
    print(f"[{label}] codes that differ from the oracle's on the reference: {(gq != wq).mean():.3e}")


# bf16 at 16384 blocks (the reference alone leaves about 1e-4 of them undecided: the cap of 1e-3 needs thousands to mean anything); fp16 and
# fp32 at 4120 (an odd row count, more than one workgroup)
TOL = [(torch.bfloat16, 1024, 1024), (torch.float16, 515, 512), (torch.float32, 515, 512)]


@pytest.mark.parametrize("dtype,rows,h", TOL, ids=[f"{str(d)[6:]}-{r}x{h}" for d, r, h in TOL])
def test_tolerance(dga, oracle, dtype, rows, h):
    x, grad, ref, bound = _tol_case(dtype, rows, h, rows * 3 + h)
    gx = torch.empty_like(x)
    q, sf = dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, grad_x_out=gx, sync=True)
    # the same values as fp32 inputs: the kernel's arithmetic is fp32 after the load, so grad_x_out is then the gradient it quantised
    gx32 = torch.empty(x.shape, dtype=torch.float32, device="cuda")
    q32, sf32 = dga.silu_and_mul_backward_per_token_cast_to_fp8(x.float(), grad.float(), grad_x_out=gx32, sync=True)
    assert torch.equal(q32.view(torch.uint8), q.view(torch.uint8)) and torch.equal(sf32.view(torch.int32), sf.view(torch.int32))
    assert (_u8(gx32.to(dtype)) == _u8(gx)).all(), "grad_x_out is not the RNE of the fp32 gradient"
    _check_tolerance(oracle, f"{dtype} {rows}x{h}", gx32.cpu().numpy().astype(np.float64), _u8(q), sf.cpu().numpy(), ref, bound)


# ---- edges

def test_edge_values(dga, oracle):
    """H = 256, fp32 inputs, gate in [20, 60] elsewhere (so everything else is exact).  Row 0: an all-zero grad block -> scale 1 and codes 0
    in both halves.  Row 1: NaN in gate (block 0) and in up (block 1); row 2: NaN in grad -> NaN codes (& 0x7F == 0x7F) in both halves for
    gate and grad, in dgate alone for up; the rest of each block quantised as if the NaN were absent.  Row 3: gate = -120 and -1e4 -> zero
    codes in both halves, no NaN, neighbours untouched."""
    h = 256
    rng = np.random.default_rng(5)
    gate = rng.uniform(20.0, 60.0, (4, h)).astype(np.float32)
    up = (rng.standard_normal((4, h)) * 3.0).astype(np.float32)
    grad = (rng.standard_normal((4, h)) * 0.5).astype(np.float32)
    grad[0, :128] = 0.0
    gate[1, 5] = np.nan; up[1, 130] = np.nan; grad[2, 200] = np.nan
    gate[3, 3] = -120.0; gate[3, 200] = -1e4
    x = torch.from_numpy(np.concatenate([gate, up], axis=1)).cuda()
    gx = torch.empty_like(x)
    q, sf = dga.silu_and_mul_backward_per_token_cast_to_fp8(x, torch.from_numpy(grad).cuda(), grad_x_out=gx, sync=True)
    gq, gsf, ggx = _u8(q), sf.cpu().numpy(), gx.cpu().numpy()
    with np.errstate(invalid="ignore"):
        want = np.concatenate([grad * up, grad * gate], axis=1).astype(np.float32)
    nan_at = [(1, 5), (1, h + 5), (1, 130), (2, 200), (2, h + 200)]            # up reaches dgate only: (1, h + 130) is an ordinary element
    zero_at = [(3, 3), (3, h + 3), (3, 200), (3, h + 200)]
    for rc in nan_at + zero_at:
        want[rc] = 0.0                                                         # "as if the NaN were absent"; silu(-120), silu'(-120): 0
    assert not np.isnan(want).any()
    wq, wsf = oracle.quant_1x128(want)
    assert (gsf.view(np.uint32) == wsf.view(np.uint32)).all(), "scales differ"
    # zero codes: 0 * u keeps the product's sign, and the quantiser encodes -0 as 0x80 (the oracle does: the bytes are compared below)
    assert gsf[0, 0] == 1.0 and gsf[0, 2] == 1.0 and (gq[0, :128] & 0x7F == 0).all() and (gq[0, h:h + 128] & 0x7F == 0).all()
    keep = np.ones((4, 2 * h), bool)
    for rc in nan_at:
        assert (gq[rc] & 0x7F) == 0x7F and np.isnan(ggx[rc]), rc
        keep[rc] = False
    for rc in zero_at:
        assert (gq[rc] & 0x7F) == 0 and ggx[rc] == 0.0, rc
        keep[rc] = False
    assert (gq[keep] == wq[keep]).all()
    assert (ggx[keep] == want[keep]).all() and not np.isnan(ggx[3]).any()


# ---- in the pipeline

def test_graph_capture_of_the_backward_chain_follows_masked_m(dga, oracle):
    """One captured graph: masked GEMM -> grad_h [4, 24, 128] bf16, the operator on a fixed x -> (dq, dsf) with K = 2H = 256, a second
    masked GEMM on (dq, dsf).  masked_m is rewritten in place between replays; each replay equals the eager chain under the same counts
    bit for bit on the valid rows, and leaves the other rows of every buffer alone."""
    G, mmax, K1, H, N2 = 4, 24, 256, 128, 128
    A, SFA, W1, SF1, W2, SF2 = [], [], [], [], [], []
    for i in range(G):
        a, sfa, b, sfb = oracle.make_inputs(mmax, H, K1, seed=500 + i)
        _, _, b2, sfb2 = oracle.make_inputs(mmax, N2, 2 * H, seed=600 + i)
        A.append(a); SFA.append(sfa); W1.append(b); SF1.append(sfb); W2.append(b2); SF2.append(sfb2)
    a, sfa, w1, sf1, w2, sf2 = (torch.from_numpy(np.stack(l)).cuda() for l in (A, SFA, W1, SF1, W2, SF2))
    x = _tol_case(torch.bfloat16, G * mmax, H, 29)[0].view(G, mmax, 2 * H)
    masked = torch.tensor(MASKS, dtype=torch.int32, device="cuda")

    def buffers():
        grad_h = torch.full((G, mmax, H), 0x7FC1, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        q = torch.full((G, mmax, 2 * H), SENTINEL_Q, dtype=torch.uint8, device="cuda")
        sf = torch.full((G, mmax, 2), SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
        out = torch.full((G, mmax, N2), 0x7FC1, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        return grad_h, q, sf, out

    def chain(grad_h, q, sf, out):
        dga.m_grouped_gemm_fp8_fp8_bf16_nt_masked((a, sfa), (w1, sf1), grad_h, masked, mmax)
        dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad_h, masked_m=masked, out=(q, sf))
        dga.m_grouped_gemm_fp8_fp8_bf16_nt_masked((q, sf), (w2, sf2), out, masked, mmax)

    fresh = buffers()
    static = buffers()
    chain(*static); torch.cuda.synchronize()           # eager once: the library is loaded and every workspace exists
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain(*static)                                 # ... and the capture stream's own
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        chain(*static)
    torch.cuda.synchronize()
    for counts in (MASKS, [24, 0, 9, 2]):
        masked.copy_(torch.tensor(counts, dtype=torch.int32, device="cuda"))
        for s, f in zip(static, fresh):
            s.copy_(f)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [_u8(t).reshape(G * mmax, -1).copy() for t in static]
        eager = buffers()
        chain(*eager); torch.cuda.synchronize()
        want = [_u8(t).reshape(G * mmax, -1) for t in eager]
        sent = [_u8(t).reshape(G * mmax, -1) for t in fresh]
        valid = np.concatenate([np.arange(counts[g]) + g * mmax for g in range(G)]).astype(np.int64)
        rest = np.setdiff1d(np.arange(G * mmax), valid)
        for name, g_, w_, s_ in zip(("grad_h", "dq", "dsf", "out"), got, want, sent):
            assert (g_[valid] == w_[valid]).all(), (name, counts)
            assert (g_[rest] == s_[rest]).all(), (name, counts)
        assert got[3][valid].view(np.uint16).any() and not (got[3][valid].view(np.uint16) == 0x7FC1).any()


def test_the_pybind_entry_gives_the_same_bytes(dga):
    from deepgemm_ascend_amd import build_ext
    build_ext.build()
    from deepgemm_ascend_amd import deep_gemm_cpp as ext
    G, mmax, h = 4, 24, 256
    x, grad, _, _ = _tol_case(torch.bfloat16, G * mmax, h, 23)
    x, grad = x.view(G, mmax, 2 * h), grad.view(G, mmax, h)
    masked = torch.tensor(MASKS, dtype=torch.int32, device="cuda")
    gx = torch.zeros_like(x)
    q, sf = dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, masked_m=masked, grad_x_out=gx, sync=True)
    egx = torch.zeros_like(x)
    eq, esf = ext.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, masked_m=masked, grad_x_out=egx)
    torch.cuda.synchronize()
    assert eq.dtype == torch.float8_e4m3fn and eq.shape == q.shape and esf.shape == sf.shape
    for g in range(G):
        assert torch.equal(eq[g, :MASKS[g]].view(torch.uint8), q[g, :MASKS[g]].view(torch.uint8))
        assert torch.equal(esf[g, :MASKS[g]].view(torch.int32), sf[g, :MASKS[g]].view(torch.int32))
    assert torch.equal(egx.view(torch.int16), gx.view(torch.int16)) and bool(gx[1].any())
    fq, fsf = ext.silu_and_mul_backward_per_token_cast_to_fp8(x[1], grad[1])
    wq, wsf = dga.silu_and_mul_backward_per_token_cast_to_fp8(x[1].contiguous(), grad[1].contiguous(), sync=True)
    torch.cuda.synchronize()
    assert torch.equal(fq.view(torch.uint8), wq.view(torch.uint8)) and torch.equal(fsf.view(torch.int32), wsf.view(torch.int32))
