"""GPU: silu_and_mul_per_token_cast_to_fp8 = per_token_cast_to_fp8(silu(gate) * up) with the product kept in fp32.

Exact family: for gate >= 20 the fp32 product is fl32(gate * up) exactly (1 + exp(-g) rounds to 1), so codes and scales equal the
oracle's quantiser on that product byte for byte, in every row layout.  Tolerance family: for |gate| <= 16 the fp32 product is within
relative EPS = 2^-18 of the real-number value (DESIGN.md "Fused SiLU-and-multiply quantiser"); scales, codes and the share of codes
that differ from the oracle's are bounded from that.  Then the operator between the two masked GEMMs of an expert MLP, under graph
capture, and through the pybind module."""
import numpy as np
import pytest
import torch

from fused_bounds import EPS, _e4m3_rne_satfinite, _h_ref     # (moved there unchanged: tests/test_moe_mlp_step_gpu.py shares them)

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SENTINEL_Q = 0xA5
SENTINEL_SF = 0x7FC0A5A5            # a NaN pattern the kernel never writes (its scales are positive and finite)
MASKS = [0, 24, 1, 17]


def _u8(t):
    return t.view(torch.uint8).cpu().numpy()


def _sentinels(shape_q, shape_sf):
    q = torch.full(shape_q, SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sf = torch.full(shape_sf, SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    return q, sf


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _exact_inputs(lead, h, dtype, seed):
    """gate uniform in [20, 60], up N(0, 3^2), both rounded to the input type; x = [gate | up]."""
    g = _gen(seed)
    gate = (torch.rand(lead + (h,), device="cuda", generator=g) * 40.0 + 20.0).to(dtype)
    gate = gate.clamp(20.0, 60.0)
    up = (torch.randn(lead + (h,), device="cuda", generator=g) * 3.0).to(dtype)
    return torch.cat([gate, up], dim=-1).contiguous(), gate, up


def _exact_want(oracle, gate, up, ue8m0):
    """oracle.quant_1x128(fl32(gate * up)) on the rows flattened."""
    gf = gate.float().cpu().numpy().reshape(-1, gate.shape[-1])
    uf = up.float().cpu().numpy().reshape(-1, up.shape[-1])
    return oracle.quant_1x128((gf * uf).astype(np.float32), ue8m0=ue8m0)


def _assert_rows_exact(gq, gsf, wq, wsf, rows):
    assert (gsf[rows].view(np.uint32) == wsf[rows].view(np.uint32)).all(), "scales differ"
    bad = np.nonzero(gq[rows] != wq[rows])
    assert bad[0].size == 0, f"{bad[0].size} codes differ, first at row {rows[bad[0][0]]}, column {bad[1][0]}"


# (2048, 2048): the launcher has no size-dependent path (one kernel, one block per 16 lanes); the issue's stand-in for "large"
FLAT = [(3, 128), (64, 512), (17, 77), (130, 1000), (33, 1004), (2048, 2048)]


@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("rows,h", FLAT)
def test_exact_flat(dga, oracle, rows, h, dtype, ue8m0):
    x, gate, up = _exact_inputs((rows,), h, dtype, seed=rows * 7 + h)
    q, sf = dga.silu_and_mul_per_token_cast_to_fp8(x, use_ue8m0=ue8m0, sync=True)
    assert q.dtype == torch.float8_e4m3fn and tuple(q.shape) == (rows, h) and tuple(sf.shape) == (rows, (h + 127) // 128)
    wq, wsf = _exact_want(oracle, gate, up, ue8m0)
    _assert_rows_exact(_u8(q), sf.cpu().numpy(), wq, wsf, np.arange(rows))


@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_exact_masked(dga, oracle, dtype, ue8m0):
    """Valid rows exact; every masked row of q and sf still holds the sentinel bytewise."""
    G, mmax, h = 4, 24, 256
    x, gate, up = _exact_inputs((G, mmax), h, dtype, seed=11)
    masked = torch.tensor(MASKS, dtype=torch.int32, device="cuda")
    q, sf = _sentinels((G, mmax, h), (G, mmax, 2))
    rq, rsf = dga.silu_and_mul_per_token_cast_to_fp8(x, masked_m=masked, out=(q, sf), use_ue8m0=ue8m0, sync=True)
    assert rq.dtype == torch.float8_e4m3fn and rq.data_ptr() == q.data_ptr() and rsf is sf
    wq, wsf = _exact_want(oracle, gate, up, ue8m0)
    gq, gsf = _u8(q).reshape(G * mmax, h), sf.cpu().numpy().reshape(G * mmax, 2)
    valid = np.concatenate([np.arange(MASKS[g]) + g * mmax for g in range(G)]).astype(np.int64)
    _assert_rows_exact(gq, gsf, wq, wsf, valid)
    rest = np.setdiff1d(np.arange(G * mmax), valid)
    assert rest.size == G * mmax - sum(MASKS)
    assert (gq[rest] == SENTINEL_Q).all(), "a masked row of q was written"
    assert (gsf[rest].view(np.uint32) == SENTINEL_SF).all(), "a masked row of sf was written"


M_INDICES = [0] * 10 + [-1] * 6 + [1] * 13 + [-1] * 3 + [2] * 7 + [-1] * 1      # 40 rows, three segments with -1 tails


@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_exact_contiguous(dga, oracle, dtype, ue8m0):
    rows, h = 40, 384
    assert len(M_INDICES) == rows
    x, gate, up = _exact_inputs((rows,), h, dtype, seed=13)
    idx = torch.tensor(M_INDICES, dtype=torch.int32, device="cuda")
    q, sf = _sentinels((rows, h), (rows, 3))
    dga.silu_and_mul_per_token_cast_to_fp8(x, m_indices=idx, out=(q.view(torch.float8_e4m3fn), sf), use_ue8m0=ue8m0, sync=True)
    wq, wsf = _exact_want(oracle, gate, up, ue8m0)
    gq, gsf = _u8(q), sf.cpu().numpy()
    valid = np.nonzero(np.array(M_INDICES) >= 0)[0]
    rest = np.nonzero(np.array(M_INDICES) < 0)[0]
    _assert_rows_exact(gq, gsf, wq, wsf, valid)
    assert (gq[rest] == SENTINEL_Q).all(), "a padding row of q was written"
    assert (gsf[rest].view(np.uint32) == SENTINEL_SF).all(), "a padding row of sf was written"


def test_edge_values(dga, oracle):
    """H = 256, fp32 inputs.  Row 0: an all-zero up block -> scale 1, codes 0.  Row 1: NaN in gate (block 0) and in up (block 1) ->
    codes with & 0x7F == 0x7F, the rest of each block quantised as if the NaN were absent.  Row 2: gate = -120 and -1e4 inside
    ordinary blocks decode to 0 and leave the rest alone."""
    h = 256
    rng = np.random.default_rng(5)
    gate = rng.uniform(20.0, 60.0, (3, h)).astype(np.float32)
    up = (rng.standard_normal((3, h)) * 3.0).astype(np.float32)
    up[0, :128] = 0.0
    gate[1, 5] = np.nan; up[1, 130] = np.nan
    gate[2, 3] = -120.0; gate[2, 200] = -1e4
    x = torch.from_numpy(np.concatenate([gate, up], axis=1)).cuda()
    q, sf = dga.silu_and_mul_per_token_cast_to_fp8(x, sync=True)
    gq, gsf = _u8(q), sf.cpu().numpy()
    want_h = (gate * up).astype(np.float32)
    want_h[1, 5] = 0.0; want_h[1, 130] = 0.0            # "as if the NaN were absent"
    want_h[2, 3] = 0.0; want_h[2, 200] = 0.0            # silu(-120), silu(-1e4): below every e4m3 step of any block here
    wq, wsf = oracle.quant_1x128(want_h)
    assert (gsf.view(np.uint32) == wsf.view(np.uint32)).all(), "scales differ"
    assert gsf[0, 0] == 1.0 and (gq[0, :128] == 0).all()
    assert (gq[1, 5] & 0x7F) == 0x7F and (gq[1, 130] & 0x7F) == 0x7F
    assert (gq[2, 3] & 0x7F) == 0 and (gq[2, 200] & 0x7F) == 0
    keep = np.ones((3, h), bool)
    keep[1, 5] = keep[1, 130] = keep[2, 3] = keep[2, 200] = False
    assert (gq[keep] == wq[keep]).all()


# ---- tolerance family

def _tol_inputs(lead, h, dtype, seed):
    g = _gen(seed)
    gate = (torch.randn(lead + (h,), device="cuda", generator=g) * 3.0).clamp(-16.0, 16.0).to(dtype)
    up = (torch.randn(lead + (h,), device="cuda", generator=g) * 3.0).to(dtype)
    return torch.cat([gate, up], dim=-1).contiguous(), gate, up


def _check_tolerance(oracle, gq, gsf, href, ue8m0, rows, label):
    """Checks 1 (scales) and 2 (codes) of the tolerance family on the rows `rows` of flattened outputs, and the share of codes that
    differ from the oracle's; prints each figure before it asserts.  (Check 3 as the issue words it: test_share_off_the_oracle.)"""
    gq, gsf, href = gq[rows], gsf[rows].astype(np.float64), href[rows]
    n, h = href.shape
    hb = (h + 127) // 128
    pad = np.zeros((n, hb * 128)); pad[:, :h] = np.abs(href.astype(np.float64))
    amax = pad.reshape(n, hb, 128).max(axis=2)
    sref = np.where(amax > 0, amax / 448.0, 1.0)
    # 1. scales
    if not ue8m0:
        err = np.abs(gsf - sref) / sref
        print(f"[{label}] scales: max relative error {err.max():.3e} (bound {EPS + 2.0 ** -23:.3e})")
        assert (np.abs(gsf - sref) <= (EPS + 2.0 ** -23) * sref).all()
    else:
        mant, _ = np.frexp(gsf)
        assert (mant == 0.5).all(), "a scale is not a power of two"
        up2 = 2.0 ** np.ceil(np.log2(sref))
        near_below = sref >= up2 * (1 - EPS)                 # the device may see a value just above the power: the next one
        near_above = sref <= (up2 / 2) * (1 + EPS)           # ... or just at / below the power underneath: that one
        ok = (gsf == up2) | (near_below & (gsf == 2 * up2)) | (near_above & (gsf == up2 / 2))
        print(f"[{label}] ue8m0 scales: {int((gsf != up2).sum())} of {gsf.size} on a neighbouring power")
        assert ok.all()
    # 2. codes, every element
    dec = oracle.e4m3fn_table()[gq].astype(np.float64)
    y = href.astype(np.float64) / np.repeat(gsf, 128, axis=1)[:, :h]
    b0, b1 = _e4m3_rne_satfinite(oracle, y * (1 - 2 * EPS)), _e4m3_rne_satfinite(oracle, y * (1 + 2 * EPS))
    lo, hi = np.minimum(b0, b1), np.maximum(b0, b1)
    outside = (dec < lo) | (dec > hi) | np.isnan(dec)
    print(f"[{label}] codes: {int(outside.sum())} of {dec.size} outside [RNE(y(1-2eps)), RNE(y(1+2eps))]; "
          f"{int((lo != hi).sum())} elements have two admissible codes")
    assert not outside.any()
    # the codes alone against the oracle's on h_ref: what a relative perturbation of h_ref flips (2^-20, 2^-18, 2^-16: 1.3e-5, 1.3e-5,
    # 5.2e-5 of the codes of these inputs, each by one step); far inside the cap of the share test below
    wq, _ = oracle.quant_1x128(href, ue8m0=ue8m0)
    flips = (gq != wq).mean()
    print(f"[{label}] codes that differ from the oracle's on h_ref: {flips:.3e}")
    if href.size >= 50000:
        assert flips <= 1e-3


def _share_off_the_oracle(oracle, gq, gsf, href, ue8m0, label):
    """Check 3: the share of elements whose dequantised value (code x its own scale) differs from that of oracle.quant_1x128(h_ref),
    compared as codes where the two scales are bit-equal."""
    h = href.shape[1]
    wq, wsf = oracle.quant_1x128(href, ue8m0=ue8m0)
    tab = oracle.e4m3fn_table().astype(np.float64)
    same_scale = np.repeat(gsf.view(np.uint32) == wsf.view(np.uint32), 128, axis=1)[:, :h]
    gdec = tab[gq] * np.repeat(gsf.astype(np.float64), 128, axis=1)[:, :h]
    wdec = tab[wq] * np.repeat(wsf.astype(np.float64), 128, axis=1)[:, :h]
    differ = np.where(same_scale, gq != wq, gdec != wdec)
    print(f"[{label}] share differing from the oracle on h_ref: {differ.mean():.3e} ({(gq != wq).mean():.3e} as codes alone; "
          f"{1 - same_scale.mean():.3e} of the elements sit in blocks whose scale is not bit-equal)")
    return differ.mean()


TOL_FLAT = [(torch.bfloat16, 64, 512), (torch.bfloat16, 17, 77), (torch.bfloat16, 256, 1024), (torch.float32, 130, 1000),
            (torch.float16, 130, 1000)]


@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
@pytest.mark.parametrize("dtype,rows,h", TOL_FLAT, ids=[f"{str(d)[6:]}-{r}x{h}" for d, r, h in TOL_FLAT])
def test_tolerance_flat(dga, oracle, dtype, rows, h, ue8m0):
    x, gate, up = _tol_inputs((rows,), h, dtype, seed=rows * 3 + h)
    q, sf = dga.silu_and_mul_per_token_cast_to_fp8(x, use_ue8m0=ue8m0, sync=True)
    _check_tolerance(oracle, _u8(q), sf.cpu().numpy(), _h_ref(gate, up), ue8m0, np.arange(rows), f"{dtype} {rows}x{h} ue8m0={ue8m0}")


@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
@pytest.mark.parametrize("dtype,rows,h", [c for c in TOL_FLAT if c[1] * c[2] >= 50000],
                         ids=[f"{str(d)[6:]}-{r}x{h}" for d, r, h in TOL_FLAT if r * h >= 50000])
def test_share_off_the_oracle(dga, oracle, dtype, rows, h, ue8m0):
    """Check 3 of the tolerance family on the cases of >= 50 000 elements: at most 1e-3 of the elements may differ from
    oracle.quant_1x128(h_ref) dequantised with its own scale, compared as codes when the scales are bit-equal.  An element of a block
    whose fp32 scale is a ULP off the reference's differs whatever its code, so this holds only because the kernel rounds the block
    amax from an fp64 value of silu(g) * u (with the amax taken from the fp32 product alone 0.40 of the elements differed, all of
    them through the scale: the codes alone differ in < 4e-6)."""
    x, gate, up = _tol_inputs((rows,), h, dtype, seed=rows * 3 + h)
    q, sf = dga.silu_and_mul_per_token_cast_to_fp8(x, use_ue8m0=ue8m0, sync=True)
    share = _share_off_the_oracle(oracle, _u8(q), sf.cpu().numpy(), _h_ref(gate, up), ue8m0, f"{dtype} {rows}x{h} ue8m0={ue8m0}")
    assert share <= 1e-3


@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
def test_tolerance_masked(dga, oracle, ue8m0):
    G, mmax, h = 4, 24, 256
    x, gate, up = _tol_inputs((G, mmax), h, torch.bfloat16, seed=17)
    masked = torch.tensor(MASKS, dtype=torch.int32, device="cuda")
    q, sf = _sentinels((G, mmax, h), (G, mmax, 2))
    dga.silu_and_mul_per_token_cast_to_fp8(x, masked_m=masked, out=(q, sf), use_ue8m0=ue8m0, sync=True)
    gq, gsf = _u8(q).reshape(G * mmax, h), sf.cpu().numpy().reshape(G * mmax, 2)
    valid = np.concatenate([np.arange(MASKS[g]) + g * mmax for g in range(G)]).astype(np.int64)
    rest = np.setdiff1d(np.arange(G * mmax), valid)
    assert (gq[rest] == SENTINEL_Q).all() and (gsf[rest].view(np.uint32) == SENTINEL_SF).all()
    _check_tolerance(oracle, gq, gsf, _h_ref(gate, up), ue8m0, valid, f"masked ue8m0={ue8m0}")


# ---- in the pipeline

def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def test_between_the_two_masked_gemms(dga, oracle):
    """GEMM1 (masked) -> [G,32,512] bf16 -> the fused op -> GEMM2 (masked) on the device's (q, sf); GEMM2's output against the
    oracle's masked GEMM on those same device bytes: the layout written is the one the GEMM reads."""
    G, mmax, K, H, N2 = 4, 32, 256, 256, 128
    masks = [0, 32, 5, 17]
    masked_np = np.array(masks, np.int32)
    masked = torch.from_numpy(masked_np).cuda()
    A, SFA, W13, SF13, W2, SF2 = [], [], [], [], [], []
    for i in range(G):
        a, sfa, b, sfb = oracle.make_inputs(mmax, 2 * H, K, seed=300 + i)
        _, _, b2, sfb2 = oracle.make_inputs(mmax, N2, H, seed=400 + i)
        A.append(a); SFA.append(sfa); W13.append(b); SF13.append(sfb); W2.append(b2); SF2.append(sfb2)
    dev = lambda l: torch.from_numpy(np.stack(l)).cuda()
    gate_up = torch.zeros((G, mmax, 2 * H), dtype=torch.bfloat16, device="cuda")
    dga.m_grouped_gemm_fp8_fp8_bf16_nt_masked((dev(A), dev(SFA)), (dev(W13), dev(SF13)), gate_up, masked, expected_m=max(masks))
    q = torch.zeros((G, mmax, H), dtype=torch.uint8, device="cuda")
    sf = torch.ones((G, mmax, H // 128), dtype=torch.float32, device="cuda")
    dga.silu_and_mul_per_token_cast_to_fp8(gate_up, masked_m=masked, out=(q, sf))
    sentinel = np.uint16(0x7FC1)
    init = np.full((G, mmax, N2), sentinel, np.uint16)
    out = torch.from_numpy(init.view(np.int16)).cuda().view(torch.bfloat16)
    dga.m_grouped_gemm_fp8_fp8_bf16_nt_masked((q, sf), (dev(W2), dev(SF2)), out, masked, expected_m=max(masks), sync=True)
    hq, hsf = q.cpu().numpy(), sf.cpu().numpy()
    for g in range(G):
        assert (hq[g, masks[g]:] == 0).all() and (hsf[g, masks[g]:] == 1.0).all(), "the fused op wrote a masked row"
        assert masks[g] == 0 or hq[g, :masks[g]].any()
    w2, sf2 = np.stack(W2), np.stack(SF2)
    want = oracle.m_grouped_gemm_fp8_fp8_bf16_nt_masked(hq, hsf, w2, sf2, init, masked_np, threads=4)
    got = _bits(out)
    for g in range(G):
        mm = masks[g]
        assert (got[g, mm:] == sentinel).all()
        if mm:
            oracle.assert_parity(got[g, :mm], want[g, :mm], hq[g, :mm], hsf[g, :mm], w2[g], sf2[g])


def test_graph_capture_follows_masked_m(dga, oracle):
    """One capture of the masked call (one stream, one kernel); the counts and the sentinels are rewritten on the device between two
    replays, and the second replay writes exactly the rows of the new counts."""
    G, mmax, h = 4, 24, 256
    x, gate, up = _exact_inputs((G, mmax), h, torch.bfloat16, seed=19)
    wq, wsf = _exact_want(oracle, gate, up, False)
    masked = torch.tensor(MASKS, dtype=torch.int32, device="cuda")
    q, sf = _sentinels((G, mmax, h), (G, mmax, 2))
    dga.silu_and_mul_per_token_cast_to_fp8(x, masked_m=masked, out=(q, sf), sync=True)     # warm: the library is loaded before capture
    fresh_q, fresh_sf = _sentinels((G, mmax, h), (G, mmax, 2))
    q.copy_(fresh_q); sf.copy_(fresh_sf)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dga.silu_and_mul_per_token_cast_to_fp8(x, masked_m=masked, out=(q, sf))
    for counts in (MASKS, [24, 0, 9, 2]):
        masked.copy_(torch.tensor(counts, dtype=torch.int32, device="cuda"))
        q.copy_(fresh_q); sf.copy_(fresh_sf)
        graph.replay()
        torch.cuda.synchronize()
        gq, gsf = _u8(q).reshape(G * mmax, h), sf.cpu().numpy().reshape(G * mmax, 2)
        valid = np.concatenate([np.arange(counts[g]) + g * mmax for g in range(G)]).astype(np.int64)
        rest = np.setdiff1d(np.arange(G * mmax), valid)
        _assert_rows_exact(gq, gsf, wq, wsf, valid)
        assert (gq[rest] == SENTINEL_Q).all() and (gsf[rest].view(np.uint32) == SENTINEL_SF).all(), counts


def test_the_pybind_entry_gives_the_same_bytes(dga):
    from deepgemm_ascend_amd import build_ext
    build_ext.build()
    from deepgemm_ascend_amd import deep_gemm_cpp as ext
    G, mmax, h = 4, 24, 256
    x, _, _ = _tol_inputs((G, mmax), h, torch.bfloat16, seed=23)
    masked = torch.tensor(MASKS, dtype=torch.int32, device="cuda")
    q, sf = dga.silu_and_mul_per_token_cast_to_fp8(x, masked_m=masked, sync=True)
    eq, esf = ext.silu_and_mul_per_token_cast_to_fp8(x, masked_m=masked)
    torch.cuda.synchronize()
    assert eq.dtype == torch.float8_e4m3fn and eq.shape == q.shape and esf.shape == sf.shape
    for g in range(G):
        assert torch.equal(eq[g, :MASKS[g]].view(torch.uint8), q[g, :MASKS[g]].view(torch.uint8))
        assert torch.equal(esf[g, :MASKS[g]].view(torch.int32), sf[g, :MASKS[g]].view(torch.int32))
    fq, fsf = ext.silu_and_mul_per_token_cast_to_fp8(x[1])
    wq, wsf = dga.silu_and_mul_per_token_cast_to_fp8(x[1].contiguous(), sync=True)
    torch.cuda.synchronize()
    assert torch.equal(fq.view(torch.uint8), wq.view(torch.uint8)) and torch.equal(fsf.view(torch.int32), wsf.view(torch.int32))
