"""GPU: per_block_cast_to_fp8_transposed against its one definition -- per group oracle.quant_128x128 of w[g]^T, and of w[g] for the row-wise
output -- and against per_block_cast_to_fp8 on the same slices.  Scales are compared as uint32 and codes as bytes: there is no tolerance
anywhere (the GEMM test compares bf16 bits of two runs).  Every output goes through out=, pre-filled with 0xA5 codes and 0x7FC0A5A5 scales,
so an element the kernel leaves unwritten shows; the sentinel bytes around misaligned outputs show a write outside them.
tests/test_block_cast_transposed.py states on the oracle alone that the two halves of the definition are transposes of each other."""
import numpy as np
import pytest
import torch

import block_cast_cases as B

pytestmark = pytest.mark.gpu

SENTINEL_Q, SENTINEL_SF = 0xA5, 0x7FC0A5A5


def _same(gq, gsf, wq, wsf, x, what):
    gsf, wsf = np.ascontiguousarray(gsf, np.float32), np.ascontiguousarray(wsf, np.float32)
    assert gsf.shape == wsf.shape and gq.shape == wq.shape, (what, gsf.shape, wsf.shape, gq.shape, wq.shape)
    assert not (gsf.view(np.uint32) == SENTINEL_SF).any(), f"{what}: a scale was not written"
    sbad = np.nonzero(gsf.view(np.uint32) != wsf.view(np.uint32))
    assert sbad[0].size == 0, f"{what}: {sbad[0].size} scales differ, first at {[int(i[0]) for i in sbad]}: " \
                              f"{gsf.view(np.uint32)[sbad][0]:#x} vs {wsf.view(np.uint32)[sbad][0]:#x}"
    bad = np.nonzero(gq != wq)
    assert bad[0].size == 0, f"{what}: {bad[0].size} of {gq.size} codes differ, first at {[int(i[0]) for i in bad]}: " \
                             f"{gq[bad][0]:#x} vs {wq[bad][0]:#x} for w={x[bad][0]!r}"


def _sentinels(shape_q, shape_sf):
    return (torch.full(shape_q, SENTINEL_Q, dtype=torch.uint8, device="cuda"),
            torch.full(shape_sf, SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32))


def _out_shapes(shape):
    lead, (n, k) = tuple(shape[:-2]), shape[-2:]
    nb, kb = (n + 127) // 128, (k + 127) // 128
    return (lead + (k, n), lead + (kb, nb)), (lead + (n, k), lead + (nb, kb))


def _run(dga, oracle, w_t, rowwise=False, ue8m0=False, existing=True):
    """One call into sentinel-filled out= tensors, compared with the definition and (existing) with per_block_cast_to_fp8 slice by slice.
    Returns the device outputs, nested as the entry returns them."""
    ts, rs = _out_shapes(tuple(w_t.shape))
    qt, sft = _sentinels(*ts)
    out = (qt, sft)
    if rowwise:
        q, sf = _sentinels(*rs)
        out = (out, (q, sf))
    res = dga.per_block_cast_to_fp8_transposed(w_t, rowwise=rowwise, use_ue8m0=ue8m0, out=out, sync=True)
    rt = res[0] if rowwise else res
    assert rt[0].dtype == torch.float8_e4m3fn and rt[0].data_ptr() == qt.data_ptr() and rt[1] is sft and tuple(rt[0].shape) == ts[0]
    w = w_t.float().cpu().numpy()
    (wqt, wsft), (wq, wsf) = B.reference(oracle, w, ue8m0)
    _same(qt.cpu().numpy(), sft.cpu().numpy(), wqt, wsft, np.swapaxes(w, -1, -2), "transposed")
    if rowwise:
        assert res[1][0].dtype == torch.float8_e4m3fn and res[1][0].data_ptr() == q.data_ptr() and res[1][1] is sf
        _same(q.cpu().numpy(), sf.cpu().numpy(), wq, wsf, w, "row-wise")
    if existing:
        w3 = w_t.reshape((-1,) + tuple(w_t.shape[-2:]))
        for g in range(w3.shape[0]):
            eq, esf = dga.per_block_cast_to_fp8(w3[g].t().contiguous(), use_ue8m0=ue8m0)
            _same(qt.reshape((-1,) + ts[0][-2:])[g].cpu().numpy(), sft.reshape((-1,) + ts[1][-2:])[g].cpu().numpy(),
                  eq.view(torch.uint8).cpu().numpy(), esf.cpu().numpy(), w3[g].float().cpu().numpy().T, f"transposed against per_block_cast_to_fp8, group {g}")
            if rowwise:
                eq, esf = dga.per_block_cast_to_fp8(w3[g], use_ue8m0=ue8m0)
                _same(q.reshape((-1,) + rs[0][-2:])[g].cpu().numpy(), sf.reshape((-1,) + rs[1][-2:])[g].cpu().numpy(),
                      eq.view(torch.uint8).cpu().numpy(), esf.cpu().numpy(), w3[g].float().cpu().numpy(), f"row-wise against per_block_cast_to_fp8, group {g}")
    return res


def _randn(shape, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, device="cuda", generator=g) * 3.0).to(dtype)


DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
ROWWISE = pytest.mark.parametrize("rowwise", [False, True], ids=["transposed", "rowwise"])
UE8M0 = pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])


@DTYPES
@ROWWISE
@UE8M0
@pytest.mark.parametrize("shape", B.SHAPES + [B.SHAPE_2D], ids=lambda s: "x".join(map(str, s)))
def test_shapes(dga, oracle, shape, ue8m0, rowwise, dtype):
    res = _run(dga, oracle, _randn(shape, dtype, sum(shape) * 7 + rowwise), rowwise=rowwise, ue8m0=ue8m0)
    if ue8m0:
        bits = (res[0] if rowwise else res)[1].view(torch.int32)
        assert bool(((bits & 0x007FFFFF) == 0).all()) and bool((bits > 0).all()), "a scale is not a power of two"


def test_without_out_and_the_two_forms_agree(dga, oracle):
    """Without out= the results are new float8_e4m3fn / float32 tensors with the same contents; (qt, sft) does not depend on rowwise; the 2-D
    form is the grouped form of one group."""
    w = _randn((3, 200, 136), torch.bfloat16, 3)
    (qt, sft), (q, sf) = _run(dga, oracle, w, rowwise=True)
    qt0, sft0 = _run(dga, oracle, w)
    (qt1, sft1), (q1, sf1) = dga.per_block_cast_to_fp8_transposed(w, rowwise=True, sync=True)
    qt2, sft2 = dga.per_block_cast_to_fp8_transposed(w[1], sync=True)
    for t in (qt1, q1, qt2):
        assert t.dtype == torch.float8_e4m3fn and t.is_contiguous()
    b = lambda t: t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t.view(torch.int32)
    for got, want in ((qt0, qt), (sft0, sft), (qt1, qt), (sft1, sft), (q1, q), (sf1, sf), (qt2, qt[1]), (sft2, sft[1])):
        assert got.shape == want.shape and torch.equal(b(got), b(want))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_misaligned_pointers(dga, oracle, dtype):
    """A shape that allows the 16- and 8-byte accesses, (3, 200, 136), on pointers that do not: w one element (fp32: 4-byte aligned, not
    16) into a buffer and still contiguous, qt 3 bytes and q 1 byte into theirs.  The same bytes as on aligned tensors, none outside."""
    g, n, k = 3, 200, 136
    w0 = _randn((g, n, k), dtype, 23)
    wb = torch.empty(g * n * k + 8, dtype=dtype, device="cuda")
    w = wb[1:1 + g * n * k].view(g, n, k)
    w.copy_(w0)
    qtb = torch.full((g * n * k + 8,), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    qb = torch.full((g * n * k + 8,), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    qt, q = qtb[3:3 + g * n * k].view(g, k, n), qb[1:1 + g * n * k].view(g, n, k)
    assert w.is_contiguous() and w.data_ptr() % 16 and w.data_ptr() % w.element_size() == 0 and qt.data_ptr() % 8 and q.data_ptr() % 8
    _, sft = _sentinels((1,), (g, 2, 2))
    _, sf = _sentinels((1,), (g, 2, 2))
    dga.per_block_cast_to_fp8_transposed(w, rowwise=True, out=((qt, sft), (q, sf)), sync=True)
    wn = w0.float().cpu().numpy()
    (wqt, wsft), (wq, wsf) = B.reference(oracle, wn)
    _same(qt.cpu().numpy(), sft.cpu().numpy(), wqt, wsft, np.swapaxes(wn, -1, -2), "transposed")
    _same(q.cpu().numpy(), sf.cpu().numpy(), wq, wsf, wn, "row-wise")
    for b, lo in ((qtb, 3), (qb, 1)):
        assert (b[:lo] == SENTINEL_Q).all().item() and (b[lo + g * n * k:] == SENTINEL_Q).all().item(), "bytes outside the slice were written"


# ---- special values

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@UE8M0
def test_special_values(dga, oracle, ue8m0, dtype):
    """block_cast_cases.special_values (bf16: rounded to it, where fp32 max becomes +Inf and the signalling NaNs quiet ones): NaN, +-Inf,
    -0 and subnormals in interior and edge tiles, an all-zero tile, a NaN-only tile, a tile whose only non-zero is fp32 max -- against the
    oracle and against per_block_cast_to_fp8, byte for byte."""
    w = torch.from_numpy(B.special_values()).cuda().to(dtype)
    (qt, sft), (q, sf) = _run(dga, oracle, w, rowwise=True, ue8m0=ue8m0)
    q8 = q.view(torch.uint8)
    assert sf[2, 0, 0].item() == 1.0 and sf[2, 0, 1].item() == 1.0 and not (q8[2, :128, :128] & 0x7F).any().item()
    assert torch.isinf(sf[1, 0, 0]).item() and q8[1, 3, 4].item() == 0x7F and q8[1, 199, 135].item() == 0xFF
    assert q8[2, 100, 133].item() & 0x7F == 0x7F          # (the sign of a NaN that was rounded to bf16 is the conversion's business)
    assert q8[0, 0, 0].item() == 0x7F and q8[0, 1, 1].item() == 0x80 and q8[3, 7, 7].item() == 0x7F
    if dtype == torch.float32:
        assert q8[2, 131, 66].item() == (0x78 if ue8m0 else 0x7E) and np.isfinite(sf[2, 1, 0].item()) and q8[2, 100, 133].item() == 0xFF
    _run(dga, oracle, w, ue8m0=ue8m0)


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_signalling_nans_of_the_16_bit_types(dga, oracle, kind):
    """16-bit signalling NaNs of both signs at the end of a lane's, a wave's and the workgroup's reduction order, and a tile whose only
    non-zero is one: the maximum ignores them all (scale 1 for that tile), the codes are sign | 0x7F."""
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[kind]
    snan = {"bf16": 0x7F81, "fp16": 0x7D01}[kind]
    bits = _randn((2, 130, 136), dtype, 17).view(torch.int16).cpu().numpy().view(np.uint16).copy()
    for i, (r, c) in enumerate(((7, 7), (31, 127), (32, 0), (127, 127), (129, 135), (128, 0), (0, 135))):
        bits[0, r, c] = snan | (0x8000 if i % 2 else 0)
    bits[1, 128:, :128] = 0
    bits[1, 129, 5] = snan | 0x8000
    w = torch.from_numpy(bits.view(np.int16)).cuda().view(dtype)
    (qt, sft), (q, sf) = _run(dga, oracle, w, rowwise=True)
    q8 = q.view(torch.uint8)
    assert q8[0, 7, 7].item() == 0x7F and q8[0, 31, 127].item() == 0xFF and q8[1, 129, 5].item() == 0xFF
    assert sf[1, 1, 0].item() == 1.0 and np.isfinite(sf.cpu().numpy()).all() and torch.count_nonzero(q8[1, 128:, :128]).item() == 1


# ---- the tile maximum in every lane, pass and column slot

def test_amax_in_every_lane_pass_and_slot(dga, oracle):
    """block_cast_cases.amax_positions as one [256, 128, 128] grouped call: a lane, a cross-lane move or a wave that the reduction drops
    gives the scale of max / 3."""
    w = B.amax_positions()
    (qt, sft), (q, sf) = _run(dga, oracle, torch.from_numpy(w).cuda(), rowwise=True, existing=False)
    want = (np.abs(w).max(axis=(1, 2)) / np.float32(448.0)).astype(np.float32)
    assert np.array_equal(sft.cpu().numpy().reshape(256).view(np.uint32), want.view(np.uint32))
    assert np.isin(qt.view(torch.uint8).cpu().numpy(), (0x7E, 0xFE)).sum() == 256          # one +-448 per tile


# ---- rounding ties

@UE8M0
def test_rounding_ties(dga, oracle, ue8m0):
    """64 tie tiles (cast_cases.tie_tiles through tiles_to_matrix, scale exponents inside and at both ends of quant8's fast path) as one 2-D
    [1024, 1024] call: both outputs against the oracle."""
    _run(dga, oracle, torch.from_numpy(B.tie_matrix()).cuda(), rowwise=True, ue8m0=ue8m0, existing=False)


# ---- handed to the GEMMs

def test_handed_to_the_masked_grouped_gemm(dga, oracle):
    """The weights of tests/test_moe_mlp_step_gpu.py (G = 4, D = 384, H = 256): one call each on W1 [G, 2H, D] and W2 [G, D, H] with
    rowwise=True gives the four tensors its _inputs builds in a per-expert loop, and m_grouped_gemm_fp8_fp8_bf16_nt_masked with strict=True
    gives the same bf16 bits on them, taken as they are, as on the stacked ones -- fprop on (q, sf), dgrad on (qt, sft)."""
    import moe_mlp_ref as R
    import test_moe_mlp_step_gpu as S
    case = R.make_case(0)
    lay = S.Layout("masked", case["tokens"])
    inp = S._inputs(dga, lay, case)
    mine = {}
    for name, key in (("w1", "W1"), ("w2", "W2")):
        w = torch.from_numpy(np.stack(case[key]).astype(np.float32)).cuda()
        ts, rs = _out_shapes(tuple(w.shape))
        out = (_sentinels(*ts), _sentinels(*rs))
        mine[name + "t"], mine[name] = dga.per_block_cast_to_fp8_transposed(w, rowwise=True, out=out, sync=True)
    for name in ("w1", "w2", "w1t", "w2t"):
        (gq, gsf), (wq, wsf) = mine[name], inp[name]
        assert gq.shape == wq.shape and gsf.shape == wsf.shape, name
        assert torch.equal(gq.view(torch.uint8), wq.view(torch.uint8)) and torch.equal(gsf.view(torch.int32), wsf.view(torch.int32)), name
    counts = inp["counts"]
    gen = torch.Generator(device="cuda").manual_seed(5)
    for name, kdim, ndim in (("w1", R.D, 2 * R.H), ("w2", R.H, R.D), ("w1t", 2 * R.H, R.D), ("w2t", R.D, R.H)):
        x = torch.randn((R.G * R.MMAX, kdim), device="cuda", generator=gen).bfloat16()
        xq, xsf = dga.per_token_cast_to_fp8(x)
        lhs = (xq.view(R.G, R.MMAX, kdim), xsf.view(R.G, R.MMAX, -1))
        outs = []
        for rhs in (mine[name], inp[name]):
            o = torch.zeros((R.G, R.MMAX, ndim), dtype=torch.bfloat16, device="cuda")
            dga.m_grouped_gemm_fp8_fp8_bf16_nt_masked(lhs, rhs, o, counts, R.MMAX, strict=True, sync=True)
            outs.append(o.view(torch.int16))
        assert torch.equal(outs[0], outs[1]), name
        assert outs[0][0, :case["tokens"][0]].any().item()


def test_the_flat_form_into_the_dense_gemm(dga, oracle):
    """The 2-D results as the rhs of gemm_fp8_fp8_bf16_nt: strict=True is the oracle's fp32 chain on those bytes."""
    m, n, k = 70, 200, 136
    w = _randn((n, k), torch.bfloat16, 9)
    (qt, sft), (q, sf) = _run(dga, oracle, w, rowwise=True)
    for rhs, kk, nn in (((q, sf), k, n), ((qt, sft), n, k)):
        xq, xsf = dga.per_token_cast_to_fp8(_randn((m, kk), torch.bfloat16, kk))
        out = torch.zeros((m, nn), dtype=torch.bfloat16, device="cuda")
        dga.gemm_fp8_fp8_bf16_nt((xq, xsf), rhs, out, strict=True, sync=True)
        want = oracle.gemm_fp8_fp8_bf16_nt(xq.view(torch.uint8).cpu().numpy(), xsf.cpu().numpy(), rhs[0].view(torch.uint8).cpu().numpy(),
                                           rhs[1].cpu().numpy(), threads=4)
        assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), want)


# ---- in the pipeline

def test_graph_capture(dga, oracle):
    """One call with rowwise=True and out= captured on a side stream after an eager warm-up on it; w is overwritten in place, one replay
    gives the result of the new values."""
    shape = (3, 200, 136)
    w = _randn(shape, torch.bfloat16, 51)
    ts, rs = _out_shapes(shape)
    (qt, sft), (q, sf) = _sentinels(*ts), _sentinels(*rs)
    call = lambda: dga.per_block_cast_to_fp8_transposed(w, rowwise=True, out=((qt, sft), (q, sf)))
    call(); torch.cuda.synchronize()                       # eager once: the library is loaded
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    torch.cuda.synchronize()
    w.copy_(_randn(shape, torch.bfloat16, 52))
    for t in (qt, q):
        t.fill_(SENTINEL_Q)
    sft.view(torch.int32).fill_(SENTINEL_SF); sf.view(torch.int32).fill_(SENTINEL_SF)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in (qt, sft, q, sf)]
    (eqt, esft), (eq, esf) = _run(dga, oracle, w, rowwise=True, existing=False)        # an eager call on the new values, itself checked
    for g, e in zip(got, (eqt, esft, eq, esf)):
        assert torch.equal(g.view(torch.uint8), e.view(torch.uint8))


def test_pybind_matches_the_python_entry(dga):
    from deepgemm_ascend_amd import deep_gemm_cpp
    for shape in ((3, 200, 136), (130, 257)):
        w = _randn(shape, torch.bfloat16, 61)
        qt, sft = dga.per_block_cast_to_fp8_transposed(w, sync=True)
        pq, psf = deep_gemm_cpp.per_block_cast_to_fp8_transposed(w)
        torch.cuda.synchronize()
        assert pq.dtype == torch.float8_e4m3fn and pq.shape == qt.shape and psf.shape == sft.shape
        assert torch.equal(pq.view(torch.uint8), qt.view(torch.uint8)) and torch.equal(psf.view(torch.int32), sft.view(torch.int32))
