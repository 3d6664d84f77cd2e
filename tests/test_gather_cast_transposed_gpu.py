"""GPU: gather_per_token_cast_to_fp8_transposed against its definition -- per_token_cast_to_fp8_transposed on the gathered tensor torch
materialises, whole tensors compared as bytes and scale bits -- on the smallest shapes that reach every path of the kernel.

1-D index: T = 300 (three token blocks, the last partial, the middle one without a valid row), S = 50 source rows, index_div = 3, so
P = 150 pairs and every source row is read several times; H = 384 (whole tiles), 136 (a channel tail on the vector path), 100 (the bounded
path).  Index values -1, P, 2^62 and -2^63 exclude.  The source rows and the row scales no valid slot names hold NaN.  The outputs are
pre-filled with 0xA5 bytes and 0x7FC0A5A5 scales: the excluded rows of (q, sf) keep them, every element of qt and sft is written.
2-D index: G = 3, Mmax = 256, masked_m = [200, 0, 1], stale entries at and beyond masked_m[g]."""
import numpy as np
import pytest
import torch

import moe_mlp_ref as R

pytestmark = pytest.mark.gpu

T, S, DIV = 300, 50, 3
P = S * DIV
DEAD_ROWS = (7, 23, 49)                                   # source rows no valid slot names
OUTSIDE = (-1, P, 1 << 62, -(1 << 63))
SENTINEL_Q, SENTINEL_SF = 0xA5, 0x7FC0A5A5
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
_CASES = {}


def _index(seed=0):
    """int64 [T]: block 0 mostly valid, block 1 (128 .. 255) without a valid row, block 2 (44 rows) valid but for a few."""
    rng = np.random.default_rng(seed)
    live = np.array([p for p in range(P) if p // DIV not in DEAD_ROWS], np.int64)
    idx = rng.choice(live, size=T)
    idx[:DIV * 2] = np.arange(DIV * 2)                    # (source rows 0 and 1 through every pair of theirs)
    out = np.array(OUTSIDE, np.int64)
    idx[128:256] = out[np.arange(128) % 4]
    for r in (3, 17, 64, 127, 256, 280, 299):
        idx[r] = out[r % 4]
    return idx


def _case(dtype, h):
    """The device tensors of a case, once per process: src with NaN in the dead rows, the index, row scales with 0, a negative value and
    2^-20 on pairs valid slots name and NaN on the pairs none names."""
    if (dtype, h) not in _CASES:
        g = torch.Generator().manual_seed(1000 + h)
        src = torch.randn(S, h, generator=g).to(DTYPES[dtype])
        src[list(DEAD_ROWS)] = float("nan")
        if dtype == "bf16":
            src.view(torch.int16)[list(DEAD_ROWS)] = 0x7FC1
        idx = _index()
        valid = (idx >= 0) & (idx < P)
        scale = torch.randn(P, generator=g)
        named = np.zeros(P, bool)
        named[idx[valid]] = True
        scale[torch.from_numpy(~named)] = float("nan")
        first = [int(v) for v in dict.fromkeys(idx[valid].tolist())][:3]
        scale[first[0]], scale[first[1]], scale[first[2]] = 0.0, -1.5, 2.0 ** -20
        _CASES[(dtype, h)] = (src.cuda(), torch.from_numpy(idx).cuda(), scale.cuda(), valid)
    return _CASES[(dtype, h)]


def _materialise(src, idx, scale, valid):
    """xg [T, H] as torch makes it (NaN on the excluded rows: the reference must not read them either) and m_indices."""
    ok = torch.from_numpy(valid).to(src.device)
    safe = torch.where(ok, idx, torch.zeros_like(idx))
    rows = src[safe // DIV]
    xg = rows if scale is None else scale[safe][:, None] * rows.float()
    xg = torch.where(ok[:, None], xg, torch.full_like(xg, float("nan"))).contiguous()
    return xg, torch.where(ok, 0, -1).to(torch.int32)


def _filled(h, t_n, lead, ldqt=None):
    """out= pre-filled: ((qt, sft), (q, sf))."""
    ldqt = t_n if ldqt is None else ldqt
    byt = lambda *s: torch.full(s, SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sfs = lambda *s: torch.full(s, SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    return (byt(h, ldqt)[:, :t_n], sfs(h, (t_n + 127) // 128)), (byt(*lead, h), sfs(*lead, (h + 127) // 128))


def _bits(t):
    return (t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.uint8)).contiguous().cpu().numpy()


def _assert_same(got, want, valid, what):
    """((qt, sft), (q, sf)) or (qt, sft) against the reference's: qt and sft whole, (q, sf) on the valid rows, sentinels on the others."""
    rowwise = isinstance(got[0], tuple)
    (qt, sft), (wqt, wsft) = (got[0], want[0]) if rowwise else (got, want)
    assert np.array_equal(_bits(qt), _bits(wqt)), f"{what}: qt"
    assert np.array_equal(_bits(sft), _bits(wsft)), f"{what}: sft"
    if rowwise:
        (q, sf), (wq, wsf) = got[1], want[1]
        q, sf, wq, wsf = (_bits(t).reshape(valid.size, -1) for t in (q, sf, wq, wsf))
        assert np.array_equal(q[valid], wq[valid]), f"{what}: q on the valid rows"
        assert np.array_equal(sf[valid], wsf[valid]), f"{what}: sf on the valid rows"
        assert (q[~valid] == SENTINEL_Q).all() and (sf[~valid] == SENTINEL_SF).all(), f"{what}: an excluded row of (q, sf) was written"


FLAGS = [(rw, al, ue) for rw in (False, True) for al in (False, True) for ue in (False, True)]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "row_scale"])
@pytest.mark.parametrize("h", [384, 136, 100])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_the_result_is_the_transposing_quantiser_on_the_materialised_gather(dga, dtype, h, scaled):
    src, idx, scale, valid = _case(dtype, h)
    scale = scale if scaled else None
    xg, m_indices = _materialise(src, idx, scale, valid)
    assert xg.dtype == (torch.float32 if scaled else DTYPES[dtype]) and bool(torch.isnan(xg[128:256]).all())
    for rowwise, aligned, ue8m0 in FLAGS:
        what = f"rowwise={rowwise} aligned_rows={aligned} use_ue8m0={ue8m0}"
        kw = dict(rowwise=rowwise, aligned_rows=aligned, use_ue8m0=ue8m0)
        out, ref_out = (_filled(h, T, (T,), 384 if aligned else T) for _ in range(2))      # the reference writes on sentinels too
        want = dga.per_token_cast_to_fp8_transposed(xg, m_indices=m_indices, out=ref_out if rowwise else ref_out[0], **kw)
        got = dga.gather_per_token_cast_to_fp8_transposed(src, idx, index_div=DIV, row_scale=scale, out=out if rowwise else out[0], **kw)
        torch.cuda.synchronize()
        _assert_same(got, want, valid, what)
        gqt, wqt = (got[0][0], want[0][0]) if rowwise else (got[0], want[0])
        assert gqt.dtype == torch.float8_e4m3fn and tuple(gqt.shape) == (h, T) and gqt.stride(0) == (384 if aligned else T)
        assert getattr(gqt, "_dga_zero_padded", False) == aligned == getattr(wqt, "_dga_zero_padded", False), what
        if aligned:                                                          # the tails of the rows are zero
            assert tuple(out[0][0]._base.shape) == (h, 384) and not out[0][0]._base[:, T:].any(), what
        # every element of qt and sft was written: the block without a valid row is code 0 under scale 1
        assert not _bits(gqt)[:, 128:256].any() and (_bits(got[0][1] if rowwise else got[1])[:, 1] == 0x3F800000).all(), what
    # ... and without out=: the same bytes in tensors of the entry's own
    got = dga.gather_per_token_cast_to_fp8_transposed(src, idx, index_div=DIV, row_scale=scale)
    want = dga.per_token_cast_to_fp8_transposed(xg, m_indices=m_indices)
    torch.cuda.synchronize()
    _assert_same(got, want, valid, "no out=")


def test_the_identity_index_is_the_transposing_quantiser_itself(dga):
    """index_div = 1, index = arange: no row excluded, T = S = 300 and a 128-aligned T = 256."""
    for t_n in (300, 256):
        x = torch.randn(t_n, 384, generator=torch.Generator().manual_seed(t_n)).to(torch.bfloat16).cuda()
        idx = torch.arange(t_n, dtype=torch.int64, device="cuda")
        got = dga.gather_per_token_cast_to_fp8_transposed(x, idx, rowwise=True)
        want = dga.per_token_cast_to_fp8_transposed(x, rowwise=True)
        torch.cuda.synchronize()
        for a, b in zip(got[0] + got[1], want[0] + want[1]):
            assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "row_scale"])
def test_one_bf16_case_against_the_cpu_oracle(dga, oracle, scaled):
    """H = 136: the definition from the host's own gather, through moe_mlp_ref's links."""
    src, idx, scale, valid = _case("bf16", 136)
    (qt, sft), (q, sf) = dga.gather_per_token_cast_to_fp8_transposed(src, idx, index_div=DIV, row_scale=scale if scaled else None, rowwise=True)
    torch.cuda.synchronize()
    ix = idx.cpu().numpy()
    xg = np.zeros((T, 136), np.float32)
    xg[valid] = src.float().cpu().numpy()[ix[valid] // DIV]
    if scaled:
        xg[valid] = np.multiply(scale.cpu().numpy()[ix[valid]][:, None], xg[valid], dtype=np.float32)
    assert np.isfinite(xg).all()
    wqt, wsft = R.link_quant_tokens(xg, valid, oracle)
    assert np.array_equal(_bits(qt), wqt) and np.array_equal(_bits(sft), wsft.view(np.int32))
    wq, wsf = R.link_quant_rows(xg[valid], oracle)
    assert np.array_equal(_bits(q)[valid], wq) and np.array_equal(_bits(sf)[valid], wsf.view(np.int32))


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "row_scale"])
@pytest.mark.parametrize("dtype,h", [("bf16", 384), ("fp16", 136), ("fp32", 100)])
def test_the_masked_table_reads_nothing_beyond_masked_m(dga, dtype, h, scaled):
    """G = 3, Mmax = 256, masked_m = [200, 0, 1].  The entries at and beyond masked_m[g] hold 2^62 and valid-looking values that name the NaN
    rows (and NaN scales): the result equals the 1-D call on the flattened table with those entries set to -1."""
    g_n, mmax, masked = 3, 256, np.array([200, 0, 1], np.int32)
    src, _, scale, _ = _case(dtype, h)
    scale = scale if scaled else None
    rng = np.random.default_rng(5)
    live = np.array([p for p in range(P) if p // DIV not in DEAD_ROWS], np.int64)
    if scaled:                                                               # (pairs whose scale is not NaN: the ones the 1-D case names)
        live = live[~np.isnan(scale.cpu().numpy()[live])]
    table = rng.choice(live, size=(g_n, mmax))
    table[0, 5], table[0, 130] = -1, P                                       # excluded inside masked_m too
    inside = np.arange(mmax)[None, :] < masked[:, None]
    flat = np.where(inside, table, -1).reshape(-1)
    stale = np.where(rng.random((g_n, mmax)) < 0.5, 1 << 62, np.array(DEAD_ROWS, np.int64)[rng.integers(0, 3, (g_n, mmax))] * DIV)
    table = np.where(inside, table, stale)
    valid = (flat >= 0) & (flat < P)
    t_n = g_n * mmax
    kw = dict(index_div=DIV, row_scale=scale, rowwise=True)
    got = dga.gather_per_token_cast_to_fp8_transposed(src, torch.from_numpy(table).cuda(), masked_m=torch.from_numpy(masked).cuda(),
                                                      out=_filled(h, t_n, (g_n, mmax)), **kw)
    want = dga.gather_per_token_cast_to_fp8_transposed(src, torch.from_numpy(flat).cuda(), out=_filled(h, t_n, (t_n,)), **kw)
    torch.cuda.synchronize()
    assert tuple(got[1][0].shape) == (g_n, mmax, h) and tuple(got[1][1].shape) == (g_n, mmax, (h + 127) // 128)
    _assert_same(got, want, valid, "masked against flat")
    assert not np.isnan(_bits(got[0][1]).view(np.float32)).any() and not (_bits(got[0][0]) == 0x7F).any()     # no NaN row was read
    assert not _bits(got[0][0])[:, 256:512].any()                             # expert 1 is empty: codes 0
