"""GPU: sparse_mla_fwd_fp8 and mla_kv_cast_to_fp8_paged.  The attention's contract is a composition -- sparse_mla_fwd_fp8(q, cache, ...) is
sparse_mla_fwd(q, deq(cache), ...) byte for byte, NaN in exactly the same elements -- so its tests compare the two kernels' outputs as bits,
deq from tests/sparse_mla_fp8_ref.py (numpy, a 256-entry table), into outputs pre-filled with a NaN pattern.  One test involves no other
kernel: with one valid position the weight is exactly 1 and out is the selected row's dequantised bits, for every finite code under every
scale.  Then the composition at every head count on random data (the cache written by the new writer), under peaked and negated scales and
over 64 tiles; NaN and inf in a selected row; every unselected row and every padding byte 0xFF; the cache shapes and the ends of the
addressing; the writer against per_token_cast_to_fp8 and the bytes it must not touch; two runs and one captured graph of writer ->
attention."""
import numpy as np
import pytest
import torch

import sparse_mla_fp8_ref as F
import sparse_mla_ref as R
from sparse_mla_support import _bf16, _deq_tensor, _filled, _nan16, _nan32, _view, _written_by_the_writer

pytestmark = pytest.mark.gpu

SCALE4 = R.SCALE4
FINITE_SCALES = (1.0, 0.3, 2.0 ** -140, 2.0 ** 120, 0.0, -1.5)          # the finite ones of test_sparse_mla_fp8.py's list


# ---- helpers ----------------------------------------------------------------------------------------------------------------------

def _call(fn, q, kv, idx, scale, offsets=None):
    """(out bits uint16, lse bits uint32) of one call into pre-filled outputs"""
    out, lse = _filled(q.shape[0], q.shape[1])
    got = fn(q, kv, idx, scale, 512, offsets, out=out, lse=lse, sync=True)
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == lse.data_ptr()
    return out.view(torch.int16).cpu().numpy().view(np.uint16), lse.cpu().numpy().view(np.uint32)


def _same(got, want):
    """byte for byte wherever `want` is not NaN, NaN in exactly the same elements; returns the number of NaN elements"""
    (o, l), (wo, wl) = got, want
    assert np.array_equal(_nan16(o), _nan16(wo)) and np.array_equal(_nan32(l), _nan32(wl))
    assert np.array_equal(o[~_nan16(wo)], wo[~_nan16(wo)]) and np.array_equal(l[~_nan32(wl)], wl[~_nan32(wl)])
    return int(_nan16(wo).sum()) + int(_nan32(wl).sum())


def _composed(dga, q, buf, page, idx, scale, offsets=None, idx_d=None):
    """both sides of the contract on a host buffer: (fp8 kernel on the cache, bf16 kernel on its dequantised rows)"""
    t = torch.from_numpy(buf).cuda()
    idx_d = torch.from_numpy(np.ascontiguousarray(idx)).cuda() if idx_d is None else idx_d
    off_d = None if offsets is None else torch.from_numpy(offsets).cuda()
    got = _call(dga.sparse_mla_fwd_fp8, q, _view(t, page), idx_d, scale, off_d)
    want = _call(dga.sparse_mla_fwd, q, _deq_tensor(buf, page), idx_d, scale, off_d)
    return got, want


def _random_rows(s, seed, finite=True):
    """(codes, scales, rope_bits) of s rows: any finite code, scales of both signs over a few binades, rope values normal samples"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (s, F.LATENT)).astype(np.uint8)
    if finite:
        codes[(codes & 0x7F) == 0x7F] = 0x3C
    scales = (rng.choice([-1.0, 1.0], (s, F.GROUPS)) * 2.0 ** rng.uniform(-9, -5, (s, F.GROUPS))).astype(np.float32)
    rope = F.bf16_bits(rng.standard_normal((s, F.ROPE)).astype(np.float32))
    return codes, scales, rope


_CASES = {}


def _case(dga, name, h):
    """(q on the device, the written cache as a host buffer [11 or 33, 64 x 656 + 48], indices, S of the cache) of sparse_mla_ref's cases"""
    if (name, h) not in _CASES:
        q, kv, idx = R.random_case(h) if name == "random" else R.long_case(h)
        buf = _written_by_the_writer(dga, kv, 64, 48)
        idx = idx.copy()
        idx[idx >= kv.shape[0]] = buf.shape[0] * 64 + 3               # the positions beyond S stay beyond the cache's whole blocks
        _CASES[(name, h)] = (_bf16(q), buf, idx)
    return _CASES[(name, h)]


# ---- 1. every code and scale, exact, no other kernel involved -----------------------------------------------------------------------

def test_every_code_under_every_scale_is_its_dequantised_bits(dga):
    """topk = 1 and q = 0: the weight of the one valid position is exactly 1 and lse is 0, so out[m, h, :] is deq[row, :512] -- but for
    the sign of a zero: the products are summed from +0 on the matrix pipe, and +0 + -0 is +0 (the bf16 kernel returns +0 for a -0 in
    its cache alike).  Row i holds the codes 128 (i % 2) .. in each of its four groups, group g under scale (i // 2 + g) % 6 of the finite
    scales; a NaN code and a product that is not finite in bf16 (2^120 times 2 and more) are replaced by code 0."""
    h, rows = 16, 12
    codes = np.stack([np.tile((np.arange(128) + 128 * (i % 2)).astype(np.uint8), 4) for i in range(rows)])
    scales = np.array([[FINITE_SCALES[(i // 2 + g) % 6] for g in range(4)] for i in range(rows)], np.float32)
    rope = np.zeros((rows, F.ROPE), np.uint16)
    bad = ~np.isfinite(F.bits_to_f32(F.deq_bits(codes, scales, rope)[:, :F.LATENT]))
    assert bad.any()                                                    # the NaN codes and the overflowing products
    codes[bad] = 0
    want = F.deq_bits(codes, scales, rope)[:, :F.LATENT]
    assert np.isfinite(F.bits_to_f32(want)).all()
    seen = {(int(c), float(s)) for i in range(rows) for g in range(4) for c, s in zip(codes[i, 128 * g:128 * g + 128], [scales[i, g]] * 128)}
    for sc in FINITE_SCALES:                                            # all 254 finite codes under every scale (2^120: those that stay finite)
        have = {c for c, s in seen if s == np.float32(sc)}
        assert len(have) == 254 if sc != 2.0 ** 120 else len(have) >= 200, (sc, len(have))
    assert ((want & 0x7F80) == 0).sum() > 400 and (want == 0x8000).any()                  # subnormal results and negative zeros among them
    buf = F.pack(codes, scales, rope, 4, 4 * F.ROW + 32)
    idx = np.arange(rows, dtype=np.int32)[:, None]
    q = torch.zeros((rows, h, R.D_QK), dtype=torch.bfloat16, device="cuda")
    out, lse = _call(dga.sparse_mla_fwd_fp8, q, _view(torch.from_numpy(buf).cuda(), 4), torch.from_numpy(idx).cuda(), 0.25)
    plus = np.where(want == 0x8000, 0, want).astype(np.uint16)
    assert np.array_equal(out, np.broadcast_to(plus[:, None, :], (rows, h, F.LATENT)))
    assert (lse == 0).all()


def test_rope_values_reach_the_scores_as_stored(dga):
    """q is zero but for small integers in the rope columns, the rope values are small integers, topk = 1: the score is their exact dot
    product times sm_scale = 2^-3 and lse is that score.  The kernel forms it as (dot fl32(sm_scale log2 e)) ln 2 in float32, which is
    the value asserted on the bits (a product with log2 e and one with ln 2 are not the identity in float32, so 'dot sm_scale exactly'
    would ask for other arithmetic than sparse_mla_fwd's); it is within 2^-22 of dot sm_scale.  out is the latent part's bits."""
    h, rows, scale = 16, 6, 2.0 ** -3
    rng = np.random.default_rng(3)
    codes, scales, _ = _random_rows(rows, 4)
    scales = np.abs(scales)
    codes[codes == 0x80] = 0                                             # (no -0: see the test above)
    rope_v = rng.integers(-8, 9, (rows, F.ROPE)).astype(np.float32)
    rope_v[:, 0] = np.arange(1, rows + 1)                                # no two rows alike
    qv = np.zeros((rows, h, R.D_QK), np.float32)
    qv[:, :, F.LATENT:] = rng.integers(-4, 5, (rows, h, F.ROPE))
    buf = F.pack(codes, scales, F.bf16_bits(rope_v), 1, F.ROW + 16)
    idx = np.arange(rows, dtype=np.int32)[::-1].copy()[:, None]
    out, lse = _call(dga.sparse_mla_fwd_fp8, _bf16(qv), _view(torch.from_numpy(buf).cuda(), 1), torch.from_numpy(idx).cuda(), scale)
    dot = np.einsum("mhd,md->mh", qv[:, :, F.LATENT:], rope_v[idx[:, 0]]).astype(np.float32)
    assert len(np.unique(dot)) > 20
    want = (dot * np.float32(scale * 1.4426950408889634)) * np.float32(0.693147180559945309)
    assert np.array_equal(lse, want.astype(np.float32).view(np.uint32))
    assert (np.abs(lse.view(np.float32).astype(np.float64) - dot.astype(np.float64) * scale) <= 2.0 ** -22 * np.abs(dot) * scale).all()
    deq = F.deq_bits(codes, scales, F.bf16_bits(rope_v))[idx[:, 0], :F.LATENT]
    assert np.array_equal(out, np.broadcast_to(deq[:, None, :], (rows, h, F.LATENT)))


# ---- 2. composition ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", R.ALL_HEADS)
def test_composition_on_random_data_at_every_head_count(dga, h):
    q, buf, idx = _case(dga, "random", h)
    assert buf.shape == (11, 64 * F.ROW + 48)
    rows, valid = R.rows_of(idx, buf.shape[0] * 64)
    assert valid.sum(axis=1).tolist() == [318, 298, 318, 318, 318] and (idx == -1).any() and (idx >= 704).any() and idx[2, 40] == idx[2, 41]
    got, want = _composed(dga, q, buf, 64, idx, SCALE4)
    assert _same(got, want) == 0
    # and what it is a composition of is attention over the written rows: the outputs are within the bf16 kernel's bound of the reference
    kv = F.deq(*F.unpack(buf, 64))
    ref = R.reference(q.float().cpu().numpy(), kv, idx, SCALE4)
    out = F.bits_to_f32(got[0]).astype(np.float64)
    assert (np.abs(out - ref["out"]) <= R.bound_out(ref, SCALE4, idx.shape[1])).all()
    assert (np.abs(got[1].view(np.float32) - ref["lse"]) <= R.bound_lse(ref, SCALE4, idx.shape[1])).all()


@pytest.mark.parametrize("sign", (1, -1), ids=("plus", "minus"))
@pytest.mark.parametrize("h", R.PEAK_HEADS)
def test_composition_under_peaked_and_negated_scales(dga, h, sign):
    q, buf, idx = _case(dga, "random", h)
    assert _same(*_composed(dga, q, buf, 64, idx, sign * R.PEAK * SCALE4)) == 0


def test_composition_over_64_tiles(dga):
    q, buf, idx = _case(dga, "long", 128)
    assert idx.shape == (2, 2048) and buf.shape[0] == 33
    assert _same(*_composed(dga, q, buf, 64, idx, SCALE4)) == 0


# ---- 3. NaN and inf ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ("NaN code", "NaN scale", "inf scale", "NaN rope value"))
def test_nan_and_inf_in_a_selected_row(dga, what):
    h = 64
    q, buf, idx = _case(dga, "random", h)
    idx = idx.copy()
    row = int(idx[0, 5])
    idx[2, 100] = row                                                   # tokens 0 and 2 select the row ...
    for t in (1, 3, 4):
        idx[t][idx[t] == row] = (row + 1) % R.S4                        # ... the others do not
    clean = _composed(dga, q, buf, 64, idx, SCALE4)
    assert _same(*clean) == 0
    bad = buf.copy()
    at = int(F.row_at(row, 64, buf.shape[1]))
    flat = bad.reshape(-1)
    if what == "NaN code":
        flat[at + 300] = 0xFF
    elif what == "NaN scale":
        flat[at + F.SCALES_AT + 4:at + F.SCALES_AT + 8] = np.array([np.nan], np.float32).view(np.uint8)
    elif what == "inf scale":
        flat[at + F.SCALES_AT + 8:at + F.SCALES_AT + 12] = np.array([np.inf], np.float32).view(np.uint8)
    else:
        flat[at + F.ROPE_AT + 2 * 17:at + F.ROPE_AT + 2 * 17 + 2] = np.array([0x7FC1], np.uint16).view(np.uint8)
    got, want = _composed(dga, q, bad, 64, idx, SCALE4)
    assert _same(got, want) > 0                                         # NaN where the composition has it, and nowhere else
    hit = np.zeros(R.M4, bool)
    hit[[0, 2]] = True
    assert _nan16(got[0][hit]).any() and _nan32(got[1][hit]).all()      # the row's tokens are poisoned through their scores ...
    assert np.array_equal(got[0][~hit], clean[0][0][~hit]) and np.array_equal(got[1][~hit], clean[0][1][~hit])   # ... the others not by a bit


# ---- 4. nothing else is read ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", (16, 80))
def test_no_unselected_row_and_no_padding_byte_is_read(dga, h):
    s, page, pad = 40, 8, 64
    idx, off, want_rows = R.extremes_case(s)
    keep = sorted(set(sum(want_rows, [])))
    assert len(keep) < s // 2
    codes, scales, rope = _random_rows(s, 21)
    stride = page * F.ROW + pad
    clean = F.pack(codes, scales, rope, page, stride, fill=0)
    mask = F.row_bytes_mask(keep, s // page, page, stride)
    dirty = np.where(mask, clean, 0xFF).astype(np.uint8)                 # every unselected row and every byte between blocks
    assert (dirty[:, page * F.ROW:] == 0xFF).all() and (~mask).sum() == clean.size - len(keep) * F.ROW
    zero = torch.zeros((5, h, R.D_QK), dtype=torch.bfloat16, device="cuda")
    a = _call(dga.sparse_mla_fwd_fp8, zero, _view(torch.from_numpy(clean).cuda(), page), torch.from_numpy(idx).cuda(), 0.25, torch.from_numpy(off).cuda())
    b = _call(dga.sparse_mla_fwd_fp8, zero, _view(torch.from_numpy(dirty).cuda(), page), torch.from_numpy(idx).cuda(), 0.25, torch.from_numpy(off).cuda())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not _nan16(b[0]).any() and not _nan32(b[1]).any()
    got, want = _composed(dga, zero, dirty, page, idx, 0.25, off)      # (the bf16 side reads NaN rows nowhere either)
    assert _same(got, want) == 0 and np.array_equal(got[0], b[0])
    counts = [len(w) for w in want_rows]
    assert counts == [4, 0, 0, 8, 2]
    lse = b[1].view(np.float32)
    for t, n in enumerate(counts):
        if n == 0:
            assert (b[0][t] == 0).all() and np.isneginf(lse[t]).all()   # the empty token: +0 and -inf
        else:
            assert np.allclose(lse[t], np.log(n), rtol=1e-6)
    # under scores that differ as well: the selected rows alone decide
    q = _bf16(np.random.default_rng(h).integers(-2, 3, size=(5, h, R.D_QK)).astype(np.float32) / 8)
    assert _same(*_composed(dga, q, dirty, page, idx, 0.25, off)) == 0


# ---- 5. geometry ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", (16, 80))
@pytest.mark.parametrize("layout", ("flat, padded rows", "page 16", "one row", "page 64, last row of the last block", "page 3"))
def test_cache_shapes_and_the_ends_of_the_addressing(dga, layout, h):
    s, page, pad = {"flat, padded rows": (50, 1, 48), "page 16": (48, 16, 16), "one row": (1, 1, 0),
                    "page 64, last row of the last block": (192, 64, 0), "page 3": (21, 3, 16)}[layout]
    topk, m = 70, 3
    rng = np.random.default_rng(len(layout) + h)
    codes, scales, rope = _random_rows(s, 30 + s)
    buf = F.pack(codes, scales, rope, page, page * F.ROW + pad, fill=0xFF)
    idx = np.full((m, topk), -1, np.int32)
    idx[0, 41] = s - 1                                                  # one valid position, in the second tile: the last row of the last block
    idx[1, 3:67] = rng.integers(0, s, 64)
    idx[1, 3], idx[1, 66] = s - 1, 0
    idx[1, [0, 1, 67, 68]] = [s, 2 ** 31 - 1, -2 ** 31, s + 1]
    idx[2, ::2] = s                                                      # nothing valid
    q = _bf16(rng.integers(-2, 3, size=(m, h, R.D_QK)).astype(np.float32) / 8)
    got, want = _composed(dga, q, buf, page, idx, 0.25)
    assert _same(got, want) == 0
    assert (got[0][2] == 0).all() and np.isneginf(got[1].view(np.float32)[2]).all() and np.isfinite(got[1].view(np.float32)[:2]).all()
    # indices as a column slice of a wider tensor, and as [M, 1, topk]: the same bytes
    wide = torch.from_numpy(np.concatenate([idx, np.zeros((m, 9), np.int32)], axis=1)).cuda()[:, :topk]
    assert wide.stride(0) == topk + 9
    t = torch.from_numpy(buf).cuda()
    for idx_d in (wide, torch.from_numpy(idx).cuda().view(m, 1, topk)):
        again = _call(dga.sparse_mla_fwd_fp8, q, _view(t, page), idx_d, 0.25)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    if page == 1 and pad == 0:                                          # the four-dimensional form of a flat cache
        again = _call(dga.sparse_mla_fwd_fp8, q, t.view(s, 1, 1, F.ROW), torch.from_numpy(idx).cuda(), 0.25)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    # M == 0: nothing to launch, empty outputs
    none = dga.sparse_mla_fwd_fp8(q[:0], _view(t, page), wide[:0], 0.25, sync=True)
    assert none[0].shape == (0, h, R.D_V) and none[1].shape == (0, h)


# ---- 6. the writer -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ("plain", "ue8m0, column slices"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16, torch.float16), ids=("fp32", "bf16", "fp16"))
def test_the_writer_against_per_token_cast_and_the_bytes_it_leaves(dga, dtype, variant):
    t_n, page, nb, pad = 37, 16, 5, 32                                  # 37 tokens: no multiple of the 4 a workgroup takes
    ue8m0 = variant != "plain"
    g = torch.Generator(device="cpu").manual_seed(t_n + ue8m0)
    x = (torch.randn((t_n, 640), generator=g) * 3).to(dtype)
    x[3, 7], x[5, :128] = 0.0, 0.0                                       # a zero, an all-zero block (scale 1)
    if dtype == torch.bfloat16:                                         # bf16 rope values are copied as they are: NaN payloads, -0, inf
        x.view(torch.int16)[2, 512:516] = torch.tensor([0x7FC1, -0x7FFF - 1, 0x7F80, -0x0040], dtype=torch.int16)
    x = x.cuda()
    if ue8m0:
        kv_c, k_pe = x[:, :512], x[:, 512:576]                          # column slices of one [T, 640] tensor
        assert kv_c.stride(0) == 640 == k_pe.stride(0)
    else:
        kv_c, k_pe = x[:, :512].contiguous(), x[:, 512:576].contiguous()
    s = nb * page
    rng = np.random.default_rng(t_n)
    slots = rng.permutation(np.arange(1, s - 1))[:t_n].astype(np.int64)
    slots[[4, 11, 30]] = [-1, s, -2 ** 63]                               # skipped: padding, one beyond the cache, the most negative
    slots[0], slots[36] = s - 1, 0                                      # the last row of the last block, the first row
    assert len(set(slots.tolist())) == t_n
    stride = page * F.ROW + pad
    before = np.random.default_rng(9).integers(0, 256, (nb, stride)).astype(np.uint8)      # a byte pattern
    cache = torch.from_numpy(before).cuda()
    ret = dga.mla_kv_cast_to_fp8_paged(kv_c, k_pe, _view(cache, page), torch.from_numpy(slots).cuda(), use_ue8m0=ue8m0, sync=True)
    assert ret.data_ptr() == cache.data_ptr()
    after = cache.cpu().numpy()
    kept = [t for t in range(t_n) if t not in (4, 11, 30)]
    mask = F.row_bytes_mask(slots[kept], nb, page, stride)
    assert np.array_equal(after[~mask], before[~mask])                  # every byte outside the written rows is unchanged
    codes, scales, rope = F.unpack(after, page)
    wq, wsf = dga.per_token_cast_to_fp8(kv_c.contiguous(), use_ue8m0=ue8m0)
    wq, wsf = wq.view(torch.uint8).cpu().numpy(), wsf.cpu().numpy()
    assert np.array_equal(codes[slots[kept]], wq[kept]) and np.array_equal(scales[slots[kept]].view(np.uint32), wsf[kept].view(np.uint32))
    want_rope = k_pe.to(torch.bfloat16).contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    if dtype != torch.bfloat16:
        assert np.array_equal(want_rope, F.bf16_bits(k_pe.float().cpu().numpy()))      # torch's rounding is the reference's
    assert np.array_equal(rope[slots[kept]], want_rope[kept])
    if ue8m0:
        assert ((scales[slots[kept]].view(np.uint32) & 0x007FFFFF) == 0).all()          # powers of two
    # the whole buffer against the reference writer on the device's quantiser
    quant = lambda a, ue8m0=False: tuple(r.view(torch.uint8).cpu().numpy() if r.dtype != torch.float32 else r.cpu().numpy()
                                         for r in dga.per_token_cast_to_fp8(torch.from_numpy(a).cuda(), use_ue8m0=ue8m0))
    want = F.written(before, kv_c.float().cpu().numpy(), want_rope, slots, page, quant, ue8m0)
    assert np.array_equal(after, want)
    # T == 0: nothing to launch
    assert dga.mla_kv_cast_to_fp8_paged(kv_c[:0], k_pe[:0], _view(cache, page), torch.from_numpy(slots[:0]).cuda(), sync=True) is not None
    assert np.array_equal(cache.cpu().numpy(), after)


def test_the_writer_into_a_flat_cache(dga):
    t_n, s = 9, 20
    g = torch.Generator(device="cpu").manual_seed(2)
    kv_c, k_pe = torch.randn((t_n, 512), generator=g).half().cuda(), torch.randn((t_n, 64), generator=g).half().cuda()
    slots = np.array([19, 0, 7, -1, 3, 20, 11, 12, 1], np.int64)
    before = np.full((s, F.ROW + 16), 0xA5, np.uint8)
    cache = torch.from_numpy(before).cuda()
    dga.mla_kv_cast_to_fp8_paged(kv_c, k_pe, cache[:, :F.ROW], torch.from_numpy(slots).cuda(), sync=True)
    quant = lambda a, ue8m0=False: tuple(r.view(torch.uint8).cpu().numpy() if r.dtype != torch.float32 else r.cpu().numpy()
                                         for r in dga.per_token_cast_to_fp8(torch.from_numpy(a).cuda(), use_ue8m0=ue8m0))
    want = F.written(before, kv_c.float().cpu().numpy(), F.bf16_bits(k_pe.float().cpu().numpy()), slots, 1, quant)
    assert np.array_equal(cache.cpu().numpy(), want) and (want[:, F.ROW:] == 0xA5).all() and (want[[2, 4, 5]] == 0xA5).all()


# ---- 7. determinism and capture ---------------------------------------------------------------------------------------------------------

def test_two_runs_alike_and_a_captured_graph_follows_new_operands(dga):
    h, page, nb = 64, 64, 11
    q, kv, idx = R.random_case(h)
    s = R.S4
    both = _bf16(kv)
    kv_c, k_pe = both[:, :F.LATENT].contiguous(), both[:, F.LATENT:].contiguous()
    cache = torch.zeros((nb, page * F.ROW + 48), dtype=torch.uint8, device="cuda")
    slots = torch.arange(s, dtype=torch.int64, device="cuda")
    q_d, idx_d = _bf16(q), torch.from_numpy(idx.copy()).cuda()
    off_d = torch.zeros(R.M4, dtype=torch.int32, device="cuda")
    out, lse = _filled(R.M4, h)

    def layer():
        dga.mla_kv_cast_to_fp8_paged(kv_c, k_pe, _view(cache, page), slots)
        dga.sparse_mla_fwd_fp8(q_d, _view(cache, page), idx_d, SCALE4, 512, off_d, out=out, lse=lse)

    def eager():
        cache.zero_()
        fill = _filled(R.M4, h)
        out.copy_(fill[0]); lse.copy_(fill[1])
        layer()
        torch.cuda.synchronize()
        return out.view(torch.int16).cpu().numpy().copy(), lse.view(torch.int32).cpu().numpy().copy(), cache.cpu().numpy().copy()

    a, b = eager(), eager()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))              # two runs, the same bytes
    assert not _nan16(a[0].view(np.uint16)).any()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        layer()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        layer()
    # everything overwritten in place: other rows in other slots, other lists, offsets that push some positions out, another q
    g = torch.Generator(device="cpu").manual_seed(5)
    kv_c.copy_(torch.randn(kv_c.shape, generator=g).to(torch.bfloat16))
    k_pe.copy_(torch.randn(k_pe.shape, generator=g).to(torch.bfloat16))
    q_d.copy_(torch.randn(q_d.shape, generator=g).to(torch.bfloat16))
    slots.copy_(torch.from_numpy(np.random.default_rng(6).permutation(nb * page)[:s].astype(np.int64)))
    idx_d.copy_(torch.from_numpy(R.ordered(q, kv, idx, "descending")).cuda().roll(1, 0))
    off_d.copy_(torch.tensor([0, 400, -300, 7, 0], dtype=torch.int32))
    want = eager()
    cache.zero_()
    fill = _filled(R.M4, h)
    out.copy_(fill[0]); lse.copy_(fill[1])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = out.view(torch.int16).cpu().numpy(), lse.view(torch.int32).cpu().numpy(), cache.cpu().numpy()
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    assert not np.array_equal(got[0], a[0]) and not _nan16(got[0].view(np.uint16)).any()
    # and the replayed result is the composition on the cache the replay wrote
    ref = _call(dga.sparse_mla_fwd, q_d, _deq_tensor(got[2], page), idx_d, SCALE4, off_d)
    assert _same((got[0].view(np.uint16), got[1].view(np.uint32)), ref) == 0
