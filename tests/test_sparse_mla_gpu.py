"""GPU: sparse_mla_fwd against tests/sparse_mla_ref.py, into outputs pre-filled with a NaN pattern.  TILE = 32 positions is the kernel's
gathered tile; a workgroup owns 64 heads (one wave per 16), so Hq = 16 leaves three waves that only gather, 64 fills one workgroup and 128
takes two.  With q = 0 every weight is 1 and, on small-integer kv with a power-of-two number of valid positions, out is
RNE_bf16(sum v / count) bit for bit: gather, masking and duplicates are checked with no tolerance.  One key that outscores the rest by 256
gives its value row bit for bit wherever it stands in the list.  Every kind of invalid position, the offsets, a strided kv whose every
unselected row and every column >= 576 is NaN, and an index list that is a slice of a wider tensor go through the same check; normal
samples in three orders of the list stay inside the derived bound on every element; a NaN poisons what selects it and nothing else; a
captured graph follows rewritten operands; two calls give the same bytes.  The uniform, random-data and two-runs tests run at every
multiple of 16 heads up to 128, and so does a case in which every head of every token has a winning row of its own, which tells a head in
the wrong lane group, wave or block apart exactly.  The derived bound is also held on peaked and on negated scores (four times the scale,
plus and minus, in the three orders) and over 64 tiles; a zero scale gives the bits of q = 0; a cache of one row and indices and offsets
at the ends of the int32 range are exact under q = 0."""
import numpy as np
import pytest
import torch

import sparse_mla_ref as R
from sparse_mla_support import _bf16, _check, _filled

pytestmark = pytest.mark.gpu

HEADS = (16, 64, 128)                                                 # one wave of a workgroup, a whole workgroup, two
ALL_HEADS = R.ALL_HEADS                                               # and every count between: a partly filled first or second block
def _run(dga, q, kv, idx, scale, offsets=None):
    """(out as float64, its bits, lse float32) of one call into pre-filled outputs"""
    out, lse = _filled(q.shape[0], q.shape[1])
    got = dga.sparse_mla_fwd(q, kv, idx, scale, 512, offsets, out=out, lse=lse, sync=True)
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == lse.data_ptr()
    bits = out.view(torch.int16).cpu().numpy().view(np.uint16)
    return out.float().cpu().numpy().astype(np.float64), bits, lse.cpu().numpy()


def _int_kv(s, width, seed, keep=None):
    """small-integer kv [s, width] (|v| <= 8, as float32), NaN in the columns >= 576 and, given keep, in every row outside it"""
    rng = np.random.default_rng(seed)
    kv = rng.integers(-8, 9, size=(s, width)).astype(np.float32)
    kv[:, R.D_QK:] = np.nan
    if keep is not None:
        gone = np.ones(s, bool)
        gone[keep] = False
        kv[gone] = np.nan
    return kv


def _selected(idx, s, offsets=None):
    rows, valid = R.rows_of(idx, s, offsets)
    return np.unique(rows[valid])


def _pow2(n):
    return n > 0 and n & (n - 1) == 0


# ---- 1. exact, uniform ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", ALL_HEADS)
def test_uniform_weights_are_exact_at_power_of_two_counts(dga, h):
    s, topk = 200, 192
    rng = np.random.default_rng(h)
    idx = np.full((4, topk), -1, np.int32)
    for t, count in enumerate((1, 2, 64, 128)):
        where = np.sort(rng.choice(topk, count, replace=False))
        rows = rng.integers(0, s, count)                                # (with replacement: duplicates, each counted once per position)
        if count >= 64:
            rows[1] = rows[0]
        idx[t, where] = rows
        rest = np.setdiff1d(np.arange(topk), where)
        idx[t, rest[::3]] = s + (rest[::3] % 5)                          # >= S
        idx[t, rest[1::3]] = -2 - rest[1::3]                             # negatives other than -1
    kv = _int_kv(s, R.D_QK, 5)
    q = np.zeros((4, h, R.D_QK), np.float32)
    ref = R.reference(q, kv, idx, 0.3)
    assert ref["count"].tolist() == [1, 2, 64, 128] and np.allclose(ref["lse"], np.log(ref["count"])[:, None])
    got = _run(dga, _bf16(q), _bf16(kv), torch.from_numpy(idx).cuda(), 0.3)
    _check(got, ref, 0.3, topk, exact_rows=range(4))


# ---- 2. exact, one-hot ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", HEADS)
def test_a_key_that_outscores_the_rest_by_256_gives_its_row(dga, h):
    s, topk, scale = 150, 100, 2.0 ** -3
    rng = np.random.default_rng(100 + h)
    kv = rng.integers(-1, 2, size=(s, R.D_QK)).astype(np.float32)
    kv[:, 0] = 0
    q = rng.integers(-1, 2, size=(3, h, R.D_QK)).astype(np.float32)
    q[:, :, 0] = 64
    winners = (7, 8, 9)
    kv[list(winners), 0] = 64                                           # 64 * 64 / 8 = 512 above, the rest within 575 / 8 of 0
    others = np.setdiff1d(np.arange(s), winners)
    idx = rng.choice(others, (3, topk)).astype(np.int32)
    idx[0, 3] = winners[0]                                              # in the first tile
    idx[1, 97] = winners[1]                                             # in the last, ragged tile
    idx[2, 70:] = -1
    idx[2, 69] = winners[2]                                             # the last valid position, a tile of padding behind it
    ref = R.reference(q, kv, idx, scale)
    rows, valid = R.rows_of(idx, s)
    for t in range(3):                                                   # the margin the case is built for
        sc = scale * (q[t].astype(np.float64) @ kv[rows[t][valid[t]]].astype(np.float64).T)
        top = np.sort(sc, axis=1)
        assert (top[:, -1] - top[:, -2] >= 256).all()
    out, bits, lse = got = _run(dga, _bf16(q), _bf16(kv), torch.from_numpy(idx).cuda(), scale)
    for t in range(3):
        want = R.bf16_bits(kv[winners[t], :R.D_V])
        assert np.array_equal(bits[t], np.broadcast_to(want, (h, R.D_V))), t
    _check(got, ref, scale, topk, out_bound=False)


# ---- 3. masking and layout -------------------------------------------------------------------------------------------------------

def _mask_case(topk, s):
    """eight tokens, one kind of list each: (indices int32 [8, topk], offsets int32 [8])"""
    rng = np.random.default_rng(topk)
    idx = np.full((8, topk), -1, np.int32)
    off = np.zeros(8, np.int32)
    half = 1 << (max(topk // 2, 1).bit_length() - 1)                  # a power of two of valid positions where the list allows one
    idx[0] = rng.permutation(s - 20)[:topk]                             # all valid, distinct
    idx[1, :half] = rng.integers(0, s - 20, half)                       # -1 padding at the end
    idx[2, :2 * half:2] = rng.integers(0, s - 20, half)                # -1 in the middle
    idx[3] = np.where(np.arange(topk) % 4 == 0, rng.integers(0, s - 30, topk),
                      np.where(np.arange(topk) % 4 == 1, s + np.arange(topk), -3 - np.arange(topk)))   # >= S, negatives other than -1
    off[3] = 5
    idx[4] = np.repeat(rng.integers(0, s - 20, (topk + 3) // 4), 4)[:topk]                               # duplicates
    if topk > R.TILE:
        late = 1 << ((topk - R.TILE).bit_length() - 1)
        idx[5, R.TILE:R.TILE + late] = rng.integers(0, s - 20, late)    # a first tile with no valid position, then valid ones
    else:
        idx[5, -1] = 3
    # token 6: none at all
    idx[7] = s - 1 - (np.arange(topk) % 16)                             # valid-looking, but the offset pushes all but those at s - 16 out
    off[7] = 15
    return idx, off


@pytest.mark.parametrize("layout", ("wide", "plain"))
@pytest.mark.parametrize("topk", (1, 64, 100, 192))
@pytest.mark.parametrize("h", HEADS)
def test_masking_and_layout(dga, h, topk, layout):
    s, scale = 300, 0.25
    idx, off = _mask_case(topk, s)
    keep = _selected(idx, s, off)
    assert len(keep) < s - 20                                           # rows nobody selects remain, and they hold NaN
    if layout == "wide":                                                # stride 640 with NaN behind column 576; indices a column slice
        kv = _int_kv(s, 640, 9, keep)
        kv_d = _bf16(kv)[:, :R.D_QK]
        wide = np.concatenate([idx, np.full((8, 7), int(np.setdiff1d(np.arange(s), keep)[0]), np.int32)], axis=1)
        idx_d = torch.from_numpy(wide).cuda()[:, :topk]
        assert kv_d.stride(0) == 640 and idx_d.stride(0) == topk + 7
    else:                                                               # the [S, 1, 576] and [M, 1, topk] forms, contiguous
        kv = _int_kv(s, R.D_QK, 9, keep)
        kv_d = _bf16(kv).view(s, 1, R.D_QK)
        idx_d = torch.from_numpy(idx).cuda().view(8, 1, topk)
    off_d = torch.from_numpy(off).cuda()
    zero = np.zeros((8, h, R.D_QK), np.float32)
    ref = R.reference(zero, kv, idx, scale, off)
    assert ref["count"][6] == 0 and ref["count"][0] == topk and 1 <= ref["count"][7] < topk or topk == 1
    exact = [t for t in range(8) if _pow2(int(ref["count"][t]))]
    assert len(exact) >= 2
    _check(_run(dga, _bf16(zero), kv_d, idx_d, scale, off_d), ref, scale, topk, exact_rows=exact)
    # the same lists under scores that differ: small-integer q, so the weights are no longer uniform
    q = np.random.default_rng(h + topk).integers(-2, 3, size=(8, h, R.D_QK)).astype(np.float32) / 8
    ref = R.reference(q, kv, idx, scale, off)
    _check(_run(dga, _bf16(q), kv_d, idx_d, scale, off_d), ref, scale, topk)


# ---- 4. the bound on random data -------------------------------------------------------------------------------------------------

M4, S4, TOPK4, SCALE4 = R.M4, R.S4, R.TOPK4, R.SCALE4
_random_case, _ordered = R.random_case, R.ordered               # (the generators: tests/sparse_mla_ref.py)


@pytest.mark.parametrize("order", ("random", "ascending", "descending"))
@pytest.mark.parametrize("h", ALL_HEADS)
def test_derived_bound_on_random_data(dga, h, order):
    q, kv, base = _random_case(h)
    idx = _ordered(q, kv, base, order)
    ref = R.reference(q, kv, idx, SCALE4)
    assert ref["count"].tolist() == [318, 298, 318, 318, 318] == R.rows_of(base, S4)[1].sum(axis=1).tolist()
    worst, worst_lse = _check(_run(dga, _bf16(q), _bf16(kv), torch.from_numpy(idx.copy()).cuda(), SCALE4), ref, SCALE4, TOPK4)
    print("Hq=%d %s: worst error / bound = %.4f (out), %.4f (lse)" % (h, order, worst, worst_lse))


# ---- 5. NaN ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", HEADS)
def test_a_nan_poisons_what_selects_it_and_nothing_else(dga, h):
    q, kv, idx = (a.copy() for a in _random_case(h))
    row = int(idx[0, 5])
    idx[2, 100] = row                                                   # tokens 0 and 2 select the row ...
    for t in (1, 3, 4):
        idx[t][idx[t] == row] = (row + 1) % S4                          # ... the others do not
    idx_d = torch.from_numpy(idx).cuda()
    clean = _run(dga, _bf16(q), _bf16(kv), idx_d, SCALE4)
    kv2 = kv.copy()
    kv2[row, 530] = np.nan                                              # (a rope column: it reaches the output through the scores alone)
    out, bits, lse = _run(dga, _bf16(q), _bf16(kv2), idx_d, SCALE4)
    assert np.isnan(out[[0, 2]]).all() and np.isnan(lse[[0, 2]]).all()
    assert np.array_equal(bits[[1, 3, 4]], clean[1][[1, 3, 4]]) and np.array_equal(lse[[1, 3, 4]].view(np.uint32), clean[2][[1, 3, 4]].view(np.uint32))
    q2 = q.copy()
    q2[1, h - 3, 100] = np.nan
    out, bits, lse = _run(dga, _bf16(q2), _bf16(kv), idx_d, SCALE4)
    hit = np.zeros((M4, h), bool)
    hit[1, h - 3] = True
    assert np.isnan(out[hit]).all() and np.isnan(lse[hit]).all()
    assert np.array_equal(bits[~hit], clean[1][~hit]) and np.array_equal(lse[~hit].view(np.uint32), clean[2][~hit].view(np.uint32))


# ---- 6. captured graph -----------------------------------------------------------------------------------------------------------

def test_a_captured_graph_follows_new_operands(dga):
    h = 64
    q, kv, idx = _random_case(h)
    q_d, kv_d, idx_d = _bf16(q), _bf16(kv), torch.from_numpy(idx.copy()).cuda()
    off_d = torch.zeros(M4, dtype=torch.int32, device="cuda")
    out, lse = _filled(M4, h)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dga.sparse_mla_fwd(q_d, kv_d, idx_d, SCALE4, 512, off_d, out=out, lse=lse)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        dga.sparse_mla_fwd(q_d, kv_d, idx_d, SCALE4, 512, off_d, out=out, lse=lse)
    first = out.clone()
    # everything overwritten in place: other scores, other values, other lists, offsets that push some positions out
    g = torch.Generator(device="cpu").manual_seed(5)
    q_d.copy_(torch.randn(q_d.shape, generator=g).to(torch.bfloat16))
    kv_d.copy_(torch.randn(kv_d.shape, generator=g).to(torch.bfloat16))
    idx_d.copy_(torch.from_numpy(_ordered(q, kv, idx, "descending")).cuda().roll(1, 0))
    off_d.copy_(torch.tensor([0, 400, -300, 7, 0], dtype=torch.int32))
    out.copy_(_filled(M4, h)[0]); lse.copy_(_filled(M4, h)[1])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    fresh_out, fresh_lse = dga.sparse_mla_fwd(q_d, kv_d, idx_d, SCALE4, 512, off_d, sync=True)
    assert torch.equal(out.view(torch.int16), fresh_out.view(torch.int16)) and torch.equal(lse.view(torch.int32), fresh_lse.view(torch.int32))
    assert not torch.equal(out.view(torch.int16), first.view(torch.int16)) and not torch.isnan(out.float()).any()
    ref = R.reference(q_d.float().cpu().numpy(), kv_d.float().cpu().numpy(), idx_d.cpu().numpy(), SCALE4, off_d.cpu().numpy())
    assert 0 < ref["count"][1] < 300 and 0 < ref["count"][2] < 300
    bits = out.view(torch.int16).cpu().numpy().view(np.uint16)
    _check((out.float().cpu().numpy().astype(np.float64), bits, lse.cpu().numpy()), ref, SCALE4, TOPK4)


# ---- 7. outputs and determinism ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", ALL_HEADS)
def test_outputs_in_place_and_two_runs_alike(dga, h):
    q, kv, idx = _random_case(h)
    q_d, kv_d, idx_d = _bf16(q), _bf16(kv), torch.from_numpy(idx.copy()).cuda()
    a = _run(dga, q_d, kv_d, idx_d, SCALE4)                             # (out= and lse= written in place and returned: _run)
    b = _run(dga, q_d, kv_d, idx_d, SCALE4)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    out, lse = dga.sparse_mla_fwd(q_d, kv_d, idx_d, SCALE4, sync=True)   # the allocating call
    assert out.shape == (M4, h, R.D_V) and out.dtype == torch.bfloat16 and lse.shape == (M4, h) and lse.dtype == torch.float32
    assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), a[1])
    assert np.array_equal(lse.cpu().numpy().view(np.uint32), a[2].view(np.uint32))
    # the grid order changes no bit
    lin = dga.sparse_mla_fwd(q_d, kv_d, idx_d, SCALE4, sync=True, _flags=1)
    assert torch.equal(lin[0].view(torch.int16), out.view(torch.int16)) and torch.equal(lin[1].view(torch.int32), lse.view(torch.int32))
    # M == 0: nothing to launch, empty outputs
    none = dga.sparse_mla_fwd(q_d[:0], kv_d, idx_d[:0], SCALE4, sync=True)
    assert none[0].shape == (0, h, R.D_V) and none[1].shape == (0, h)


# ---- 8. every head count, the heads told apart --------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", ALL_HEADS)
def test_every_head_gets_its_own_winner_at_every_head_count(dga, h):
    """A partly filled first (32, 48) or second (80, 96, 112) head block: which waves compute, which rows of the q image are filled and
    how many heads the second block owns all follow Hq.  Every head of every token has a winner of its own, so a head in the wrong
    lane group, wave or block shows as another row's bits."""
    q, kv, idx, scale, win = R.winners_case(h)
    ref = R.reference(q, kv, idx, scale)
    assert np.array_equal(ref["lse"], np.full((R.WIN_M, h), 512.0))
    out, bits, lse = got = _run(dga, _bf16(q), _bf16(kv), torch.from_numpy(idx.copy()).cuda(), scale)
    assert R.heads_off_their_winner(bits, kv, win) == []
    _check(got, ref, scale, R.WIN_TOPK, out_bound=False)               # (lse within its bound of 512; out is exact above)


# ---- 9. the softmax off the flat distributions ------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ("random", "ascending", "descending"))
@pytest.mark.parametrize("sign", (1, -1), ids=("plus", "minus"))
@pytest.mark.parametrize("h", R.PEAK_HEADS)
def test_derived_bound_on_peaked_and_negated_scores(dga, h, sign, order):
    """R.PEAK times the scale: a few positions hold nearly all the weight, the running maximum moves by large steps when the list
    ascends and alpha becomes tiny; a negative scale turns the order of the scores round.  (test_sparse_mla.py: the spread stays below
    60 nat, every weight of the reference is a normal fp32 number relative to the largest.)"""
    scale = sign * R.PEAK * SCALE4
    q, kv, base = _random_case(h)
    idx = _ordered(q, kv, base, order)
    ref = R.reference(q, kv, idx, scale)
    worst, worst_lse = _check(_run(dga, _bf16(q), _bf16(kv), torch.from_numpy(idx.copy()).cuda(), scale), ref, scale, TOPK4)
    print("Hq=%d scale %+d SCALE4 %s: worst error / bound = %.4f (out), %.4f (lse)" % (h, sign * R.PEAK, order, worst, worst_lse))


@pytest.mark.parametrize("h", ALL_HEADS)
def test_a_zero_scale_is_q_equal_to_zero_bit_for_bit(dga, h):
    s, topk = 200, 192
    rng = np.random.default_rng(300 + h)
    idx = np.full((4, topk), -1, np.int32)
    for t, count in enumerate((1, 2, 64, 128)):
        idx[t, np.sort(rng.choice(topk, count, replace=False))] = rng.integers(0, s, count)
    kv = _int_kv(s, R.D_QK, 6)
    q = _random_case(h)[0][:4]
    zero = np.zeros_like(q)
    idx_d, kv_d = torch.from_numpy(idx).cuda(), _bf16(kv)
    ref = R.reference(q, kv, idx, 0.0)
    assert ref["count"].tolist() == [1, 2, 64, 128] and np.array_equal(ref["out"], R.reference(zero, kv, idx, 0.3)["out"])
    base = _run(dga, _bf16(zero), kv_d, idx_d, 0.3)
    for scale in (0.0, -0.0):
        got = _run(dga, _bf16(q), kv_d, idx_d, scale)
        _check(got, ref, scale, topk, exact_rows=range(4))
        assert np.array_equal(got[1], base[1]) and np.array_equal(got[2].view(np.uint32), base[2].view(np.uint32))


@pytest.mark.parametrize("h", (16, 128))
def test_derived_bound_over_64_tiles(dga, h):
    q, kv, idx = R.long_case(h)
    topk = idx.shape[1]
    assert topk == 2048 == 64 * R.TILE
    ref = R.reference(q, kv, idx, SCALE4)
    assert ref["count"].tolist() == [topk, topk]
    q_d, kv_d, idx_d = _bf16(q), _bf16(kv), torch.from_numpy(idx.copy()).cuda()
    a = _run(dga, q_d, kv_d, idx_d, SCALE4)
    worst, worst_lse = _check(a, ref, SCALE4, topk)
    print("Hq=%d topk=2048: worst error / bound = %.4f (out), %.4f (lse)" % (h, worst, worst_lse))
    b = _run(dga, q_d, kv_d, idx_d, SCALE4)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


# ---- 10. the ends of the addressing ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ("plain", "three"))
@pytest.mark.parametrize("h", (16, 80))
def test_a_cache_of_one_row(dga, h, layout):
    topk = 70
    kv = _int_kv(1, R.D_QK, 12)
    idx = np.full((3, topk), -1, np.int32)
    idx[0, 41] = 0                                                      # one valid position, in the second tile
    idx[1, 3:67] = 0                                                    # 64 of them, over three tiles
    idx[1, [0, 1, 67, 68]] = [1, 2 ** 31 - 1, -2 ** 31, 1]              # anything else is out of a range of one row
    idx[2, ::2] = 1                                                     # nothing valid
    kv_d = _bf16(kv) if layout == "plain" else _bf16(kv).view(1, 1, R.D_QK)
    zero = np.zeros((3, h, R.D_QK), np.float32)
    ref = R.reference(zero, kv, idx, 0.5)
    assert ref["count"].tolist() == [1, 64, 0]
    out, bits, lse = got = _run(dga, _bf16(zero), kv_d, torch.from_numpy(idx).cuda(), 0.5)
    _check(got, ref, 0.5, topk, exact_rows=range(3))
    assert np.array_equal(bits[:2], np.broadcast_to(R.bf16_bits(kv[0, :R.D_V]), (2, h, R.D_V)))     # the row itself, both times
    # one token as well: M = 1, S = 1
    got = _run(dga, _bf16(zero[:1]), kv_d, torch.from_numpy(idx[1:2].copy()).cuda(), 0.5)
    _check(got, {k: v[1:2] for k, v in ref.items()}, 0.5, topk, exact_rows=range(1))


@pytest.mark.parametrize("h", (16, 80))
def test_indices_and_offsets_at_the_ends_of_int32(dga, h):
    s = 40
    idx, off, want = R.extremes_case(s)
    keep = _selected(idx, s, off)
    assert sorted(set(sum(want, []))) == keep.tolist() and len(keep) < s // 2
    kv = _int_kv(s, R.D_QK, 13, keep)                                   # every row nobody selects is NaN
    zero = np.zeros((5, h, R.D_QK), np.float32)
    ref = R.reference(zero, kv, idx, 0.25, off)
    assert ref["count"].tolist() == [4, 0, 0, 8, 2]
    got = _run(dga, _bf16(zero), _bf16(kv), torch.from_numpy(idx).cuda(), 0.25, torch.from_numpy(off).cuda())
    _check(got, ref, 0.25, idx.shape[1], exact_rows=range(5))
