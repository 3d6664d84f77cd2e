"""GPU: split-topk sparse MLA decode -- sparse_mla_fwd_partial / sparse_mla_fwd_fp8_partial, sparse_mla_merge and the two-launch
sparse_mla_fwd_split / sparse_mla_fwd_fp8_split -- on sparse_mla_ref's small cases.  What is exact is checked on the bits: one split is the
one-pass kernel; a head whose winner outscores everything by 512 is its winner's row and the winning split's lse, whatever the number of
splits; a list that repeats its first half gives two equal partials and the half's out; an empty split weighs nothing; the fp8 cache's
partials are the bf16 kernel's on the dequantised rows; sparse_mla_fwd_split is the merge of the partials.  Everything else is held to
the bound tests/sparse_mla_split_ref.py derives, every element, the worst ratio printed.  Every partial call here runs into buffers of 64
splits pre-filled with a NaN pattern: all of [:P] must be written and nothing of [P:]."""
import numpy as np
import pytest
import torch

import sparse_mla_fp8_ref as F
import sparse_mla_ref as R
import sparse_mla_split_ref as X
from sparse_mla_support import NAN_FILL, _bf16, _deq_tensor, _filled, _nan16, _nan32, _view, _written_by_the_writer

pytestmark = pytest.mark.gpu

SCALE4 = R.SCALE4
LINEAR_GRID = 1                                                         # DGA_SPARSE_MLA_LINEAR_GRID


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------

def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()                # (a copy: the cases are read-only)


def _partial(fn, q, kv, idx, scale, p, offsets=None, flags=0):
    """(partial_out bits uint32 [P, M, H, 512], partial_lse bits uint32 [P, M, H], the two device tensors) of one call into buffers of
    64 splits pre-filled with a NaN pattern: the effective P leads the returned tensors, every element of [:P] was written, none of [P:]"""
    m, h = q.shape[0], q.shape[1]
    po = torch.full((64, m, h, R.D_V), NAN_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    pl = torch.full((64, m, h), NAN_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    got = fn(q, kv, idx, scale, p, 512, offsets, partial_out=po, partial_lse=pl, sync=True, _flags=flags)
    eff = X.effective_splits(idx.shape[-1], p)
    assert got[0].shape == (eff, m, h, R.D_V) and got[1].shape == (eff, m, h)
    assert got[0].data_ptr() == po.data_ptr() and got[1].data_ptr() == pl.data_ptr()
    ob, lb = po.view(torch.int32).cpu().numpy().view(np.uint32), pl.view(torch.int32).cpu().numpy().view(np.uint32)
    assert (ob[eff:] == NAN_FILL).all() and (lb[eff:] == NAN_FILL).all()
    assert not (ob[:eff] == NAN_FILL).any() and not (lb[:eff] == NAN_FILL).any()
    return ob[:eff], lb[:eff], got[0], got[1]


def _bits(out, lse):
    return out.view(torch.int16).cpu().numpy().view(np.uint16), lse.view(torch.int32).cpu().numpy().view(np.uint32)


def _merge(dga, po, pl):
    out, lse = _filled(po.shape[1], po.shape[2])
    got = dga.sparse_mla_merge(po, pl, out=out, lse=lse, sync=True)
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == lse.data_ptr()
    return _bits(out, lse)


def _split(fn, q, kv, idx, scale, p, offsets=None):
    out, lse = _filled(q.shape[0], q.shape[1])
    got = fn(q, kv, idx, scale, 512, offsets, p, out, lse, True)
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == lse.data_ptr()
    return _bits(out, lse)


def _one_pass(fn, q, kv, idx, scale, offsets=None):
    out, lse = _filled(q.shape[0], q.shape[1])
    fn(q, kv, idx, scale, 512, offsets, out=out, lse=lse, sync=True)
    return _bits(out, lse)


def _values(bits):
    out, lse = bits
    return F.bits_to_f32(out).astype(np.float64), lse.view(np.float32).astype(np.float64)


_REFS = {}


def _ref(key, q, kv, idx, scale):
    """the float64 reference of a case, computed once"""
    if key not in _REFS:
        _REFS[key] = R.reference(q, kv, idx, scale)
    return _REFS[key]


def _hold(dga, key, q, kv, idx, scale, splits):
    """sparse_mla_fwd_split at every P of `splits` against the derived bound, every element: the worst ratios (out, lse)"""
    ref = _ref(key, q, kv, idx, scale)
    q_d, kv_d, idx_d = _bf16(q), _bf16(kv), _dev(idx)
    topk, worst = idx.shape[1], [0.0, 0.0]
    for p in splits:
        ob, lb, po, pl = _partial(dga.sparse_mla_fwd_partial, q_d, kv_d, idx_d, scale, p)
        got = _merge(dga, po, pl)
        assert np.array_equal(_split(dga.sparse_mla_fwd_split, q_d, kv_d, idx_d, scale, p)[0], got[0])
        out, lse = _values(got)
        pl64 = lb.view(np.float32).astype(np.float64)
        maxlse = np.where(np.isfinite(pl64), np.abs(pl64), 0.0).max(axis=0)
        eff = X.effective_splits(topk, p)
        ro = X.worst_ratio(out, ref["out"], X.bound_out(ref, scale, topk, eff, maxlse))
        rl = X.worst_ratio(lse, ref["lse"], X.bound_lse(ref, scale, topk, eff, maxlse))
        print(f"{key} P={p}: worst error / bound out {ro:.4f} lse {rl:.4f}")
        assert ro <= 1 and rl <= 1, (key, p, ro, rl)
        worst = [max(worst[0], ro), max(worst[1], rl)]
    return worst


# ---- 1. one split is the one-pass kernel -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cache", ("bf16", "fp8"))
@pytest.mark.parametrize("h", R.ALL_HEADS)
def test_one_split_is_the_one_pass_kernel_byte_for_byte(dga, h, cache):
    for name in ("random", "winners"):
        if name == "random":
            q, kv, idx = R.random_case(h)
            scale = SCALE4
        else:
            q, kv, idx, scale, _ = R.winners_case(h)
        q_d, idx_d = _bf16(q), _dev(idx)
        if cache == "fp8":
            kv_d = _view(_dev(_written_by_the_writer(dga, kv, 64, 48)), 64)
            one, split = dga.sparse_mla_fwd_fp8, dga.sparse_mla_fwd_fp8_split
        else:
            kv_d, one, split = _bf16(kv), dga.sparse_mla_fwd, dga.sparse_mla_fwd_split
        want = _one_pass(one, q_d, kv_d, idx_d, scale)
        got = _split(split, q_d, kv_d, idx_d, scale, 1)
        assert not _nan16(want[0]).any() and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name


# ---- 2. one winner per head --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", (2, 3, 5))
@pytest.mark.parametrize("h", R.ALL_HEADS)
def test_every_head_gets_its_winners_row_and_the_winning_splits_lse(dga, h, p):
    """The other splits score at most 0 + ln 160 against the winner's 512, and exp(-507) is below float32's smallest subnormal: their
    weights are exactly 0, L = 1, and the result is the winning split's row and lse bit for bit.  A split, head, wave or token in the
    wrong workspace slot shows as another row's bits."""
    q, kv, idx, scale, win = R.winners_case(h)
    q_d, kv_d, idx_d = _bf16(q), _bf16(kv), _dev(idx)
    ob, lb, po, pl = _partial(dga.sparse_mla_fwd_partial, q_d, kv_d, idx_d, scale, p)
    out, lse = _merge(dga, po, pl)
    assert R.heads_off_their_winner(out, kv, win) == []
    ws = X.winner_splits(idx, win, p)
    assert X.heads_off_their_winning_split(lse, lb, ws) == []
    # the winning split's own partial is the row as float32, and the whole call gives the same bytes
    rows = np.take_along_axis(ob, ws[None, :, :, None], axis=0)[0]
    assert np.array_equal(rows, X.f32_bits(kv[win][:, :, :R.D_V]))
    again = _split(dga.sparse_mla_fwd_split, q_d, kv_d, idx_d, scale, p)
    assert np.array_equal(again[0], out) and np.array_equal(again[1], lse)


# ---- 3. two identical halves ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", (16, 128))
def test_a_list_that_repeats_its_first_half(dga, h):
    """w = 1 for both splits, L = 2, N = 2 po: out is the half's out exactly.  Only P = 2 is exact under the sequential sum: with more
    equal splits L = 3, 5, ... and N (1 / L) rounds."""
    q, kv, idx = R.random_case(h)
    half = idx[:, :160]
    twice = np.concatenate([half, half], axis=1)
    q_d, kv_d = _bf16(q), _bf16(kv)
    ob, lb, po, pl = _partial(dga.sparse_mla_fwd_partial, q_d, kv_d, _dev(twice), SCALE4, 2)
    assert np.array_equal(ob[0], ob[1]) and np.array_equal(lb[0], lb[1])
    out, lse = _merge(dga, po, pl)
    want = _one_pass(dga.sparse_mla_fwd, q_d, kv_d, _dev(half), SCALE4)
    assert np.array_equal(out, want[0])
    target = want[1].view(np.float32).astype(np.float64) + np.log(2.0)
    merged = dict(lse=target)
    ratio = X.worst_ratio(lse.view(np.float32), target, X.merge_bound_lse(merged, 2))
    print(f"lse against the half's lse + ln 2: worst error / bound {ratio:.4f}")
    assert ratio <= 1


# ---- 4. the derived bound --------------------------------------------------------------------------------------------------------------

SPLITS = (2, 3, 7, 10)


@pytest.mark.parametrize("order", ("random", "ascending", "descending"))
@pytest.mark.parametrize("h", R.PEAK_HEADS)
def test_derived_bound_on_random_data(dga, h, order):
    q, kv, idx = R.random_case(h)
    _hold(dga, ("random", h, order), q, kv, R.ordered(q, kv, idx, order), SCALE4, SPLITS)


@pytest.mark.parametrize("h", R.PEAK_HEADS)
def test_derived_bound_on_a_ragged_list_split_unevenly(dga, h):
    q, kv, idx = R.random_case(h)
    assert X.split_ranges(X.tiles_of(313), 3) == [(0, 3), (3, 6), (6, 10)] and 313 % 32
    _hold(dga, ("sliced", h), q, kv, np.ascontiguousarray(idx[:, :313]), SCALE4, SPLITS)


@pytest.mark.parametrize("sign", (1, -1), ids=("plus", "minus"))
@pytest.mark.parametrize("h", R.PEAK_HEADS)
def test_derived_bound_on_peaked_and_negated_scores(dga, h, sign):
    q, kv, idx = R.random_case(h)
    _hold(dga, ("peaked", h, sign), q, kv, R.ordered(q, kv, idx, "ascending"), sign * R.PEAK * SCALE4, SPLITS)


def test_derived_bound_with_one_tile_a_split(dga):
    q, kv, idx = R.long_case(16)
    _hold(dga, ("long", 16), q, kv, idx, SCALE4, (16, 64))


# ---- 5. empty splits ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cache", ("bf16", "fp8"))
@pytest.mark.parametrize("h", (16, 80))
def test_empty_splits_weigh_nothing(dga, h, cache):
    """-inf never meets -inf: an empty split has lse -inf under a finite maximum (w = 0), a token of empty splits has mu = 0"""
    q, kv, idx = R.random_case(h)
    idx = idx.copy()
    idx[1, 160:] = -1                                                   # token 1: the second split is padding
    idx[2, :160] = R.S4 + 9                                             # token 2: the first split is out of range
    idx[3, :] = -1                                                      # token 3: nothing valid
    q_d, idx_d = _bf16(q), _dev(idx)
    if cache == "fp8":
        kv_d = _view(_dev(_written_by_the_writer(dga, kv, 64, 48)), 64)
        idx_d = _dev(np.where(idx >= R.S4, 11 * 64 + 3, idx).astype(np.int32))
        partial, one = dga.sparse_mla_fwd_fp8_partial, dga.sparse_mla_fwd_fp8
    else:
        kv_d, partial, one = _bf16(kv), dga.sparse_mla_fwd_partial, dga.sparse_mla_fwd
    ob, lb, po, pl = _partial(partial, q_d, kv_d, idx_d, SCALE4, 2)
    neg_inf = np.uint32(0xFF800000)
    assert (lb[1, 1] == neg_inf).all() and (ob[1, 1] == 0).all() and (lb[0, 2] == neg_inf).all() and (ob[0, 2] == 0).all()
    assert (lb[:, 3] == neg_inf).all() and (ob[:, 3] == 0).all()                          # +0 and -inf in every split
    out, lse = _merge(dga, po, pl)
    want = _one_pass(one, q_d, kv_d, idx_d, SCALE4)                     # (= the P = 1 bytes: test 1)
    for t in (1, 2):                                                    # the one non-empty split alone decides: w = 1, L = 1
        assert np.array_equal(out[t], want[0][t]) and np.array_equal(lse[t], want[1][t]), t
    assert (out[3] == 0).all() and (lse[3] == neg_inf).all()
    assert not _nan16(out).any() and not _nan32(lse).any()


# ---- 6. NaN ------------------------------------------------------------------------------------------------------------------------------

def _nan_case(h):
    q, kv, idx = R.random_case(h)
    idx = idx.copy()
    row = int(idx[0, 5])                                                # in split 0 of token 0 ...
    idx[2, 250] = row                                                   # ... and in a later split of token 2
    for t in (1, 3, 4):
        idx[t][idx[t] == row] = (row + 1) % R.S4
    idx[4, :] = -1
    idx[4, 7] = row                                                     # token 4: its only valid position is the row
    return q, kv, idx, row


@pytest.mark.parametrize("p", (2, 5))
def test_a_nan_row_poisons_what_the_one_pass_kernel_poisons(dga, p):
    h = 64
    q, kv, idx, row = _nan_case(h)
    kv = kv.copy()
    kv[row, 530] = np.nan
    q_d, kv_d, idx_d = _bf16(q), _bf16(kv), _dev(idx)
    want = _one_pass(dga.sparse_mla_fwd, q_d, kv_d, idx_d, SCALE4)
    got = _split(dga.sparse_mla_fwd_split, q_d, kv_d, idx_d, SCALE4, p)
    assert np.array_equal(_nan16(got[0]), _nan16(want[0])) and np.array_equal(_nan32(got[1]), _nan32(want[1]))
    assert _nan16(got[0][[0, 2, 4]]).all() and _nan32(got[1][[0, 2, 4]]).all()           # token 4: NaN, not +0
    assert not _nan16(got[0][[1, 3]]).any() and not _nan32(got[1][[1, 3]]).any()


@pytest.mark.parametrize("what", ("NaN code", "NaN scale", "inf scale", "NaN rope value"))
def test_nan_and_inf_in_a_selected_row_of_the_fp8_cache(dga, what):
    h = 64
    q, kv, idx, row = _nan_case(h)
    buf = _written_by_the_writer(dga, kv, 64, 48).copy()
    at = int(F.row_at(row, 64, buf.shape[1]))
    flat = buf.reshape(-1)
    if what == "NaN code":
        flat[at + 300] = 0xFF
    elif what == "NaN scale":
        flat[at + F.SCALES_AT + 4:at + F.SCALES_AT + 8] = np.array([np.nan], np.float32).view(np.uint8)
    elif what == "inf scale":
        flat[at + F.SCALES_AT + 8:at + F.SCALES_AT + 12] = np.array([np.inf], np.float32).view(np.uint8)
    else:
        flat[at + F.ROPE_AT + 2 * 17:at + F.ROPE_AT + 2 * 17 + 2] = np.array([0x7FC1], np.uint16).view(np.uint8)
    idx = np.where(idx >= R.S4, 11 * 64 + 3, idx).astype(np.int32)
    q_d, kv_d, idx_d = _bf16(q), _view(_dev(buf), 64), _dev(idx)
    want = _one_pass(dga.sparse_mla_fwd_fp8, q_d, kv_d, idx_d, SCALE4)
    for p in (2, 5):
        got = _split(dga.sparse_mla_fwd_fp8_split, q_d, kv_d, idx_d, SCALE4, p)
        assert np.array_equal(_nan16(got[0]), _nan16(want[0])) and np.array_equal(_nan32(got[1]), _nan32(want[1])), p
        assert _nan16(got[0][[0, 2, 4]]).any() and _nan32(got[1][[0, 2, 4]]).all() and not _nan16(got[0][[1, 3]]).any()


# ---- 7. nothing else is touched ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", (16, 80))
def test_unselected_rows_wider_columns_and_padding_bytes_do_not_reach_the_result(dga, h):
    q, kv, idx = R.random_case(h)
    q_d, idx_d = _bf16(q), _dev(idx)
    clean = _partial(dga.sparse_mla_fwd_partial, q_d, _bf16(kv), idx_d, SCALE4, 3)
    rows, valid = R.rows_of(idx, R.S4)
    used = np.zeros(R.S4, bool)
    used[rows[valid]] = True
    assert 0 < (~used).sum()
    wide = np.full((R.S4, 640), np.nan, np.float32)                      # columns >= 576 and every unselected row: NaN
    wide[used, :R.D_QK] = kv[used]
    dirty = _partial(dga.sparse_mla_fwd_partial, q_d, _bf16(wide)[:, :R.D_QK], idx_d, SCALE4, 3)
    assert np.array_equal(dirty[0], clean[0]) and np.array_equal(dirty[1], clean[1]) and not _nan32(dirty[0]).any()
    # the fp8 cache: every unselected row and every byte between blocks 0xFF (NaN codes, NaN scales, NaN rope values)
    buf = _written_by_the_writer(dga, kv, 64, 48)
    idx8 = np.where(idx >= R.S4, 11 * 64 + 3, idx).astype(np.int32)
    mask = F.row_bytes_mask(np.flatnonzero(used), buf.shape[0], 64, buf.shape[1])
    ff = np.where(mask, buf, 0xFF).astype(np.uint8)
    a = _partial(dga.sparse_mla_fwd_fp8_partial, q_d, _view(_dev(buf), 64), _dev(idx8), SCALE4, 3)
    b = _partial(dga.sparse_mla_fwd_fp8_partial, q_d, _view(_dev(ff), 64), _dev(idx8), SCALE4, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not _nan32(b[0]).any() and not _nan32(b[1]).any()
    # the merge of a buffer of 64 splits whose [P:] is the NaN pattern reads nothing of it
    ob, lb, po, pl = dirty
    assert po.shape[0] == 3 and po.untyped_storage().nbytes() == 64 * R.M4 * h * R.D_V * 4
    out, lse = _merge(dga, po, pl)
    assert not _nan16(out).any() and not _nan32(lse).any()
    fresh = dga.sparse_mla_merge(po.clone(), pl.clone(), sync=True)
    assert np.array_equal(_bits(*fresh)[0], out) and np.array_equal(_bits(*fresh)[1], lse)


# ---- 8. composition ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", (1, 3, 64))
def test_the_fp8_partials_are_the_bf16_partials_on_the_dequantised_rows(dga, page):
    h = 80
    q, kv, idx = R.random_case(h)
    buf = _written_by_the_writer(dga, kv, page, 16 if page != 64 else 48)
    s = buf.shape[0] * page
    idx = np.where(idx >= R.S4, s + 3, idx).astype(np.int32)
    q_d, idx_d = _bf16(q), _dev(idx)
    for p in (1, 4, 10):
        a = _partial(dga.sparse_mla_fwd_fp8_partial, q_d, _view(_dev(buf), page), idx_d, SCALE4, p)
        b = _partial(dga.sparse_mla_fwd_partial, q_d, _deq_tensor(buf, page), idx_d, SCALE4, p)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not _nan32(a[0]).any(), p
        both = _split(dga.sparse_mla_fwd_fp8_split, q_d, _view(_dev(buf), page), idx_d, SCALE4, p)
        merged = _merge(dga, a[2], a[3])
        assert np.array_equal(both[0], merged[0]) and np.array_equal(both[1], merged[1]), p


@pytest.mark.parametrize("h", (16, 128))
def test_the_split_call_is_the_merge_of_the_partials(dga, h):
    q, kv, idx = R.random_case(h)
    off = np.array([0, 40, -30, 7, 0], np.int32)
    q_d, kv_d, idx_d, off_d = _bf16(q), _bf16(kv), _dev(idx), _dev(off)
    for p in (1, 2, 9, 64):
        ob, lb, po, pl = _partial(dga.sparse_mla_fwd_partial, q_d, kv_d, idx_d, SCALE4, p, off_d)
        merged = _merge(dga, po, pl)
        got = _split(dga.sparse_mla_fwd_split, q_d, kv_d, idx_d, SCALE4, p, off_d)
        assert np.array_equal(got[0], merged[0]) and np.array_equal(got[1], merged[1]), p
    # num_splits=None: the rule; at this size it splits, and the result is the explicit call's
    rule = dga.sparse_mla_num_splits(R.M4, h, R.TOPK4, q_d.device)
    assert rule == min(torch.cuda.get_device_properties(0).multi_processor_count // (R.M4 * -(-h // 64)), 10 // 4) == 2
    out, lse = dga.sparse_mla_fwd_split(q_d, kv_d, idx_d, SCALE4, index_offsets=off_d, sync=True)
    want = _split(dga.sparse_mla_fwd_split, q_d, kv_d, idx_d, SCALE4, rule, off_d)
    assert np.array_equal(_bits(out, lse)[0], want[0]) and np.array_equal(_bits(out, lse)[1], want[1])
    # ... and where the rule says 1 (a short list) it is the one-pass operator's launch
    short = _dev(np.ascontiguousarray(idx[:, :100]))
    out, lse = dga.sparse_mla_fwd_split(q_d, kv_d, short, SCALE4, index_offsets=off_d, sync=True)
    want = _one_pass(dga.sparse_mla_fwd, q_d, kv_d, short, SCALE4, off_d)
    assert np.array_equal(_bits(out, lse)[0], want[0]) and np.array_equal(_bits(out, lse)[1], want[1])
    # M == 0: nothing to launch
    none = dga.sparse_mla_fwd_split(q_d[:0], kv_d, idx_d[:0], SCALE4, num_splits=4, sync=True)
    assert none[0].shape == (0, h, R.D_V) and none[1].shape == (0, h)
    none = dga.sparse_mla_fwd_partial(q_d[:0], kv_d, idx_d[:0], SCALE4, 4, sync=True)
    assert none[0].shape == (4, 0, h, R.D_V) and dga.sparse_mla_merge(*none, sync=True)[0].shape == (0, h, R.D_V)


# ---- 9. determinism and capture --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cache", ("bf16", "fp8"))
def test_two_runs_and_the_linear_grid_give_the_same_bytes(dga, cache):
    h = 128
    q, kv, idx = R.random_case(h)
    q_d, idx_d = _bf16(q), _dev(idx)
    if cache == "fp8":
        kv_d, fn = _view(_dev(_written_by_the_writer(dga, kv, 64, 48)), 64), dga.sparse_mla_fwd_fp8_partial
        idx_d = _dev(np.where(idx >= R.S4, 11 * 64 + 3, idx).astype(np.int32))
    else:
        kv_d, fn = _bf16(kv), dga.sparse_mla_fwd_partial
    for p in (3, 10):
        a = _partial(fn, q_d, kv_d, idx_d, SCALE4, p)
        b = _partial(fn, q_d, kv_d, idx_d, SCALE4, p)
        c = _partial(fn, q_d, kv_d, idx_d, SCALE4, p, flags=LINEAR_GRID)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
        m1, m2 = _merge(dga, a[2], a[3]), _merge(dga, c[2], c[3])
        assert np.array_equal(m1[0], m2[0]) and np.array_equal(m1[1], m2[1])


def test_a_captured_graph_of_the_two_launches_follows_new_operands(dga):
    h, p = 64, 3
    q, kv, idx = R.random_case(h)
    q_d, kv_d, idx_d = _bf16(q), _bf16(kv), _dev(idx.copy())
    off_d = torch.zeros(R.M4, dtype=torch.int32, device="cuda")
    out, lse = _filled(R.M4, h)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dga.sparse_mla_fwd_split(q_d, kv_d, idx_d, SCALE4, 512, off_d, p, out, lse)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        dga.sparse_mla_fwd_split(q_d, kv_d, idx_d, SCALE4, 512, off_d, p, out, lse)
    first = out.clone()
    g = torch.Generator(device="cpu").manual_seed(5)
    q_d.copy_(torch.randn(q_d.shape, generator=g).to(torch.bfloat16))
    kv_d.copy_(torch.randn(kv_d.shape, generator=g).to(torch.bfloat16))
    idx_d.copy_(_dev(R.ordered(q, kv, idx, "descending")).roll(1, 0))
    off_d.copy_(torch.tensor([0, 400, -300, 7, 0], dtype=torch.int32))
    out.copy_(_filled(R.M4, h)[0]); lse.copy_(_filled(R.M4, h)[1])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = _bits(out, lse)
    want = _split(dga.sparse_mla_fwd_split, q_d, kv_d, idx_d, SCALE4, p, off_d)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(got[0], _bits(first, lse)[0]) and not _nan16(got[0]).any()


# ---- 10. the merge on its own --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", (1, 2, 64))
@pytest.mark.parametrize("h", (16, 128))
def test_the_merge_against_float64_on_host_made_partials(dga, h, p):
    m = 3
    rng = np.random.default_rng(100 * h + p)
    po = rng.standard_normal((p, m, h, R.D_V)).astype(np.float32)
    pl = rng.uniform(-40, 40, (p, m, h)).astype(np.float32)
    pl[0, 1, 3] = -np.inf                                               # one empty split of one head
    po[0, 1, 3] = 0
    pl[:, 2, 5], po[:, 2, 5] = -np.inf, 0                               # one head without anything
    if p > 1:
        pl[1, 0, :] = pl[0, 0, :]                                       # ties at the top
    want = X.merge(po, pl)
    out, lse = _values(_merge(dga, _dev(po), _dev(pl)))
    assert (out[2, 5] == 0).all() and np.isneginf(lse[2, 5])
    ro = X.worst_ratio(out, want["out"], X.merge_bound_out(want, p))
    rl = X.worst_ratio(lse, want["lse"], X.merge_bound_lse(want, p))
    print(f"merge P={p} Hq={h}: worst error / bound out {ro:.4f} lse {rl:.4f}")
    assert ro <= 1 and rl <= 1
    if p == 1:                                                          # RNE_bf16(po) and partial_lse, bit for bit
        got = _merge(dga, _dev(po), _dev(pl))
        assert np.array_equal(got[0], R.bf16_bits(po[0])) and np.array_equal(got[1], X.f32_bits(pl[0]))
