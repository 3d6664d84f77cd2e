"""GPU: sparse_mla_fwd against tests/sparse_mla_ref.py, into outputs pre-filled with a NaN pattern.  TILE = 32 positions is the kernel's
gathered tile; a workgroup owns 64 heads (one wave per 16), so Hq = 16 leaves three waves that only gather, 64 fills one workgroup and 128
takes two.  With q = 0 every weight is 1 and, on small-integer kv with a power-of-two number of valid positions, out is
RNE_bf16(sum v / count) bit for bit: gather, masking and duplicates are checked with no tolerance.  One key that outscores the rest by 256
gives its value row bit for bit wherever it stands in the list.  Every kind of invalid position, the offsets, a strided kv whose every
unselected row and every column >= 576 is NaN, and an index list that is a slice of a wider tensor go through the same check; normal
samples in three orders of the list stay inside the derived bound on every element; a NaN poisons what selects it and nothing else; a
captured graph follows rewritten operands; two calls give the same bytes."""
import functools

import numpy as np
import pytest
import torch

import sparse_mla_ref as R

pytestmark = pytest.mark.gpu

HEADS = (16, 64, 128)
NAN_FILL = 0x7FC12345
NAN_FILL16 = 0x7FC5


def _bf16(a):
    """the bf16 device tensor of float values that bf16 holds exactly (NaN allowed)"""
    a = np.asarray(a, dtype=np.float32)
    t = torch.from_numpy(a.copy()).to(torch.bfloat16)
    assert np.array_equal(t.float().numpy(), a, equal_nan=True)
    return t.cuda()


def _filled(m, h):
    out = torch.full((m, h, R.D_V), NAN_FILL16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    lse = torch.full((m, h), NAN_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    return out, lse


def _run(dga, q, kv, idx, scale, offsets=None):
    """(out as float64, its bits, lse float32) of one call into pre-filled outputs"""
    out, lse = _filled(q.shape[0], q.shape[1])
    got = dga.sparse_mla_fwd(q, kv, idx, scale, 512, offsets, out=out, lse=lse, sync=True)
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == lse.data_ptr()
    bits = out.view(torch.int16).cpu().numpy().view(np.uint16)
    return out.float().cpu().numpy().astype(np.float64), bits, lse.cpu().numpy()


def _check(got, ref, scale, topk, exact_rows=(), out_bound=True):
    """every element of out and lse against the reference: +0 and -inf for a token without a valid position, the bits of
    RNE_bf16(out) on the tokens of exact_rows, the derived bounds everywhere (out_bound=False: of lse alone -- the bound of out is
    relative to the weighted values and has no room for weights that underflow fp32, which the one-hot case is made of)"""
    out, bits, lse = got
    assert not np.isnan(out).any() and not np.isnan(lse).any()
    empty = ref["count"] == 0
    assert (bits[empty] == 0).all() and np.isneginf(lse[empty]).all()
    assert np.isfinite(lse[~empty]).all()
    for t in exact_rows:
        assert np.array_equal(bits[t], R.bf16_bits(ref["out"][t])), t
    err, bar = np.abs(out - ref["out"]), R.bound_out(ref, scale, topk)
    if not out_bound:
        err = np.zeros_like(err)
    assert (err <= bar).all(), (int((err > bar).sum()), np.argwhere(err > bar)[:4])
    lerr, lbar = np.abs(lse[~empty].astype(np.float64) - ref["lse"][~empty]), R.bound_lse(ref, scale, topk)[~empty]
    assert (lerr <= lbar).all(), (float((lerr / lbar).max()), np.argwhere(lerr > lbar)[:4])
    both = float((err[~empty] / np.maximum(bar[~empty], 1e-300)).max()) if (~empty).any() else 0.0
    return both, float((lerr / lbar).max()) if (~empty).any() else 0.0


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

@pytest.mark.parametrize("h", HEADS)
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

M4, S4, TOPK4, SCALE4 = 5, 700, 320, 576 ** -0.5


@functools.lru_cache(maxsize=None)
def _random_case(h):
    """normal samples rounded to bf16 and an index list with a few invalid positions (read-only once built)"""
    g = torch.Generator(device="cpu").manual_seed(31 + h)
    q = torch.randn((M4, h, R.D_QK), generator=g).to(torch.bfloat16).float().numpy()
    kv = torch.randn((S4, R.D_QK), generator=g).to(torch.bfloat16).float().numpy()
    rng = np.random.default_rng(h)
    idx = np.stack([rng.permutation(S4)[:TOPK4] for _ in range(M4)]).astype(np.int32)
    idx[:, 17], idx[:, 200], idx[1, 300:] = -1, S4 + 3, -1
    idx[2, 40] = idx[2, 41]                                            # a duplicate
    for a in (q, kv, idx):
        a.setflags(write=False)
    return q, kv, idx


def _ordered(q, kv, idx, order):
    """the positions of every token's list reordered: as drawn, or by the score of head 0 (invalid positions keep to the end)"""
    if order == "random":
        return idx
    out = idx.copy()
    rows, valid = R.rows_of(idx, kv.shape[0])
    for t in range(idx.shape[0]):
        sc = kv[np.where(valid[t], rows[t], 0)].astype(np.float64) @ q[t, 0].astype(np.float64)
        sc = np.where(valid[t], sc if order == "ascending" else -sc, np.inf)
        out[t] = idx[t][np.argsort(sc, kind="stable")]
    return out


@pytest.mark.parametrize("order", ("random", "ascending", "descending"))
@pytest.mark.parametrize("h", HEADS)
def test_derived_bound_on_random_data(dga, h, order):
    q, kv, base = _random_case(h)
    idx = _ordered(q, kv, base, order)
    ref = R.reference(q, kv, idx, SCALE4)
    assert ref["count"].tolist() == [318, 298, 318, 318, 318]
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

@pytest.mark.parametrize("h", HEADS)
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
