"""GPU: indexer_topk against tests/indexer_topk_ref.py.  Every comparison is torch.equal with the numpy reference on the very input; the
inputs are float32 arrays built on the host, `out` starts as 7s, and the logits sit in a buffer one column wider than N unless a case says
otherwise (so the rows are 4 bytes apart from any alignment the kernel might hope for).  C is the kernel's candidate buffer."""
import numpy as np
import pytest
import torch

import indexer_topk_ref as R

pytestmark = pytest.mark.gpu

KS = (1, 7, 64, 2048)
NAN = np.float32("nan")


def _cand():
    from deepgemm_ascend_amd import api
    return api.INDEXER_TOPK_CANDIDATES


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _view(x, pad=1):
    """the device tensor of x as a column slice of a buffer `pad` columns wider, the spare columns NaN"""
    m, n = x.shape
    wide = np.full((m, n + pad), NAN, np.float32)
    wide[:, :n] = x
    view = _dev(wide)[:, :n]
    assert pad == 0 or m < 2 or view.stride(0) == n + pad
    return view


def _call(dga, x, k, pad=1, **kw):
    out = torch.full((x.shape[0], k), 7, dtype=torch.int32, device="cuda")
    args = {name: _dev(v) if isinstance(v, np.ndarray) else v for name, v in kw.items()}
    got = dga.indexer_topk(_view(x, pad), k, out=out, sync=True, **args)
    assert got is out
    return out.cpu()


def _check(dga, x, k, pad=1, **kw):
    got, want = _call(dga, x, k, pad, **kw), torch.from_numpy(R.reference(x, k, **kw))
    assert got.dtype == torch.int32 and torch.equal(got, want), (torch.nonzero((got != want).any(dim=1)).flatten().tolist()[:8], k)
    return got


def _i32(*values):
    return np.array(values, np.int32)


@pytest.mark.parametrize("k", KS)
def test_rows_no_longer_than_k_read_no_logits(dga, k):
    lengths = [0, 1, k - 1, k, k + 1, k + 1, 0, k]
    n = k + 9
    x = np.full((8, n), NAN, np.float32)
    x[4:6] = R.normal_rows(2, n, seed=k)                                  # the two rows that are read
    for lo in (0, 3):
        starts = _i32(*([lo] * 8))
        got = _check(dga, x, k, row_starts=starts, row_ends=starts + _i32(*lengths))
        assert (got[0] == -1).all() and got[1, 0] == lo and got[3].tolist() == list(range(lo, lo + k)) and (got[4] >= lo).all()


@pytest.mark.parametrize("k", KS)
def test_misaligned_rows_and_both_ragged_ends(dga, k):
    n, m = 2 * 4096 + 301, 12
    x = R.normal_rows(m, n, seed=10 + k)
    starts = _i32(*[(1, 3, 5)[r % 3] for r in range(m)])
    ends = _i32(*[n - r for r in range(m)])                               # every residue of hi, rows 4 (N + 1) bytes apart
    _check(dga, x, k, row_starts=starts, row_ends=ends)
    _check(dga, x, k, row_starts=starts, row_ends=ends, relative=True)
    _check(dga, x, k, pad=0, row_starts=starts, row_ends=ends)           # ... and N itself odd


@pytest.mark.parametrize("k", KS)
def test_random_normal_rows(dga, k):
    x = R.normal_rows(8, 65536 + 17, seed=k)
    got = _check(dga, x, k)
    again = _call(dga, x, k)
    assert torch.equal(got, again)                                        # two calls, identical bytes
    assert (got >= 0).all() and (got[:, 1:] > got[:, :-1]).all()


@pytest.mark.parametrize("k", KS)
def test_nothing_outside_the_range_matters(dga, k):
    m, n = 9, 3 * 4096 + 50
    x = R.normal_rows(m, n, seed=20 + k)
    starts = _i32(0, 1, 2, 3, 4, 700, 4096, 4097, 5000)
    ends = _i32(n - 5, n - 4, n - 3, n - 2, n - 1, n - 700, n - 4096, 9000, 5000 + k + 1)
    inside = (np.arange(n)[None] >= starts[:, None]) & (np.arange(n)[None] < ends[:, None])
    clean = np.where(inside, x, -np.float32("inf")).astype(np.float32)
    want = _check(dga, clean, k, row_starts=starts, row_ends=ends)
    for fill in (np.float32("inf"), NAN, np.float32(3e38)):
        dirty = np.where(inside, x, fill).astype(np.float32)
        assert torch.equal(_check(dga, dirty, k, row_starts=starts, row_ends=ends), want)


@pytest.mark.parametrize("k", KS)
def test_a_row_of_equal_values_gives_the_lowest_columns(dga, k):
    n = 2 * _cand() + 133
    x = R.equal_rows(8, n)
    got = _check(dga, x, k)
    assert torch.equal(got, torch.arange(k, dtype=torch.int32).expand(8, k))
    starts = _i32(1, 2, 3, 4, 5, 6, 7, 4099)
    got = _check(dga, x, k, row_starts=starts, row_ends=_i32(*([n] * 8)))
    assert torch.equal(got, torch.from_numpy(starts)[:, None] + torch.arange(k, dtype=torch.int32)[None])


@pytest.mark.parametrize("k", KS)
def test_a_boundary_inside_the_ties(dga, k):
    _check(dga, R.two_valued_rows(8, 2 * _cand() + 99, k, seed=1), k)     # more ties than the candidate buffer holds
    _check(dga, R.two_valued_rows(8, k + 40, k, seed=2), k)               # ... and a handful


@pytest.mark.parametrize("k", KS)
def test_rows_that_share_every_top_digit(dga, k):
    x = R.shared_digit_rows(8, _cand() + 1234, seed=k)                    # the first bin overflows the candidate buffer
    _check(dga, x, k)
    _check(dga, -x, k)


@pytest.mark.parametrize("k", KS)
def test_a_misleading_sample_changes_nothing(dga, k):
    """The kernel guesses a lower bound of the threshold from 4096 columns spread evenly over the row -- four at 4 (t G // 1024), t < 1024,
    G the row's 16-byte groups -- and falls back to counting walks when the guess gathers fewer than k or more than C keys.  Rows whose
    sampled columns alone are large (too few above the guess) and rows whose sampled columns alone are small (too many)."""
    n = 3 * _cand()
    groups = n // 4
    sampled = (4 * (np.arange(1024) * groups // 1024)[:, None] + np.arange(4)[None]).ravel()
    x = R.normal_rows(8, n, seed=70 + k)
    x[:4] -= 100.0
    x[:4, sampled] += 100.0
    x[4:, sampled] -= 100.0
    _check(dga, x, k, pad=0)                                              # (rows 16-byte aligned: the sample is where the docstring says)
    _check(dga, x, k)


@pytest.mark.parametrize("k", KS)
def test_neighbours_that_differ_in_the_lowest_bit(dga, k):
    x = R.lowest_bit_rows(8, 3 * 4096 + 7, k, seed=k)
    got = _check(dga, x, k)
    for r in range(8):
        picked = R.bits(x[r, got[r].numpy()])
        assert (picked == 0x3F800001).sum() == 1 and (picked == 0x3F800000).sum() == 0


@pytest.mark.parametrize("k", KS)
def test_sorted_rows(dga, k):
    n = 20011
    x = np.sort(R.normal_rows(8, n, seed=30 + k), axis=1)
    x[4:] = x[4:, ::-1]
    got = _check(dga, x, k)
    assert got[0].tolist() == list(range(n - k, n)) and got[7].tolist() == list(range(k))


@pytest.mark.parametrize("k", KS)
def test_special_values_around_the_threshold(dga, k):
    x = R.special_rows(8, k + 4096 + 77, k, seed=k)
    got = _check(dga, x, k)
    for r in range(8):
        keys = R.key(x[r])
        assert np.array_equal(np.sort(got[r].numpy()), np.nonzero(keys >= 0x80000000)[0])       # +0 in, -0 out
    _check(dga, x, max(k - 1, 1))                                         # the cut inside the +0 ties (k >= 9)
    if k < R.MAX_K:
        _check(dga, x, k + 1)                                             # ... and inside the -0 ties


@pytest.mark.parametrize("next_n", (1, 2))
@pytest.mark.parametrize("k", KS)
def test_the_lengths_form(dga, k, next_n):
    n, b = 4096 + k + 60, 8
    lens = _i32(-3, 0, 1, next_n - 1, k + next_n, n, n + 500, n - 1)      # negative, below next_n, barely longer than k, N, beyond N
    x = R.normal_rows(b * next_n, n, seed=40 + k)
    got = _check(dga, x, k, context_lens=lens, next_n=next_n)
    assert (got[:next_n] == -1).all() and (got[-1] >= 0).all()
    _check(dga, x, k, context_lens=lens, next_n=next_n, relative=True)    # lo = 0: the same numbers


@pytest.mark.parametrize("k", KS)
def test_relative_indices(dga, k):
    m, n = 8, 4096 + k + 300
    x = R.normal_rows(m, n, seed=50 + k)
    starts = _i32(0, 1, 130, 4095, 200, 7, n - k - 1, n)
    ends = _i32(n, n, n - 1, n, 200 + k, n - 9, n, n)
    got, plain = _check(dga, x, k, row_starts=starts, row_ends=ends, relative=True), _check(dga, x, k, row_starts=starts, row_ends=ends)
    shifted = plain - torch.from_numpy(starts)[:, None]
    assert torch.equal(got[plain >= 0], shifted[plain >= 0]) and (got[plain < 0] == -1).all()


@pytest.mark.parametrize("page", (64, 1))
@pytest.mark.parametrize("k", (64, 2048))
def test_physical_slots_through_the_block_table(dga, k, page):
    """The scores fall with the column apart from noise, so the selected columns lie on the first pages: entry 1 of sequence 1 is -1 and
    entry 0 of sequence 2 is num_blocks, both on selected pages; every page from `far` on is unselected and its entries are garbage."""
    b, nn = 4, 2
    n = 3 * k + 141
    max_blocks = (n + page - 1) // page
    num_blocks = b * max_blocks + 3
    rng = np.random.default_rng(k + page)
    x = (rng.standard_normal((b * nn, n)) - 8.0 / k * np.arange(n)[None]).astype(np.float32)      # column 2 k is 16 sigma down
    lens = _i32(n, n - 1, n - 130, k + 5)
    tables = rng.permutation(num_blocks)[:b * max_blocks].reshape(b, max_blocks).astype(np.int32)
    far = 2 * k // page + 1
    tables[:3, far:] = _i32(0x7FFFFFFF, -9, num_blocks + 1)[np.arange(max_blocks - far) % 3][None]
    tables[1, 1], tables[2, 0] = -1, num_blocks
    kw = dict(context_lens=lens, next_n=nn, block_tables=tables, page_size=page, num_blocks=num_blocks)
    got = _check(dga, x, k, **kw)
    columns = R.reference(x, k, context_lens=lens, next_n=nn)
    assert columns[:6].max() < far * page                                 # no garbage entry belongs to a selected column
    assert (got[2:4] == -1).sum() >= 2 and (got[4:6] == -1).sum() >= 2 and (got[:2] >= 0).all()
    assert (got[6:] >= 0).all()                                           # (sequence 3 takes nearly its whole range: real entries throughout)
    # a table shorter than the range: columns beyond it give -1
    short = dict(kw, block_tables=np.ascontiguousarray(tables[:, :max(far // 2, 1)]))
    got = _check(dga, x, k, **short)
    assert (got == -1).any()


def test_out_is_optional_and_no_rows_is_no_launch(dga):
    x = R.normal_rows(8, 5000, seed=60)
    want = torch.from_numpy(R.reference(x, 64))
    got = dga.indexer_topk(_dev(x), 64, sync=True)
    assert got.dtype == torch.int32 and got.shape == (8, 64) and torch.equal(got.cpu(), want)
    got = dga.indexer_topk(_dev(x), sync=True)                            # k = 2048
    assert got.shape == (8, 2048) and torch.equal(got.cpu(), torch.from_numpy(R.reference(x, 2048)))
    own = torch.full((8, 64), 7, dtype=torch.int32, device="cuda")
    assert dga.indexer_topk(_dev(x), 64, out=own, sync=True) is own and torch.equal(own.cpu(), want)
    empty = dga.indexer_topk(torch.empty((0, 5000), device="cuda"), 64, sync=True)
    assert empty.shape == (0, 64) and empty.dtype == torch.int32
    empty = dga.indexer_topk(torch.empty((0, 5000), device="cuda"), 64, context_lens=torch.empty(0, dtype=torch.int32, device="cuda"), next_n=2,
                             out=torch.empty((0, 64), dtype=torch.int32, device="cuda"), sync=True)
    assert empty.shape == (0, 64)
    one = R.normal_rows(1, 1, seed=0)                                     # one row, one column
    assert dga.indexer_topk(_dev(one), 3, sync=True).cpu().tolist() == [[0, -1, -1]]
