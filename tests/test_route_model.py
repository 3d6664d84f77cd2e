"""tests/route_cases.py on the CPU: the checker accepts what the numpy model of dga_route_slots (the CPU branch of
parallel._route_slots, which the gloo routing tests run on) does with every case that tests/test_rows_gpu.py gives the kernel, and
rejects assignments that break the contract.  The model fills slots in row order; the checker does not look at the order."""
import numpy as np
import pytest
import torch

from route_cases import CASES, ROWS_PER_BLOCK, buckets_of, check_route_slots, counts_before, make_keys, run_case


@pytest.mark.parametrize("name", list(CASES))
def test_model_passes_the_checker(name):
    from deepgemm_ascend_amd.parallel import _route_slots
    done = run_case(CASES[name], _route_slots, torch.device("cpu"), with_inverse=False)
    assert len(done) == len(CASES[name]["calls"])


def test_cases_reach_what_they_are_for():
    """The list, not the code under test: more than one workgroup, full and part-full buckets in one call, and a crossing of the
    capacity inside a later workgroup's rows."""
    def load(name, i=0):
        c = CASES[name]
        keys = make_keys(c["calls"][i])
        valid, bucket, _ = buckets_of(keys, c["key_div"], c["key_sub"], c["key_mul"], c["buckets"])
        return c, keys, valid, np.bincount(bucket[valid], minlength=c["buckets"])
    assert sorted(c["calls"][0]["rows"] for n, c in CASES.items() if n.startswith("block-")) == \
        [1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK, ROWS_PER_BLOCK + 1, 3 * ROWS_PER_BLOCK + 17]
    for name, lo, hi in (("prod-cap128", 0.3, 0.7), ("prod-cap160", 0.0, 0.05)):
        c, keys, valid, hist = load(name)
        assert keys.size == 8 * ROWS_PER_BLOCK and c["buckets"] == 256 and valid.all()
        assert lo < (hist > c["cap"]).mean() <= hi and (hist > c["cap"]).any()
    c, keys, valid, hist = load("hot-cap5000")
    assert ROWS_PER_BLOCK < c["cap"] < 2 * ROWS_PER_BLOCK and hist.max() == keys.size == 3 * ROWS_PER_BLOCK
    c, keys, valid, hist = load("payload-keys")
    assert (keys == -1).any() and (keys >= c["buckets"]).any() and valid.any()
    for name in ("source-chunks", "source-ranks"):
        c, keys, valid, hist = load(name)
        assert keys.size == 2 * ROWS_PER_BLOCK + 100 and (hist > 0).all() and (hist > c["cap"]).any() and (hist < c["cap"]).any()
    c, keys, valid, hist = load("buckets-4096")
    assert keys.size <= ROWS_PER_BLOCK and (hist > c["cap"]).any() and hist[-1] > 0


# ---- the checker rejects what breaks the contract: a small call by hand, then one thing wrong at a time

def _good():
    # 3 buckets, cap 2, bucket 1 holds one row already; rows 0..6: buckets 0, 1, 1 (dropped: full), 2, unused, no bucket, 0
    return dict(keys=np.array([0, 1, 1, 2, -1, 3, 0], np.int32), key_div=1, key_sub=0, key_mul=1, buckets=3, cap=2,
                counts_before=np.array([0, 1, 0]), counts_after=np.array([2, 2, 1]), dest=np.array([1, 3, -1, 4, -1, -1, 0]),
                overflow_before=5, overflow_after=6, tags=np.array([0, 0, -9, 0, 0, -9]), tag_sentinel=-9,
                inverse=np.array([106, 100, -7, 101, 103, -7]), inverse_sentinel=-7, inverse_base=100)


def test_checker_accepts_the_hand_made_call():
    check_route_slots(**_good())
    other = _good()                      # the other row of the full bucket is dropped, the rows of bucket 0 swap: as good
    other.update(dest=np.array([0, -1, 3, 4, -1, -1, 1]), inverse=np.array([100, 106, -7, 102, 103, -7]))
    check_route_slots(**other)


@pytest.mark.parametrize("name", ["block-3x+17", "prod-cap128", "hot-cap5000", "accumulate", "source-chunks"])
def test_checker_accepts_another_order(name):
    """An assignment no row-order model gives: blocks of 4096 rows reserve a range per bucket each, the last block first, and inside a
    block the last row takes the first slot; the rows a block cannot place are the tail of its range (the device kernel's scheme)."""
    c = CASES[name]
    keys = make_keys(c["calls"][0])
    n, cap = c["buckets"], c["cap"]
    valid, bucket, tag = buckets_of(keys, c["key_div"], c["key_sub"], c["key_mul"], n)
    before = np.zeros(n, np.int64) if c["counts"] == "zero" else counts_before(c)[:n].astype(np.int64)
    counts, dest, overflow = before.copy(), np.full(keys.size, -1, np.int64), 0
    for r0 in reversed(range(0, keys.size, ROWS_PER_BLOCK)):
        rows = np.arange(r0, min(keys.size, r0 + ROWS_PER_BLOCK))[::-1]
        rows = rows[valid[rows]]
        for b in np.unique(bucket[rows]):
            mine = rows[bucket[rows] == b]
            slot = counts[b] + np.arange(mine.size)
            dest[mine[slot < cap]] = b * cap + slot[slot < cap]
            overflow += int((slot >= cap).sum())
            counts[b] = min(cap, counts[b] + mine.size)
    words = np.full(n * cap, -9, np.int64)
    words[dest[dest >= 0]] = tag[dest >= 0]
    check_route_slots(keys, c["key_div"], c["key_sub"], c["key_mul"], n, cap, before, counts, dest, 3, 3 + overflow, tags=words,
                      tag_sentinel=-9)
    from deepgemm_ascend_amd.parallel import _route_slots
    m_counts, m_dest = torch.from_numpy(before.astype(np.int32)), torch.empty(keys.size, dtype=torch.int64)
    _route_slots(torch.from_numpy(keys), 4, 0, keys.size, n, cap, m_counts, m_dest, torch.zeros(1, dtype=torch.int32),
                 key_div=c["key_div"], key_sub=c["key_sub"], key_mul=c["key_mul"], zero_counts=False)
    assert np.array_equal(m_counts.numpy(), counts) and not np.array_equal(m_dest.numpy(), dest), "this is the row order again"


@pytest.mark.parametrize("what,change", [
    ("two rows in one slot", dict(dest=np.array([1, 3, -1, 4, -1, -1, 1]))),
    ("a slot past counts_after", dict(dest=np.array([1, 3, -1, 5, -1, -1, 0]))),
    ("a row in the neighbour bucket's slot", dict(dest=np.array([1, -1, -1, 3, -1, -1, 0]))),
    ("a slot below counts_before", dict(dest=np.array([1, 2, -1, 4, -1, -1, 0]))),
    ("a count one short", dict(counts_after=np.array([1, 2, 1]))),
    ("a count one over", dict(counts_after=np.array([2, 2, 2]))),
    ("a count past the capacity", dict(counts_after=np.array([2, 3, 1]))),
    ("a row that fits dropped", dict(dest=np.array([1, 3, -1, -1, -1, -1, 0]))),
    ("an unused row placed", dict(dest=np.array([1, 3, -1, 4, 5, -1, 0]), counts_after=np.array([2, 2, 2]))),
    ("a key without a bucket placed", dict(dest=np.array([1, 3, -1, 4, -1, 5, 0]), counts_after=np.array([2, 2, 2]))),
    ("overflow overwritten", dict(overflow_after=1)),
    ("overflow not counted", dict(overflow_after=5)),
    ("a wrong tag", dict(tags=np.array([0, 0, -9, 1, 0, -9]))),
    ("a tag in a slot no row took", dict(tags=np.array([0, 0, 0, 0, 0, -9]))),
    ("inverse names another row", dict(inverse=np.array([100, 106, -7, 101, 103, -7]))),
    ("inverse without its base", dict(inverse=np.array([6, 0, -7, 1, 3, -7]))),
    ("inverse written in a slot no row took", dict(inverse=np.array([106, 100, -7, 101, 103, 104]))),
])
def test_checker_rejects(what, change):
    bad = _good()
    bad.update(change)
    with pytest.raises(AssertionError):
        check_route_slots(**bad)


def test_checker_rejects_a_corrupted_model_result():
    """The same on a case of the list: the model's own dest, then two rows of the hot bucket moved into one slot."""
    from deepgemm_ascend_amd.parallel import _route_slots
    c = CASES["hot-cap5000"]
    keys = make_keys(c["calls"][0])
    counts = torch.zeros(c["buckets"], dtype=torch.int32)
    dest = torch.empty(keys.size, dtype=torch.int64)
    overflow = torch.zeros(1, dtype=torch.int32)
    _route_slots(torch.from_numpy(keys), 4, 0, keys.size, c["buckets"], c["cap"], counts, dest, overflow)
    args = (keys, 1, 0, 1, c["buckets"], c["cap"], np.zeros(c["buckets"], np.int32), counts.numpy())
    check_route_slots(*args, dest.numpy(), 0, int(overflow[0]))
    twice = dest.numpy().copy()
    twice[ROWS_PER_BLOCK] = twice[0]
    with pytest.raises(AssertionError):
        check_route_slots(*args, twice, 0, int(overflow[0]))
