"""The contract of dga_route_slots as one order-independent checker, and the cases it is run on (tests/test_route_model.py runs them
on the numpy model of deepgemm_ascend_amd/parallel.py, tests/test_rows_gpu.py on the kernel).  Plain numpy, seeded; a helper
module, not a conftest.

  check_route_slots   what one call must have done to counts, dest, overflow, tags and inverse, whatever order the rows arrived in
  CASES               the calls: where one workgroup ends (4096 rows), many workgroups on few buckets, accumulating counts, keys and
                      tags at a byte stride inside payload rows, the chunk-major key mode
  run_case            fills the buffers of a case with sentinels, makes its calls through a given routing function, checks each
"""
import numpy as np
import torch

ROWS_PER_BLOCK = 4096                        # csrc/dga_rows.hip ROUTE_ROWS_PER_BLOCK: the rows of one workgroup
FILL = 0xA5                                  # every byte the call may write, and every byte round it, holds this before the call
TAG_SENTINEL = np.frombuffer(bytes([FILL] * 4), np.int32)[0]     # negative: no tag (0 <= key % key_div) equals it
INV_SENTINEL = -7                            # no row number (r + inverse_base >= 0) equals it
GUARD = 3                                    # entries behind counts[buckets), dest[rows) and overflow[1) that must not change


def buckets_of(keys, key_div, key_sub, key_mul, buckets):
    """(valid bool [rows], bucket int64 [rows], tag int64 [rows]) by the rule of include/dga_hip.h; bucket and tag mean nothing
    where valid is False."""
    key = np.asarray(keys).astype(np.int64)
    k = np.where(key >= 0, key, 0)
    hi, lo = k // key_div, k % key_div
    bucket = (lo // key_sub) * key_mul + hi if key_sub else hi
    valid = (key >= 0) & (hi < (key_mul if key_sub else buckets)) & (bucket < buckets)
    return valid, bucket, lo


def check_route_slots(keys, key_div, key_sub, key_mul, buckets, cap, counts_before, counts_after, dest, overflow_before,
                      overflow_after, tags=None, tag_sentinel=None, inverse=None, inverse_sentinel=None, inverse_base=0):
    """Raises AssertionError unless (counts_after, dest, overflow_after, tags, inverse) is a result the contract allows for this
    call.  Which rows of an over-full bucket are dropped, and the order of the rows inside a bucket, are free.
    tags / inverse: the int32 / int64 word of every slot [buckets * cap] after the call; tag_sentinel / inverse_sentinel: what the
    words held before it (a scalar, or an array of the same length when earlier calls have filled some)."""
    keys = np.asarray(keys)
    assert keys.dtype == np.int32 and keys.ndim == 1
    rows = keys.size
    cb = np.asarray(counts_before).astype(np.int64)
    ca = np.asarray(counts_after).astype(np.int64)
    dest = np.asarray(dest).astype(np.int64)
    assert cb.shape == (buckets,) and ca.shape == (buckets,) and dest.shape == (rows,)
    assert ((cb >= 0) & (cb <= cap)).all(), "the contract covers 0 <= counts_before <= cap only"
    valid, bucket, tag = buckets_of(keys, key_div, key_sub, key_mul, buckets)
    hist = np.bincount(bucket[valid], minlength=buckets).astype(np.int64)

    assert (dest[~valid] == -1).all(), f"rows without a bucket were placed: {np.flatnonzero(~valid & (dest != -1))[:8]}"
    want = np.minimum(cap, cb + hist)
    assert np.array_equal(ca, want), f"counts: buckets {np.flatnonzero(ca != want)[:8]} hold {ca[ca != want][:8]}, want {want[ca != want][:8]}"
    over = np.maximum(0, cb + hist - cap)
    assert int(overflow_after) - int(overflow_before) == int(over.sum()), \
        f"overflow went from {overflow_before} to {overflow_after}, {int(over.sum())} rows do not fit"

    placed = valid & (dest != -1)
    at = np.flatnonzero(placed)
    d = dest[at]
    assert ((d >= 0) & (d < buckets * cap)).all(), f"dest outside [0, buckets * cap): rows {at[(d < 0) | (d >= buckets * cap)][:8]}"
    wrong = d // max(cap, 1) != bucket[at]
    assert not wrong.any(), f"rows {at[wrong][:8]} lie in buckets {(d // max(cap, 1))[wrong][:8]}, their own are {bucket[at][wrong][:8]}"
    b_of_slot = np.repeat(np.arange(buckets, dtype=np.int64), ca - cb)
    first = np.cumsum(ca - cb) - (ca - cb)
    slots = b_of_slot * cap + cb[b_of_slot] + (np.arange(b_of_slot.size) - first[b_of_slot])     # every b * cap + s, cb <= s < ca
    got = np.sort(d)
    assert got.size == slots.size and np.array_equal(got, slots), \
        "the placed rows do not take every slot counts_before <= s < counts_after of their bucket exactly once " \
        f"({got.size} rows placed, {slots.size} slots, {got.size - np.unique(got).size} rows share a slot with another)"
    dropped = np.bincount(bucket[valid & (dest == -1)], minlength=buckets)
    assert np.array_equal(dropped, over), f"dropped rows per bucket: buckets {np.flatnonzero(dropped != over)[:8]}"

    for name, words, sentinel, value in (("tags", tags, tag_sentinel, tag[at]), ("inverse", inverse, inverse_sentinel, at + inverse_base)):
        if words is None:
            continue
        words = np.asarray(words).astype(np.int64)
        assert words.shape == (buckets * cap,)
        expect = np.array(np.broadcast_to(np.asarray(sentinel).astype(np.int64), words.shape))
        expect[d] = value
        bad = np.flatnonzero(words != expect)
        assert bad.size == 0, f"{name}: slots {bad[:8]} hold {words[bad[:8]]}, want {expect[bad[:8]]}"


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# One case = one or more calls on the same counts / overflow / inverse (every call after the first accumulates: zero_counts = False,
# inverse_base = the rows of the calls before it).  Per call: rows, the seed, and how the keys are drawn --
#   key_hi    keys are uniform in [0, key_hi)                     hot      every row carries this key instead
#   unused    this share of the rows is -1 (a few: other negatives) beyond   this share is >= key_hi (no bucket)
# Per case: the key mode (key_div, key_sub, key_mul), where the keys lie (key_stride, key_off: bytes; the other bytes of the key rows
# are 0xFF, as the sharded forward's header clearing leaves unused payload rows), the counts before the first call ("zero": the call
# zeroes them itself, zero_counts = True, they hold junk before; "random": uniform in [0, cap] with buckets 0..3 full and 4..7 empty,
# zero_counts = False), the tags ("words": int32 [slots]; (row_bytes, offset): inside uint8 [slots, row_bytes] rows) and whether a
# single drop would be a failure of the case itself (no_drop).

def _case(name, buckets, cap, calls, key_div=1, key_sub=0, key_mul=1, key_stride=4, key_off=0, counts="zero", tags="words",
          no_drop=False):
    calls = [dict(dict(key_hi=buckets * key_div, hot=None, unused=0.0, beyond=0.0), **c) for c in calls]
    return dict(name=name, buckets=buckets, cap=cap, calls=calls, key_div=key_div, key_sub=key_sub, key_mul=key_mul,
                key_stride=key_stride, key_off=key_off, counts=counts, tags=tags, no_drop=no_drop)


B = ROWS_PER_BLOCK
CASES = [
    # where one workgroup ends: 37 buckets, int64 ids read through their low words (the source side's key layout), nothing drops
    _case("block-1", 37, 1, [dict(rows=1, seed=101)], key_stride=8, no_drop=True),
    _case("block-4095", 37, 256, [dict(rows=B - 1, seed=102)], key_stride=8, no_drop=True),
    _case("block-4096", 37, 256, [dict(rows=B, seed=103)], key_stride=8, no_drop=True),
    _case("block-4097", 37, 256, [dict(rows=B + 1, seed=104)], key_stride=8, no_drop=True),
    _case("block-3x+17", 37, 512, [dict(rows=3 * B + 17, seed=105)], key_stride=8, no_drop=True),
    _case("rows-0-zeroing", 37, 64, [dict(rows=0, seed=106)]),
    _case("rows-0-keeping", 37, 64, [dict(rows=0, seed=107)], counts="random"),
    # the size the kernel is built for: 8 workgroups reserve in 256 buckets whose mean load is the capacity / well below it
    _case("prod-cap128", 256, 128, [dict(rows=32768, seed=111)]),
    _case("prod-cap160", 256, 160, [dict(rows=32768, seed=112)]),
    # one bucket takes every row of three workgroups
    _case("hot-fits", 3, 3 * B, [dict(rows=3 * B, seed=121, hot=1)], no_drop=True),
    _case("hot-cap5000", 3, 5000, [dict(rows=3 * B, seed=122, hot=1)]),
    _case("hot-cap0", 3, 0, [dict(rows=3 * B, seed=123, hot=1)]),
    # the receiving side's shape: counts carry on from earlier calls, some buckets are full before the call
    _case("accumulate", 64, 256, [dict(rows=6000, seed=131), dict(rows=5000, seed=132, unused=0.05)], counts="random"),
    # keys in the header of K = 7168 payload rows; unused rows are all 0xFF, a few keys name no bucket
    _case("payload-keys", 32, 12, [dict(rows=300, seed=141, unused=0.15, beyond=0.05)], key_stride=7408, key_off=7392,
          counts="random"),
    # the source side: 256 experts, 8 ranks x 32 experts each, 2 chunks of 16 -> bucket = chunk * 8 + rank, tag = expert on its rank,
    # written into the header of the payload row the token will travel in
    _case("source-chunks", 16, 500, [dict(rows=2 * B + 100, seed=151, key_hi=256, unused=0.02, beyond=0.02)], key_div=32, key_sub=16,
          key_mul=8, key_stride=8, tags=(48, 36)),
    _case("source-ranks", 8, 1000, [dict(rows=2 * B + 100, seed=152, key_hi=256, unused=0.02, beyond=0.02)], key_div=32,
          key_stride=8, tags=(48, 36)),
    # the ABI's largest bucket count, one workgroup
    _case("buckets-4096", 4096, 2, [dict(rows=B, seed=161, beyond=0.01)]),
]
CASES = {c["name"]: c for c in CASES}


def make_keys(call):
    """int32 [rows] of one call."""
    rng = np.random.default_rng(call["seed"])
    rows, hi = call["rows"], call["key_hi"]
    keys = rng.integers(0, hi, size=rows).astype(np.int64) if call["hot"] is None else np.full(rows, call["hot"], np.int64)
    u = rng.random(rows)
    beyond = u < call["beyond"]
    keys[beyond] = np.where(rng.random(rows) < 0.25, 0x7FFFFFFF, hi + rng.integers(0, 5, size=rows))[beyond]
    unused = (u >= call["beyond"]) & (u < call["beyond"] + call["unused"])
    keys[unused] = np.where(rng.random(rows) < 0.1, -0x80000000, -1)[unused]
    return keys.astype(np.int32)


def key_buffer(keys, stride, off):
    """uint8 [rows * stride]: key r at byte r * stride + off, every other byte 0xFF."""
    buf = np.full((keys.size, stride), 0xFF, np.uint8)
    buf[:, off:off + 4] = keys.astype("<i4").view(np.uint8).reshape(-1, 4)
    return buf.reshape(-1)


def counts_before(case):
    """int32 [buckets + GUARD]: what the counts tensor holds before the first call (the guard entries must keep their value)."""
    rng = np.random.default_rng(case["calls"][0]["seed"] + 7)
    n, cap = case["buckets"], case["cap"]
    c = rng.integers(0, cap + 1, size=n + GUARD).astype(np.int32)
    if case["counts"] == "random":
        c[:4], c[4:8] = cap, 0
    else:
        c[:n] = rng.integers(-5, 1 << 20, size=n)           # junk the call has to zero
    c[n:] = TAG_SENTINEL
    return c


def run_case(case, route, device, with_inverse):
    """Make the calls of `case` through route(keys, key_stride, key_off, rows, buckets, cap, counts, dest, overflow, key_div=, key_sub=,
    key_mul=, zero_counts=, tags=, tag_stride=, tag_off=, inverse=, inverse_base=) (the signature of parallel._route_slots) on
    tensors of `device` and check each one; returns the (overflow added, rows placed) of every call."""
    n, cap = case["buckets"], case["cap"]
    slots = n * cap
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    host = lambda t: t.cpu().numpy().copy()
    counts = dev(counts_before(case))
    overflow = dev(np.array([1000] + [int(TAG_SENTINEL)] * GUARD, np.int32))       # non-zero: the call adds to it
    tag_bytes, tag_off = (4, 0) if case["tags"] == "words" else case["tags"]
    tags = dev(np.full((slots, tag_bytes), FILL, np.uint8)) if slots else None
    inverse = dev(np.full(slots + GUARD, INV_SENTINEL, np.int64)) if with_inverse and slots else None
    done, base = [], 0
    for i, call in enumerate(case["calls"]):
        keys = make_keys(call)
        rows = keys.size
        kbuf = key_buffer(keys, case["key_stride"], case["key_off"])
        tkeys = dev(kbuf)
        dest = dev(np.full(rows + GUARD, -5, np.int64))
        zero = case["counts"] == "zero" and i == 0
        cb, ob = host(counts), host(overflow)
        tb = host(tags) if tags is not None else None
        ib = host(inverse) if inverse is not None else None
        route(tkeys, case["key_stride"], case["key_off"], rows, n, cap, counts, dest, overflow, key_div=case["key_div"],
              key_sub=case["key_sub"], key_mul=case["key_mul"], zero_counts=zero, tags=tags, tag_stride=tag_bytes, tag_off=tag_off,
              inverse=inverse, inverse_base=base)
        ca, oa, d = host(counts), host(overflow), host(dest)
        word = lambda t: np.ascontiguousarray(t[:, tag_off:tag_off + 4]).view("<i4").reshape(-1)
        check_route_slots(keys, case["key_div"], case["key_sub"], case["key_mul"], n, cap, np.zeros(n, np.int32) if zero else cb[:n],
                          ca[:n], d[:rows], ob[0], oa[0],
                          tags=word(host(tags)) if tags is not None else None, tag_sentinel=word(tb) if tags is not None else None,
                          inverse=host(inverse)[:slots] if inverse is not None else None,
                          inverse_sentinel=ib[:slots] if inverse is not None else None, inverse_base=base)
        # nothing round the outputs moved, and the inputs are as they were
        assert np.array_equal(ca[n:], cb[n:]) and np.array_equal(oa[1:], ob[1:]) and (d[rows:] == -5).all()
        assert np.array_equal(host(tkeys), kbuf)
        if tags is not None:
            ta = host(tags)
            ta[:, tag_off:tag_off + 4] = tb[:, tag_off:tag_off + 4]
            assert np.array_equal(ta, tb), "bytes of the tag rows outside the tag words changed"
        if inverse is not None:
            assert (host(inverse)[slots:] == INV_SENTINEL).all()
        added = int(oa[0]) - int(ob[0])
        assert not (case["no_drop"] and added), f"{case['name']}: the case is meant to fit, {added} rows were dropped"
        done.append((added, int((d[:rows] >= 0).sum())))
        base += rows
    return done
