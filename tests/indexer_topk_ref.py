"""The numpy reference of indexer_topk (include/dga_hip.h, dga_indexer_topk) and the builders of its test cases.  Everything is defined on
the bits: key(x) = bits(x) ^ (0xFFFFFFFF if the sign bit is set else 0x80000000), every NaN 0xFFFFFFFF; column a precedes column b iff its
key is greater, or equal and a < b.  reference() is the definition read literally: a stable argsort of the key, descending, the first
c = min(hi - lo, k), sorted by column, mapped, padded with -1.  literal_loop() picks the columns one by one without sorting."""
import numpy as np

MAX_K = 2048


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def key(x):
    """uint32 keys of a float32 array"""
    b = bits(x)
    k = b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def ranges(m, n, row_starts=None, row_ends=None, context_lens=None, next_n=1):
    """(lo, hi) int64 [m], as the device forms them"""
    assert (row_starts is None) == (row_ends is None) and (row_starts is None or context_lens is None)
    if row_starts is not None:
        lo = np.clip(np.asarray(row_starts, np.int64), 0, n)
        hi = np.clip(np.asarray(row_ends, np.int64), 0, n)
    elif context_lens is not None:
        assert next_n in (1, 2) and m == len(context_lens) * next_n
        ctx = np.clip(np.repeat(np.asarray(context_lens, np.int64), next_n), 0, n)
        lo = np.zeros(m, np.int64)
        hi = np.maximum(ctx - next_n + np.arange(m) % next_n + 1, 0)
    else:
        lo, hi = np.zeros(m, np.int64), np.full(m, n, np.int64)
    return lo, hi


def mapped(col, row, lo, next_n=1, relative=False, block_tables=None, page_size=64, num_blocks=None):
    """what is written for the selected column `col` of row `row`"""
    assert not (relative and block_tables is not None)
    if relative:
        return col - lo
    if block_tables is None:
        return col
    page = col // page_size
    if page >= block_tables.shape[1]:
        return -1
    blk = int(block_tables[row // next_n, page])
    if blk < 0 or blk >= num_blocks:
        return -1
    return blk * page_size + col % page_size


def reference(logits, k, row_starts=None, row_ends=None, context_lens=None, next_n=1, relative=False, block_tables=None, page_size=64,
              num_blocks=None):
    """int32 [M, k]"""
    logits = np.asarray(logits)
    m, n = logits.shape
    assert logits.dtype == np.float32 and 1 <= k <= MAX_K and n >= 1
    assert block_tables is None or context_lens is not None
    lo, hi = ranges(m, n, row_starts, row_ends, context_lens, next_n)
    out = np.full((m, k), -1, np.int32)
    for r in range(m):
        a, b = int(lo[r]), int(hi[r])
        if b <= a:
            continue
        c = min(b - a, k)
        if b - a <= k:
            cols = np.arange(a, b)
        else:
            order = np.argsort(np.uint32(0xFFFFFFFF) - key(logits[r, a:b]), kind="stable")[:c]
            cols = np.sort(order) + a
        out[r, :c] = [mapped(int(col), r, a, next_n, relative, block_tables, page_size, num_blocks) for col in cols]
    return out


def literal_loop(logits, k, **kw):
    """the same by picking, c times, the first column of the order among those left -- tiny rows only"""
    logits = np.asarray(logits)
    m, n = logits.shape
    names = ("next_n", "relative", "block_tables", "page_size", "num_blocks")
    lo, hi = ranges(m, n, kw.get("row_starts"), kw.get("row_ends"), kw.get("context_lens"), kw.get("next_n", 1))
    out = np.full((m, k), -1, np.int32)
    for r in range(m):
        a, b = int(lo[r]), int(hi[r])
        left = list(range(a, b))
        keys = {col: int(key(logits[r, col:col + 1])[0]) for col in left}
        picked = []
        for _ in range(min(len(left), k)):
            best = left[0]
            for col in left[1:]:
                if keys[col] > keys[best]:           # (columns ascend: an equal key never replaces an earlier column)
                    best = col
            picked.append(best)
            left.remove(best)
        for i, col in enumerate(sorted(picked)):
            out[r, i] = mapped(col, r, a, **{name: kw[name] for name in names if name in kw})
    return out


# ---- case builders: (logits float32 [M, N], keyword arguments of reference()) -------------------------------------------------------

def from_bits(words):
    return np.asarray(words, np.uint32).view(np.float32)


SPECIALS = from_bits([0xFFC00001, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000, 0x00000001, 0x3F800000, 0x7F800000, 0x7FC00000])
# -NaN, -inf, -1, -0, +0, the least subnormal, 1, +inf, NaN


def normal_rows(m, n, seed):
    return np.random.default_rng(seed).standard_normal((m, n)).astype(np.float32)


def equal_rows(m, n):
    """rows of one value each: finite, zero of both signs, infinite of both signs, NaN"""
    values = from_bits([0x3FC00000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xC0490FDB, 0x00000001])
    return np.repeat(values[np.arange(m) % len(values), None], n, axis=1)


def two_valued_rows(m, n, k, seed):
    """each row: k - 5 - r columns of 2.5 among columns of 1.25 -- the cut falls 5 + r columns into the ties"""
    rng = np.random.default_rng(seed)
    x = np.full((m, n), 1.25, np.float32)
    for r in range(m):
        x[r, rng.choice(n, size=max(k - 5 - r, 0), replace=False)] = 2.5
    return x


def shared_digit_rows(m, n, seed):
    """1 + i 2^-23, permuted: sign, exponent and the top mantissa bits are shared by the whole row (n <= 2^21)"""
    assert n <= 1 << 21
    rng = np.random.default_rng(seed)
    return np.stack([from_bits(np.uint32(0x3F800000) + rng.permutation(n).astype(np.uint32)) for _ in range(m)])


def lowest_bit_rows(m, n, k, seed):
    """the k-th and (k + 1)-th keys of a row differ in the lowest bit: k - 1 values in [2, 3), then 0x3F800001, 0x3F800000, the rest below 0.9"""
    assert n >= k + 1
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 0.9, size=(m, n)).astype(np.float32)
    for r in range(m):
        at = rng.permutation(n)[:k + 1]
        x[r, at[:k - 1]] = rng.uniform(2.0, 3.0, size=k - 1).astype(np.float32)
        x[r, at[k - 1:]] = from_bits([0x3F800001, 0x3F800000])
    return x


def special_rows(m, n, k, seed):
    """exactly k columns whose key is at least key(+0) -- NaN of both signs' payloads, +inf, normals, subnormals, +0 -- and below the cut
    -0, negative subnormals, negatives, -inf: the cut falls between -0 and +0"""
    assert n >= k + 8
    rng = np.random.default_rng(seed)
    x = np.empty((m, n), np.float32)
    for r in range(m):
        top = from_bits([0x00000000, 0x7FC00000, 0xFFC00123, 0x7F800000, 0x00000001, 0x007FFFFF, 0x3F800000, 0x00000000])[:k]
        top = np.concatenate([top, np.zeros(max(k - len(top), 0), np.float32)])                 # ... and +0 for the rest
        low = from_bits([0x80000000, 0x80000001, 0x807FFFFF, 0xBF800000, 0xFF800000, 0x80000000])
        low = np.concatenate([low, from_bits(np.full(n - k - len(low), 0x80000000, np.uint32))])     # ... and -0 for the rest
        x[r] = np.concatenate([top, low])[rng.permutation(n)]
    return x
