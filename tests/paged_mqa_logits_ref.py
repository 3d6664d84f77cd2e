"""float64 reference, the cache layout and the case builder of fp8_paged_mqa_logits and per_token_cast_to_fp8_paged
(tests/test_paged_mqa_logits.py, tests/test_paged_mqa_logits_gpu.py).

    ctx_i       = min(max(context_lens[i], 0), N, 64 max_blocks)
    hi_r        = max(ctx_i - next_n + j + 1, 0)                              row r = i next_n + j
    key n of sequence i = key n % 64 of block block_tables[i, n // 64]
    logits[r,n] = kscale * sum_h weights[r,h] * max(sum_d q[i,j,h,d] k[d], 0)  for n < hi_r,   -inf for hi_r <= n < N

A block of the cache is 8448 bytes: the codes of its 64 keys, key-major, then their 64 float32 scales.  The arithmetic is
mqa_logits_ref.reference's on the gathered operands, per sequence; that module is imported and not changed.  numpy on the host; the cases
are computed once per argument set (functools.lru_cache) and their arrays are read-only."""
import functools

import numpy as np

import mqa_logits_ref as M

D = M.D
BLOCK_KV, BLOCK_BYTES = 64, 8448
SCALES_AT = BLOCK_KV * D
PAD_BYTE = 0xA5
UNUSED = (-1, 0x7FFFFFFF)          # what the unused table entries hold, alternating


def pack(k_codes, kscale, stride=BLOCK_BYTES):
    """uint8 [num_blocks, stride]: block b = k_codes[b] ([64, 128] codes, key-major) then kscale[b] ([64] float32); the bytes from 8448 to a
    larger stride hold PAD_BYTE.  The cache is the view [:, :8448] of it."""
    nb = k_codes.shape[0]
    assert k_codes.shape == (nb, BLOCK_KV, D) and k_codes.dtype == np.uint8 and kscale.shape == (nb, BLOCK_KV) and stride >= BLOCK_BYTES
    buf = np.full((nb, stride), PAD_BYTE, np.uint8)
    buf[:, :SCALES_AT] = k_codes.reshape(nb, SCALES_AT)
    buf[:, SCALES_AT:BLOCK_BYTES] = np.ascontiguousarray(kscale, np.float32).view(np.uint8).reshape(nb, 4 * BLOCK_KV)
    return buf


def unpack(buf):
    """(codes uint8 [num_blocks, 64, 128], scales float32 [num_blocks, 64]) of a packed cache"""
    nb = buf.shape[0]
    scales = np.ascontiguousarray(buf[:, SCALES_AT:BLOCK_BYTES]).view(np.float32).reshape(nb, BLOCK_KV)
    return buf[:, :SCALES_AT].reshape(nb, BLOCK_KV, D).copy(), scales.copy()


def gather(buf, table_row, count):
    """(kg uint8 [count, 128], sg float32 [count], ok bool [count]): keys 0 .. count - 1 of the sequence behind table_row.  A page whose
    entry lies outside [0, num_blocks) has ok False (zero codes, scale 1: nothing is read through it)."""
    codes, scales = unpack(buf)
    nb = buf.shape[0]
    kg, sg, ok = np.zeros((count, D), np.uint8), np.ones(count, np.float32), np.zeros(count, bool)
    for p in range((count + BLOCK_KV - 1) // BLOCK_KV):
        e = int(table_row[p])
        lo, hi = p * BLOCK_KV, min((p + 1) * BLOCK_KV, count)
        if 0 <= e < nb:
            kg[lo:hi], sg[lo:hi], ok[lo:hi] = codes[e, :hi - lo], scales[e, :hi - lo], True
    return kg, sg, ok


def clamp_ctx(context_lens, n, max_blocks):
    return np.minimum(np.clip(np.asarray(context_lens, np.int64), 0, n), BLOCK_KV * max_blocks)


def row_ends(context_lens, next_n, n, max_blocks):
    """hi int64 [B next_n]"""
    ctx = clamp_ctx(context_lens, n, max_blocks)
    return np.maximum(ctx[:, None] - next_n + np.arange(next_n)[None, :] + 1, 0).reshape(-1)


def written(context_lens, next_n, n, max_blocks, clean):
    """bool [B next_n, N]: the elements a call writes -- all of them with clean_logits, else the columns below 64 ceil(ctx_i / 64)"""
    ctx = clamp_ctx(context_lens, n, max_blocks)
    end = np.full_like(ctx, n) if clean else np.minimum((ctx + BLOCK_KV - 1) // BLOCK_KV * BLOCK_KV, n)
    return np.repeat(np.arange(n)[None, :] < end[:, None], next_n, axis=0)


def reference(q, buf, weights, context_lens, tables, n):
    """(logits float64 [B next_n, N], mag float64 [B next_n, N]): the definition, through mqa_logits_ref.reference on each sequence's
    gathered operands.  -inf at and beyond hi_r and on the columns of a needed page whose entry is out of range; mag is 0 there."""
    b, nn, h, d = q.shape
    assert d == D and weights.shape == (b * nn, h) and tables.shape[0] == b and len(context_lens) == b
    ctx = clamp_ctx(context_lens, n, tables.shape[1])
    hi = row_ends(context_lens, nn, n, tables.shape[1])
    logits, mag = np.full((b * nn, n), -np.inf), np.zeros((b * nn, n))
    for i in range(b):
        c = int(ctx[i])
        if c == 0:
            continue
        rows = slice(i * nn, (i + 1) * nn)
        kg, sg, ok = gather(buf, tables[i], c)
        lg, mg = M.reference(q[i], kg, sg, weights[rows], np.zeros(nn, np.int32), hi[rows].astype(np.int32))
        logits[rows, :c] = np.where(ok[None, :], lg, -np.inf)
        mag[rows, :c] = np.where(ok[None, :] & ~np.isneginf(lg), mg, 0.0)
    return logits, mag


def literal_loop(q, buf, weights, context_lens, tables, n):
    """The definition, literally (tiny shapes only)."""
    b, nn, h, _ = q.shape
    nb, max_blocks = buf.shape[0], tables.shape[1]
    out = np.full((b * nn, n), -np.inf)
    for i in range(b):
        ctx = min(max(int(context_lens[i]), 0), n, BLOCK_KV * max_blocks)
        for j in range(nn):
            r = i * nn + j
            for col in range(max(ctx - nn + j + 1, 0)):
                e = int(tables[i, col // BLOCK_KV])
                if not 0 <= e < nb:
                    continue
                block = buf[e]
                k = block[D * (col % BLOCK_KV):D * (col % BLOCK_KV + 1)]
                kscale = float(block[SCALES_AT + 4 * (col % BLOCK_KV):SCALES_AT + 4 * (col % BLOCK_KV + 1)].copy().view(np.float32)[0])
                total = 0.0
                for hh in range(h):
                    s = 0.0
                    for dd in range(D):
                        s += float(M.TABLE[q[i, j, hh, dd]]) * float(M.TABLE[k[dd]])
                    total += float(weights[r, hh]) * max(s, 0.0)
                out[r, col] = kscale * total
    return out


def make_tables(lens, n, max_blocks, seed, share=None, spare=2):
    """(tables int32 [B, max_blocks], num_blocks): each sequence's needed pages name distinct physical blocks, a random permutation of all
    of them; share = (i0, i1) makes page 0 of sequence i1 the block of page 0 of sequence i0; the unused entries hold UNUSED, alternating;
    `spare` blocks are named by nobody."""
    rng = np.random.default_rng([seed, len(lens), n, max_blocks])
    ctx = clamp_ctx(lens, n, max_blocks)
    need = ((ctx + BLOCK_KV - 1) // BLOCK_KV).astype(int)
    num_blocks = max(int(need.sum()) + spare, 1)
    perm = list(rng.permutation(num_blocks))
    tables = np.empty((len(lens), max_blocks), np.int64)
    for i, cnt in enumerate(need):
        for p in range(max_blocks):
            tables[i, p] = perm.pop() if p < cnt else UNUSED[(i + p) % 2]
    if share is not None:
        i0, i1 = share
        assert need[i0] >= 1 and need[i1] >= 1
        tables[i1, 0] = tables[i0, 0]
    return tables.astype(np.int32), num_blocks


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def exact_case(h, nn, lens, n, max_blocks, share=None, seed=0):
    """(q [B, nn, h, 128] codes, buf [num_blocks, 8448], weights [B nn, h], context_lens int32 [B], tables, logits float64 [B nn, N]) on the
    exactly summable operands of mqa_logits_ref.exact_operands"""
    b = len(lens)
    tables, num_blocks = make_tables(lens, n, max_blocks, seed, share)
    q, k, kscale, weights = M.exact_operands(b * nn, num_blocks * BLOCK_KV, h, seed)
    buf = pack(k.reshape(num_blocks, BLOCK_KV, D), kscale.reshape(num_blocks, BLOCK_KV))
    q = q.reshape(b, nn, h, D).copy()
    weights = weights.copy()
    lens = np.asarray(lens, np.int32)
    want, _ = reference(q, buf, weights, lens, tables, n)
    return _frozen(q, buf, weights, lens, tables, want)


@functools.lru_cache(maxsize=None)
def all_codes_case(h, nn, mirrored=False):
    """(q [B, nn, h, 128], buf, weights [B nn, h], context_lens [B], tables, N, logits float64 [B nn, N]): mqa_logits_ref.all_codes_operands
    with its keys packed into pages, twice (two physical copies, in a permuted order, among blocks nobody names); the even sequences
    share one table, the odd ones the other; every sequence has the whole width as its length, so row r = i next_n + j is token r of the
    prefill case short of its last next_n - 1 - j keys; kscale = 1"""
    n = M.MIRROR_N if mirrored else M.CODES_N
    pages = (n + BLOCK_KV - 1) // BLOCK_KV
    q, k, weights, _ = M.all_codes_operands(h, mirrored, pages * BLOCK_KV)
    assert q.shape[0] % nn == 0
    b = q.shape[0] // nn
    rng = np.random.default_rng([h, nn, int(mirrored)])
    num_blocks = 2 * pages + 3
    where = rng.permutation(num_blocks)[:2 * pages].reshape(2, pages)         # physical block of page p of copy c
    codes = np.full((num_blocks, BLOCK_KV, D), M.NAN_CODE, np.uint8)             # a block nobody names holds NaN codes
    codes[where.reshape(-1)] = np.tile(k.reshape(pages, BLOCK_KV, D), (2, 1, 1))
    buf = pack(codes, np.ones((num_blocks, BLOCK_KV), np.float32))
    tables = where[np.arange(b) % 2].astype(np.int32)
    lens = np.full(b, n, np.int32)
    q = q.reshape(b, nn, h, D).copy()
    want, _ = reference(q, buf, weights, lens, tables, n)
    return _frozen(q, buf) + (weights,) + _frozen(lens, tables) + (n,) + _frozen(want)
