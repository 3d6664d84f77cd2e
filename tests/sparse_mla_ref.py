"""The float64 reference of sparse_mla_fwd on its bf16 inputs, and the bounds its GPU tests hold the kernel to.

    valid(m, j)   indices[m, j] >= 0 and 0 <= r < S with r = indices[m, j] + index_offsets[m]
    s_j           sm_scale sum_d q[m, h, d] kv[r_j, d]          over the valid positions, duplicates once per position
    lse           ln sum_j exp(s_j)                             -inf for a token without a valid position
    out           sum_j exp(s_j - lse) kv[r_j, :512]            +0 for such a token
    A             sum_j p_j |kv[r_j, c]| / sum_j p_j            what the bound of out is relative to
    mag           max_j sum_d |q[m, h, d] kv[r_j, d]|           what the any-order fp32 bound of a score is relative to

Only the rows the valid positions name are read, and only their first 576 columns, so NaN anywhere else in kv does not reach the result.

The bounds (u = 2^-24; DESIGN.md, "Sparse MLA attention", derives them from the kernel's order of operations):
    e_s       sm_scale (576 + 2) u mag: 576 products summed in fp32 in any order, the scale rounded once and multiplied once
    c(topk)   (72 + 1.25 topk + 2 ceil(topk / 32)) u
    out       |got - out| <= (2^-8 + 2 e_s + c) A + 2^-9 |out|
    lse       |got - lse| <= e_s + (40 + topk / 4 + ceil(topk / 32)) u + 4 u (|lse| + ln topk)
"""
import functools

import numpy as np

D_QK, D_V, TILE = 576, 512, 32
U = 2.0 ** -24
ALL_HEADS = tuple(range(16, 129, 16))                    # every head count the operator accepts


def bf16_round(x):
    """x (exactly representable in float32) rounded to bf16, ties to even; float64 out"""
    f = np.ascontiguousarray(x, dtype=np.float32)
    assert np.array_equal(f.astype(np.float64), np.asarray(x, dtype=np.float64), equal_nan=True)
    b = f.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    return np.where(np.isnan(f), np.nan, r.view(np.float32)).astype(np.float64)


def bf16_bits(x):
    """the 16 bits of bf16_round(x)"""
    return (np.ascontiguousarray(bf16_round(x), dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def rows_of(indices, s, index_offsets=None):
    """(rows int64 [M, topk], valid bool [M, topk]) of an int32 index list"""
    idx = np.asarray(indices).astype(np.int64)
    idx = idx.reshape(idx.shape[0], idx.shape[-1])
    rows = idx if index_offsets is None else idx + np.asarray(index_offsets).astype(np.int64)[:, None]
    return rows, (idx >= 0) & (rows >= 0) & (rows < s)


def reference(q, kv, indices, sm_scale, index_offsets=None):
    """q float [M, H, 576], kv float [S, >= 576] (the values the bf16 tensors hold), indices int32 [M, topk] ->
    dict(out [M, H, 512], lse [M, H], A [M, H, 512], mag [M, H], count [M]), all float64 but count"""
    q = np.asarray(q, dtype=np.float64)
    m, h, d = q.shape
    assert d == D_QK
    kv = np.asarray(kv)
    rows, valid = rows_of(indices, kv.shape[0], index_offsets)
    out, a = np.zeros((m, h, D_V)), np.zeros((m, h, D_V))
    lse, mag = np.full((m, h), -np.inf), np.zeros((m, h))
    for t in range(m):
        sel = rows[t][valid[t]]
        if len(sel) == 0:
            continue
        k = kv[sel, :D_QK].astype(np.float64)                    # [n, 576]: only the selected rows, only their 576 columns
        s = sm_scale * (q[t] @ k.T)                               # [h, n]
        mag[t] = (np.abs(q[t]) @ np.abs(k).T).max(axis=1)
        with np.errstate(invalid="ignore"):
            top = s.max(axis=1, keepdims=True)
            p = np.exp(s - top)
            l = p.sum(axis=1, keepdims=True)
            lse[t] = (top + np.log(l))[:, 0]
            out[t] = (p @ k[:, :D_V]) / l
            a[t] = (p @ np.abs(k[:, :D_V])) / l
    return dict(out=out, lse=lse, A=a, mag=mag, count=valid.sum(axis=1))


def direct(q, kv, indices, sm_scale, index_offsets=None):
    """the definition as a loop over tokens, heads and positions (tiny cases only): (out, lse)"""
    m, h, _ = q.shape
    topk = indices.shape[-1]
    out, lse = np.zeros((m, h, D_V)), np.full((m, h), -np.inf)
    for t in range(m):
        for hh in range(h):
            total, acc = 0.0, np.zeros(D_V)
            for j in range(topk):
                i = int(indices[t, j])
                r = i + (0 if index_offsets is None else int(index_offsets[t]))
                if i < 0 or r < 0 or r >= kv.shape[0]:
                    continue
                w = np.exp(sm_scale * float(np.dot(q[t, hh].astype(np.float64), kv[r, :D_QK].astype(np.float64))))
                total += w
                acc += w * kv[r, :D_V]
            if total > 0:
                out[t, hh], lse[t, hh] = acc / total, np.log(total)
    return out, lse


def e_s(sm_scale, mag):
    return abs(sm_scale) * (D_QK + 2) * U * mag


def c_of(topk):
    return (72 + 1.25 * topk + 2 * -(-topk // TILE)) * U


def bound_out(ref, sm_scale, topk):
    """the bar of every element of out: (2^-8 + 2 e_s + c) A + 2^-9 |out|"""
    return (2.0 ** -8 + 2 * e_s(sm_scale, ref["mag"])[:, :, None] + c_of(topk)) * ref["A"] + 2.0 ** -9 * np.abs(ref["out"])


def bound_lse(ref, sm_scale, topk):
    """the bar of every finite element of lse"""
    lse = np.where(np.isfinite(ref["lse"]), ref["lse"], 0.0)
    return e_s(sm_scale, ref["mag"]) + (40 + topk / 4 + -(-topk // TILE)) * U + 4 * U * (np.abs(lse) + np.log(max(topk, 2)))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def scores(q, kv, indices, sm_scale, index_offsets=None):
    """per token, the float64 scores [h, n] of its valid positions, in list order"""
    rows, valid = rows_of(indices, kv.shape[0], index_offsets)
    return [sm_scale * (np.asarray(q[t], np.float64) @ np.asarray(kv[rows[t][valid[t]], :D_QK], np.float64).T) for t in range(len(rows))]


def score_spread(q, kv, indices, sm_scale, index_offsets=None):
    """the largest max - min of one head's scores over its token's valid positions, in nat"""
    return max(float((s.max(axis=1) - s.min(axis=1)).max()) for s in scores(q, kv, indices, sm_scale, index_offsets) if s.shape[1])


# ---- normal samples: the operands of the derived-bound tests ----------------------------------------------------------------------

M4, S4, TOPK4, SCALE4 = 5, 700, 320, 576 ** -0.5
PEAK = 4                 # the factor on SCALE4 of the peaked cases: the spread stays below SPREAD_MAX (test_sparse_mla.py asserts it)
SPREAD_MAX = 60.0        # nat: the smallest weight is e^-60 = 2^-86.6 of the largest, 40 binades inside fp32's normal range
PEAK_HEADS = (16, 48, 128)


@functools.lru_cache(maxsize=None)
def random_case(h):
    """normal samples rounded to bf16 and an index list with a few invalid positions (read-only once built)"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(31 + h)
    q = torch.randn((M4, h, D_QK), generator=g).to(torch.bfloat16).float().numpy()
    kv = torch.randn((S4, D_QK), generator=g).to(torch.bfloat16).float().numpy()
    rng = np.random.default_rng(h)
    idx = np.stack([rng.permutation(S4)[:TOPK4] for _ in range(M4)]).astype(np.int32)
    idx[:, 17], idx[:, 200], idx[1, 300:] = -1, S4 + 3, -1
    idx[2, 40] = idx[2, 41]                                            # a duplicate
    return _frozen(q, kv, idx)


def ordered(q, kv, idx, order):
    """the positions of every token's list reordered: as drawn, or by the score of head 0 (invalid positions keep to the end)"""
    if order == "random":
        return idx
    out = idx.copy()
    rows, valid = rows_of(idx, kv.shape[0])
    for t in range(idx.shape[0]):
        sc = kv[np.where(valid[t], rows[t], 0)].astype(np.float64) @ q[t, 0].astype(np.float64)
        sc = np.where(valid[t], sc if order == "ascending" else -sc, np.inf)
        out[t] = idx[t][np.argsort(sc, kind="stable")]
    return out


@functools.lru_cache(maxsize=None)
def long_case(h):
    """topk = 2048 (64 tiles), every position valid and distinct: (q [2, h, 576], kv [2100, 576], indices [2, 2048]) on normal samples"""
    import torch
    m, s, topk = 2, 2100, 2048
    g = torch.Generator(device="cpu").manual_seed(77 + h)
    q = torch.randn((m, h, D_QK), generator=g).to(torch.bfloat16).float().numpy()
    kv = torch.randn((s, D_QK), generator=g).to(torch.bfloat16).float().numpy()
    rng = np.random.default_rng(1000 + h)
    idx = np.stack([rng.permutation(s)[:topk] for _ in range(m)]).astype(np.int32)
    return _frozen(q, kv, idx)


# ---- one winner per head: the heads told apart exactly ---------------------------------------------------------------------------

WIN_M, WIN_S, WIN_TOPK, WIN_SCALE, WIN_INVALID = 3, 400, 160, 2.0 ** -3, 8


@functools.lru_cache(maxsize=None)
def winners_case(h, seed=0):
    """(q [3, h, 576], kv [400, 576], indices int32 [3, 160], sm_scale, winner_rows int64 [3, h]): head hh of token t scores exactly 512
    against row winner_rows[t, hh] and 0 or -512 against every other row of the token's list, so out[t, hh] is that row's first 512
    columns bit for bit and lse is 512.
    kv holds small integers in the value columns and zeros in the 64 rope columns, but for 128 rows W: W_i has +64 in rope column i
    (i < 64), W_{64 + i} has -64 there.  q[t, hh] is zero but for +-64 in the rope column of its winner: 64 * 64 / 8 = 512 against it,
    -512 against the row of the opposite sign, 0 against everything else.  A token's h winners are a random choice of the 128, in a
    random order over the heads; its list holds them and rows outside W, the winners dealt over the tiles in turn (every tile has
    some), at random positions; WIN_INVALID positions hold -1: the last three of the list (a ragged last tile) and one more in every tile."""
    assert h in ALL_HEADS
    rng = np.random.default_rng([seed, h])
    tiles = WIN_TOPK // TILE
    assert tiles + 3 == WIN_INVALID
    kv = rng.integers(-8, 9, size=(WIN_S, D_QK)).astype(np.float32)
    kv[:, D_V:] = 0
    w_rows = rng.permutation(WIN_S)[:128]
    for i in range(64):
        kv[w_rows[i], D_V + i], kv[w_rows[64 + i], D_V + i] = 64, -64
    others = np.setdiff1d(np.arange(WIN_S), w_rows)
    q = np.zeros((WIN_M, h, D_QK), np.float32)
    idx = np.full((WIN_M, WIN_TOPK), -1, np.int32)
    win = np.zeros((WIN_M, h), np.int64)
    for t in range(WIN_M):
        chosen = rng.permutation(128)[:h]                              # head hh -> W_chosen[hh]
        for hh, w in enumerate(chosen):
            q[t, hh, D_V + w % 64] = 64 if w < 64 else -64
            win[t, hh] = w_rows[w]
        free = np.ones(WIN_TOPK, bool)
        free[WIN_TOPK - 3:] = False
        free[np.arange(tiles) * TILE + rng.integers(0, TILE - 3, tiles)] = False    # and one in every tile: 3 + 5 = WIN_INVALID
        for i, hh in enumerate(rng.permutation(h)):                    # winners: tile i % tiles, a free position of it
            tile = i % tiles
            pos = tile * TILE + rng.choice(np.flatnonzero(free[tile * TILE:(tile + 1) * TILE]))
            idx[t, pos], free[pos] = win[t, hh], False
        idx[t, free] = rng.choice(others, int(free.sum()))
    return _frozen(q, kv, idx) + (WIN_SCALE,) + _frozen(win)


def winner_bits(kv, winner_rows):
    """uint16 [M, h, 512]: the bf16 bits of every head's winning row (the row itself, not the float64 out: its e^-512 tail would turn a
    +0 into -0)"""
    return bf16_bits(np.asarray(kv)[np.asarray(winner_rows), :D_V])


def heads_off_their_winner(bits, kv, winner_rows):
    """the (token, head) pairs whose 512 output bit patterns are not their winner's row: empty when the kernel is right"""
    return [tuple(p) for p in np.argwhere((np.asarray(bits) != winner_bits(kv, winner_rows)).any(axis=2))]


# ---- indices and offsets at the ends of the int32 range --------------------------------------------------------------------------

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def extremes_case(s=40, topk=40):
    """(indices int32 [5, topk], offsets int32 [5], the rows int64 each token's valid positions name, in list order).  rows_of forms
    index + offset in int64 and is the definition; the sums of tokens 1 and 2 do not fit an int32."""
    idx = np.full((5, topk), -1, np.int32)
    off = np.array([-INT_MAX + 5, INT_MAX, INT_MIN, 0, 7], np.int64).astype(np.int32)
    # token 0: the largest index under the most negative offset that keeps it valid names row 5; INT_MAX - k names row 5 - k
    idx[0, [0, 9, 33, 39]] = [INT_MAX, INT_MAX - 2, INT_MAX - 5, INT_MAX]
    idx[0, [1, 34]] = [INT_MIN, INT_MAX - 6]                           # negative; row -1
    # token 1: INT_MAX + INT_MAX = 2^32 - 2 and 3 + INT_MAX = 2^31 + 2 are beyond every S: nothing valid
    idx[1, [0, 5, 32]] = [INT_MAX, 3, INT_MIN]
    # token 2: 5 + INT_MIN and INT_MAX + INT_MIN = -1 are negative rows, INT_MIN + INT_MIN = -2^32 is 0 modulo 2^32: nothing valid
    idx[2, [2, 31, 39]] = [5, INT_MAX, INT_MIN]
    # token 3: no offset; the two ends of the range beside eight ordinary positions
    idx[3, [0, 1, 38, 39]] = [INT_MIN, INT_MAX, INT_MAX, INT_MIN]
    idx[3, 2:34:4] = [3, 17, s - 1, 0, 17, 22, 9, 30]
    # token 4: an ordinary offset; s - 7 + 7 = s is out, INT_MAX + 7 is out, two ordinary positions
    idx[4, [0, 1, 35, 36, 37]] = [s - 7, INT_MAX, INT_MIN, s - 8, 4]
    want = [[5, 3, 0, 5], [], [], [3, 17, s - 1, 0, 17, 22, 9, 30], [s - 1, 11]]
    return idx, off, want
