"""float64 reference, operand generators and the error bound of fp8_mqa_logits (tests/test_mqa_logits.py, tests/test_mqa_logits_gpu.py).

    s[m,h,n]    = sum_d q[m,h,d] k[n,d]                                   (e4m3 codes, d < 128)
    logits[m,n] = kscale[n] * sum_h weights[m,h] * max(s[m,h,n], 0)       for clamp(ks[m]) <= n < clamp(ke[m]),   -inf elsewhere

Everything here is numpy on the host and is computed once per shape (functools.lru_cache); the arrays it hands out are read-only."""
import functools

import numpy as np

D = 128
HEADS = (32, 64)
BM, BN = 64, 256          # the kernel's token run and key block (DGA_MQA_LOGITS_BLOCK_M / _N)
NAN_CODE = 0x7F


def e4m3_table():
    """OCP e4m3fn as float64: bias 7, no infinity, S.1111.111 = NaN."""
    v = np.arange(256, dtype=np.int64)
    e, m = (v >> 3) & 0xF, v & 0x7
    val = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    val = np.where((e == 0xF) & (m == 0x7), np.nan, val)
    return np.where(v & 0x80, -val, val)


TABLE = e4m3_table()
# the codes of the multiples of 0.5 with magnitude <= 2 (one zero)
HALVES = np.array([int(np.flatnonzero(TABLE == v)[0]) for v in np.arange(-4, 5) / 2.0], dtype=np.uint8)


def clamp_ranges(ks, ke, n):
    return np.clip(np.asarray(ks, np.int64), 0, n), np.clip(np.asarray(ke, np.int64), 0, n)


def in_range(ks, ke, n):
    """bool [M, N]: clamp(ks[m]) <= n < clamp(ke[m])"""
    lo, hi = clamp_ranges(ks, ke, n)
    col = np.arange(n)[None, :]
    return (col >= lo[:, None]) & (col < hi[:, None])


def reference(q, k, kscale, weights, ks, ke, table=TABLE):
    """(logits float64 [M, N] with -inf outside the ranges, mag float64 [M, N] = kscale[n] sum_h |weights| sum_d |q k|).  q uint8 [M, H, 128],
    k uint8 [N, 128] codes.  A NaN code makes its row (q) or column (k) NaN inside the ranges, as the definition's arithmetic does.
    (table: another decoding of the 256 codes -- what a wrong conversion would compute, for the tests of the checkers themselves.)"""
    m, h, d = q.shape
    n = k.shape[0]
    assert d == D and k.shape == (n, D) and weights.shape == (m, h) and kscale.shape == (n,)
    qf, kf = table[q].reshape(m * h, d), table[k]
    w = weights.astype(np.float64)
    with np.errstate(invalid="ignore"):
        s = (qf @ kf.T).reshape(m, h, n)
        s = np.where(s < 0, 0.0, s)                                     # (keeps a NaN)
        logits = (w[:, :, None] * s).sum(axis=1) * kscale.astype(np.float64)[None, :]
        sabs = (np.nan_to_num(np.abs(qf)) @ np.nan_to_num(np.abs(kf)).T).reshape(m, h, n)
    mag = (np.abs(w)[:, :, None] * sabs).sum(axis=1) * np.abs(kscale.astype(np.float64))[None, :]
    return np.where(in_range(ks, ke, n), logits, -np.inf), mag


def triple_loop(q, k, kscale, weights, ks, ke):
    """The definition, literally (tiny shapes only)."""
    m_n, h_n, _ = q.shape
    n_n = k.shape[0]
    out = np.full((m_n, n_n), -np.inf)
    for m in range(m_n):
        lo, hi = min(max(int(ks[m]), 0), n_n), min(max(int(ke[m]), 0), n_n)
        for n in range(lo, hi):
            total = 0.0
            for h in range(h_n):
                s = 0.0
                for d in range(D):
                    s += float(TABLE[q[m, h, d]]) * float(TABLE[k[n, d]])
                total += float(weights[m, h]) * max(s, 0.0)
            out[m, n] = float(kscale[n]) * total
    return out


def bound(h):
    """|got - exact| <= bound(H) * mag on every in-range element.  2^-22: the bf16-exact figure of harness/tolerance.py for the matrix
    instruction's own summation of 128 exact products (profiles/r02_mfma_forms.txt measured 2^-25 per block).  (H + 3) 2^-24: the any-order
    fp32 bound for one product rounding, H - 1 additions and the final scale, with relu(s) <= sum_d |q k|."""
    return 2.0 ** -22 + (h + 3) * 2.0 ** -24


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def exact_operands(m, n, h, seed=0):
    """(q codes [m, h, 128], k codes [n, 128], kscale [n], weights [m, h]) whose result is exact in fp32 in any order: codes from the multiples
    of 0.5 up to 2 in magnitude (a dot product is a multiple of 0.25 of at most 2^9), weights from the multiples of 0.125 in [-4, 4), distinct
    within a token (a partial head sum is a multiple of 2^-5 below 2^17: 22 bits), kscale powers of two.  All of it random."""
    rng = np.random.default_rng([seed, m, n, h])
    q = HALVES[rng.integers(0, len(HALVES), size=(m, h, D))]
    k = HALVES[rng.integers(0, len(HALVES), size=(n, D))]
    grid = np.arange(-32, 32) / 8.0
    weights = np.stack([rng.permutation(grid)[:h] for _ in range(m)]).astype(np.float32).reshape(m, h)
    kscale = (2.0 ** rng.integers(-4, 5, size=n)).astype(np.float32)
    return _frozen(q, k, kscale, weights)


def ranges(kind, m, n):
    """int32 (ks, ke) of the named kind for m tokens over n keys."""
    i = np.arange(m, dtype=np.int64)
    if kind == "full":
        ks, ke = np.zeros(m), np.full(m, n)
    elif kind == "causal":
        ks, ke = np.zeros(m), i + 1
    elif kind == "windows":                       # ends that are no multiple of 4 or 16 and cut a 16-key tile in the middle
        ks = (i * 37 + 5) % max(n - 1, 1)
        ke = np.minimum(ks + 1 + (i * 29 + 7) % 211, n)
        ks, ke = ks | 1, ke - (ke % 4 == 0)
    elif kind == "empty":                         # ke <= ks, equal and crossed
        ks = (i * 11) % (n + 1)
        ke = ks - (i % 3)
    elif kind == "beyond":                        # ks < 0 and ke > n
        ks, ke = -1 - (i * 13) % 300, n + 1 + (i * 17) % 300
    elif kind == "mixed":                         # in one token run: rows that exclude a whole key block next to rows that include it
        third = i % 3
        ks = np.where(third == 0, 3, np.where(third == 1, BN + 9, 2 * BN + 1))
        ke = np.where(third == 0, BN - 7, np.where(third == 1, 2 * BN - 5, n))
        ks, ke = np.minimum(ks, n), np.minimum(ke, n)
    else:
        raise ValueError(kind)
    return np.asarray(ks, np.int32), np.asarray(ke, np.int32)


RANGE_KINDS = ("full", "causal", "windows", "empty", "beyond", "mixed")


@functools.lru_cache(maxsize=None)
def exact_case(m, n, h, kind="full", seed=0):
    """(q, k, kscale, weights, ks, ke, logits float64) on exactly summable operands."""
    q, k, kscale, weights = exact_operands(m, n, h, seed)
    ks, ke = ranges(kind, m, n)
    want, _ = reference(q, k, kscale, weights, ks, ke)
    return (q, k, kscale, weights) + _frozen(ks, ke, want)


def assert_same_values(got, want):
    """got float32 equals the float64 reference as values: -inf exactly where it has it, no NaN, a zero of either sign is zero"""
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    assert not np.isnan(got).any()
    bad = np.argwhere(got.astype(np.float64) != want)
    assert len(bad) == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- every e4m3 code, exactly -------------------------------------------------------------------------------------------------------

FINITE = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.uint8)         # the 254 codes that are no NaN
ONE, MINUS_ONE = (int(np.flatnonzero(TABLE == v)[0]) for v in (1.0, -1.0))
SUBNORMAL = np.array([c for c in range(256) if 1 <= c & 0x7F <= 7], dtype=np.uint8)    # 0x01 .. 0x07 and 0x81 .. 0x87
CODES_N, CODES_M = BN + 37, 2 * D                     # the keys (two blocks, the second ragged) and tokens of the direct case
MIRROR_M, MIRROR_N = 4 * BM + 38, 2 * D               # the tokens (five runs, the last ragged) and keys of the mirrored case


def code_grid(rows, offset=0):
    """uint8 [rows, 128]: FINITE[(r + 3 d + offset) % 254] -- 254 consecutive rows show every dimension every code"""
    return FINITE[(np.arange(rows)[:, None] + 3 * np.arange(D)[None, :] + offset) % len(FINITE)]


def unit_rows(rows):
    """uint8 [rows, 128]: row r is zero but for the code of +1.0 (r < 128) or -1.0 at dimension r % 128"""
    u = np.zeros((rows, D), np.uint8)
    r = np.arange(rows)
    u[r, r % D] = np.where(r < D, ONE, MINUS_ONE)
    return u


@functools.lru_cache(maxsize=None)
def all_codes_operands(h, mirrored=False, n_keys=None):
    """(q codes [M, h, 128], k codes [N, 128], weights [M, h], the head of every token that carries weight 1).
    Direct: k = code_grid (every code in every dimension), token t has one nonzero weight, 1.0, on head (7 t) % h, and that head's q is
    unit_rows' row t; the other heads hold zeros.  Mirrored: the keys are unit_rows, the weighted head of token t holds code_grid's row
    t, and every other head holds other codes (code_grid shifted by 11 per head) under weight 0.
    Every product but one a (token, key) pair is an exact zero or is multiplied by a zero weight, so a logit is relu(+-value(code)):
    exact in fp32 in any order."""
    m, n = (MIRROR_M, MIRROR_N) if mirrored else (CODES_M, CODES_N)
    n = n if n_keys is None else n_keys
    head = (7 * np.arange(m)) % h
    weights = np.zeros((m, h), np.float32)
    weights[np.arange(m), head] = 1.0
    if mirrored:
        shift = 11 * ((np.arange(h)[None, :] - head[:, None]) % h)                          # [m, h]: 0 on the weighted head
        q = FINITE[(np.arange(m)[:, None, None] + 3 * np.arange(D)[None, None, :] + shift[:, :, None]) % len(FINITE)]
        k = unit_rows(n)
    else:
        q = np.zeros((m, h, D), np.uint8)
        q[np.arange(m), head] = unit_rows(m)
        k = code_grid(n)
    return _frozen(np.ascontiguousarray(q), k, weights, head)


@functools.lru_cache(maxsize=None)
def all_codes_case(h, mirrored=False):
    """(q, k, kscale, weights, ks, ke, logits float64) of all_codes_operands under kscale = 1 and full ranges: the direct case gives
    logits[t, n] = relu(+-value(k[n, t % 128])), the mirrored one relu(+-value(q[t, (7 t) % h, n % 128]))"""
    q, k, weights, _ = all_codes_operands(h, mirrored)
    m, n = q.shape[0], k.shape[0]
    kscale = np.ones(n, np.float32)
    ks, ke = ranges("full", m, n)
    want, _ = reference(q, k, kscale, weights, ks, ke)
    return (q, k) + _frozen(kscale) + (weights,) + _frozen(ks, ke, want)


def all_codes_seen(h, mirrored=False):
    """the codes that reach a logit as the operand opposite the unit code: k[n, t % 128] over all (t, n) of the direct case,
    q[t, head_t, n % 128] of the mirrored one"""
    q, k, _, head = all_codes_operands(h, mirrored)
    if mirrored:
        return np.unique(q[np.arange(q.shape[0]), head][:, np.arange(k.shape[0]) % D])
    return np.unique(k[:, np.arange(q.shape[0]) % D])


def broken_table(kind):
    """TABLE as a wrong conversion would decode it: one subnormal code flushed to zero, or -0.5 read as +0.5"""
    t = TABLE.copy()
    if kind == "subnormal":
        t[0x03] = 0.0
    elif kind == "sign":
        t[int(np.flatnonzero(TABLE == -0.5)[0])] = 0.5
    else:
        raise ValueError(kind)
    return t
