"""The float64 reference of split-topk sparse MLA attention -- the partials of sparse_mla_fwd_partial and the merge of sparse_mla_merge --
the split rule, and the bounds the GPU tests hold the two kernels to.  Built on sparse_mla_ref, which it leaves as it is.

    tiles = ceil(topk / 32);  P = min(num_splits, tiles);  split p owns the tiles [p tiles // P, (p + 1) tiles // P)
    partial_out[p], partial_lse[p]   sparse_mla_ref.reference over the positions of split p alone (+0 and -inf without a valid one)
    merge       lse = ln sum_p exp(partial_lse[p]);  out = sum_p exp(partial_lse[p] - lse) partial_out[p];  all -inf: +0 and -inf

The bounds (u = 2^-24; DESIGN.md, "Split-topk sparse MLA decode", derives them).  The exact merge of exact partials is the whole list's
result, sum_p W_p A_p = A, and the partials see the scores the one-pass kernel sees, so (2^-8 + 2 e_s + c(topk)) A carries over.  New
is what makes a computed weight W_p differ from split to split, a relative error of at most eps_w per weight, n = 32 t positions and t
tiles in the longest split:
    36 + n / 4 + t              the partial's l: its weights (34), the lane's chain (n / 4 + 2), l alpha once a tile
    2 t + 32                    the chain of alpha (one v_exp_f32 a tile and the roundings of m - m*), which cancels between N and D inside
                                a split and does not between splits
    4 (|lse_p| + ln n)          partial_lse: v_log_f32, m + log2 l, the product with ln 2 and that constant
    98                          the merge: lse_p - mu and its product with log2 e (3 u of an exponent of at most 32 for every weight above
                                e^-32 of the largest), v_exp_f32
    c_merge     2 eps_w + (2 P + 2) u: a weight's error moves N and D;  P roundings each in L and N;  1 / L and the product with it
    out         |got - out| <= (2^-8 + 2 e_s + c(topk) + c_merge) A + 2^-9 |out|
    lse         |got - lse| <= bound_lse(topk) + eps_w + (P + 4 ln max(P, 2)) u + 2 u |lse|
The merge on its own (exact fp32 partials in): eps_w = 98 u, A = sum_p W_p |partial_out[p]|, and the final rounding at its worst case,
half a bf16 ulp = 2^-8 |out| (the attention's bar has 2^-9 |out| beside a 2^-8 A of which the rounding of P uses half; the merge alone has
no such slack to lean on):  |got - out| <= (2 eps_w + (2 P + 2) u) A + 2^-8 |out|.
"""
import numpy as np

import sparse_mla_ref as R

TILE, U, MAX_SPLITS = R.TILE, R.U, 64


def tiles_of(topk):
    return -(-topk // TILE)


def effective_splits(topk, num_splits):
    return min(num_splits, tiles_of(topk))


def split_ranges(tiles, p):
    """the tiles [lo, hi) of every split"""
    return [(i * tiles // p, (i + 1) * tiles // p) for i in range(p)]


def num_splits_rule(m, heads, topk, cus, min_tiles):
    """dga_sparse_mla_splits: max(1, min(cus // (m head_blocks), tiles // min_tiles, 64))"""
    return max(1, min(cus // (m * -(-heads // 64)), tiles_of(topk) // min_tiles, MAX_SPLITS))


def partials(q, kv, indices, sm_scale, num_splits, index_offsets=None):
    """dict(out [P, M, H, 512], lse [P, M, H], A [P, M, H, 512], P): sparse_mla_ref.reference of every split's positions"""
    idx = np.asarray(indices).reshape(np.asarray(indices).shape[0], -1)
    topk = idx.shape[1]
    p = effective_splits(topk, num_splits)
    refs = [R.reference(q, kv, idx[:, lo * TILE:min(hi * TILE, topk)], sm_scale, index_offsets) for lo, hi in split_ranges(tiles_of(topk), p)]
    return dict(out=np.stack([r["out"] for r in refs]), lse=np.stack([r["lse"] for r in refs]), A=np.stack([r["A"] for r in refs]), P=p)


def merge(partial_out, partial_lse):
    """float64 merge of [P, M, H, 512] and [P, M, H] -> dict(out, lse, A = sum_p W_p |partial_out[p]|, maxlse = max finite |partial_lse|)"""
    po, pl = np.asarray(partial_out, np.float64), np.asarray(partial_lse, np.float64)
    top = pl.max(axis=0)
    mu = np.where(np.isneginf(top), 0.0, top)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.exp(pl - mu)
        total = w.sum(axis=0)
        lse = np.where(total == 0, -np.inf, mu + np.log(total))
        wn = np.where(total == 0, 0.0, w / np.where(total == 0, 1.0, total))
    out = (wn[..., None] * np.where(wn[..., None] == 0, 0.0, po)).sum(axis=0)
    a = (wn[..., None] * np.where(wn[..., None] == 0, 0.0, np.abs(po))).sum(axis=0)
    maxlse = np.where(np.isfinite(pl), np.abs(pl), 0.0).max(axis=0)
    return dict(out=out, lse=lse, A=a, maxlse=maxlse)


def eps_w(topk, p, maxlse):
    """the relative error of one computed split weight, in absolute terms (not in u)"""
    t = -(-tiles_of(topk) // p)
    n = t * TILE
    return ((36 + n / 4 + t) + (2 * t + 32) + 4 * (np.asarray(maxlse) + np.log(n)) + 98) * U


EPS_MERGE = 98 * U


def c_merge(topk, p, maxlse):
    return 2 * eps_w(topk, p, maxlse) + (2 * p + 2) * U


def bound_out(ref, sm_scale, topk, p, maxlse):
    """the bar of every element of the merged out; ref = sparse_mla_ref.reference of the whole list"""
    return R.bound_out(ref, sm_scale, topk) + c_merge(topk, p, maxlse)[..., None] * ref["A"]


def _lse_merge(p, lse):
    return (p + 4 * np.log(max(p, 2))) * U + 2 * U * np.abs(np.where(np.isfinite(lse), lse, 0.0))


def bound_lse(ref, sm_scale, topk, p, maxlse):
    return R.bound_lse(ref, sm_scale, topk) + eps_w(topk, p, maxlse) + _lse_merge(p, ref["lse"])


def merge_bound_out(merged, p):
    """the merge's share, for exact fp32 partials: merged = merge(...) of them"""
    return (2 * EPS_MERGE + (2 * p + 2) * U) * merged["A"] + 2.0 ** -8 * np.abs(merged["out"])


def merge_bound_lse(merged, p):
    return EPS_MERGE + _lse_merge(p, merged["lse"])


# ---- the checkers of the GPU tests ---------------------------------------------------------------------------------------------------

def worst_ratio(got, want, bound):
    """max |got - want| / bound over the finite elements of want; inf where got is not finite there, or where the -inf / NaN elements of
    the two differ"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(bound, want.shape)
    if not np.array_equal(np.isneginf(got), np.isneginf(want)) or not np.array_equal(np.isnan(got), np.isnan(want)):
        return np.inf
    fin = np.isfinite(want)
    if not np.isfinite(got[fin]).all():
        return np.inf
    if not fin.any():
        return 0.0
    err, bar = np.abs(got[fin] - want[fin]), bound[fin]
    return float(np.where(err == 0, 0.0, err / np.where(bar > 0, bar, np.finfo(np.float64).tiny)).max())


def winner_splits(indices, winner_rows, num_splits):
    """int [M, H]: the split that holds the (one) position of every head's winning row in sparse_mla_ref.winners_case"""
    idx = np.asarray(indices)
    p = effective_splits(idx.shape[1], num_splits)
    owner = np.zeros(tiles_of(idx.shape[1]), np.int64)
    for i, (lo, hi) in enumerate(split_ranges(len(owner), p)):
        owner[lo:hi] = i
    out = np.zeros(winner_rows.shape, np.int64)
    for t in range(idx.shape[0]):
        for h, row in enumerate(winner_rows[t]):
            (pos,) = np.flatnonzero(idx[t] == row)
            out[t, h] = owner[pos // TILE]
    return out


def heads_off_their_winning_split(lse_bits, partial_lse_bits, wsplit):
    """the (token, head) pairs whose merged lse is not, bit for bit, the partial_lse of the split that holds the head's winner"""
    want = np.take_along_axis(np.asarray(partial_lse_bits), np.asarray(wsplit)[None], axis=0)[0]
    return [tuple(x) for x in np.argwhere(np.asarray(lse_bits) != want)]


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
