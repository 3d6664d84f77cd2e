"""The float64 reference of indexer_kl_loss on the values its inputs hold (lse and logits as given), its operands, and the bounds its GPU
tests hold the kernel to.  Over the valid positions (sparse_mla_ref.rows_of), duplicates once per position:
    p_hj = exp(sm_scale q_h . kv[r_j] - lse_h)   t_j = mean_h p_hj   L = ln sum_j exp(logits[r_j])   a_j = logits[r_j] - L   y_j = exp(a_j)
    loss = sum_j t_j (ln t_j - a_j)              d_logits_j = grad_scale (y_j - t_j)
The bounds (u = 2^-24, F = 2^-125: what a result below fp32's normal range may lose; DESIGN.md, "Indexer KL loss", derives them):
    e_x, eps_p  sparse_mla_bwd_ref's: the exponent of p and p itself; + expm1(lse_err) where lse is only known to lse_err (end to end)
    t           mean_h(eps_p p) + (Hq + 2) u t + F: an fp32 sum of Hq terms in any order, one product by (float)(1 / Hq)
    L           expm1(3 u (max - min)) + 2 u on a term of the sum, (n + 2) u for the sum of n terms, 4 u |L - max| + u |L| for the logarithm,
                its product by ln 2 and the addition;  a: that + u |a|;  y: (expm1(err_a + 2 u |a|) + 2 u) y + F
    d_logits    |grad_scale| (err_y + err_t) + 3 u |d_logits|: grad_scale rounded, the difference, the product
    loss term   t (-log1p(-err_t / t) + 3 u |ln t| + err_a + u |ln t - a|) + err_t |ln t - a| + 2 u |term|; where err_t >= t / 2 the kernel's
                t may be anything in [0, t + err_t], 0 included: (t + err_t) (150 ln 2 + |a|) + |term|
    loss        sum_j err(term_j) + (n + 3) u sum_j |term_j|: an fp32 sum of n terms of both signs in any order
"""
import functools

import numpy as np

import sparse_mla_ref as R
from mqa_logits_bwd_ref import lists

U, F, D_QK = R.U, 2.0 ** -125, R.D_QK
GRAD_SCALE = 0.37
HEADS, TOPKS = (16, 32, 48, 64, 128), (1, 31, 32, 33, 320)          # every wave split; the tile's edges and ten tiles


def reference(q, kv, indices, lse, sm_scale, logits, index_offsets=None, grad_scale=1.0, lse_err=0.0):
    """float arrays holding the tensors' values -> dict of float64: loss [M], dl and t [M, topk], err_loss, err_dl, err_t"""
    q = np.asarray(q, np.float64)
    (m, h, _), s = q.shape, kv.shape[0]
    rows, valid = R.rows_of(indices, s, index_offsets)
    r = {name: np.zeros((m, rows.shape[1])) for name in ("t", "dl", "err_t", "err_dl")}
    r.update(loss=np.zeros(m), err_loss=np.zeros(m))
    for t in range(m):
        sel, n = rows[t][valid[t]], int(valid[t].sum())
        if n == 0:
            continue
        k, ls, lg = np.asarray(kv[sel, :D_QK], np.float64), np.asarray(lse[t], np.float64), np.asarray(logits[t], np.float64)[sel]
        gap = sm_scale * (q[t] @ k.T) - ls[:, None]
        p = np.exp(gap)
        e_x = abs(sm_scale) * (D_QK + 2) * U * (np.abs(q[t]) @ np.abs(k).T) + 2 * U * np.abs(ls)[:, None] + U * np.abs(gap)
        eps_p = np.expm1(e_x) + 2 * U + np.expm1(np.broadcast_to(lse_err, np.shape(lse))[t])[:, None]
        tj = p.mean(0)
        err_t = (eps_p * p).mean(0) * (1 + (h + 2) * U) + (h + 2) * U * tj + F
        big = lg.max() + np.log(np.exp(lg - lg.max()).sum())
        a = lg - big
        err_a = np.expm1(3 * U * (lg.max() - lg.min())) + (n + 4) * U + 4 * U * abs(big - lg.max()) + U * abs(big) + U * np.abs(a)
        y = np.exp(a)
        err_y = (np.expm1(err_a + 2 * U * np.abs(a)) + 2 * U) * y + F
        lt = np.log(tj)
        term, rel = tj * (lt - a), err_t / tj
        err_term = np.where(rel < 0.5, tj * (-np.log1p(-np.minimum(rel, 0.5)) + 3 * U * np.abs(lt) + err_a + U * np.abs(lt - a)) + err_t * np.abs(lt - a)
                            + 2 * U * np.abs(term), (tj + err_t) * (150 * np.log(2.0) + np.abs(a)) + np.abs(term))
        r["t"][t, valid[t]], r["err_t"][t, valid[t]] = tj, err_t
        r["dl"][t, valid[t]] = grad_scale * (y - tj)
        r["err_dl"][t, valid[t]] = abs(grad_scale) * (err_y + err_t) + 3 * U * np.abs(grad_scale * (y - tj))
        r["loss"][t], r["err_loss"][t] = term.sum(), err_term.sum() + (n + 3) * U * np.abs(term).sum()
    return r


def kernel_order(q, kv, indices, lse, sm_scale, logits, index_offsets=None, grad_scale=1.0):
    """the same in float32 with the kernel's operations and roundings (its sums in numpy's order): (loss, d_logits, target)"""
    f = np.float32
    l2e, ln2, (m, h, _) = f(1.4426950408889634), f(0.693147180559945309), q.shape
    rows, valid = R.rows_of(indices, kv.shape[0], index_offsets)
    loss, dl, tg = np.zeros(m, f), np.zeros(rows.shape, f), np.zeros(rows.shape, f)
    for t in range(m):
        sel = rows[t][valid[t]]
        if len(sel) == 0:
            continue
        x = (q[t].astype(f) @ kv[sel, :D_QK].astype(f).T) * f(sm_scale * 1.4426950408889634) - (np.asarray(lse[t], f) * l2e)[:, None]
        tj = np.exp2(x).sum(0, dtype=f) * f(1.0 / h)
        lg = np.asarray(logits[t], f)[sel]
        a = lg - (lg.max() + np.log2(np.exp2((lg - lg.max()) * l2e).sum(dtype=f)) * ln2)
        with np.errstate(divide="ignore", invalid="ignore"):
            loss[t] = np.where(tj > 0, tj * (np.log2(tj) * ln2 - a), f(0)).sum(dtype=f)
        dl[t, valid[t]], tg[t, valid[t]] = f(grad_scale) * (np.exp2(a * l2e) - tj), tj
    return loss, dl, tg


def inside(got, ref):
    """(loss, d_logits, target or None) against the reference: every element inside its bound; the worst error / bound of each"""
    worst = []
    for g, name, bar in zip(got, ("loss", "dl", "t"), ("err_loss", "err_dl", "err_t")):
        if g is not None:
            err = np.abs(np.asarray(g, np.float64) - ref[name])
            assert np.isfinite(err).all() and (err <= ref[bar]).all(), (name, int((err > ref[bar]).sum()), np.argwhere(err > ref[bar])[:4])
            worst.append(float((err / np.maximum(ref[bar], 1e-300)).max()))
    print("worst error / bound (loss, d_logits, target): " + " ".join("%.3f" % w for w in worst))


@functools.lru_cache(maxsize=None)
def random_case(h, topk, empty_lse=-np.inf):
    """sparse_mla_ref.random_case(h)'s q and kv under lists of topk positions (-1 padding, another negative, an entry >= S, duplicates,
    token 3 all invalid), lse the float64 forward's rounded to fp32 (token 3: empty_lse), normal logits: (operands, reference)"""
    q, kv, _ = R.random_case(h)
    idx = lists(topk, seed=2, n=R.S4)
    lse = R.reference(q, kv, idx, R.SCALE4)["lse"].astype(np.float32)
    lse[3] = empty_lse
    logits = (3 * np.random.default_rng([h, topk]).standard_normal((R.M4, R.S4))).astype(np.float32)
    ops = R._frozen(q, kv, idx, lse) + (R.SCALE4,) + R._frozen(logits)
    return ops, reference(*ops, grad_scale=GRAD_SCALE)


@functools.lru_cache(maxsize=None)
def peaked_case(h):
    """random_case(h)'s lists under PEAK times the scale (one head's scores spread up to SPREAD_MAX), logits uniform over +-40, and one
    planted position a token far below everything: column 575 is 8 in every q and 0 in every kv row but row PLANT, -128 there, so
    every head scores 8 * 128 * sm_scale = 170 nat lower against it: its p, e^-170 at most, is 0 in fp32"""
    q, kv, idx = (x.copy() for x in R.random_case(h))
    q[:, :, 575], kv[:, 575], kv[PLANT, 575], idx[:, 5] = 8, 0, -128, PLANT
    scale = R.PEAK * R.SCALE4
    lse = R.reference(q, kv, idx, scale)["lse"].astype(np.float32)
    logits = np.random.default_rng(h).uniform(-40, 40, (R.M4, R.S4)).astype(np.float32)
    ops = R._frozen(q, kv, idx, lse) + (scale,) + R._frozen(logits)
    return ops, reference(*ops, grad_scale=GRAD_SCALE)


PLANT = 123
