"""The float64 reference of fp8_mqa_logits_bwd on the values the codes hold, its operands, and the bounds its GPU tests hold the kernel to
(u = 2^-24; DESIGN.md, "Sparse-attention indexer, backward", derives them), over the valid positions (sparse_mla_ref.rows_of):
    s = sum_d q k[r_j]   mask = s > 0   Gk = mask ? weights d_logits : 0   Gq = Gk kscale[r_j]
    d_weights = sum_j d_logits kscale (mask ? s : 0)     dq = sum_j Gq k[r_j,:]     dk[r_j,:] += sum_h Gk q[m,h,:]
    ambiguous   |s| <= 2^-22 sum_d |q k| (harness/tolerance.py): the mask may fall either way; the whole term goes into the bounds it feeds
    Gk, Gq      one and two fp32 products and the rounding to bf16 at 2^-9: 2^-9 + 2 u, 2^-9 + 3 u.  (One bf16 is RNE to 8 bits, 2^-8 in the
                worst case: no room here, so the kernel carries G as bf16(G) + bf16(G - bf16(G)).)  bf16 times a 4-bit code is exact in fp32
    dq          (EPS_GQ + (topk + 2) u) sum_j |Gq k|: an fp32 sum of topk terms in any order
    dk          EPS_GK sum |Gk q| + (H + n + 1) u (|prior| + sum |Gk q|): H terms on the matrix pipe, then n atomic additions, n naming the row
    d_weights   sum_j |c| 2^-22 sum_d |q k| + (topk + 3) u sum_j |c| (relu(s) + 2^-22 sum_d |q k|), c = d_logits kscale (relu is 1-Lipschitz)
"""
import functools

import numpy as np

import mqa_logits_ref as Q
import sparse_mla_ref as R

U, D, M, N = R.U, Q.D, 5, 300
EPS_GK, EPS_GQ, EPS_S = 2.0 ** -9 + 2 * U, 2.0 ** -9 + 3 * U, 2.0 ** -22


def reference(q, k, kscale, weights, indices, d_logits, index_offsets=None, rounded=False):
    """codes and float arrays -> dict of float64: dq [M, H, 128], dw [M, H], dk [N, 128] (what is added), their bounds' parts, `count`
    [N] and the number of ambiguous triples.  rounded: Gk and Gq formed in fp32 and carried as two bf16 terms, as the kernel does."""
    qf, kf, (m, h, _), n = Q.TABLE[q], Q.TABLE[k], q.shape, k.shape[0]
    rows, valid = R.rows_of(indices, n, index_offsets)
    z = lambda *shape: np.zeros(shape)
    r = dict(dq=z(m, h, D), err_dq=z(m, h, D), dw=z(m, h), err_dw=z(m, h), dk=z(n, D), err_dk=z(n, D), abs_dk=z(n, D), count=z(n), ambiguous=0)
    for t in range(m):
        sel, topk = rows[t][valid[t]], rows.shape[1]
        kk, ks, dl, w = kf[sel], kscale[sel].astype(np.float64), np.asarray(d_logits[t], np.float64)[valid[t]], weights[t].astype(np.float64)
        s, sabs = qf[t] @ kk.T, np.abs(qf[t]) @ np.abs(kk).T                                   # [h, n]
        mask, amb = s > 0, np.abs(s) <= EPS_S * sabs
        g = w[:, None] * dl[None, :]
        gk, gq = np.where(mask, g, 0.0), np.where(mask, g, 0.0) * ks
        if rounded:
            g32 = np.where(mask, w.astype(np.float32)[:, None] * dl.astype(np.float32)[None, :], np.float32(0))
            two = lambda x: R.bf16_round(x) + R.bf16_round((x - R.bf16_round(x).astype(np.float32)).astype(np.float32))
            gk, gq = two(g32), two(g32 * ks.astype(np.float32))
        c = np.abs(dl * ks)
        r["dw"][t] = (dl * ks * np.where(mask, s, 0.0)).sum(1)
        r["err_dw"][t] = (c * EPS_S * sabs).sum(1) + (topk + 3) * U * (c * (np.where(mask, s, 0.0) + EPS_S * sabs)).sum(1)
        r["dq"][t] = gq @ kk
        r["err_dq"][t] = (EPS_GQ + (topk + 2) * U) * (np.abs(g * ks * mask) @ np.abs(kk)) + 1.01 * np.abs(g * ks * amb) @ np.abs(kk)
        for name, a in (("dk", gk), ("abs_dk", np.abs(g * mask)), ("err_dk", EPS_GK * np.abs(g * mask) + 1.01 * np.abs(g * amb))):
            np.add.at(r[name], sel, a.T @ (qf[t] if name == "dk" else np.abs(qf[t])))
        np.add.at(r["count"], sel, 1)
        r["ambiguous"] += int(amb.sum())
    return r


def bound_dk(ref, heads, prior=0.0):
    return ref["err_dk"] + (heads + ref["count"][:, None] + 1) * U * (np.abs(prior) + ref["abs_dk"])


def lists(topk, seed=0, n=N):
    """int32 [M, topk] over n keys with -1 padding, a negative other than -1, an index >= n, a duplicate, and token 3 all invalid"""
    idx = np.random.default_rng([seed, topk]).integers(0, n, size=(M, topk)).astype(np.int32)
    idx[3], idx[1, topk // 2], idx[2, 0] = -1, -7, n + 3
    if topk > 4:
        idx[0, 1], idx[0, 4], idx[4, topk - 1] = -1, idx[0, 3], -1
    return idx


@functools.lru_cache(maxsize=None)
def exact_case(h, topk):
    """(q, k, kscale, weights, idx, d_logits) whose three results are exact in fp32 in any order: mqa_logits_ref.exact_operands, d_logits
    from +-2^e, e in -2 .. 2, and 0 -- NaN at every invalid position -- and the reference of it"""
    ops, idx = Q.exact_operands(M, N, h), lists(topk)
    rng = np.random.default_rng([h, topk])
    dl = (rng.choice([-1.0, 0.0, 1.0], size=idx.shape, p=[0.45, 0.1, 0.45]) * 2.0 ** rng.integers(-2, 3, size=idx.shape)).astype(np.float32)
    dl[~R.rows_of(idx, N)[1]] = np.nan
    return ops + R._frozen(idx, dl), reference(*ops, idx, dl)


@functools.lru_cache(maxsize=None)
def random_case(h, topk=200):
    """amax-quantised normal data: q and k per row to e4m3 codes, the q scale folded into normal weights, normal d_logits; and its reference"""
    import torch
    gen = torch.Generator(device="cpu").manual_seed(11 + h)

    def quantised(*shape):
        x = torch.randn(shape, generator=gen)
        scale = x.abs().amax(-1, keepdim=True) / 448.0
        return (x / scale).to(torch.float8_e4m3fn).view(torch.uint8).numpy(), scale.squeeze(-1).numpy()

    (q, qs), (k, ks) = quantised(M, h, D), quantised(N, D)
    weights = torch.randn((M, h), generator=gen).numpy() * qs
    idx = lists(topk, seed=1)
    dl = torch.randn(idx.shape, generator=gen).numpy()
    ops = R._frozen(q, k, ks, weights, idx, dl)
    return ops, reference(*ops)
