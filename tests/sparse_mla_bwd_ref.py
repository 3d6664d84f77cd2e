"""The float64 reference of sparse_mla_bwd on the values its bf16 / fp32 inputs hold, and the bounds its GPU tests hold the kernel to.

    p_j = exp(s_j - lse)   delta = sum_c out d_out   dP_j = sum_c d_out kv[r_j, c]   dS_j = sm_scale p_j (dP_j - delta)
    dq = sum_j dS_j kv[r_j, :576]      dkv[r_j, :576] += sum_h dS_j q      dkv[r_j, :512] += sum_h p_j d_out
over the valid positions (sparse_mla_ref.rows_of), duplicates once per position, lse and out as given.

The bounds (u = 2^-24; DESIGN.md, "Sparse MLA attention, backward", derives them from the kernel's order of operations):
    e_x(j)    sm_scale (576 + 2) u sum_d |q kv[r_j]| + 2 u |lse| + u |s_j - lse|: the fp32 sum of 576 products, the scale rounded and
              multiplied once, lse (float)log2 e likewise, the subtraction;  eps_p = expm1(e_x) + 2 u (v_exp_f32 at 1 ulp)
    err(dS_j) sm_scale p_j (|dP|_j + |delta|) (2^-8 + eps_p + 516 u): |dP|_j = sum_c |d_out kv|, |delta| = sum_c |out d_out| (dP - delta
              cancels); 516 u = the 512-term sums of dP and delta with their difference (513) and three roundings of the two products and
              the scale; 2^-8 = the rounding of dS to bf16 (2^-9) and as much again for everything of second order
    dq        sum_j err(dS_j) |kv[r_j, c]| + (topk + 2) u sum_j |dS_j kv[r_j, c]| + 2^-9 |dq|
    dkv       sum over the (m, j, h) that name the row of err(dS) |q| + (2^-9 + eps_p) p |d_out|, + (2 Hq n + 1) u (|what was there| +
              sum |terms|), n the positions that name the row: an fp32 sum of that many terms in any order.  No output rounding.
"""
import functools

import numpy as np

import sparse_mla_ref as R

U, D_QK, D_V = R.U, R.D_QK, R.D_V


def reference(q, kv, out, d_out, indices, lse, sm_scale, index_offsets=None, rounded=False, out_err=0.0, lse_err=0.0):
    """float arrays holding the tensors' values -> dict of float64: dq [M, H, 576], dkv [S, 576] (what is added), and what the bounds
    are made of.  rounded: p, dS and dq rounded to bf16 where the kernel rounds them (the CPU check of the bounds).  out_err [M, H, 512]
    and lse_err [M, H]: how far the out and lse the kernel is given may lie from the ones given here (the end-to-end test)."""
    q, out, d_out, lse = (np.asarray(x, np.float64) for x in (q, out, d_out, lse))
    (m, h, _), s = q.shape, kv.shape[0]
    rows, valid = R.rows_of(indices, s, index_offsets)
    z, rb = (lambda *shape: np.zeros(shape)), (lambda x: R.bf16_round(x.astype(np.float32)) if rounded else x)
    r = dict(dq=z(m, h, D_QK), err_dq=z(m, h, D_QK), abs_dq=z(m, h, D_QK), dkv=z(s, D_QK), err_dkv=z(s, D_QK), abs_dkv=z(s, D_QK), count=z(s))
    for t in range(m):
        sel = rows[t][valid[t]]
        if len(sel) == 0:
            continue
        k = np.asarray(kv[sel, :D_QK], np.float64)
        sc = sm_scale * (q[t] @ k.T)                                                     # [h, n]
        gap = sc - lse[t][:, None]
        p = np.exp(gap)
        e_x = abs(sm_scale) * (D_QK + 2) * U * (np.abs(q[t]) @ np.abs(k).T) + 2 * U * np.abs(lse[t])[:, None] + U * np.abs(gap)
        eps_p = np.expm1(e_x) + 2 * U
        delta, abs_delta = (out[t] * d_out[t]).sum(1)[:, None], np.abs(out[t] * d_out[t]).sum(1)[:, None]
        dp, abs_dp = d_out[t] @ k[:, :D_V].T, np.abs(d_out[t]) @ np.abs(k[:, :D_V]).T
        ds = sm_scale * p * (dp - delta)
        err_ds = abs(sm_scale) * p * (abs_dp + abs_delta) * (2.0 ** -8 + eps_p + 516 * U)
        # p' = p e^-el and delta' = delta + sum_c eo d_out move dS by at most sm_scale p (w (|dP - delta| + e_delta) + e_delta), p by w p
        w = np.expm1(np.broadcast_to(lse_err, lse.shape)[t])[:, None]
        e_delta = (np.broadcast_to(out_err, out.shape)[t] * np.abs(d_out[t])).sum(1)[:, None]
        err_ds = err_ds + abs(sm_scale) * p * (w * (np.abs(dp - delta) + e_delta) + e_delta)
        pb, dsb = rb(p), rb(ds)
        r["dq"][t], r["err_dq"][t], r["abs_dq"][t] = rb(dsb @ k), err_ds @ np.abs(k), np.abs(ds) @ np.abs(k)
        for name, a, b, c, e in (("dkv", dsb, q[t], pb, d_out[t]), ("err_dkv", err_ds, np.abs(q[t]), (2.0 ** -9 + eps_p + w) * p, np.abs(d_out[t])),
                                 ("abs_dkv", np.abs(ds), np.abs(q[t]), p, np.abs(d_out[t]))):
            add = a.T @ b                                                                # [n, 576]
            add[:, :D_V] += c.T @ e
            np.add.at(r[name], sel, add)
        np.add.at(r["count"], sel, 1)
    return r


def bound_dq(ref, topk):
    return ref["err_dq"] + (topk + 2) * U * ref["abs_dq"] + 2.0 ** -9 * np.abs(ref["dq"])


def bound_dkv(ref, heads, prior=0.0):
    return ref["err_dkv"] + (2 * heads * ref["count"][:, None] + 1) * U * (np.abs(prior) + ref["abs_dkv"])


@functools.lru_cache(maxsize=None)
def operands(h, topk=R.TOPK4):
    """sparse_mla_ref.random_case(h) cut to topk positions, with what a backward is given: out (bf16 values) and lse (fp32 values) of the
    float64 forward reference, d_out seeded normal samples (bf16 values): (q, kv, idx, out, lse, d_out, sm_scale), read-only"""
    import torch
    q, kv, idx = R.random_case(h)
    idx = np.ascontiguousarray(idx[:, :topk])
    if topk < R.TOPK4:
        idx[3] = -1                                                                      # a token without a valid position
    fwd = R.reference(q, kv, idx, R.SCALE4)
    d_out = torch.randn(fwd["out"].shape, generator=torch.Generator(device="cpu").manual_seed(5 + h)).to(torch.bfloat16).float().numpy()
    out = R.bf16_round(fwd["out"].astype(np.float32)).astype(np.float32)
    return R._frozen(q, kv, idx, out, fwd["lse"].astype(np.float32), d_out) + (R.SCALE4,)


@functools.lru_cache(maxsize=None)
def expected(h, topk=R.TOPK4):
    args = operands(h, topk)
    return reference(*args[:2], args[3], args[5], args[2], args[4], args[6])
