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
import numpy as np

D_QK, D_V, TILE = 576, 512, 32
U = 2.0 ** -24


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
