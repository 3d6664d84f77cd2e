"""Not a test file: the references of router_topk and router_topk_backward, and the cases tests/test_router_topk.py (CPU),
tests/test_router_topk_gpu.py and tests/test_router_layer_gpu.py share.  Imports no GPU code.
  scores64 / score_bar   the float64 scores and the relative bound the device's float32 scores are held to
  select_ref             ids and weights from a given float32 scores array: the definition, numpy float32, bit for bit
  backward_ref           the float64 backward on the same float32 scores, with the M of its bound"""
import numpy as np
import torch

T = 37                                                                    # not a multiple of the 4 tokens of a workgroup
EK = ((8, 1), (8, 8), (60, 6), (64, 2), (160, 8), (256, 8), (384, 8), (1024, 64))   # every lane width (1, 2, 4, 8, 16 experts a lane), odd sizes
GROUPED = ((256, 8, 8, 4), (64, 6, 4, 2), (16, 8, 4, 2))                  # (E, k, n_groups, topk_groups); the last keeps exactly k experts
# ... and the kernel's other ways through the groups.  Groups that are no 1, 2, 4, 8 or 16 whole lanes are valued one by one: 20 lanes
# (1 expert a lane), 1.5 lanes (4 a lane), 32 lanes (8 a lane), 20 lanes (16 a lane).  Whole-lane groups of 2 lanes and of 1 lane.
GROUPED_OTHER = ((60, 6, 3, 2), (192, 8, 32, 8), (512, 8, 2, 1), (960, 8, 3, 2), (32, 4, 16, 4), (1024, 8, 64, 3))
FUNCS, DTYPES = ("softmax", "sigmoid"), ("fp32", "bf16", "fp16")
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
ROW_ZEROS, ROW_TWO_MAXIMA, ROW_NEG_INF, ROW_NEG_INF2, ROW_NAN, FIRST_GRID, FIRST_CONTINUOUS = 0, 1, 2, 3, 4, 5, 21
SENTINEL_ID, SENTINEL_F32 = -7, 0x7FC0A5A5


def to_dtype(a, dtype):
    """float32 values exact in `dtype`."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(TORCH_DT[dtype]).float().numpy()


def tie_logits(e, k, dtype, seed=0):
    """float32 [T, e], exact in `dtype`: a row of zeros, a row with two equal maxima, two rows with -inf entries (at least max(k, 1) finite
    ones stay), a row with a NaN, rows on the grid of multiples of 0.25 in [-4, 4] (ties everywhere), and continuous rows."""
    rng = np.random.default_rng([seed, e, k, DTYPES.index(dtype)])
    x = rng.integers(-16, 17, size=(T, e)).astype(np.float32) * np.float32(0.25)
    x[FIRST_CONTINUOUS:] = to_dtype(rng.standard_normal((T - FIRST_CONTINUOUS, e)) * 3.0, dtype)
    x[ROW_ZEROS] = 0.0
    x[ROW_TWO_MAXIMA] = np.minimum(x[ROW_TWO_MAXIMA], 3.0)
    x[ROW_TWO_MAXIMA, [e // 3, e - 1]] = 3.75
    for row, frac in ((ROW_NEG_INF, 0.3), (ROW_NEG_INF2, 0.9)):
        drop = rng.random(e) < frac
        drop[rng.permutation(e)[:max(1, min(e - 1, k))]] = False
        x[row, drop] = -np.inf
    x[ROW_NAN, e // 2] = np.nan
    return x


def tie_bias(e, seed=0):
    """float32 [e] on the grid of multiples of 1/8: many experts share a bias, so ties survive the addition."""
    return np.random.default_rng([seed, e, 77]).integers(-2, 3, size=e).astype(np.float32) * np.float32(0.125)


def scores64(x, func):
    """float64 [T, e] from the logits' float64 values."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if func == "sigmoid":
            return 1.0 / (1.0 + np.exp(-x))
        ex = np.exp(x - x.max(axis=1, keepdims=True))
        return ex / ex.sum(axis=1, keepdims=True)


def lane_width(e):
    """The experts a lane of the kernel holds: the power of two with 64 V >= e."""
    return max(1, 1 << (((e + 63) // 64) - 1).bit_length())


def score_bar(e, func):
    """The relative bound on a score.  Sigmoid: 2^-18 where |x| <= 16.  Softmax, where |x - max x| <= 16: (V + 74) 2^-24, V = lane_width(e)
    -- the kernel's reduction order tightens the any-order bound (e + 128) 2^-24 of the interface.  In units of 2^-24: an exponential
    carries 16 (the subtraction) + 16 (the product with log2 e) + 2 (the hardware exponential, 1 ulp) = 34; the sum adds V - 1 roundings
    inside a lane and 6 across the lanes to the 34 of its terms; the quotient adds 1: 34 + 34 + V + 5 + 1."""
    return 2.0 ** -18 if func == "sigmoid" else (lane_width(e) + 74) * 2.0 ** -24


def score_checked(x, func):
    """bool [T, e]: where the bound applies."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        if func == "sigmoid":
            return np.abs(x) <= 16
        return np.abs(x - np.nanmax(np.where(np.isinf(x), np.nan, x), axis=1, keepdims=True)) <= 16


def selectable(scores, bias=None, n_groups=1, topk_groups=1):
    """(sel float32 [T, e], ok bool [T, e]): what the selection compares and the experts the group choice leaves."""
    s = np.ascontiguousarray(scores, np.float32)
    t_n, e = s.shape
    with np.errstate(invalid="ignore"):
        sel = s.copy() if bias is None else np.add(s, np.asarray(bias, np.float32)[None, :], dtype=np.float32)
        sel = np.where(np.isnan(sel), np.float32(-np.inf), sel).astype(np.float32)
        ok = np.ones((t_n, e), bool)
        if n_groups > 1:
            gs = e // n_groups
            top2 = -np.sort(-sel.reshape(t_n, n_groups, gs), axis=2)[:, :, :2]
            gv = np.add(top2[:, :, 0], top2[:, :, 1], dtype=np.float32)
            gv = np.where(np.isnan(gv), np.float32(-np.inf), gv)
            g = np.arange(n_groups)
            before = (gv[:, None, :] > gv[:, :, None]) | ((gv[:, None, :] == gv[:, :, None]) & (g[None, None, :] < g[None, :, None]))
            ok = np.repeat(before.sum(-1) < topk_groups, gs, axis=1)
    return sel, ok


def select_ref(scores, k, bias=None, n_groups=1, topk_groups=1, renormalize=True, scale=1.0):
    """(ids int32 [T, k], weights float32 [T, k]) from float32 scores: every operation a numpy float32 one."""
    s = np.ascontiguousarray(scores, np.float32)
    t_n, e = s.shape
    sel, avail = selectable(s, bias, n_groups, topk_groups)
    rows = np.arange(t_n)
    ids = np.empty((t_n, k), np.int32)
    for j in range(k):
        m = np.where(avail, sel, np.float32(-np.inf)).max(axis=1)
        idx = np.argmax(avail & (sel == m[:, None]), axis=1)             # the first available expert that holds the maximum (+0 == -0)
        assert avail[rows, idx].all()
        ids[:, j] = idx
        avail[rows, idx] = False
    r = s[rows[:, None], ids]
    scale = np.float32(scale)
    with np.errstate(invalid="ignore", divide="ignore"):
        if renormalize:
            d = r[:, 0].copy()
            for j in range(1, k):
                d = np.add(d, r[:, j], dtype=np.float32)
            w = np.multiply(np.divide(r, d[:, None], dtype=np.float32), scale, dtype=np.float32)
        else:
            w = np.multiply(r, scale, dtype=np.float32)
    return ids, w


def backward_ref(dw, scores, ids, func, renormalize=True, scale=1.0):
    """(ref64 [T, e], M [T, e]): the float64 backward on the float32 scores given, and the same expression with every term replaced by its
    absolute value and (1 - s) by 1.  The bound is (e + k + 8) 2^-24 M."""
    s = np.asarray(scores, np.float64)
    dw = np.asarray(dw, np.float64)
    ids = np.asarray(ids, np.int64)
    r = np.take_along_axis(s, ids, axis=1)
    if renormalize:
        d = r.sum(axis=1, keepdims=True)
        w = scale * r / d
        g = (scale * dw - (dw * w).sum(axis=1, keepdims=True)) / d
        mg = (np.abs(scale * dw) + np.abs(dw * w).sum(axis=1, keepdims=True)) / np.abs(d)
    else:
        g = scale * dw
        mg = np.abs(g)
    ds, mds = np.zeros_like(s), np.zeros_like(s)
    np.put_along_axis(ds, ids, g, axis=1)
    np.put_along_axis(mds, ids, mg, axis=1)
    if func == "sigmoid":
        return ds * s * (1.0 - s), mds * np.abs(s)
    dot = (g * r).sum(axis=1, keepdims=True)
    return s * (ds - dot), np.abs(s) * (mds + (mg * np.abs(r)).sum(axis=1, keepdims=True))


def backward_bar(e, k):
    return (e + k + 8) * 2.0 ** -24


def round_to(a, dtype):
    """float32 -> the bits a tensor of `dtype` holds after rounding to nearest even (no NaN among the values)."""
    a = np.ascontiguousarray(a, np.float32)
    if dtype == "fp32":
        return a.view(np.uint32)
    if dtype == "fp16":
        return a.astype(np.float16).view(np.uint16)
    u = a.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def continuous_case(e, k, func, with_bias, dtype="fp32"):
    """Continuous random logits for the check against torch.topk: (x float32 [T, e] exact in dtype, bias or None, want = torch.topk's ids
    of the float64 sel, sorted, [T, k]).  The seed is the first one at which, in the float64 reference alone, every row's k-th and (k+1)-th
    sel differ by more than the margin -- twice the score bar of the larger of the two scores, plus the rounding of the bias addition --, so
    that no row has to be left out; the caller asserts it again (margin_ok)."""
    for seed in range(1000):
        rng = np.random.default_rng([seed, e, k, FUNCS.index(func), int(with_bias)])
        x = to_dtype(rng.standard_normal((T, e)) * 2.0, dtype)
        bias = (rng.standard_normal(e) * 0.05).astype(np.float32) if with_bias else None
        if margin_ok(x, bias, k, func).all():
            sel = scores64(x, func) + (bias.astype(np.float64) if with_bias else 0.0)
            want = np.sort(torch.topk(torch.from_numpy(sel), k, dim=1).indices.numpy(), axis=1)
            return x, bias, want
    raise AssertionError("no seed separates the k-th and the (k+1)-th value on every row")


def margin_ok(x, bias, k, func):
    """bool [T]: the row's k-th and (k+1)-th float64 sel are further apart than the device's scores may move them."""
    p = scores64(x, func)
    e = p.shape[1]
    if k == e:
        return np.ones(p.shape[0], bool)
    sel = p + (bias.astype(np.float64) if bias is not None else 0.0)
    order = np.argsort(-sel, axis=1, kind="stable")
    a, b = order[:, k - 1], order[:, k]
    rows = np.arange(p.shape[0])
    margin = 2.0 * score_bar(e, func) * np.maximum(p[rows, a], p[rows, b])
    if bias is not None:
        margin = margin + 2.0 ** -23 * np.maximum(np.abs(sel[rows, a]), np.abs(sel[rows, b]))
    return sel[rows, a] - sel[rows, b] > margin
