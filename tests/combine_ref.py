"""Not a test file: the numpy float32 reference of combine_tokens (its definition, so the comparison is bit for bit), the float64 reference
and error bar of combine_tokens_weight_grad, and the cases tests/test_combine_tokens.py (CPU) and tests/test_combine_tokens_gpu.py share.
Imports no GPU code."""
import numpy as np
import torch

T, S = 37, 300
KS, HS, DTYPES = (1, 2, 8), (384, 100, 7176), ("bf16", "fp16", "fp32")     # 7176 = 897 chunks of 8: the split of a long row
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
EMPTY_TOKEN = 5                                                           # its choices are all dropped: a row of +0
OUTSIDE = (-1, S, S + 5, 1 << 62, -(1 << 63))                             # dest values that drop a choice


def valid(dest, s_n):
    return (dest >= 0) & (dest < s_n)


def make_case(k, h, dtype, seed=0):
    """src [S, h] as float32 values exact in `dtype` with NaN in every row no valid choice names, dest int64 [T, k] with dropped choices of
    every kind and one token without a valid one, weights float32 [T, k] (NaN on the dropped choices: they are skipped, not multiplied),
    grad [T, h] like src."""
    rng = np.random.default_rng([seed, k, h, DTYPES.index(dtype)])
    dest = rng.integers(0, S, size=(T, k)).astype(np.int64)
    drop = rng.random((T, k)) < 0.2
    drop[EMPTY_TOKEN] = True
    drop[0, 0] = False                                                   # (k = 1: still a valid choice somewhere, whatever the draw)
    dest[drop] = rng.choice(np.array(OUTSIDE, np.int64), size=int(drop.sum()))
    dest[1, k - 1] = S                                                   # the first index past the end, always present
    to_dt = lambda a: torch.from_numpy(a.astype(np.float32)).to(TORCH_DT[dtype]).float().numpy()
    src = to_dt(rng.standard_normal((S, h)))
    used = np.zeros(S, bool)
    used[dest[valid(dest, S)]] = True
    src[~used] = np.nan
    w = rng.standard_normal((T, k)).astype(np.float32)
    w[~valid(dest, S)] = np.nan
    grad = to_dt(rng.standard_normal((T, h)))
    return {"src": src, "dest": dest, "w": w, "grad": grad, "k": k, "h": h, "dtype": dtype}


def combine_partial_sums(src, dest, w=None):
    """The definition, step by step: [(ok [T], prod [T, h] float32, acc [T, h] float32 after choice j)] for j = 0 .. k - 1, every operation
    a numpy float32 one (one rounding each)."""
    src = np.ascontiguousarray(src, np.float32)
    s_n = src.shape[0]
    acc = np.zeros((dest.shape[0], src.shape[1]), np.float32)
    steps = []
    with np.errstate(invalid="ignore"):
        for j in range(dest.shape[1]):
            ok = valid(dest[:, j], s_n)
            rows = src[np.where(ok, dest[:, j], 0)]
            prod = rows if w is None else np.multiply(np.where(ok, w[:, j], np.float32(0))[:, None].astype(np.float32), rows, dtype=np.float32)
            acc = np.where(ok[:, None], np.add(acc, prod, dtype=np.float32), acc)
            steps.append((ok, prod, acc))
    return steps


def combine_ref(src, dest, w=None):
    """float32 [T, h]: acc after the last choice."""
    return combine_partial_sums(src, dest, w)[-1][2]


def round_to(acc, dtype):
    """float32 -> the bits out holds: uint32 for fp32, uint16 for the 16-bit types (round to nearest even; the cases hold no NaN in a sum)."""
    acc = np.ascontiguousarray(acc, np.float32)
    if dtype == "fp32":
        return acc.view(np.uint32)
    if dtype == "fp16":
        return acc.astype(np.float16).view(np.uint16)
    u = acc.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def weight_grad_ref(src, grad, dest):
    """(ref64 [T, k], bar [T, k]): the float64 dot products (0 on dropped choices) and the any-order bound for a float32 sum of h products
    each rounded at most once, (h + 2) 2^-24 sum_c |src grad|."""
    s_n, h = src.shape
    ok = valid(dest, s_n)
    rows = np.where(ok[..., None], src.astype(np.float64)[np.where(ok, dest, 0)], 0.0)          # [T, k, h]
    g = grad.astype(np.float64)[:, None, :]
    return (rows * g).sum(-1), (h + 2) * 2.0 ** -24 * np.abs(rows * g).sum(-1)
