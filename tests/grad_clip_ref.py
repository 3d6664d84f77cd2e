"""Not a test file: the definitions of grad_sumsq and grad_clip_scalars in numpy and math, the bound of the device's float64 sum, and the
cases tests/test_grad_clip.py (CPU), tests/test_grad_clip_gpu.py and tests/test_grad_clip_layer_gpu.py share.  Imports no GPU code.
  sumsq          the sum of the squares of a list of arrays: each square exact in float64, summed by math.fsum (the correctly rounded sum)
  bound          what the device's sum may differ from it by: (n + 1) 2^-53 sumsq for n elements, whatever the order of the additions
  clip_scalars   (norm, coef, grad_scale, skip) of the definition in float64, rounded once to float32
  bf16           float32 values rounded to nearest even to bfloat16, as float32"""
import math

import numpy as np

CHUNK = 16384                                          # DGA_GRAD_SUMSQ_CHUNK: elements of one tensor per stage-1 workgroup
SIZES = (0, 1, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
U64 = 2.0 ** -53


def bf16(a):
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)
    return np.where(np.isnan(a), a, r.view(np.float32))


def sumsq(arrays):
    """fsum over the float64 squares of every element of every array (float32 values: the squares are exact).  A NaN or an infinity
    among the elements gives NaN or +inf as the device's additions do: +inf without a NaN, NaN with one."""
    squares = [np.square(np.asarray(a, np.float64).ravel()) for a in arrays]
    flat = np.concatenate(squares) if squares else np.zeros(0)
    if not np.isfinite(flat).all():
        return float("nan") if np.isnan(flat).any() else float("inf")
    return math.fsum(flat.tolist())


def count(arrays):
    return int(sum(np.asarray(a).size for a in arrays))


def bound(n, exact):
    """n - 1 additions of non-negative terms in any order err by at most (n - 1) u (1 + O(n u)) of the exact sum; the reference's own
    rounding adds one u: (n + 1) u covers both for every n < 2^26."""
    return (n + 1) * U64 * exact


def clip_scalars(ss, max_norm, pre_scale=1.0, eps=1e-6):
    """-> (norm float32, coef float32, grad_scale float32 = step_scalars[3], skip int).  min(1, q) is `q if q < 1 else 1`: a NaN quotient
    (0 / 0) gives 1."""
    ss, mx, ps, e = np.float64(ss), np.float64(max_norm), np.float64(pre_scale), np.float64(eps)
    with np.errstate(all="ignore"):
        finite = bool(np.isfinite(ss))
        normd = ps * np.sqrt(ss)
        q = mx / (normd + e)
        coefd = q if q < 1.0 else np.float64(1.0)
        norm = np.float32(normd)
        coef = np.float32(coefd) if finite else np.float32(0)
        scale = np.float32(ps * coefd) if finite else np.float32(0)
    return norm, coef, scale, 0 if finite else 1


INF, NAN = float("inf"), float("nan")
# (sumsq, max_norm, pre_scale, eps, every float64 operation exact: nothing is left to the root's or the quotient's rounding)
CLIP_TABLE = (
    (4.0 ** 3, 2.0, 1.0, 0.0, True),                   # norm 8 > 2: clips to exactly 1/4
    (4.0 ** 5, 64.0, 0.5, 0.0, True),                  # norm 16 of the unscaled gradients < 64: coef 1, grad_scale 1/2
    (4.0 ** -20, 2.0 ** -30, 2.0 ** -3, 0.0, True),    # tiny: norm 2^-23, coef 2^-7
    (4.0 ** 40, 1.0, 2.0 ** -10, 0.0, True),           # a norm beyond fp32's integers: 2^30, coef 2^-30
    (4.0 ** 2, INF, 1.0, 0.0, True),                   # max_norm = inf never clips
    (4.0 ** 2, 0.0, 1.0, 0.0, True),                   # max_norm = 0: coef 0
    (0.0, 1.0, 1.0, 0.0, True),                        # x / 0 = inf: coef 1
    (0.0, 0.0, 1.0, 0.0, True),                        # 0 / 0: coef 1
    (4.0 ** 200, 1.0, 1.0, 0.0, True),                 # a norm fp32 cannot hold: norm inf in fp32, sumsq finite: coef 2^-200 -> 0, no skip
    (3.0, 1.0, 1.0, 1e-6, False),                      # clipping, inexact root and quotient
    (1234.5678, 10.0, 1.0 / 1024, 1e-6, False),        # a loss scale: not clipping
    (1234.5678, 0.01, 1.0 / 1024, 1e-6, False),        # ... clipping
    (7.0e9, 1.0, 1.0 / 65536, 1e-6, False),
    (1e-30, 1.0, 1.0, 1e-6, False),                    # eps dominates
    (5.0, INF, 3.0, 1e-6, False),
    (0.0, 1.0, 1.0, 1e-6, False),
    (INF, 1.0, 1.0, 1e-6, False),                      # skip
    (NAN, 1.0, 0.5, 0.0, False),                       # skip
    (INF, INF, 1.0, 1e-6, False),                      # skip
)
