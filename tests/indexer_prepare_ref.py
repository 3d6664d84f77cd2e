"""Not a test file: the definitions of indexer_prepare_q / indexer_prepare_k / indexer_prepare_backward that tests/test_indexer_prepare.py
(CPU) and tests/test_indexer_prepare_gpu.py share.  Imports no GPU code.
  rope32 / hadamard32 / stats32 / norm32   numpy float32, every operation one rounding, in the kernel's order: what the device computes to the bit
  rope64 / hadamard64 / stats64            float64: a complex RoPE, a Sylvester Hadamard matrix, torch.nn.functional.layer_norm's formula
Bounds, u = 2^-24, none from the kernel's output:
  ROT_BAR   |y32 - y64| <= (7 + 4) u sum|r| C per element, r the RoPE'd float32 row both start from: an element of the butterfly is a sum
            of the 128 inputs, each passing through 7 additions (gamma_7 sum|r|); the 4: the product by C, C's own rounding, second order.
  MEAN_BAR  |mean - exact| <= 130 u mean|x|: a float32 sum of 128 terms in ANY order errs by at most gamma_127 sum|x| < 130 u sum|x| (the
            kernel's order, 8 in the lane and a tree of depth 4, gives 11 u); the division by 128 is exact.
  RSTD_BAR  rstd within (128 / 2 + 8) u relative of (mean((x - mean32)^2) + fl32(eps))^(-1/2) in float64, mean32 the RETURNED mean: d = fl(x -
            mean32) and fl(d^2) carry 3 u on each term, the any-order sum 127 u, the addition of eps 1 u: 131 u on the argument, halved by
            the inverse square root, plus the correctly rounded square root and division, 1 u each (with second order: below 68 u)."""
import numpy as np

import rms_norm_ref as N
import router_ref as R

U = 2.0 ** -24
D, HALF = 128, 32
C = np.float32(128 ** -0.5)
ROT_BAR, MEAN_BAR, RSTD_BAR = (7 + 4) * U, 130 * U, (D / 2 + 8) * U
DTYPES, TORCH_DT, SENTINEL_F32, bits_of, to_dtype, round_to = R.DTYPES, R.TORCH_DT, R.SENTINEL_F32, N.bits_of, R.to_dtype, R.round_to
H64 = np.ones((1, 1))
for _ in range(7):
    H64 = np.kron(np.array([[1.0, 1.0], [1.0, -1.0]]), H64)      # Sylvester: natural order


def table(p, seed=0):
    """cos_sin float32 [p, 64]: cos of frequency i in column i, sin in column 32 + i, at angles position * 10000^(-i / 32) + a random phase."""
    ang = np.arange(p)[:, None] * 10000.0 ** (-np.arange(HALF) / HALF)[None, :] + np.random.default_rng(seed).uniform(0, 6.28, (p, HALF))
    return np.concatenate((np.cos(ang), np.sin(ang)), axis=1).astype(np.float32)


def _pairs(interleaved):
    return (slice(0, 64, 2), slice(1, 64, 2)) if interleaved else (slice(0, HALF), slice(HALF, 64))


def rope32(x, cs, interleaved, transposed=False):
    """x float32 [R, 128], cs float32 [R, 64] (the rows' table entries): a' = fl(fl(a c) - fl(b s)), b' = fl(fl(a s) + fl(b c)); transposed: -s."""
    ia, ib = _pairs(interleaved)
    c, s = cs[:, :HALF], (-cs[:, HALF:] if transposed else cs[:, HALF:])
    out = np.array(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        out[:, ia], out[:, ib] = x[:, ia] * c - x[:, ib] * s, x[:, ia] * s + x[:, ib] * c
    return out


def hadamard32(x):
    """The butterfly in natural order, strides 1 .. 64, then fl(t C)."""
    y = np.array(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for h in (1, 2, 4, 8, 16, 32, 64):
            t = y.reshape(-1, D // (2 * h), 2, h)
            y = np.stack((t[:, :, 0] + t[:, :, 1], t[:, :, 0] - t[:, :, 1]), axis=2).reshape(-1, D)
        return y * C


def _sum32(x):
    """A row's float32 sum in the kernel's order: the 8 elements of a lane ascending, then the tree over lanes l ^ 1, 2, 4, 8."""
    lanes = x.reshape(-1, 16, 8)
    p = lanes[:, :, 0]
    for j in range(1, 8):
        p = p + lanes[:, :, j]
    while p.shape[1] > 1:
        p = p[:, 0::2] + p[:, 1::2]
    return p[:, 0]


def stats32(x, eps):
    """(mean, rstd) float32 in the kernel's order."""
    mean = _sum32(x) * np.float32(2.0 ** -7)
    d = x - mean[:, None]
    return mean, np.float32(1.0) / np.sqrt(_sum32(d * d) * np.float32(2.0 ** -7) + np.float32(eps))


def norm32(x, mean, rstd, gamma, beta):
    """z = fl(fl(fl(fl(x - mean) rstd) gamma) + beta) from the statistics given (no beta: no addition)."""
    z = ((x - mean[:, None]) * rstd[:, None]) * gamma[None, :]
    return z if beta is None else z + beta[None, :]


def stats64(x, eps, mean=None):
    """float64 layer_norm statistics of the float32 x; with `mean`, the variance about that mean."""
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=1) if mean is None else np.asarray(mean, np.float64)
    return mu, 1.0 / np.sqrt(((x - mu[:, None]) ** 2).mean(axis=1) + np.float64(np.float32(eps)))


def rope64(x, cs, interleaved, transposed=False):
    """float64, as a complex product: (a + i b) (c + i s), the conjugate factor for the transpose."""
    ia, ib = _pairs(interleaved)
    x, cs = np.asarray(x, np.float64), np.asarray(cs, np.float64)
    w = cs[:, :HALF] + 1j * (-cs[:, HALF:] if transposed else cs[:, HALF:])
    z = (x[:, ia] + 1j * x[:, ib]) * w
    out = x.copy()
    out[:, ia], out[:, ib] = z.real, z.imag
    return out


def hadamard64(x):
    return np.asarray(x, np.float64) @ H64 * np.float64(C)


def rows(r, dtype, seed=0, scale=1.5):
    """float32 [r, 128] exact in `dtype`."""
    return to_dtype(np.random.default_rng([seed, r, DTYPES.index(dtype)]).standard_normal((r, D)) * scale, dtype)


def prepared32(x, cs, interleaved, norm=None):
    """The float32 y the quantiser gets; norm = (mean, rstd, gamma, beta) as the device returned / was given them."""
    return hadamard32(rope32(x if norm is None else norm32(x, *norm), cs, interleaved))


def backward32(g, cs, interleaved, row_div=None):
    with np.errstate(invalid="ignore", divide="ignore"):
        return rope32(hadamard32(g if row_div is None else g / row_div[:, None]), cs, interleaved, transposed=True)
