"""Not a test file: the references of rms_norm_per_token_cast_to_fp8 and rms_norm_backward, their bounds, and the cases
tests/test_rms_norm.py (CPU), tests/test_rms_norm_gpu.py and tests/test_rms_norm_layer_gpu.py share.  Imports no GPU code.
  residual_ref / y_ref / norm_bits     the definition below rstd in numpy float32: bit for bit what the device writes from a given rstd
  rstd64 / rstd_bar                    the float64 statistic on the same z and the relative bound the device's float32 rstd is held to
  forward64 / backward64               the float64 forward and backward (checked against torch.autograd on the CPU)
  dx_bar / dweight_bar                 the bounds of the backward, with rstd taken as given"""
import numpy as np

import router_ref as R

U = 2.0 ** -24
MAX_H = 16384
DTYPES, TORCH_DT = R.DTYPES, R.TORCH_DT
CANONICAL_NAN = 0x7FC00000
EPS = 1e-6

# ---- the forward's cases: every H with five of (T, dtype, weight's dtype, residual, use_ue8m0), every value of each met
HS = (1, 7, 8, 127, 128, 129, 136, 512, 520, 2048, 2056, 7168, 16384)
TS = (1, 3, 5, 257)
FORWARD_CASES = tuple((h, TS[n % 4], DTYPES[n % 3], bool((n // 2) % 2), bool((n // 3) % 2), bool((n // 7) % 2))
                      for n, h in ((i * 5 + k, h) for i, h in enumerate(HS) for k in range(5)))
# (H, (lanes on a row, passes)) at every H where the forward kernel's geometry changes
FORWARD_GEOMETRY = ((128, (16, 1)), (256, (32, 1)), (512, (64, 1)), (1024, (64, 2)), (2048, (64, 4)), (4096, (128, 4)), (8192, (256, 4)),
                    (MAX_H, (256, 8)))

# ---- the backward's: {1, 5, 300} x {7, 136, 2048, 7168}, and at T = 5 the H that take the kernel's other geometries
BACKWARD_TH = tuple((t, h) for t in (1, 5, 300) for h in (7, 136, 2048, 7168)) + ((5, 512), (5, 520), (5, 4096), (5, MAX_H))
BACKWARD_GEOMETRY = ((128, (16, 1)), (256, (32, 1)), (512, (64, 1)), (1024, (64, 2)), (2048, (128, 2)), (4096, (256, 2)), (8192, (512, 2)),
                     (MAX_H, (1024, 2)))


def geometry(table, h):
    return next(g for top, g in table if h <= top)


def chunk_rows(t_n):
    """Rows of one stage-one chunk of the backward's dweight: max(8, ceil(T / 1024))."""
    return max(8, -(-t_n // 1024))


def to_dtype(a, dtype):
    return R.to_dtype(a, dtype)


def bits_of(t):
    """A torch tensor's bits as numpy: uint32 for float32, uint16 for the 16-bit types, uint8 for codes."""
    import torch
    view = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()]
    return t.contiguous().view(view).cpu().numpy().view({4: np.uint32, 2: np.uint16, 1: np.uint8}[t.element_size()])


def from_bits(bits, dtype):
    """uint16 / uint32 bits of `dtype` -> float32 values."""
    if dtype == "fp32":
        return bits.view(np.float32)
    if dtype == "fp16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def forward_inputs(h, t_n, dtype, w_f32, seed=0):
    """x, residual float32 [T, h] exact in `dtype`, weight float32 [h] exact in its own dtype (fp32 with w_f32, else `dtype`)."""
    rng = np.random.default_rng([seed, h, t_n, DTYPES.index(dtype)])
    x = to_dtype(rng.standard_normal((t_n, h)) * 1.5, dtype)
    res = to_dtype(rng.standard_normal((t_n, h)) * 0.75, dtype)
    w = (1.0 + 0.25 * rng.standard_normal(h)).astype(np.float32)
    return x, res, w if w_f32 else to_dtype(w, dtype)


def residual_ref(x, res, dtype):
    """-> (the bits residual_out holds, z = their float32 values): RNE(fl32(x + residual))."""
    bits = R.round_to(np.add(x, res, dtype=np.float32), dtype)
    return bits, from_bits(bits, dtype)


def y_ref(z, rstd, w):
    """y = fl32(fl32(z rstd) w) from the rstd the device returned, a NaN replaced by the one NaN 0x7FC00000."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        y = np.multiply(np.multiply(z, rstd[:, None], dtype=np.float32), w[None, :], dtype=np.float32)
    y.view(np.uint32)[np.isnan(y)] = CANONICAL_NAN
    return y


def norm_bits(y, dtype):
    """The bits norm_out holds: RNE(y); the one NaN becomes 0x7FC0 / 0x7E00 / itself."""
    with np.errstate(invalid="ignore", over="ignore"):
        return R.round_to(y, dtype)


def rstd64(z, eps):
    """float64 (mean(z^2) + fl32(eps))^(-1/2) on the float32 z."""
    z = np.asarray(z, np.float64)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        return 1.0 / np.sqrt((z * z).mean(axis=1) + np.float64(np.float32(eps)))


def rstd_bar(h):
    """|rstd - exact| <= (h / 2 + 6) u exact: gamma(h) of a sum of non-negative terms in any order, halved by the inverse square root,
    plus the division by h, the addition of eps and a 1-ULP reciprocal square root."""
    return (h / 2 + 6) * U


def forward64(x, res, w, eps):
    """float64 y = rms_norm(x + res) w, without any rounding in between."""
    z = np.asarray(x, np.float64) + (0.0 if res is None else np.asarray(res, np.float64))
    return z * (1.0 / np.sqrt((z * z).mean(axis=1, keepdims=True) + eps)) * np.asarray(w, np.float64)[None, :]


def backward_inputs(t_n, h, dtype, w_f32, seed=0):
    """grad_y, z float32 [T, h] exact in `dtype`, weight, and rstd float32 [T] (the float64 statistic of z rounded: "as given")."""
    z, gy, w = forward_inputs(h, t_n, dtype, w_f32, seed + 100)
    gy = to_dtype(gy * np.float32(0.5), dtype)
    return gy, z, w, rstd64(z, EPS).astype(np.float32)


def backward64(gy, z, w, rstd):
    """float64 on the float32 inputs, rstd as given -> dx, dweight, and what the bounds are made of: |g|, |x^|, |c|, A, sum_t |gy x^|."""
    gy, z, w, rstd = (np.asarray(a, np.float64) for a in (gy, z, w, rstd))
    xh = z * rstd[:, None]
    g = gy * w[None, :]
    c = (g * xh).mean(axis=1, keepdims=True)
    dx = rstd[:, None] * (g - xh * c)
    a = np.abs(g * xh).mean(axis=1, keepdims=True)
    return dx, (gy * xh).sum(axis=0), dict(g=np.abs(g), xh=np.abs(xh), c=np.abs(c), a=a, rstd=rstd[:, None], dw_abs=np.abs(gy * xh).sum(axis=0))


def dx_bar(m, h):
    """|dx - exact| <= u rstd (4 |g| + |x^| (6 |c| + (h + 8) A)): g, x^ and their product carry 3 roundings and the row sum h - 1 more
    on A, the division one; x^ c two more on |x^ c|; the subtraction and the last product one each on |g| + |x^ c|, g's own one on |g|:
    3 |g| + 4 |x^ c| + (h + 3) |x^| A, with slack."""
    return U * m["rstd"] * (4 * m["g"] + m["xh"] * (6 * m["c"] + (h + 8) * m["a"]))


def dweight_bar(m, t_n):
    """|dweight - exact| <= (T + 4) u sum_t |grad_y x^|: x^'s rounding, the product's, and at most T + 2 additions over both stages."""
    return (t_n + 4) * U * m["dw_abs"]
