"""Not a test file: the definition of adamw_per_block_cast_to_fp8_transposed in numpy, the bounds of its float32 arithmetic against float64,
and the cases tests/test_adamw_cast.py (CPU), tests/test_adamw_cast_gpu.py and tests/test_adamw_cast_layer_gpu.py share.  Imports no GPU
code.
  scalars                the four values of a step {lr, bc1, bc2s, grad_scale}: float64 on the host, rounded once (adamw_step_scalars)
  step                   one step in `dtype` (float32: bit for bit what the device leaves in w, m, v; float64: the exact value it is held to)
  stored / moment_bits   a moment as the device stores it (RNE to bfloat16, or as it is) and its bits
  bars                   the bounds of the float32 step against the float64 one on the same inputs and scalars"""
import numpy as np

U = 2.0 ** -24
BETA1, BETA2, EPS, LR, WD = 0.9, 0.95, 1e-8, 3e-4, 0.1
SHAPES = ((1, 1, 1), (1, 128, 128), (2, 136, 264), (3, 130, 100), (5, 127, 7), (2, 257, 129), (1, 8, 1024), (256, 384))
DTYPES = ("fp32", "bf16")


def f32(x):
    """A Python number as the float32 a launch argument becomes, back as a Python float."""
    return float(np.float32(x))


def scalars(step, lr, beta1, beta2, grad_scale=1.0, dtype=np.float32):
    """{lr, bc1, bc2s, grad_scale}: bc1 = 1 - beta1^step, bc2s = sqrt(1 - beta2^step), in float64, then `dtype`."""
    return np.array([lr, 1.0 - float(beta1) ** step, np.sqrt(1.0 - float(beta2) ** step), grad_scale], np.float64).astype(dtype)


def step(w, m, v, grad, sc, beta1=BETA1, beta2=BETA2, eps=EPS, weight_decay=0.0, dtype=np.float32):
    """One step, every operation in `dtype` and rounded on its own: -> (w', m', v') with the UNROUNDED moments (stored() gives what a
    bfloat16 moment keeps).  The inputs and every scalar are converted to `dtype` as they are given: float32 values stay what they are."""
    t = dtype
    w, m, v, grad = (np.asarray(a).astype(t) for a in (w, m, v, grad))
    lr, bc1, bc2s, gs = (t(x) for x in np.asarray(sc))
    b1, b2, eps, wd = t(beta1), t(beta2), t(eps), t(weight_decay)
    one = t(1)
    with np.errstate(all="ignore"):
        g = grad * gs
        m1 = b1 * m + (one - b1) * g
        v1 = b2 * v + ((one - b2) * g) * g
        den = np.sqrt(v1) / bc2s + eps
        w1 = w * (one - lr * wd)
        w2 = w1 - (lr / bc1) * (m1 / den)
    for a in (g, m1, v1, den, w2):
        assert a.dtype == t
    return w2, m1, v1


def moment_bits(a, moment):
    """float32 -> the bits a moment tensor of type `moment` holds: round to nearest even to bfloat16 (a NaN stays a NaN), or as it is."""
    a = np.ascontiguousarray(a, np.float32)
    if moment == "fp32":
        return a.view(np.uint32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(a), ((u >> 16) | 0x40).astype(np.uint16), r)


def stored(a, moment):
    """float32 -> the float32 value of what a moment tensor of type `moment` holds."""
    if moment == "fp32":
        return np.ascontiguousarray(a, np.float32)
    return (moment_bits(a, moment).astype(np.uint32) << 16).view(np.float32)


def same_bits(got_bits, want_bits, want_values):
    """Bit for bit where the reference is a number; where it is a NaN the other is a NaN too (IEEE leaves a NaN's sign and payload open).
    -> the indices that differ."""
    nan = np.isnan(want_values)
    width = got_bits.dtype.itemsize * 8
    exp_all, frac = ((0x7F80, 0x007F) if width == 16 else (0x7F800000, 0x007FFFFF))
    got_nan = ((got_bits & exp_all) == exp_all) & ((got_bits & frac) != 0)
    return np.nonzero(np.where(nan, ~got_nan, got_bits != want_bits))


def bars(w, m, v, grad, sc, beta1=BETA1, beta2=BETA2, eps=EPS, weight_decay=0.0):
    """The float64 step on the same float32 inputs and scalars and the bounds the float32 step is held to ("Optimizer"):
    with M = |beta1 m| + |(1 - beta1) g|,
      |m' - exact| <= 3 u M,   |v' - exact| <= 5 u v',   |w' - exact| <= u (5 |w| + (lr / bc1) (4 M + 10 |m'|) / den)
    -> ((w', m', v') exact, (w_bar, m_bar, v_bar))."""
    f = np.float64
    exact = step(w, m, v, grad, sc, beta1, beta2, eps, weight_decay, dtype=f)
    lr, bc1, bc2s, gs = (f(x) for x in np.asarray(sc))
    g = np.asarray(grad).astype(f) * gs
    big_m = np.abs(f(beta1) * np.asarray(m).astype(f)) + np.abs((1.0 - f(beta1)) * g)
    den = np.sqrt(exact[2]) / bc2s + f(eps)
    w_bar = U * (5.0 * np.abs(np.asarray(w).astype(f)) + (lr / bc1) * (4.0 * big_m + 10.0 * np.abs(exact[1])) / den)
    return exact, (w_bar, 3.0 * U * big_m, 5.0 * U * exact[2])


def inputs(shape, grad_dtype="fp32", moment="fp32", seed=0, zero_moments=False):
    """(w, m, v, grad) float32 arrays of `shape`, grad exact in grad_dtype and the moments exact in `moment`: weights of size 0.05, gradients
    of size 1e-3 over three decades, moments that such gradients leave behind."""
    rng = np.random.default_rng([seed, len(shape)] + list(shape))
    w = (rng.standard_normal(shape) * 0.05).astype(np.float32)
    grad = (rng.standard_normal(shape) * 1e-3 * 10.0 ** rng.uniform(-2, 1, shape)).astype(np.float32)
    m = (rng.standard_normal(shape) * 5e-4).astype(np.float32)
    v = (np.square(rng.standard_normal(shape) * 1e-3) + 1e-12).astype(np.float32)
    if zero_moments:
        m, v = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    return w, stored(m, moment), stored(v, moment), stored(grad, grad_dtype)
