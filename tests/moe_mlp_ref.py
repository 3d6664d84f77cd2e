"""Not a test file: a plain numpy float64 reference of one training step of a MoE expert MLP, for tests/test_moe_mlp_ref.py (CPU) and
tests/test_moe_mlp_step_gpu.py.  Imports no GPU code; the quantisers come from the `oracle` module the caller passes in.

Per expert g: tokens X_g [t_g, D], W1_g [2H, D] (rows 0..H-1 gate, rows H..2H-1 up), W2_g [D, H], dOut_g [t_g, D].
  Y1 = X W1^T        h = silu(Y1[:, :H]) Y1[:, H:]        Out = h W2^T
  grad_h = dOut W2   dY1 = [grad_h up silu'(gate) | grad_h silu(gate)]   dX = dY1 W1   dW2 = dOut^T h   dW1 = dY1^T X
A step is a dict: "Y1", "h", "Out", "grad_h", "dY1", "dX" are lists of G float64 arrays [t_g, .], "dW1" [G, 2H, D] and "dW2" [G, D, H]."""
import numpy as np

from fused_bounds import _e4m3_rne_satfinite

D, H, G = 384, 256, 4               # three k blocks and 1.5 output tiles of 256; each half of 2H has two 1x128 blocks
TOKENS = (200, 0, 77, 1)
MMAX = 256                          # the masked layout's rows per expert: two 128-token blocks


# ---- number formats

def bf16_rne(x):
    """float64 -> fl32 -> bf16 by round-to-nearest-even, as float64: what a kernel that accumulates in fp32 and stores bf16 writes."""
    u = np.ascontiguousarray(x, np.float64).astype(np.float32).view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    r = np.where((u & 0x7FFFFFFF) > 0x7F800000, u | 0x00400000, r).astype(np.uint32)
    return r.view(np.float32).astype(np.float64)


def bf16_bits_to_f64(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def dequant_1x128(q, sf, table):
    """codes [rows, k] with one scale per 1x128 block [rows, ceil(k/128)] -> float64."""
    k = q.shape[-1]
    return table.astype(np.float64)[q] * np.repeat(np.asarray(sf, np.float64), 128, axis=-1)[..., :k]


def dequant_128x128(q, sf, table):
    """codes [rows, k] with one scale per 128x128 block [ceil(rows/128), ceil(k/128)] -> float64."""
    rows, k = q.shape
    s = np.repeat(np.repeat(np.asarray(sf, np.float64), 128, axis=0)[:rows], 128, axis=1)[:, :k]
    return table.astype(np.float64)[q] * s


# ---- the activation and its backward, float64

def sigmoid(g):
    return 1.0 / (1.0 + np.exp(-g))


def act(y1):
    """h = silu(gate) up from Y1 = [gate | up]."""
    h = y1.shape[-1] // 2
    g, u = y1[..., :h], y1[..., h:]
    return g * sigmoid(g) * u


def act_bwd(y1, grad_h):
    """dY1 = [grad_h up silu'(gate) | grad_h silu(gate)], silu'(g) = s + g s (1 - s) with 1 - s = exp(-g) s."""
    h = y1.shape[-1] // 2
    g, u = y1[..., :h], y1[..., h:]
    s = sigmoid(g)
    return np.concatenate([grad_h * u * (s + g * s * (np.exp(-g) * s)), grad_h * g * s], axis=-1)


# ---- inputs

def make_case(seed, tokens=TOKENS, d=D, h=H):
    """X and dOut N(0, 1) rounded to bf16 (the device tensors are bf16), W1 N(0, 4/D) and W2 N(0, 1/H) in fp32: the gates are N(0, 2^2), so
    they cover the root of silu' at -1.28 and reach both tails of the sigmoid (|g| up to about 8), and h is of order 1.  The same arrays on
    every machine.  The recipe is fixed subject to one condition on the reference alone, which tests/test_moe_mlp_ref.py asserts: among
    the emulated step's errors on seeds 0 .. 7 seed 0 is not the largest for any output (see ERROR_SEEDS)."""
    rng = np.random.default_rng(seed)
    case = {"tokens": tuple(tokens), "X": [], "dOut": [], "W1": [], "W2": []}
    for t in tokens:
        case["X"].append(bf16_rne(rng.standard_normal((t, d))))
        case["dOut"].append(bf16_rne(rng.standard_normal((t, d))))
        case["W1"].append((rng.standard_normal((2 * h, d)) * (2.0 / np.sqrt(d))).astype(np.float32).astype(np.float64))
        case["W2"].append((rng.standard_normal((d, h)) / np.sqrt(h)).astype(np.float32).astype(np.float64))
    return case


# ---- the step

def step_exact(case):
    """The unquantised step in float64."""
    out = {k: [] for k in ("Y1", "h", "Out", "grad_h", "dY1", "dX", "dW1", "dW2")}
    for x, w1, w2, do in zip(case["X"], case["W1"], case["W2"], case["dOut"]):
        y1 = x @ w1.T
        hh = act(y1)
        grad_h = do @ w2
        dy1 = act_bwd(y1, grad_h)
        for k, v in (("Y1", y1), ("h", hh), ("Out", hh @ w2.T), ("grad_h", grad_h), ("dY1", dy1), ("dX", dy1 @ w1), ("dW2", do.T @ hh),
                     ("dW1", dy1.T @ x)):
            out[k].append(v)
    out["dW1"], out["dW2"] = np.stack(out["dW1"]), np.stack(out["dW2"])
    return out


def _pad128(x):
    pad = -x.shape[0] % 128
    return np.concatenate([x, np.zeros((pad, x.shape[1]))]) if pad else x


def step_emulated(case, oracle=None):
    """The step with the library's roundings at the library's places: oracle.quant_1x128 on every activation the device quantises -- row-wise
    for the forward and dgrad GEMMs, and on the transpose of the expert's tokens padded with zeros to whole 128-token blocks (an excluded
    token counts as zero, and both layouts start every expert on a block boundary) for the weight gradients --, oracle.quant_128x128 on W
    and W^T, bf16 RNE of fl32 wherever a GEMM writes bf16 and for grad_x_out, float64 products of the dequantised operands, float64 SiLU
    on the bf16 Y1.  The quantisers see fl32 of the float64 value (the device keeps h and dY1 in fp32 and never rounds them to 16 bits
    first).  oracle=None switches every rounding off: the result is step_exact's up to summation order."""
    if oracle is None:
        rows = tokens = blocks = store = lambda v: v
    else:
        tab = oracle.e4m3fn_table()
        rows = lambda v: dequant_1x128(*oracle.quant_1x128(v.astype(np.float32)), tab)
        tokens = lambda v: dequant_1x128(*oracle.quant_1x128(np.ascontiguousarray(_pad128(v).T.astype(np.float32))), tab).T
        blocks = lambda v: dequant_128x128(*oracle.quant_128x128(v.astype(np.float32)), tab)
        store = bf16_rne
    out = {k: [] for k in ("Y1", "h", "Out", "grad_h", "dY1", "dX", "dW1", "dW2")}
    for x, w1, w2, do in zip(case["X"], case["W1"], case["W2"], case["dOut"]):
        if x.shape[0] == 0:                                                       # an empty expert: nothing to quantise, zero gradients
            for k, width in (("Y1", w1.shape[0]), ("h", w2.shape[1]), ("Out", w2.shape[0]), ("grad_h", w2.shape[1]), ("dY1", w1.shape[0]),
                             ("dX", w1.shape[1])):
                out[k].append(np.zeros((0, width)))
            out["dW1"].append(np.zeros(w1.shape)); out["dW2"].append(np.zeros(w2.shape))
            continue
        w1q, w2q = blocks(w1), blocks(w2)                                         # forward operands
        w1tq, w2tq = blocks(np.ascontiguousarray(w1.T)), blocks(np.ascontiguousarray(w2.T))     # dgrad operands: W^T quantised on its own
        y1 = store(rows(x) @ w1q.T)                                               # F1 row-wise, F2
        hh = act(y1)                                                              # F3: fp32 on the device, never stored
        o = store(rows(hh) @ w2q.T)                                               # F3 row-wise, F4
        grad_h = store(rows(do) @ w2tq.T)                                         # B1 row-wise, B2
        dy1_32 = act_bwd(y1, grad_h)                                              # B3: quantised from fp32 ...
        dy1 = store(dy1_32)                                                       # ... and written to grad_x_out in bf16
        dx = store(rows(dy1_32) @ w1tq.T)                                         # B4
        n = x.shape[0]
        dw2 = tokens(do)[:n].T @ tokens(hh)[:n]                                   # F1/B1/F3 transposed, B5 (the zero padding adds nothing)
        dw1 = tokens(dy1)[:n].T @ tokens(x)[:n]                                   # B6: dY1 is the bf16 tensor here
        for k, v in (("Y1", y1), ("h", hh), ("Out", o), ("grad_h", grad_h), ("dY1", dy1), ("dX", dx), ("dW2", dw2), ("dW1", dw1)):
            out[k].append(v)
    out["dW1"], out["dW2"] = np.stack(out["dW1"]), np.stack(out["dW2"])
    return out


def rel_error(got, want):
    """Relative Frobenius error over all experts; got and want are lists of arrays or stacked arrays."""
    g = np.concatenate([np.asarray(v, np.float64).ravel() for v in got])
    w = np.concatenate([np.asarray(v, np.float64).ravel() for v in want])
    return float(np.linalg.norm(g - w) / np.linalg.norm(w))


ERROR_KEYS = ("Out", "dX", "dW1", "dW2")
ERROR_SEEDS = tuple(range(8))
"""The device runs seed 0 and is held to the largest emulated error of these seeds.  On the same data the device and the emulation differ
by accumulation order and by codes flipped within the activation bounds, a few 1e-6 of the error, of either sign: were seed 0 the largest
of the eight for some output, the bar there would be the emulation on identical data and that sign would decide.  Hence the condition on
the recipe above, with a margin of 2^-10 of the error."""
_ERRORS = {}


def emulated_errors(oracle, seed):
    """Relative Frobenius error of step_emulated against step_exact on make_case(seed), per ERROR_KEYS; computed once per process."""
    if seed not in _ERRORS:
        case = make_case(seed)
        emu, exact = step_emulated(case, oracle), step_exact(case)
        _ERRORS[seed] = tuple(rel_error(emu[k], exact[k]) for k in ERROR_KEYS)
    return _ERRORS[seed]


# ---- one link at a time: from the bytes that went into a link to its float64 result

def link_quant_rows(x, oracle, ue8m0=False):
    """F1 / B1 row-wise: per_token_cast_to_fp8's definition on the rows given."""
    return oracle.quant_1x128(np.ascontiguousarray(x, np.float32), ue8m0=ue8m0)


def link_quant_tokens(x, valid, oracle):
    """F1 / B1 / B6 transposed: the definition on x^T with the rows outside `valid` (bool [T]) as zeros, whatever they hold."""
    x0 = np.where(valid[:, None], np.asarray(x, np.float32), np.float32(0.0))
    return oracle.quant_1x128(np.ascontiguousarray(x0.T))


def link_wgrad(da, db):
    """B5 / B6 for one expert: (ref, S) = (da db^T, |da| |db|^T) from the dequantised float64 slices [M, k] and [N, k] of its tokens."""
    return da @ db.T, np.abs(da) @ np.abs(db).T


def e4m3_spacing(y):
    """The distance between neighbouring e4m3 values at |y| (float64, |y| <= 448): 2^(floor(log2 |y|) - 3), 2^-9 below 2^-6."""
    a = np.maximum(np.abs(y), 2.0 ** -6)
    return 2.0 ** (np.floor(np.log2(a)) - 3)


def expected_boundary_share(ref, bound, scale):
    """The share of elements whose float64 value ref lies within `bound` of an e4m3 rounding boundary when a value sits anywhere in its
    cell with equal probability: mean of min(1, 2 bound / (spacing(ref / scale) scale)).  `scale` per element."""
    return float(np.minimum(1.0, 2.0 * bound / (e4m3_spacing(ref / scale) * scale)).mean())


# ---- the tolerance family's codes: which ones the element bounds admit, and how many elements they may excuse

CAP_RELATIVE = 2.0 ** -10
"""h and dup.  Their bound is relative, 2^-18 |v|: the band around a rounding boundary is 2 * 2^-18 |v| wide and an e4m3 cell at least
2^-4 |v| (three mantissa bits; wider below 2^-6), so at most 2^-13 of the elements can sit in a band.  The cap leaves 8x."""


def code_interval(oracle, ref, bound, scale):
    """(lo, hi): the e4m3 values RNE((ref -+ bound) / scale), ordered.  A code is admissible when its value lies in [lo, hi]; lo == hi
    wherever the float64 value is further than its bound from every rounding boundary."""
    b0, b1 = _e4m3_rne_satfinite(oracle, (ref - bound) / scale), _e4m3_rne_satfinite(oracle, (ref + bound) / scale)
    return np.minimum(b0, b1), np.maximum(b0, b1)


def dgate_cap(ref, bound, scale):
    """The cap on the share of dgate elements a neighbouring code is excused for.  dgate's bound is not relative to the value:
    bound = 2^-17 |d u| (s + |g| s (1 - s)) = 2^-17 |v| R(g),  R(g) = (s + |g| s (1 - s)) / |s + g s (1 - s)|.
    R = 1 for g >= 0, where the count for h applies with 2^-17: 2 * 2^-17 / 2^-4 = 2^-12.  For g < 0 the denominator is silu'(g), which has
    a root at g0 = -1.2785; near it R ~ 2 / |g - g0| (numerator 2 s(g0) = 0.436, silu''(g0) = 0.218), so the share of a band in its cell
    grows without limit and no constant holds for every distribution of gates: the integral of min(1, 2^-12 R(g)) over gates of density
    p around g0 is about p 2^-10 (1 + ln 2^11), 1.4 * 2^-10 at the p = 0.16 of N(0, 2^2) gates, on top of 2^-12 elsewhere (with the narrowest
    cell everywhere: an upper estimate).  So the expected share is taken
    over the elements the link was actually given, each with its own bound and its own cell under its block's scale
    (expected_boundary_share: float64 reference values only, nothing the device computed), and the cap leaves the same 8x."""
    return 8.0 * expected_boundary_share(ref, bound, scale)
