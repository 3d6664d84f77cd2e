"""Inputs built to sit where an fp8 quantiser can go wrong (tests/test_cast_cases.py states what they must achieve on the oracle
alone, tests/test_cast_rounding_gpu.py runs the kernels on them).  Plain numpy, seeded; a helper module, not a conftest.

  tie_blocks / tie_tiles   quotients x / s within two fp32 ULP of a midpoint between adjacent e4m3fn values
  all_16bit_blocks         every bf16 / fp16 bit pattern, each at several quotients
  one_hot_blocks           the block maximum in every lane and element position of the reductions
"""
import numpy as np

F32_MAX = np.float32(3.4028234663852886e38)


def e4m3_values() -> np.ndarray:
    """The 127 non-negative finite e4m3fn values 0 .. 448 in code order, float64 (stated here, not taken from the oracle)."""
    c = np.arange(127)
    e, m = c >> 3, c & 7
    return np.where(e == 0, m / 8.0 * 2.0 ** -6, (1 + m / 8.0) * 2.0 ** (e - 7.0))


def e4m3_midpoints() -> np.ndarray:
    """The 126 midpoints between adjacent values: at most 5 significant bits, exact in fp32."""
    v = e4m3_values()
    mid = (v[:-1] + v[1:]) / 2
    assert (mid.astype(np.float32).astype(np.float64) == mid).all()
    return mid.astype(np.float32)


# exponents e of the block maximum a = u 2^e, u in [1, 2): the scale s = a / 448 has exponent e - 9 or e - 8
TIE_EXPS_INTERIOR = list(range(-20, 20))
TIE_EXPS_ENDS = list(range(-58, -50)) + list(range(68, 75))      # s from 2^-67 to 2^-59 and from 2^59 to 2^66: both sides of 2^+-63
TIE_EXPS_GENERAL = [-126, -124, -121, -119, -118, -117, -110, -100, -80, 80, 100, 120, 125, 126, 127]   # subnormal s ... a near 2^128
TIE_EXPS = TIE_EXPS_INTERIOR + TIE_EXPS_ENDS + TIE_EXPS_GENERAL
# the same for the fused SiLU kernel, whose `up` input is the tie value times 2^-5 and has to stay normal: the smallest element is
# about 2^-10 s = 2^(e - 19), so e >= -100 keeps up above 2^-124
TIE_EXPS_FUSED = TIE_EXPS_INTERIOR + TIE_EXPS_ENDS + [-100, -90, -80, 80, 100, 120, 125, 126, 127]


def _draw_amax(rng, n, scale_exps):
    e = rng.choice(np.asarray(list(scale_exps), np.int64), size=n)
    u = rng.uniform(1.0, 2.0, size=n)
    a = np.minimum(np.ldexp(u, e), np.float64(F32_MAX)).astype(np.float32)
    return a, (a / np.float32(448.0)).astype(np.float32)            # s = fl32(a / 448), the quantisers' own scale


def _ties(rng, a, s, n):
    """[len(a), n] values fl32(mid * s) with the bit pattern moved by -2 .. +2 and a random sign; an element whose magnitude
    would exceed the block's a keeps the unmoved value."""
    mids = e4m3_midpoints()
    x0 = (mids[rng.integers(0, mids.size, size=(a.size, n))] * s[:, None]).astype(np.float32)
    bits = x0.view(np.int32).astype(np.int64) + rng.integers(-2, 3, size=x0.shape)
    x = np.clip(bits, 0, 0x7F7FFFFF).astype(np.int32).view(np.float32)
    x = np.where(x > a[:, None], x0, x)
    return np.where(rng.integers(0, 2, size=x.shape) == 1, -x, x).astype(np.float32)


def tie_blocks(n_blocks, scale_exps, seed) -> np.ndarray:
    """fp32 [n_blocks, 128]: column 0 is the block maximum a, the other 127 columns are ties against s = fl32(a / 448)."""
    rng = np.random.default_rng(seed)
    a, s = _draw_amax(rng, n_blocks, scale_exps)
    x = np.empty((n_blocks, 128), np.float32)
    x[:, 0] = a
    x[:, 1:] = _ties(rng, a, s, 127)
    return x


def tie_tiles(n_tiles, scale_exps, seed) -> np.ndarray:
    """fp32 [n_tiles, 128, 128]: the same for the 128x128 quantiser, one a per tile (a tile's maximum is the largest of its rows'),
    at a random place of the tile; the other 16383 elements are ties."""
    rng = np.random.default_rng(seed)
    a, s = _draw_amax(rng, n_tiles, scale_exps)
    x = _ties(rng, a, s, 128 * 128)
    x[np.arange(n_tiles), rng.integers(0, 128 * 128, size=n_tiles)] = a
    return x.reshape(n_tiles, 128, 128)


def tiles_to_matrix(tiles, tiles_per_row) -> np.ndarray:
    """[n, 128, 128] -> [n / tiles_per_row * 128, tiles_per_row * 128] with tile i at block row i // tiles_per_row."""
    n = tiles.shape[0]
    assert n % tiles_per_row == 0
    return np.ascontiguousarray(tiles.reshape(n // tiles_per_row, tiles_per_row, 128, 128).transpose(0, 2, 1, 3)
                                .reshape(n // tiles_per_row * 128, tiles_per_row * 128))


# ---- 16-bit patterns

def bits16_to_f32(kind, bits) -> np.ndarray:
    bits = np.ascontiguousarray(bits, np.uint16)
    if kind == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    assert kind == "fp16"
    with np.errstate(invalid="ignore"):                             # (signalling NaN patterns are among the inputs)
        return bits.view(np.float16).astype(np.float32)


def _f64_to_bits16(kind, v) -> np.ndarray:
    """Non-negative finite float64 -> the nearest pattern of the type, clamped to its largest finite value."""
    if kind == "fp16":
        return np.minimum(v, 65504.0).astype(np.float16).view(np.uint16)
    u = np.minimum(v, np.float64(F32_MAX)).astype(np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.minimum(r, 0x7F7F).astype(np.uint16)


# distinct mantissas 1, 1.25, 1.5, 1.75, 1.125, 1.375, 1 between 1 and 2^12.  An element of magnitude |x| meets the quotients
# 448 |x| / (f m): from 448 down to 2^-3.2 for the elements near their chunk's maximum m, through e4m3's subnormal range
# (below 2^-6) and below 2^-10 (code 0) for the small elements of the chunks that span many binades.
FACTORS = (1.0, 2.5, 12.0, 56.0, 288.0, 1408.0, 4096.0)


def all_16bit_blocks(kind, factors=FACTORS) -> np.ndarray:
    """uint16 [rows, 128]: the 65 536 patterns in chunks of 127 consecutive ones (the last chunk is the last 127 patterns); per chunk
    and factor f one block [f m, chunk], m the chunk's largest finite magnitude and f m clamped to the type's largest finite value
    (0 where the chunk is all NaN), and per chunk one block [+inf, chunk]: the infinite-maximum rule on every pattern.  A chunk
    that holds an Inf has an infinite maximum whatever column 0 says, so it appears once more with its Inf and NaN patterns
    replaced by +0: its finite patterns meet finite scales too.  Rows are ordered chunk-major, the factors then the +inf block."""
    inf_bits = 0x7F80 if kind == "bf16" else 0x7C00
    starts = list(range(0, 65536 - 126, 127))
    if starts[-1] + 127 < 65536:
        starts.append(65536 - 127)
    chunks = [np.arange(s0, s0 + 127, dtype=np.uint16) for s0 in starts]
    for c in list(chunks):
        if ((c & 0x7FFF) == inf_bits).any():
            chunks.append(np.where((c & 0x7FFF) >= inf_bits, 0, c).astype(np.uint16))
    rows = []
    for c in chunks:
        mag = bits16_to_f32(kind, c & 0x7FFF)
        fin = np.isfinite(mag)
        m = float(mag[fin].max()) if fin.any() else 0.0
        for f in factors:
            rows.append(np.concatenate([_f64_to_bits16(kind, np.array([f * m])), c]))
        rows.append(np.concatenate([np.array([inf_bits], np.uint16), c]))
    return np.stack(rows).astype(np.uint16)


# ---- the block maximum in every position

def one_hot_blocks(mode, seed=0) -> np.ndarray:
    """Noise |x| <= 1 (a multiple of 2^-7: exact in bf16 too) plus one element of magnitude 100 with alternating sign.
    "1x128":    fp32 [128, 128], block i has it at column i: every lane of the 16-lane row and every element of a lane.
    "128x128":  fp32 [384, 128, 128]; tile r < 128 has it at (r, 37 r mod 128), tile 128 + c at (29 c mod 128, c), and tile 256 + r
                at (r, (37 r + 64) mod 128), the other half of row r: the first two families alone reach 192 of the workgroup's 256
                (row, column half) threads, with the third every thread holds it at least once, and so does every one of a
                thread's 64 element positions."""
    rng = np.random.default_rng(seed)
    i = np.arange(128)
    sign = np.where(i % 2 == 0, 100.0, -100.0).astype(np.float32)
    if mode == "1x128":
        x = (rng.integers(-128, 129, size=(128, 128)) / 128.0).astype(np.float32)
        x[i, i] = sign
        return x
    assert mode == "128x128"
    x = (rng.integers(-128, 129, size=(384, 128, 128)) / 128.0).astype(np.float32)
    x[i, i, (37 * i) % 128] = sign
    x[128 + i, (29 * i) % 128, i] = -sign
    x[256 + i, i, (37 * i + 64) % 128] = sign
    return x
