"""CPU: what the inputs of tests/cast_cases.py must achieve, checked with the oracle alone, so that the GPU tests built on them
(tests/test_cast_rounding_gpu.py) cannot quietly go soft; and the oracle's rule for a block whose maximum is infinite."""
import numpy as np
import pytest

import cast_cases as C


def _move(x, d):
    """Every element d ULP away from zero (d < 0: towards it), magnitudes kept inside [0, the largest finite]."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    mag = np.clip((b & 0x7FFFFFFF) + d, 0, 0x7F7FFFFF)
    return ((b & 0x80000000) | mag).astype(np.uint32).view(np.float32)


def _codes(oracle, y):
    """The oracle's fp32 -> e4m3fn conversion on an array (through quant_1x128 on blocks [448, 127 values]: the scale is 1)."""
    flat = np.ascontiguousarray(y, np.float32).ravel()
    pad = (-flat.size) % 127
    blocks = np.concatenate([flat, np.zeros(pad, np.float32)]).reshape(-1, 127)
    x = np.concatenate([np.full((blocks.shape[0], 1), 448.0, np.float32), np.clip(blocks, -448.0, 448.0)], axis=1)
    q, sf = oracle.quant_1x128(x)
    assert (sf == 1.0).all()
    return q[:, 1:].ravel()[:flat.size].reshape(np.shape(y))


def test_midpoints_are_exact_and_tie():
    mid = C.e4m3_midpoints()
    v = C.e4m3_values()
    assert mid.size == 126 and v[0] == 0.0 and v[-1] == 448.0 and (np.diff(v) > 0).all()
    assert ((mid.astype(np.float64) > v[:-1]) & (mid.astype(np.float64) < v[1:])).all()


@pytest.mark.parametrize("seed", [1, 2])
def test_tie_blocks_are_sensitive(oracle, seed):
    x = C.tie_blocks(400, range(-20, 20), seed)
    assert x.shape == (400, 128) and x.dtype == np.float32
    q, sf = oracle.quant_1x128(x)
    assert (np.abs(x).max(axis=1) == x[:, 0]).all() and (sf[:, 0] == x[:, 0] / np.float32(448.0)).all()
    # one ULP up in magnitude changes the code of at least a tenth of the non-amax elements (the amax stays: the scale is the same)
    y = _move(x, 1)
    y[:, 0] = x[:, 0]
    y = np.where(np.abs(y) > x[:, :1], x, y)
    q1, sf1 = oracle.quant_1x128(y)
    assert (sf1.view(np.uint32) == sf.view(np.uint32)).all()
    share = (q1 != q)[:, 1:].mean()
    print(f"codes that change when x moves one ULP: {share:.3f}")
    assert share >= 0.10
    # a quantiser that multiplies by the rounded reciprocal and corrects nothing differs in at least 1 % of the elements
    r = (np.float32(1.0) / sf).astype(np.float32)
    mutant = _codes(oracle, (x * r).astype(np.float32))
    share = (mutant != q).mean()
    print(f"x * fl32(1/s) differs in {share:.3f} of the elements, {(mutant != q).any(axis=1).mean():.2f} of the blocks")
    assert share >= 0.01


def test_tie_exponents_reach_every_path(oracle):
    """The GPU tests' exponents put the scale inside the fast path, on both sides of each of its ends (2^-63, 2^63), and beyond:
    subnormal scales and a block maximum in the last binade."""
    x = C.tie_blocks(4096, C.TIE_EXPS, 3)
    _, sf = oracle.quant_1x128(x)
    e = (sf[:, 0].view(np.uint32) >> 23).astype(np.int64) - 127
    have = set(e.tolist())
    assert set(range(-65, -60)) <= have and set(range(61, 65)) <= have, sorted(have)
    assert set(range(-25, 8)) <= have
    assert -127 in have and x[:, 0].max() >= 2.0 ** 127 and np.isfinite(x).all()
    assert ((sf[:, 0] >= 2.0 ** -63) & (sf[:, 0] < 2.0 ** 63)).mean() > 0.4
    # the fused kernel's: up = x / 32 stays normal, so gate * up = 32 * up is x again
    y = C.tie_blocks(4096, C.TIE_EXPS_FUSED, 4)
    up = (y * np.float32(2.0 ** -5)).astype(np.float32)
    assert (np.abs(up) >= 2.0 ** -126).all() and ((up * np.float32(32.0)).astype(np.float32) == y).all()
    t = C.tie_tiles(4, C.TIE_EXPS_INTERIOR, 5)
    m = C.tiles_to_matrix(t, 2)
    assert m.shape == (256, 256) and (m[128:, :128] == t[2]).all() and (m[:128, 128:] == t[1]).all()


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_all_16bit_blocks_cover(oracle, kind):
    b = C.all_16bit_blocks(kind)
    nf = len(C.FACTORS)
    assert b.dtype == np.uint16 and b.shape[1] == 128 and b.shape[0] % (nf + 1) == 0
    mant = {np.frexp(f)[0] for f in C.FACTORS}
    assert nf >= 6 and len(mant) >= 6 and min(C.FACTORS) >= 1 and max(C.FACTORS) <= 2 ** 12
    assert np.unique(b[:, 1:]).size == 65536, "a pattern is missing"
    v = C.bits16_to_f32(kind, b)
    q, sf = oracle.quant_1x128(v)
    inf_led = (np.arange(b.shape[0]) % (nf + 1)) == nf
    # column 0 is the block's maximum wherever the chunk is finite
    chunk_finite = np.isfinite(np.where(np.isnan(v[:, 1:]), 0.0, v[:, 1:])).all(axis=1)
    amax = np.where(np.isnan(v), 0.0, np.abs(v)).max(axis=1)
    assert (v[chunk_finite, 0] == amax[chunk_finite]).all()
    assert np.isinf(sf[~chunk_finite | inf_led]).all() and np.isfinite(sf[chunk_finite & ~inf_led]).all()
    # the quotients reach the normal range, the subnormal range and the values that round to zero
    mag = (q[chunk_finite & ~inf_led, 1:] & 0x7F)
    assert (mag == 0).any() and ((mag > 0) & (mag < 8)).any() and ((mag >= 8) & (mag < 0x7F)).any()
    # every finite non-zero pattern meets at least two codes, or code zero throughout if it is among the smallest inputs
    pats = np.arange(65536, dtype=np.uint16)
    val = C.bits16_to_f32(kind, pats)
    finite_nz = np.isfinite(val) & (val != 0)

    def distinct(rows):
        p = b[rows, 1:].ravel().astype(np.int64)
        c = q[rows, 1:].ravel().astype(np.int64)
        pairs = np.unique(p * 256 + c)
        count = np.bincount(pairs >> 8, minlength=65536)
        nonzero = np.bincount(p, weights=(c & 0x7F) != 0, minlength=65536) > 0
        return count, nonzero
    count, nonzero = distinct(np.ones(b.shape[0], bool))
    smallest = (pats & 0x7FFF) < 128
    ok = (count >= 2) | (~nonzero & smallest)
    assert ok[finite_nz].all(), [hex(p) for p in pats[finite_nz & ~ok][:8]]
    # ... and over the finite maxima alone, wherever the type leaves room above the pattern (a block maximum f m is clamped to the
    # largest finite value, so the patterns of the last binade meet one finite scale or two close ones)
    count, nonzero = distinct(~inf_led)
    room = np.zeros(65536, bool)
    room[finite_nz] = np.abs(val[finite_nz].astype(np.float64)) * 8 <= np.abs(val[finite_nz]).max()     # the factors 1 and 2.5 both fit
    ok = (count >= 2) | (~nonzero & smallest)
    assert ok[finite_nz & room].all(), [hex(p) for p in pats[finite_nz & room & ~ok][:8]]


@pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
def test_infinite_block_rule(oracle, ue8m0):
    """A block whose maximum is infinite: scale +inf, every finite element the zero of its own sign, +-inf and NaN sign | 0x7F --
    on the bits, not by what the host's divide makes of inf / inf."""
    inf = np.float32(np.inf)
    nan_pos = np.array([0x7FC00000, 0x7F800001, 0x7FFFFFFF], np.uint32).view(np.float32)
    nan_neg = np.array([0xFFC00000, 0xFF800001, 0xFFFFFFFF], np.uint32).view(np.float32)
    x = np.zeros((128, 256), np.float32)
    x[0, :128] = np.linspace(-3.0, 3.0, 128)                        # a finite neighbour block and row: untouched by the rule
    x[0, 128:128 + 12] = [inf, -inf, 1.0, -1.0, 0.0, -0.0, 3e38, -3e38, 1e-45, -1e-45, 448.0, -448.0]
    x[0, 140:143] = nan_pos
    x[0, 143:146] = nan_neg
    x[1, 5] = -inf                                                  # -inf alone makes the maximum infinite too
    x[1, 6] = 2.0; x[1, 7] = -2.0
    x[2, 130] = 7.0; x[2, 131] = nan_neg[0]
    want = np.zeros((3, 256), np.uint8)
    want[0, 128:128 + 12] = [0x7F, 0xFF, 0, 0x80, 0, 0x80, 0, 0x80, 0, 0x80, 0, 0x80]
    want[0, 140:143] = 0x7F
    want[0, 143:146] = 0xFF
    want[1, 5] = 0xFF; want[1, 7] = 0x80
    q, sf = oracle.quant_1x128(x[:3], ue8m0=ue8m0)
    fin, _ = oracle.quant_1x128(x[:3, :128], ue8m0=ue8m0)
    assert np.isposinf(sf[0, 1]) and np.isposinf(sf[1, 0]) and np.isfinite(sf[0, 0]) and np.isfinite(sf[2, 1])
    assert (q[0, 128:] == want[0, 128:]).all() and (q[1, :128] == want[1, :128]).all()
    assert q[2, 130] == 0x7E and q[2, 131] == 0xFF and (q[1, 128:] == 0).all() and sf[1, 1] == 1.0
    assert (q[0, :128] == fin[0]).all() and (fin[0, 0] & 0x80) == 0x80 and (fin[0, 1:127] & 0x7F).any()
    # the 128x128 form: tile (0, 1) holds the first infinite block above, tile (0, 0) the second: every element of both follows the rule
    q2, sf2 = oracle.quant_128x128(x, ue8m0=ue8m0)
    assert sf2.shape == (1, 2) and np.isposinf(sf2).all()
    assert (q2[0, 128:] == want[0, 128:]).all() and (q2[1, :128] == want[1, :128]).all()
    assert (q2[0, :128] == np.where(np.signbit(x[0, :128]), 0x80, 0)).all()
    assert q2[2, 130] == 0 and q2[2, 131] == 0xFF and (q2[3:] == 0).all()


def test_one_hot_blocks(oracle):
    x = C.one_hot_blocks("1x128")
    q, sf = oracle.quant_1x128(x)
    want = np.float32(100.0) / np.float32(448.0)
    assert x.shape == (128, 128) and (sf.view(np.uint32) == want.view(np.uint32)).all()
    i = np.arange(128)
    assert (np.abs(x).argmax(axis=1) == i).all() and (q[i, i] == np.where(i % 2 == 0, 0x7E, 0xFE)).all()
    assert (x.astype(np.float64) * 128 == np.round(x.astype(np.float64) * 128)).all(), "not exact in bf16"
    t = C.one_hot_blocks("128x128")
    assert t.shape == (384, 128, 128)
    m = t.reshape(384 * 128, 128)
    _, sf = oracle.quant_128x128(m)
    assert sf.shape == (384, 1) and (sf.view(np.uint32) == want.view(np.uint32)).all()
    pos = np.abs(t.reshape(384, -1)).argmax(axis=1)
    r, c = pos // 128, pos % 128
    assert (np.abs(t.reshape(384, -1)) == 100.0).sum() == 384 and set(np.sign(t.reshape(384, -1)[np.arange(384), pos])) == {-1.0, 1.0}
    # the kernel's geometry: thread 2 r + (c >= 64) holds row r's columns 64 (c >= 64) .. + 64
    assert len(set((2 * r + (c >= 64)).tolist())) == 256, "a thread of the workgroup never holds the maximum"
    assert len(set((c % 64).tolist())) == 64, "an element position of a thread never holds the maximum"
    assert (r[:128] == i).all() and (c[:128] == 37 * i % 128).all() and (c[128:256] == i).all() and (r[128:256] == 29 * i % 128).all()
