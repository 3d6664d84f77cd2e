"""Inputs of per_block_cast_to_fp8_transposed's tests (tests/test_block_cast_transposed.py states the oracle identity on them,
tests/test_block_cast_transposed_gpu.py runs the kernel on them) and the definition both compare with.  Plain numpy, seeded; a helper
module, not a conftest."""
import numpy as np

import cast_cases as C

# (G, N, K): the smallest input; one full tile; both edges, every vector path and several groups; N % 8 != 0 and K % 8 != 0, so every
# scalar path; the W1^T of tests/test_moe_mlp_step_gpu.py
SHAPES = [(1, 1, 1), (1, 128, 128), (3, 200, 136), (2, 130, 257), (4, 384, 256)]
SHAPE_2D = (136, 200)
F32_SNAN, F32_SNAN_NEG = 0x7F800001, 0xFFA00000


def random_weights(g, n, k, seed):
    return (np.random.default_rng(seed).standard_normal((g, n, k)) * 3.0).astype(np.float32)


def special_values():
    """fp32 [4, 200, 136]: per group the tiles (0, 0) 128 x 128 (interior), (0, 1) 128 x 8, (1, 0) 72 x 128 and (1, 1) 72 x 8 (edges).
      group 0   NaN of both signs, -0 and subnormals of both signs among ordinary values, in every tile: finite scales
      group 1   +Inf beside NaN in the interior tile, +Inf and -Inf in (0, 1), -Inf alone in the corner tile: infinite scales; (1, 0) ordinary
      group 2   (0, 0) all zero with some -0; (1, 0) zero but for one fp32 max; (0, 1) zero but for one NaN (scale 1); (1, 1) all subnormal
      group 3   signalling NaNs of both signs where a lane's, a wave's and the workgroup's reduction end, among ordinary values"""
    w = random_weights(4, 200, 136, 101)
    nan, sub = np.float32(np.nan), np.float32(1e-45)
    for r, c in ((0, 0), (5, 77), (127, 127), (64, 130), (127, 135), (128, 0), (199, 64), (150, 127), (128, 128), (199, 135)):
        w[0, r, c] = nan if (r + c) % 2 == 0 else -nan
    for r, c in ((1, 1), (100, 129), (199, 1), (198, 134)):
        w[0, r, c] = -0.0
    for r, c in ((2, 2), (101, 131), (197, 3), (197, 133)):
        w[0, r, c] = sub if r % 2 else -np.float32(1e-40)
    w[1, 3, 4] = np.inf; w[1, 3, 5] = nan; w[1, 90, 100] = -nan
    w[1, 10, 128] = np.inf; w[1, 127, 135] = -np.inf
    w[1, 199, 135] = -np.inf
    w[2] = 0.0
    w[2, 7:40, 9:50] = -0.0
    w[2, 131, 66] = C.F32_MAX
    w[2, 100, 133] = -nan
    w[2, 128:, 128:] = (np.arange(72 * 8, dtype=np.float32).reshape(72, 8) - 300) * sub
    bits = w[3].view(np.uint32)
    for r, c in ((7, 7), (63, 127), (64, 0), (127, 120), (135, 15), (199, 129)):
        bits[r, c] = F32_SNAN if (r + c) % 2 == 0 else F32_SNAN_NEG
    return w


def amax_positions():
    """fp32 [256, 128, 128]: tile i holds its maximum (100 + i, negative for odd i) in lane t = i of the kernel -- rows 8 (t / 16) .. + 7,
    columns 8 (t % 16) .. + 7 -- at pass p and column slot j with 8 p + j = 37 i mod 64 (a bijection on every 64 consecutive i: every
    (pass, slot) pair four times); everything else is fl32(max / 3) with a random sign."""
    rng = np.random.default_rng(7)
    i = np.arange(256)
    a = (100.0 + i).astype(np.float32)
    w = np.broadcast_to((a / np.float32(3.0)).astype(np.float32)[:, None, None], (256, 128, 128)).copy()
    w = np.where(rng.integers(0, 2, size=w.shape) == 1, -w, w).astype(np.float32)
    slot = (37 * i) % 64
    w[i, 8 * (i // 16) + slot // 8, 8 * (i % 16) + slot % 8] = np.where(i % 2 == 1, -a, a)
    return w


def tie_matrix():
    """fp32 [1024, 1024]: 64 tie tiles (cast_cases.tie_tiles, scale exponents inside and at both ends of quant8's fast path), 8 per row."""
    return C.tiles_to_matrix(C.tie_tiles(64, C.TIE_EXPS_INTERIOR + C.TIE_EXPS_ENDS, 53), 8)


def reference(oracle, w, ue8m0=False):
    """The definition on a float32 [G, N, K] (or [N, K]) array: per group oracle.quant_128x128 of w[g]^T and of w[g].
    Returns ((qt, sft), (q, sf)) stacked over the groups, with w's leading dimensions."""
    w3 = w.reshape((-1,) + w.shape[-2:])
    t = [oracle.quant_128x128(np.ascontiguousarray(x.T), ue8m0=ue8m0) for x in w3]
    r = [oracle.quant_128x128(np.ascontiguousarray(x), ue8m0=ue8m0) for x in w3]
    lead = w.shape[:-2]
    stack = lambda pairs, j: np.stack([p[j] for p in pairs]).reshape(lead + pairs[0][j].shape)
    return (stack(t, 0), stack(t, 1)), (stack(r, 0), stack(r, 1))


def assert_transposition_identity(oracle, w, ue8m0=False):
    """quant_128x128(w[g]^T) is quant_128x128(w[g]) with codes and scales transposed, byte for byte and bit for bit."""
    (qt, sft), (q, sf) = reference(oracle, w, ue8m0)
    assert np.array_equal(qt, np.swapaxes(q, -1, -2)), "codes"
    assert np.array_equal(sft.view(np.uint32), np.swapaxes(sf, -1, -2).view(np.uint32)), "scales"
