"""Exactly summable operands for the 16-bit GEMM family (csrc/dga_b16.hip, gemm_b16_kernel.hpp, gemm_b16_wsk_kernel.hpp,
gemm_b16_w4_kernel.hpp): with small INTEGER-valued operands every product and every partial sum is an integer below 2^24, so the
fp32 accumulation is the exact sum whatever the summation order, split-K slicing, tile, wave grid or pipeline, and the 16-bit result
is the round-to-nearest-even of that integer.  One float64 matmul is the reference of every path at once, compared bit for bit.

A plain module (no fixtures): tests/test_b16_cases.py checks it on the CPU, tests/test_b16_exact_gpu.py uses it on the GPU."""
import contextlib
import os

import numpy as np
import torch

LIM = {torch.bfloat16: 8, torch.float16: 32}      # integer operands are uniform in [-LIM, LIM]: exactly representable
KIND = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}

# ---- the shapes of tests/test_b16_exact_gpu.py (kept here so that the CPU test can hold every one to LIM^2 K < 2^24) ----------
MAIN = (300, 520, 1344)          # ragged in every dimension of every tile; 21 k steps: uneven split-K slices
MAIN_SEED = 0
PAD_K = 1000                     # K % 64 != 0: the operands go through pad_rows / the zero-filling transposition
TILES = ["16,128", "32,128", "64,128", "128,128", "128,256", "256,256", "128,128;w8"]   # ;w8: the 8-wave 128 x 128 build
SPLITS = [1, 2, 3, 5]
# workgroup split-K ($DGA_B16_WSK=1): the smallest shape per instantiation of launch_b16_wsk's selection on 256 CUs
# (nt = ceil(N / 16) n-tiles over g = min(nt, CUs) workgroups, per = ceil(nt / g)), plus N % 16 != 0 and K % 64 != 0
WSK_SHAPES = [
    (5, 48, 64),                  # <1,4>: per = 1, one k step: seven of the eight waves own nothing
    (8, 512, 2048),               # <1,4>
    (16, 16 * 256 + 16, 2048),    # <2,3>: per = 2
    (9, 16 * 700 + 5, 1024 + 64),  # <3,2>: per = 3, N % 16 != 0, 17 k steps over 8 waves
    (16, 16 * 1300, 1152),        # <3,2>: per = 6 (two passes of three)
    (17, 80, 1024),               # <1,3,2>: two 16-row tiles of x
    (24, 16 * 300 + 7, 1152),     # <2,2,2>, N % 16 != 0
    (7, 333, 1000), (20, 333, 1000),   # K % 64 != 0: padded copies first
]
# no switch set: the shipped rules route these (tests/test_b16_exact_gpu.py cites the lines)
AUTO_SHAPES = {
    "wsk_rule_decode": (8, 512, 2048),
    "wsk_rule_two_row_tiles": (24, 1024, 2048),
    "swept_wsk": (8, 4096, 14336),
    "swept_tile": (20, 576, 7168),
    "cost_model": (1000, 4100, 4096),
    "unsplit_without_workspace": (64, 4096, 1024),
}
TAIL_KS = (64, 192)
CHILD_SHAPES = [(512, 768, 256), (700, 1000, 192), (256, 256, 64)]
CHILD_NN_ODD = (300, 523, 192)
SMALL = (150, 264, 192)          # guard bands, no-workspace entries
SMALL_KS = (192, 100, 72, 96, 320, 328)


def all_gpu_ks():
    """Every K the GPU tests feed integer operands of either dtype at."""
    ks = {MAIN[2], PAD_K, *TAIL_KS, *SMALL_KS}
    for shapes in (WSK_SHAPES, AUTO_SHAPES.values(), CHILD_SHAPES):
        ks.update(k for _, _, k in shapes)
    return sorted(ks)


def int_operands(dtype, shape, seed, lim=None):
    """Integer-valued CPU tensor of `dtype`, uniform in [-lim, lim] (default LIM[dtype])."""
    lim = LIM[dtype] if lim is None else lim
    v = np.random.default_rng(seed).integers(-lim, lim + 1, size=shape)
    return torch.from_numpy(v.astype(np.float32)).to(dtype)


def operands(dtype, m, n, k, seed, layout="nt", batch=None):
    """x [M,K] and w [N,K] ("nt", the operator) or y [K,N] ("nn", run_mmad_*), with a leading batch axis if asked."""
    lead = () if batch is None else (batch,)
    x = int_operands(dtype, lead + (m, k), 2 * seed)
    w = int_operands(dtype, lead + ((n, k) if layout == "nt" else (k, n)), 2 * seed + 1)
    return x, w


def exact(x, w_or_y, layout="nt"):
    """float64 matmul (on the device the operands lie on), returned as a numpy array.  Exact for integer operands inside the limits
    (every partial sum is an integer far below 2^53).  Exact-zero sums are +0: the kernels' accumulators start at +0, so a sum that
    cancels, or a sum of -0 products, is +0."""
    a, b = x.double(), w_or_y.double()
    s = a @ (b.transpose(-1, -2) if layout == "nt" else b)
    return s.cpu().numpy() + 0.0


def exact_special(x, w):
    """As exact(x, w, "nt") for operands that hold NaN / Inf / -0: the IEEE result, with rows of x and rows of w that hold a
    non-finite value summed explicitly (no BLAS shortcuts around 0 x Inf), everything else by the float64 matmul."""
    xd, wd = x.double().cpu().numpy(), w.double().cpu().numpy()
    with np.errstate(all="ignore"):
        s = np.where(np.isfinite(xd), xd, 0.0) @ np.where(np.isfinite(wd), wd, 0.0).T
        for r in np.flatnonzero(~np.isfinite(xd).all(axis=1)):
            s[r, :] = (xd[r][None, :] * wd).sum(axis=1)
        for c in np.flatnonzero(~np.isfinite(wd).all(axis=1)):
            s[:, c] = (xd * wd[c][None, :]).sum(axis=1)
        return s + 0.0


def _f32_bits(s):
    f = np.asarray(s, dtype=np.float64).astype(np.float32)
    assert np.array_equal(f.astype(np.float64), np.asarray(s, dtype=np.float64), equal_nan=True), "not exactly held in float32"
    return f.view(np.uint32).astype(np.int64)


def _to16(s, dtype, rne):
    """float32-exact values -> bf16 / fp16 bits in integer arithmetic; rne=False truncates toward zero (the mutation)."""
    u = _f32_bits(s)
    sign, e, man = (u >> 31) & 1, (u >> 23) & 0xFF, u & 0x7FFFFF
    if dtype == torch.bfloat16:
        h = u >> 16
        if rne:
            h = (u + 0x7FFF + (h & 1)) >> 16
        h = np.where((e == 255) & (man != 0), (sign << 15) | 0x7FC0, h)
        return h.astype(np.uint16)
    assert dtype == torch.float16
    # normal results: unbiased exponent >= -14
    hn = (np.maximum(e - 112, 0) << 10) | (man >> 13)
    rem, half = man & 0x1FFF, 0x1000
    if rne:
        hn = hn + ((rem > half) | ((rem == half) & ((hn & 1) == 1)))
    hn = np.where(e - 112 >= 31, 0x7C00 if rne else 0x7BFF, np.minimum(hn, 0x7C00))
    # subnormal results: 2^-24 units; the 24-bit significand shifted right by 126 - e (25 or more: below half a unit)
    sh = np.clip(126 - e, 14, 25)
    sig = man | 0x800000
    hs = sig >> sh
    srem, shalf = sig & ((1 << sh) - 1), 1 << (sh - 1)
    if rne:
        hs = hs + ((srem > shalf) | ((srem == shalf) & ((hs & 1) == 1)))
    hs = np.where(126 - e > 25, 0, hs)
    h = np.where(e >= 113, hn, np.where(e == 0, 0, hs))
    h = np.where(e == 255, np.where(man != 0, 0x7E00, 0x7C00), h)
    return ((sign << 15) | h).astype(np.uint16)


def round16_bits(s, dtype):
    """The bf16 / fp16 bits of the exactly held values `s` under round-to-nearest-even; fp16 rounds to +-Inf from 65520 upward."""
    return _to16(s, dtype, True)


def trunc16_bits(s, dtype):
    """What an epilogue that truncated instead of rounding would store (the harness's own mutation check)."""
    return _to16(s, dtype, False)


def f32_bits(s):
    return _f32_bits(s).astype(np.uint32)


def want_bits(s, out_dtype):
    return f32_bits(s) if out_dtype == torch.float32 else round16_bits(s, out_dtype)


def tie_stats(s, dtype):
    """Shares of the outputs that are exact ties (and which way they round), whose discarded bits are at or above one half (where a
    truncating conversion or a wrong tie rule has something to get wrong) and that truncation toward zero would in fact change (the
    former without the ties that round down anyway)."""
    u = _f32_bits(s)
    if dtype == torch.bfloat16:
        tie, odd, upper = (u & 0xFFFF) == 0x8000, ((u >> 16) & 1) == 1, (u & 0xFFFF) >= 0x8000
    else:
        assert np.abs(s).max() < 65504 and (np.abs(s)[s != 0] >= 2.0 ** -14).all()     # normal fp16 results only
        tie, odd, upper = (u & 0x1FFF) == 0x1000, ((u >> 13) & 1) == 1, (u & 0x1FFF) >= 0x1000
    return {"ties": float(tie.mean()), "ties_up": float((tie & odd).mean()), "ties_down": float((tie & ~odd).mean()),
            "upper_half": float(upper.mean()), "truncation": float((round16_bits(s, dtype) != trunc16_bits(s, dtype)).mean()), "max_abs": float(np.abs(s).max())}


def _is_nan_bits(b, kind):
    b = b.astype(np.int64)
    if kind == "bf16":
        return (b & 0x7FFF) > 0x7F80
    if kind == "fp16":
        return (b & 0x7FFF) > 0x7C00
    return (b & 0x7FFFFFFF) > 0x7F800000


def bits_of(t):
    """The bits of a torch tensor (bf16 / fp16 -> uint16, fp32 -> uint32) as a numpy array."""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def mismatch(got_bits, want, kind):
    """None if `got_bits` is `want` bit for bit -- where `want` is a NaN any NaN will do (position only: no sign, no payload) --
    else the message: the count of differing outputs and the first few (index, got, want)."""
    got_bits, want = np.asarray(got_bits), np.asarray(want)
    assert got_bits.shape == want.shape and got_bits.dtype == want.dtype, (got_bits.shape, want.shape, got_bits.dtype, want.dtype)
    if np.array_equal(got_bits, want):
        return None
    wn = _is_nan_bits(want, kind)
    bad = np.where(wn, ~_is_nan_bits(got_bits, kind), got_bits != want)
    if not bad.any():
        return None
    idx = np.argwhere(bad)
    first = ", ".join(f"{tuple(int(v) for v in i)}: got {int(got_bits[tuple(i)]):#x} want {int(want[tuple(i)]):#x}" for i in idx[:6])
    return f"{len(idx)} of {want.size} outputs differ; first {first}"


def assert_exact(got, s, what="", want=None):
    """`got` (torch tensor, any device) holds the bits of the exact result `s` rounded to its dtype (`want`: those bits, if the
    caller keeps them)."""
    msg = mismatch(bits_of(got), want_bits(s, got.dtype) if want is None else want, KIND[got.dtype])
    assert msg is None, f"{what}: {msg}"


@contextlib.contextmanager
def switches(plan=None, deep=None, wsk=None):
    """The per-call development switches of the 16-bit paths (csrc/dga_b16.hip, read per call under $DGA_B16_DEV=1, which
    tests/conftest.py sets): $DGA_B16_PLAN "bm,bn,splitk[,tail[,w8]]", $DGA_B16_DEEP "0"/"1", $DGA_B16_WSK "0"/"1".  An argument
    left None leaves its variable as it is; all three are restored on the way out."""
    names = {"DGA_B16_PLAN": plan, "DGA_B16_DEEP": deep, "DGA_B16_WSK": wsk}
    old = {k: os.environ.get(k) for k in names}
    try:
        for k, v in names.items():
            if v is not None:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def plan_of(tile, split, tail=0):
    """"bm,bn" or "bm,bn;w8" + split-K (+ sub-tile tail) -> the $DGA_B16_PLAN string."""
    base, w8 = tile.split(";")[0], ";" in tile
    if w8:
        return f"{base},{split},0,1"
    return f"{base},{split},{tail}" if tail else f"{base},{split}"
