"""The harness of tests/test_b16_exact_gpu.py, checked on the CPU: the integer rounding of b16_cases.round16_bits against torch's
conversions, the limits inside which the float64 matmul is the exact reference of every 16-bit GEMM path, that the main shape's
expected outputs are rich in rounding ties (so a truncating or wrongly rounding epilogue cannot pass), and that the comparison
function itself notices a truncated result and a single dropped product."""
import numpy as np
import pytest
import torch

import b16_cases as C

DTYPES = [torch.bfloat16, torch.float16]


def _torch_bits(v, dtype):
    return torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dtype).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_round16_bits_is_torch_rounding_on_every_integer(dtype):
    v = np.arange(-70000, 70001, dtype=np.float64)
    assert np.array_equal(C.round16_bits(v, dtype), _torch_bits(v, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_round16_bits_on_every_exact_tie(dtype):
    """Every midpoint between two neighbouring finite 16-bit values of either sign (exactly held in float32): the even
    neighbour, both directions occurring."""
    pos = np.arange(0x0001 if dtype == torch.float16 else 0x0080, 0x7C00 if dtype == torch.float16 else 0x7F80, dtype=np.uint16)
    lo = torch.from_numpy(pos[:-1].view(np.int16)).view(dtype).double().numpy()
    hi = torch.from_numpy(pos[1:].view(np.int16)).view(dtype).double().numpy()
    mid = (lo + hi) / 2
    even = np.where(pos[:-1] & 1, pos[1:], pos[:-1])
    for sgn, sbit in ((1.0, 0), (-1.0, 0x8000)):
        got = C.round16_bits(sgn * mid, dtype)
        assert np.array_equal(got, even | sbit)
        assert np.array_equal(got, _torch_bits(sgn * mid, dtype))
    assert (even == pos[:-1]).any() and (even == pos[1:]).any()
    # ... and a hair to either side of the midpoint goes to the nearer neighbour (float32 has the bits to spare)
    near = mid.astype(np.float32).view(np.uint32).astype(np.int64)
    for d, want in ((-1, pos[:-1]), (1, pos[1:])):
        assert np.array_equal(C.round16_bits((near + d).astype(np.uint32).view(np.float32).astype(np.float64), dtype), want)


def test_fp16_overflow_boundary_and_specials():
    v = np.array([65504, 65519, 65519.996, 65520, 65536, 1e9, -65519, -65520, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    want = np.array([0x7BFF, 0x7BFF, 0x7BFF, 0x7C00, 0x7C00, 0x7C00, 0xFBFF, 0xFC00, 0x7C00, 0xFC00, 0, 0x8000], dtype=np.uint16)
    assert np.array_equal(C.round16_bits(v.astype(np.float64), torch.float16), want)
    assert np.array_equal(_torch_bits(v, torch.float16), want)
    for dtype in DTYPES:
        nan = C.round16_bits(np.array([np.nan]), dtype)
        assert C.mismatch(nan, _torch_bits([np.nan], dtype), C.KIND[dtype]) is None
    # subnormal results (the subnormal-input cases produce them) and random float32 values
    rng = np.random.default_rng(1)
    sub = (rng.integers(-(1 << 22), 1 << 22, size=20000) * 2.0 ** -34)
    rnd = rng.standard_normal(20000).astype(np.float32).astype(np.float64) * 2.0 ** rng.integers(-30, 18, size=20000)
    for v in (sub, rnd):
        for dtype in DTYPES:
            assert np.array_equal(C.round16_bits(v, dtype), _torch_bits(v, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_gpu_shape_is_exactly_summable(dtype):
    lim = C.LIM[dtype]
    x = C.int_operands(dtype, (64, 4096), 5)
    assert float(x.float().abs().max()) == lim and bool((x.float() == x.float().round()).all())
    assert torch.equal(x.float().to(dtype), x)          # exactly representable
    for k in C.all_gpu_ks():
        assert lim * lim * k < 2 ** 24, (dtype, k)
    assert max(C.all_gpu_ks()) == 14336


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [C.MAIN[2], C.PAD_K])
def test_the_main_shape_cannot_go_vacuous(dtype, k):
    """Shares at K = 1344, seed 0: bf16 21.5 % ties (10.8 % / 10.7 % each way), 38.6 % with the discarded bits at or above one half,
    27.9 % changed by truncation toward zero, max |S| 3920; fp16 17.0 % (8.6 % / 8.5 %), 43.7 %, 35.2 %, max |S| 56329.  (The
    second figure less the ties that round down is the third: those truncation gets right by luck.  The third follows from the mix of
    ulps -- 0 below 256, 1/4 at ulp 2, 3/8 at ulp 4, 7/16 at ulp 8 -- under |S| ~ N(0, 24 * 24 * K): a quarter at the least.)"""
    m, n, _ = C.MAIN
    x, w = C.operands(dtype, m, n, k, C.MAIN_SEED)
    s = C.exact(x, w)
    st = C.tie_stats(s, dtype)
    print(C.KIND[dtype], k, st)
    assert st["ties"] >= 0.10 and st["ties_up"] >= 0.05 and st["ties_down"] >= 0.05 and st["upper_half"] >= 0.30
    assert st["truncation"] >= 0.25
    assert abs(st["upper_half"] - st["ties_down"] - st["truncation"]) < 1e-12
    assert st["max_abs"] < 2 ** 24 and (dtype != torch.float16 or st["max_abs"] < 65504)
    assert not np.signbit(s[s == 0]).any()
    # the same through the batched NN operands of run_mmad_rtc (fp32 out: no rounding, the bound alone)
    xb, yb = C.operands(dtype, m, 523, k, C.MAIN_SEED, "nn", batch=2)
    sb = C.exact(xb, yb, "nn")
    assert sb.shape == (2, m, 523) and np.abs(sb).max() < 2 ** 24
    assert np.array_equal(sb[1], xb[1].double().numpy() @ yb[1].double().numpy())


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_comparison_notices_truncation_and_one_dropped_product(dtype):
    m, n, k = C.MAIN
    x, w = C.operands(dtype, m, n, k, C.MAIN_SEED)
    s = C.exact(x, w)
    kind = C.KIND[dtype]
    good = C.round16_bits(s, dtype)
    assert C.mismatch(good.copy(), good, kind) is None
    # a kernel whose epilogue truncated
    msg = C.mismatch(C.trunc16_bits(s, dtype), good, kind)
    assert msg is not None and "outputs differ" in msg and int(msg.split()[0]) >= 0.25 * s.size
    # a kernel that dropped ONE product of ONE output: a product large enough to move the rounded value, then the fp32 output on
    # the smallest non-zero product
    xd, wd = x.double().numpy(), w.double().numpy()
    r, c = 123, 457
    prods = xd[r] * wd[c]
    dropped = s.copy()
    dropped[r, c] -= prods[np.argmax(np.abs(prods))]
    assert C.round16_bits(dropped, dtype)[r, c] != good[r, c]
    msg = C.mismatch(C.round16_bits(dropped, dtype), good, kind)
    assert msg is not None and msg.startswith("1 of ") and f"({r}, {c})" in msg
    small = s.copy()
    small[r, c] -= prods[prods != 0][np.argmin(np.abs(prods[prods != 0]))]
    msg = C.mismatch(C.f32_bits(small), C.f32_bits(s), "fp32")
    assert msg is not None and msg.startswith("1 of ")
    # NaN positions: any NaN matches a wanted NaN, a number does not, and a NaN where a number is wanted does not
    nan = {"bf16": (0x7FC0, 0xFFFF), "fp16": (0x7E00, 0xFFFF)}[kind]
    want = good.copy(); want[0, 0] = nan[0]
    got = want.copy(); got[0, 0] = nan[1]
    assert C.mismatch(got, want, kind) is None
    assert C.mismatch(good, want, kind) is not None and C.mismatch(want, good, kind) is not None


def test_exact_special_is_the_ieee_result():
    x = C.int_operands(torch.float16, (9, 40), 3)
    w = C.int_operands(torch.float16, (11, 40), 4)
    x[1, 5] = float("nan"); w[2, 7] = float("inf"); w[6, 9] = float("-inf"); x[3, 7] = 0.0; x[4] = -0.0
    s = C.exact_special(x, w)
    xd, wd = x.double().numpy(), w.double().numpy()
    with np.errstate(all="ignore"):
        want = np.array([[sum(xd[i, t] * wd[j, t] for t in range(40)) for j in range(11)] for i in range(9)]) + 0.0
    assert np.array_equal(np.isnan(s), np.isnan(want)) and np.array_equal(s[~np.isnan(s)], want[~np.isnan(want)])
    assert np.isnan(s[1]).all() and np.isnan(s[3, 2]) and np.isnan(s[4, 2]) and np.isnan(s[4, 6])
    assert (s[4, [0, 1, 3, 4, 5]] == 0).all() and not np.signbit(s[4, [0, 1, 3, 4, 5]]).any()
    assert np.isinf(s[0, 2]) or np.isnan(s[0, 2])


def test_switches_sets_and_restores(monkeypatch):
    import os
    monkeypatch.setenv("DGA_B16_PLAN", "64,128,2")
    monkeypatch.delenv("DGA_B16_DEEP", raising=False)
    monkeypatch.delenv("DGA_B16_WSK", raising=False)
    with C.switches(plan="256,256,1", deep="1"):
        assert os.environ["DGA_B16_PLAN"] == "256,256,1" and os.environ["DGA_B16_DEEP"] == "1" and "DGA_B16_WSK" not in os.environ
        with C.switches(wsk="0"):
            assert os.environ["DGA_B16_WSK"] == "0" and os.environ["DGA_B16_PLAN"] == "256,256,1"
        assert "DGA_B16_WSK" not in os.environ
    assert os.environ["DGA_B16_PLAN"] == "64,128,2" and "DGA_B16_DEEP" not in os.environ
    assert C.plan_of("128,128;w8", 3) == "128,128,3,0,1" and C.plan_of("256,256", 1, 64) == "256,256,1,64"
