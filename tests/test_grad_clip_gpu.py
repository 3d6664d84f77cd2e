"""GPU: grad_sumsq and grad_clip_scalars against their definitions (tests/grad_clip_ref.py).  The sum of squares is held to
|sumsq - fsum| <= (n + 1) 2^-53 fsum, to the exact integer where the data make every addition exact, and to the same 8 bytes wherever the
tensor lies and however often it runs; the scalars to the float64 definition rounded once, bit for bit on every row: the device's
float64 root and quotient are the correctly rounded ones, as numpy's are (on an MI355X no row differed in any place)."""
import numpy as np
import pytest
import torch

import grad_clip_ref as R

pytestmark = pytest.mark.gpu

C = R.CHUNK
DTYPES = ("fp32", "bf16")
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _exact_in(a, kind):
    return np.ascontiguousarray(a, np.float32) if kind == "fp32" else R.bf16(a)


def _dev(a, kind):
    """float32 values exact in `kind` -> a device tensor of that dtype."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(TORCH_DT[kind]).cuda()


def _bits(t):
    return int(t.cpu().numpy().view(np.uint64)[0])


def _value(t):
    return float(t.cpu().numpy()[0])


def _normal(n, kind, seed):
    rng = np.random.default_rng([seed, n])
    return _exact_in(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n), kind)


def _within(got, arrays):
    exact, n = R.sumsq(arrays), R.count(arrays)
    err, bar = abs(got - exact), R.bound(n, exact)
    print("n = %d: |sumsq - fsum| = %.3g, bound %.3g" % (n, err, bar))
    assert err <= bar, (got, exact)


@pytest.mark.parametrize("kind", DTYPES)
@pytest.mark.parametrize("n", R.SIZES)
def test_sizes_on_normal_data(dga, n, kind):
    a = _normal(n, kind, seed=1)
    got = dga.grad_sumsq(_dev(a, kind), sync=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == (1,)
    _within(_value(got), [a])
    if n == 0:
        assert _bits(got) == 0


@pytest.mark.parametrize("kind,top", (("fp32", 1024), ("bf16", 256)))
def test_integer_data_sum_exactly(dga, kind, top):
    """Integers: every square and every partial sum is an integer below 2^53, so every addition is exact in float64 -- and the sum is
    beyond 2^24, where a float32 accumulator loses integers."""
    n = 3 * C + 5
    a = np.random.default_rng(3).integers(-top, top + 1, n).astype(np.float32)
    assert np.array_equal(_exact_in(a, kind), a)
    exact = int(np.square(a.astype(np.int64)).sum())
    assert 2 ** 24 < exact < 2 ** 53 and float(np.float32(exact)) != exact     # float32 cannot even hold the result
    got = dga.grad_sumsq(_dev(a, kind), sync=True)
    assert _value(got) == float(exact) and int(_value(got)) == exact


def test_range(dga):
    n = 3 * C + 5
    big = np.where(np.arange(n) % 2 == 0, 3e19, -3e19).astype(np.float32)
    with np.errstate(over="ignore"):
        assert np.isinf(np.square(big)).all()                                     # the squares overflow float32
    got = _value(dga.grad_sumsq(_dev(big, "fp32"), sync=True))
    assert np.isfinite(got)
    _within(got, [big])
    tiny = np.full(n, 2.0 ** -140, np.float32)
    assert 0 < tiny[0] < np.float32(2.0 ** -126)                                  # a float32 subnormal
    got = _value(dga.grad_sumsq(_dev(tiny, "fp32"), sync=True))
    assert got == n * 2.0 ** -280


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf), ids=("nan", "+inf", "-inf"))
def test_one_non_finite_element_makes_the_sum_non_finite(dga, bad):
    arrays = [_normal(C + 1, "fp32", 4), _normal(7, "bf16", 5), _normal(2 * C + 3, "fp32", 6)]
    kinds = ("fp32", "bf16", "fp32")
    clean = _value(dga.grad_sumsq([_dev(a, k) for a, k in zip(arrays, kinds)], sync=True))
    assert np.isfinite(clean)
    _within(clean, arrays)
    arrays[2][-1] = bad                                                           # the last element of the last chunk of the list
    got = _value(dga.grad_sumsq([_dev(a, k) for a, k in zip(arrays, kinds)], sync=True))
    assert np.isnan(got) if np.isnan(bad) else got == np.inf
    arrays[2][-1], arrays[1][3] = 1.0, bad                                        # ... and of a short bfloat16 tensor in the middle
    got = _value(dga.grad_sumsq([_dev(a, k) for a, k in zip(arrays, kinds)], sync=True))
    assert not np.isfinite(got)


@pytest.mark.parametrize("kind", DTYPES)
def test_alignment_does_not_change_the_bits(dga, kind):
    n = 2 * C + 3
    a = _normal(n, kind, seed=7)
    fresh = _dev(a, kind)
    assert fresh.data_ptr() % 16 == 0
    want = _bits(dga.grad_sumsq(fresh, sync=True))
    _within(_value(dga.grad_sumsq(fresh, sync=True)), [a])
    for shift in (1, 3):
        buf = torch.zeros(n + 8, dtype=TORCH_DT[kind], device="cuda")
        view = buf[shift:shift + n]
        view.copy_(fresh)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        assert _bits(dga.grad_sumsq(view, sync=True)) == want, shift


def test_a_mixed_list_of_130_tensors(dga):
    """Three stage-1 launches (64 list entries each at most): the bound, the same bits twice, and accumulate=True."""
    arrays, kinds = [], []
    for i in range(130):
        kinds.append(DTYPES[i % 2])
        arrays.append(_normal(R.SIZES[i % len(R.SIZES)], kinds[-1], seed=100 + i))
    assert len(arrays) > 2 * 64 and any(a.size == 0 for a in arrays)
    tensors = [_dev(a, k) for a, k in zip(arrays, kinds)]
    first = dga.grad_sumsq(tensors, sync=True)
    _within(_value(first), arrays)
    again = dga.grad_sumsq(tuple(tensors), sync=True)
    assert _bits(again) == _bits(first)
    prefill = 12345.678
    out = torch.tensor([prefill], dtype=torch.float64, device="cuda")
    assert dga.grad_sumsq(tensors, out=out, accumulate=True, sync=True) is out
    assert _value(out) == prefill + _value(first)                                  # fl64(prefill + sum): one float64 addition
    assert _bits(dga.grad_sumsq(tensors, out=out, sync=True)) == _bits(first)      # without accumulate out is overwritten
    empty = torch.tensor([3.0], dtype=torch.float64, device="cuda")
    dga.grad_sumsq([torch.zeros(0, device="cuda")], out=empty, accumulate=True, sync=True)
    assert _value(empty) == 3.0
    dga.grad_sumsq([torch.zeros(0, device="cuda")], out=empty, sync=True)
    assert _bits(empty) == 0


def _f32_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _same(got, want):
    """Bit for bit; a NaN for a NaN (IEEE leaves its sign and payload open)."""
    return bool(np.isnan(got)) if np.isnan(want) else _f32_bits(got) == _f32_bits(want)


@pytest.mark.parametrize("row", range(len(R.CLIP_TABLE)))
def test_clip_scalars_against_the_definition(dga, row):
    ss, max_norm, pre_scale, eps, exact = R.CLIP_TABLE[row]
    sumsq = torch.tensor([ss], dtype=torch.float64, device="cuda")
    before = np.array([0.1, 0.2, 0.3, 0.4], np.float32)
    sc = torch.from_numpy(before.copy()).cuda()
    outs = (torch.full((1,), 7.0, device="cuda"), torch.full((1,), 7.0, device="cuda"), torch.full((1,), 7, dtype=torch.int32, device="cuda"))
    res = dga.grad_clip_scalars(sumsq, sc, max_norm, pre_scale=pre_scale, eps=eps, out=outs, sync=True)
    assert res.norm is outs[0] and res.coef is outs[1] and res.skip is outs[2]
    norm, coef, scale, skip = R.clip_scalars(ss, max_norm, pre_scale, eps)
    got_sc = sc.cpu().numpy()
    got = (res.norm.item(), res.coef.item(), float(got_sc[3]))
    differ = [name for name, g, w in zip(("norm", "coef", "grad_scale"), got, (norm, coef, scale)) if _f32_bits(g) != _f32_bits(w) and not np.isnan(w)]
    print("row %d: %s; differing in the last place: %s" % (row, got, differ or "none"))
    assert int(res.skip.item()) == skip and skip == (0 if np.isfinite(ss) else 1)
    assert np.array_equal(got_sc[:3].view(np.uint32), before[:3].view(np.uint32)), "step_scalars[0..2] were written"
    if skip:
        assert _f32_bits(got[1]) == 0 and _f32_bits(got[2]) == 0 and not np.isfinite(got[0])
    for name, g, w in zip(("norm", "coef", "grad_scale"), got, (norm, coef, scale)):
        assert _same(np.float32(g), w), (name, g, w)


def test_the_fresh_outputs_and_the_wrapper(dga):
    """Without out= the results are new tensors; clip_grad_norm_step_scalars is the two calls."""
    a, b = _normal(C + 9, "fp32", 8), _normal(300, "bf16", 9)
    ta, tb = _dev(a, "fp32"), _dev(b, "bf16")
    sc = torch.tensor([1e-3, 0.5, 0.5, 9.0], device="cuda")
    res = dga.clip_grad_norm_step_scalars([ta, tb], sc, 1.0, pre_scale=0.5)
    torch.cuda.synchronize()
    assert res.norm.dtype == torch.float32 and res.skip.dtype == torch.int32 and res.sumsq.dtype == torch.float64
    _within(_value(res.sumsq), [a, b])
    sc2 = torch.tensor([1e-3, 0.5, 0.5, 9.0], device="cuda")
    two = dga.grad_clip_scalars(dga.grad_sumsq((ta, tb)), sc2, 1.0, pre_scale=0.5, sync=True)
    assert torch.equal(sc, sc2) and sc[3].item() != 9.0 and all(torch.equal(x, y) for x, y in zip(res[:3], two))
    norm, coef, scale, skip = R.clip_scalars(_value(res.sumsq), 1.0, 0.5)
    assert coef < 1 and res.skip.item() == 0 and _same(np.float32(res.coef.item()), coef)
