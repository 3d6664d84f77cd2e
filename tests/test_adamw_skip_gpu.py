"""GPU: skip= of adamw_per_block_cast_to_fp8_transposed.  With skip[0] = 1 the call stores nothing to w, m and v, whatever the gradient
holds, and writes every element of every output with per_block_cast_to_fp8_transposed of the unchanged w, byte for byte; with skip[0] = 0
and with skip=None every bit of every result is what tests/adamw_ref.py defines, and the two are equal."""
import numpy as np
import pytest
import torch

import adamw_ref as A

pytestmark = pytest.mark.gpu

SHAPES = ((2, 136, 264), (1, 128, 128))
assert all(s in A.SHAPES for s in SHAPES)
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
HYPER = dict(beta1=A.BETA1, beta2=A.BETA2, eps=A.EPS, weight_decay=A.WD)
SC3 = A.scalars(3, A.LR, A.BETA1, A.BETA2, 0.5)
SENTINEL_SF = 0x7FC0A5A5

MOMENT = pytest.mark.parametrize("moment", A.DTYPES, ids=["m32", "m16"])
ROWWISE = pytest.mark.parametrize("rowwise", [False, True], ids=["transposed", "rowwise"])
SHAPE = pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))


def _state(w, m, v, g, moment):
    dev = lambda a, kind: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(TORCH_DT[kind]).cuda()
    return dev(w, "fp32"), dev(m, moment), dev(v, moment), dev(g, "fp32")


def _outs(shape, rowwise, byte):
    """out= pre-filled: codes with `byte`, scales with a NaN pattern no scale can be."""
    lead, (n, k) = tuple(shape[:-2]), shape[-2:]
    nb, kb = (n + 127) // 128, (k + 127) // 128
    q = lambda *s: torch.full(s, byte, dtype=torch.uint8, device="cuda")
    sf = lambda *s: torch.full(s, SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    t = (q(*lead, k, n), sf(*lead, kb, nb))
    return (t, (q(*lead, n, k), sf(*lead, nb, kb))) if rowwise else t


def _flat(res, rowwise):
    return list(res[0] + res[1]) if rowwise else list(res)


def _raw(t):
    return t.contiguous().view(torch.uint8)


def _flag(value):
    return torch.tensor([value], dtype=torch.int32, device="cuda")


@SHAPE
@MOMENT
@ROWWISE
def test_a_skipped_step_leaves_the_state_and_quantises_it(dga, shape, moment, rowwise):
    w, m, v, g = A.inputs(shape, "fp32", moment, seed=31)
    rng = np.random.default_rng(32)
    for bad in (np.nan, np.inf, -np.inf):                                          # sprinkled over the gradient, the corners included
        g.reshape(-1)[rng.integers(0, g.size, 20)] = bad
    g.reshape(-1)[[0, -1]] = np.nan
    results = []
    for byte in (0xA5, 0x5A):
        W, M, V, Gr = _state(w, m, v, g, moment)
        before = [t.clone() for t in (W, M, V, Gr)]
        res = dga.adamw_per_block_cast_to_fp8_transposed(W, M, V, Gr, torch.from_numpy(SC3).cuda(), rowwise=rowwise, out=_outs(shape, rowwise, byte),
                                                         skip=_flag(1), sync=True, **HYPER)
        for name, t, b in zip(("w", "m", "v", "grad"), (W, M, V, Gr), before):
            assert torch.equal(_raw(t), _raw(b)), f"{name} changed under skip = 1"
        want = dga.per_block_cast_to_fp8_transposed(W, rowwise=rowwise, sync=True)
        for got, exp in zip(_flat(res, rowwise), _flat(want, rowwise)):
            assert got.shape == exp.shape and torch.equal(_raw(got), _raw(exp)), "not per_block_cast_to_fp8_transposed(w)"
            if got.dtype == torch.float32:
                assert not bool((got.view(torch.int32) == SENTINEL_SF).any()), "a scale was not written"
        results.append([_raw(t).clone() for t in _flat(res, rowwise)])
    # the same bytes over a 0xA5 and over a 0x5A pre-fill: no byte of any output is left as it was
    assert all(torch.equal(a, b) for a, b in zip(*results))
    # a flag of any non-zero value skips
    W, M, V, Gr = _state(w, m, v, g, moment)
    dga.adamw_per_block_cast_to_fp8_transposed(W, M, V, Gr, torch.from_numpy(SC3).cuda(), rowwise=rowwise, skip=_flag(-7), sync=True, **HYPER)
    assert torch.equal(_raw(W), _raw(_state(w, m, v, g, moment)[0]))


@SHAPE
@MOMENT
@ROWWISE
def test_a_zero_flag_and_no_flag_are_the_step_there_was(dga, shape, moment, rowwise):
    w, m, v, g = A.inputs(shape, "fp32", moment, seed=33)
    w2, m2, v2 = A.step(w, m, v, g, SC3, *(A.f32(HYPER[x]) for x in ("beta1", "beta2", "eps", "weight_decay")))
    assert np.isfinite(w2).all()
    runs = []
    for skip in (_flag(0), None):
        W, M, V, Gr = _state(w, m, v, g, moment)
        res = dga.adamw_per_block_cast_to_fp8_transposed(W, M, V, Gr, torch.from_numpy(SC3).cuda(), rowwise=rowwise, out=_outs(shape, rowwise, 0xA5),
                                                         skip=skip, sync=True, **HYPER)
        for name, t, want, kind in (("w", W, w2, "fp32"), ("m", M, m2, moment), ("v", V, v2, moment)):
            got = t.view(torch.int32 if kind == "fp32" else torch.int16).cpu().numpy().view(np.uint32 if kind == "fp32" else np.uint16)
            bad = A.same_bits(got, A.moment_bits(want, kind), want)
            assert bad[0].size == 0, f"{name}: {bad[0].size} elements differ from the reference (skip = {skip})"
        want = dga.per_block_cast_to_fp8_transposed(W, rowwise=rowwise, sync=True)
        for got, exp in zip(_flat(res, rowwise), _flat(want, rowwise)):
            assert torch.equal(_raw(got), _raw(exp))
        runs.append([_raw(t).clone() for t in (W, M, V) + tuple(_flat(res, rowwise))])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
