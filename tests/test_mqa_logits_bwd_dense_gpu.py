"""GPU: fp8_mqa_logits_bwd_dense against tests/mqa_logits_bwd_ref.py (the ranges written out as lists), M = 70 tokens over N = 300 keys:
35 token pairs of the token-owned pass, two runs of 64 (the second ragged, one chunk each) and five key tiles of 64 (the last ragged) of
the key-owned one."""
import functools

import numpy as np
import pytest
import torch

import mqa_logits_bwd_ref as B
import mqa_logits_ref as Q

pytestmark = pytest.mark.gpu
M, N = 70, 300
dev = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).cuda()
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def _lists(ks, ke):
    """the [M, N] lists the reference takes: n where in range, -1 elsewhere"""
    return np.where(Q.in_range(ks, ke, N), np.arange(N, dtype=np.int32)[None, :], np.int32(-1)).astype(np.int32)


def _run(dga, q, k, kscale, w, dl, ks, ke, **kw):
    return tuple(x.cpu().numpy() for x in dga.fp8_mqa_logits_bwd_dense(dev(q), (dev(k), dev(kscale)), dev(w), dev(dl), dev(ks), dev(ke), sync=True, **kw))


@functools.lru_cache(maxsize=None)
def _exact_case(h, kind):
    """codes and weights of mqa_logits_ref.exact_operands, kscale 1 or 2, d_logits +-{0.5, 1, 2} or 0 inside the ranges and NaN outside"""
    q, k, _, w = Q.exact_operands(M, N, h)
    rng = np.random.default_rng([h, len(kind)])
    kscale = rng.choice([1.0, 2.0], size=N).astype(np.float32)
    ks, ke = Q.ranges(kind, M, N)
    dl = (rng.choice([-1.0, 0.0, 1.0], size=(M, N), p=[0.45, 0.1, 0.45]) * 2.0 ** rng.integers(-1, 2, size=(M, N))).astype(np.float32)
    dl[~Q.in_range(ks, ke, N)] = np.nan
    return (q, k, kscale, w, dl, ks, ke), B.reference(q, k, kscale, w, _lists(ks, ke), dl)


@functools.lru_cache(maxsize=None)
def _random_operands(h):
    """amax-quantised normal q and k (the q scale folded into normal weights), normal d_logits"""
    gen = torch.Generator(device="cpu").manual_seed(23 + h)

    def quantised(*shape):
        x = torch.randn(shape, generator=gen)
        scale = x.abs().amax(-1, keepdim=True) / 448.0
        return (x / scale).to(torch.float8_e4m3fn).view(torch.uint8).numpy(), scale.squeeze(-1).numpy()

    (q, qs), (k, kscale) = quantised(M, h, B.D), quantised(N, B.D)
    return q, k, kscale, torch.randn((M, h), generator=gen).numpy() * qs, torch.randn((M, N), generator=gen).numpy()


def _inside(got, ref, h, prior=0.0):
    pairs = [("dq", np.abs(got[0] - ref["dq"]), ref["err_dq"]), ("dk", np.abs(got[1].astype(np.float64) - prior - ref["dk"]), B.bound_dk(ref, h, prior)),
             ("d_weights", np.abs(got[2] - ref["dw"]), ref["err_dw"])]
    print("worst error / bound: " + " ".join("%s %.3f" % (name, float((err / np.maximum(bar, 1e-300)).max())) for name, err, bar in pairs))
    for name, err, bar in pairs:
        assert np.isfinite(err).all() and (err <= bar).all(), (name, int((err > bar).sum()), np.argwhere(err > bar)[:4])


@pytest.mark.parametrize("kind", ("full", "causal", "windows", "mixed"))
@pytest.mark.parametrize("h", Q.HEADS)
def test_exactly_summable_operands_bit_for_bit(dga, h, kind):
    """every G is exact in bf16 and every partial sum exact in fp32 (dq: quantum 2^-5, terms <= 32, <= 300 of them; dk: 2^-5, <= 16,
    <= 4480; d_weights: 2^-3, <= 2048, <= 300 -- all below 2^24 quanta): the three outputs equal the float64 reference as values"""
    ops, ref = _exact_case(h, kind)
    for name, got in zip(("dq", "dk", "dw"), _run(dga, *ops)):
        assert np.array_equal(got.astype(np.float64), ref[name]), (name, np.argwhere(got != ref[name])[:4])
    assert np.abs(ref["dk"]).max() > 0 and np.abs(ref["dq"]).max() > 0


@pytest.mark.parametrize("h", Q.HEADS)
def test_derived_bounds_on_random_data(dga, h):
    """windows ranges, dk over a non-zero prior: every element inside the existing reference's bounds"""
    q, k, kscale, w, dl = _random_operands(h)
    ks, ke = Q.ranges("windows", M, N)
    prior = ((np.arange(N * B.D) % 251 - 125) * 0.25).astype(np.float32).reshape(N, B.D)
    ref = B.reference(q, k, kscale, w, _lists(ks, ke), dl)
    _inside(_run(dga, q, k, kscale, w, dl, ks, ke, dk=dev(prior.copy())), ref, h, prior.astype(np.float64))


@pytest.mark.parametrize("clamped", (False, True))
def test_layouts_and_untouched_bytes(dga, clamped):
    """d_logits a column slice of a wider NaN-filled buffer, dk rows 160 apart over a byte pattern: the padding and the rows no range names
    keep their bytes, empty tokens get +0 rows of dq and d_weights; clamped: token 9 has ks < 0 and ke > N and names every row"""
    h, (q, k, kscale, w, dl) = 32, _random_operands(32)
    ks, ke = Q.ranges("windows", M, N)
    ks, ke = np.clip(ks, 70, 230).astype(np.int32), np.clip(ke, 70, 230).astype(np.int32)
    ks[3], ke[3], ks[64], ke[64], ks[69], ke[69] = 100, 100, 200, 150, N, N + 5           # empty: equal, crossed, beyond the keys
    if clamped:
        ks[9], ke[9] = -5, N + 40
    inr = Q.in_range(ks, ke, N)
    empty, unnamed = ~inr.any(1), ~inr.any(0)
    assert empty.sum() >= 3 and (unnamed.sum() == 0 if clamped else unnamed.sum() >= 100)
    wide = np.full((M, N + 20), np.nan, np.float32)
    wide[:, 8:8 + N] = np.where(inr, dl, np.nan)
    prior = ((np.arange(N * 160) % 251 - 125) * 0.25).astype(np.float32).reshape(N, 160)
    dk = dev(prior.copy())[:, :B.D]
    got = _run(dga, q, k, kscale, w, dev(wide)[:, 8:8 + N], ks, ke, dk=dk)
    _inside(got, B.reference(q, k, kscale, w, _lists(ks, ke), dl), h, prior[:, :B.D].astype(np.float64))
    full = bits(dk.as_strided((N, 160), (160, 1)).cpu().numpy())
    assert np.array_equal(full[unnamed], bits(prior)[unnamed]) and np.array_equal(full[:, B.D:], bits(prior)[:, B.D:])
    assert not bits(got[0])[empty].any() and not bits(got[2])[empty].any()


def test_reproducibility_and_graph_replay(dga):
    """two calls give the same bytes in dq, dk and d_weights; one captured graph replayed under other ranges and d_logits gives the eager
    bytes of all three (dk is added into: cleared outside the graph)"""
    h, (q, k, kscale, w, dl) = 64, _random_operands(64)
    first, second = Q.ranges("windows", M, N), Q.ranges("causal", M, N)
    a, b = _run(dga, q, k, kscale, w, dl, *first), _run(dga, q, k, kscale, w, dl, *first)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b)) and np.abs(a[1]).max() > 0
    tq, tk, tks, tw, tdl, lo, hi = (dev(x) for x in (q, k, kscale, w, dl.copy(), first[0].copy(), first[1].copy()))
    dk = torch.zeros((N, B.D), dtype=torch.float32, device="cuda")
    both = lambda out_dk: dga.fp8_mqa_logits_bwd_dense(tq, (tk, tks), tw, tdl, lo, hi, dk=out_dk)
    both(dk)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = both(dk)
    for (s, e), d in ((second, -0.5 * dl[::-1]), (first, dl), (second, dl)):
        lo.copy_(dev(s)), hi.copy_(dev(e)), tdl.copy_(dev(np.ascontiguousarray(d)))
        want = [x.clone() for x in both(torch.zeros_like(dk))]
        dk.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(out, want))
