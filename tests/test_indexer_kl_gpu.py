"""GPU: indexer_kl_loss against tests/indexer_kl_ref.py.  lse is the float64 forward reference's rounded to fp32 everywhere but in the
end-to-end test, so that these tests do not hang on the forward kernel."""
import numpy as np
import pytest
import torch

import indexer_kl_ref as K
import mqa_logits_bwd_ref as B
import sparse_mla_ref as R
from sparse_mla_support import NAN_FILL, _bf16

pytestmark = pytest.mark.gpu
raw = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).cuda()
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def _run(dga, q, kv, idx, lse, scale, logits, **kw):
    """the operator on host arrays (tensors pass through): (loss, d_logits, target) on the host"""
    dev = lambda x: x if isinstance(x, torch.Tensor) else _bf16(x)
    return tuple(o.cpu().numpy() for o in dga.indexer_kl_loss(dev(q), dev(kv), raw(idx), raw(lse), scale, raw(logits), sync=True, **{"want_target": True, **kw}))


@pytest.mark.parametrize("empty_lse", (-np.inf, np.nan))
@pytest.mark.parametrize("topk", K.TOPKS)
@pytest.mark.parametrize("h", K.HEADS)
def test_derived_bounds_on_random_data(dga, h, topk, empty_lse):
    """every wave split; one position, a short tile, one tile, a tile and one, ten tiles; token 3 has no valid position and an lse of
    -inf or NaN: +0 everywhere, as every invalid position"""
    ops, ref = K.random_case(h, topk, empty_lse)
    got = _run(dga, *ops, grad_scale=K.GRAD_SCALE)
    K.inside(got, ref)
    invalid = ~R.rows_of(ops[2], R.S4)[1]
    assert invalid[3].all() and not bits(got[0])[3] and not bits(got[1])[invalid].any() and not bits(got[2])[invalid].any()


@pytest.mark.parametrize("h", R.PEAK_HEADS)
def test_peaked_scores_and_logits(dga, h):
    """scores spread up to SPREAD_MAX, logits over +-40, and a planted position whose target is exactly 0 in fp32: the t > 0 guard"""
    ops, ref = K.peaked_case(h)
    planted = ref["t"][:, 5]
    assert (planted > 0).all() and not planted.astype(np.float32).any() and ref["t"].astype(np.float32)[:, :5].all()
    got = _run(dga, *ops, grad_scale=K.GRAD_SCALE)
    K.inside(got, ref)
    assert all(np.isfinite(g).all() for g in got) and not bits(got[2])[:, 5].any()


def _framed(shape):
    """a NaN-filled allocation and a float32 view of `shape` eight elements inside it"""
    n = int(np.prod(shape))
    whole = torch.full((n + 16,), NAN_FILL, dtype=torch.int32, device="cuda")
    return whole, whole[8:8 + n].view(torch.float32).view(shape)


def test_layouts_and_untouched_bytes(dga):
    """indices [M, 1, topk] sliced from a wider buffer and relative to offsets, kv [S, 1, 576] rows 640 apart with NaN between them, logits
    a column slice of a wider NaN buffer, the three outputs inside NaN-filled allocations: not a byte outside them changes"""
    h, topk = 48, 33
    (q, kv, idx, lse, scale, logits), ref = K.random_case(h, topk)
    off = -np.arange(1, 6, dtype=np.int32)
    wide_idx = raw(np.concatenate([np.where(idx >= 0, idx - off[:, None], idx).astype(np.int32), np.full((R.M4, 7), 3, np.int32)], axis=1))[:, None, :topk]
    wide_kv = _bf16(np.concatenate([kv, np.full((R.S4, 64), np.nan, np.float32)], axis=1))[:, None, :R.D_QK]
    wide_lg = raw(np.concatenate([np.full((R.M4, 3), np.nan, np.float32), logits, np.full((R.M4, 6), np.nan, np.float32)], axis=1))[:, 3:3 + R.S4]
    frames = [_framed(s) for s in ((R.M4,), (R.M4, topk), (R.M4, topk))]
    got = _run(dga, q, wide_kv, wide_idx, lse, scale, wide_lg, index_offsets=raw(off), grad_scale=K.GRAD_SCALE, **{n: f[1] for n, f in zip(("loss", "d_logits", "target"), frames)})
    K.inside(got, ref)
    for whole, view in frames:
        edge = torch.cat([whole[:8], whole[8 + view.numel():]])
        assert (edge == NAN_FILL).all() and not (whole[8:8 + view.numel()] == NAN_FILL).any()


@pytest.mark.parametrize("h", (16, 128))
def test_it_takes_the_forwards_lse_and_feeds_the_indexer_backward(dga, h):
    """sparse_mla_fwd's lse in, fp8_mqa_logits' logits in, d_logits out into fp8_mqa_logits_bwd beside the same indices.  The kernel is
    given lse + el with |el| <= the forward's bound_lse, so p' = p e^-el: p's relative bound grows by w = expm1(bound_lse)
    (indexer_kl_ref.reference(lse_err=)); the indexer's backward is held to its own bounds for the d_logits it was given"""
    q, kv, idx = R.random_case(h)
    gen = torch.Generator(device="cpu").manual_seed(h)

    def quantised(*shape):
        x = torch.randn(shape, generator=gen)
        s = x.abs().amax(-1, keepdim=True) / 448.0
        return (x / s).to(torch.float8_e4m3fn).view(torch.uint8).numpy(), s.squeeze(-1).numpy()

    (q8, qs), (k8, ks) = quantised(R.M4, 32, B.D), quantised(R.S4, B.D)
    w = torch.randn((R.M4, 32), generator=gen).numpy() * qs
    tq, tkv, tidx, ind = _bf16(q), _bf16(kv), raw(idx), (raw(q8), (raw(k8), raw(ks)), raw(w))
    lse = dga.sparse_mla_fwd(tq, tkv, tidx, R.SCALE4)[1]
    span = torch.zeros(R.M4, dtype=torch.int32, device="cuda"), torch.full((R.M4,), R.S4, dtype=torch.int32, device="cuda")
    logits = dga.fp8_mqa_logits(*ind, *span)
    loss, dl = dga.indexer_kl_loss(tq, tkv, tidx, lse, R.SCALE4, logits, grad_scale=K.GRAD_SCALE)
    grads = dga.fp8_mqa_logits_bwd(*ind, tidx, dl, sync=True)
    fwd = R.reference(q, kv, idx, R.SCALE4)
    K.inside((loss.cpu().numpy(), dl.cpu().numpy(), None), K.reference(q, kv, idx, fwd["lse"], R.SCALE4, logits.cpu().numpy(), grad_scale=K.GRAD_SCALE,
                                                                     lse_err=R.bound_lse(fwd, R.SCALE4, R.TOPK4)))
    ref = B.reference(q8, k8, ks, w, idx, dl.cpu().numpy())
    for got, want, bar in zip(grads, ("dq", "dk", "dw"), (ref["err_dq"], B.bound_dk(ref, 32), ref["err_dw"])):
        assert (np.abs(got.cpu().numpy() - ref[want]) <= bar).all(), want


def test_reproducibility_and_graph_replay(dga):
    """two runs give the same bytes of all three outputs; a captured graph replayed after indices, logits, lse and q were overwritten in
    place gives the eager bytes for them, twice over"""
    a, b = K.random_case(128, 320)[0], K.random_case(128, 33)[0]
    b = (b[0][::-1], b[1], np.concatenate([b[2], np.full((R.M4, 287), -1, np.int32)], axis=1)[::-1], b[3][::-1], b[4], b[5][::-1])    # (the tokens reversed)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(_run(dga, *a), _run(dga, *a)))
    tq, tkv, tidx, tlse, tlg = _bf16(a[0]), _bf16(a[1]), raw(a[2].copy()), raw(a[3].copy()), raw(a[5].copy())
    call = lambda: dga.indexer_kl_loss(tq, tkv, tidx, tlse, a[4], tlg, want_target=True)
    call()
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = call()
    for case in (b, a, b):
        tq.copy_(_bf16(np.ascontiguousarray(case[0]))), tidx.copy_(raw(np.ascontiguousarray(case[2]))), tlse.copy_(raw(np.ascontiguousarray(case[3]))), tlg.copy_(raw(np.ascontiguousarray(case[5])))
        want = [x.clone() for x in call()]
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o.view(torch.int32), x.view(torch.int32)) for o, x in zip(outs, want)) and want[1].abs().max() > 0
