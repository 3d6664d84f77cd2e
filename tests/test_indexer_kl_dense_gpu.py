"""GPU: indexer_kl_loss_dense against tests/indexer_kl_ref.py and sparse_mla_ref.py on test_indexer_kl_dense.dense_case: 5 tokens (two full
runs and a ragged one) over 700 keys (21 tiles of 32 and a ragged one), the ranges written out as [M, N] lists for the references."""
import numpy as np
import pytest
import torch

import indexer_kl_ref as K
import mqa_logits_bwd_ref as B
import sparse_mla_ref as R
from sparse_mla_support import NAN_FILL, _bf16
from test_indexer_kl_dense import KINDS, M, N, bound_lse, dense_case, lists

pytestmark = pytest.mark.gpu
raw = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).cuda()
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def _run(dga, q, kv, ks, ke, logits, scale=R.SCALE4, **kw):
    """the operator on host arrays (tensors pass through): (loss, d_logits, target, lse) on the host"""
    dev = lambda x: x if isinstance(x, torch.Tensor) else _bf16(x)
    kw = {"want_target": True, "grad_scale": K.GRAD_SCALE, **{name: raw(x) if name == "lse" else x for name, x in kw.items()}}
    loss, dl, lse, t = dga.indexer_kl_loss_dense(dev(q), dev(kv), raw(ks), raw(ke), scale, raw(logits), sync=True, **kw)
    return tuple(x.cpu().numpy() for x in (loss, dl, t, lse))


def _computed(got, ops, idx, fwd, scale, empty=()):
    """the outputs of a call that computed lse: lse inside its derived bound of the float64 one (-inf on an empty token), the others inside
    the existing reference's bounds once lse is only known to that bound"""
    bar, keep = bound_lse(fwd, scale), fwd["count"] > 0
    err = np.abs(got[3][keep] - fwd["lse"][keep])
    print("lse: worst error / bound %.4f" % float((err / bar[keep]).max()))
    assert (err <= bar[keep]).all() and np.isneginf(got[3][~keep]).all() and list(np.flatnonzero(~keep)) == list(empty)
    K.inside(got[:3], K.reference(ops[0], ops[1], idx, fwd["lse"], scale, ops[4], grad_scale=K.GRAD_SCALE, lse_err=bar))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h", K.HEADS)
def test_bounds_with_a_given_lse(dga, h, kind):
    """every wave split; token 3 is empty with an lse of NaN, logits is NaN outside the ranges: +0 there, as bits"""
    ops, idx, fwd = dense_case(h, kind)
    lse = fwd["lse"].astype(np.float32)
    lse[3] = np.nan
    got = _run(dga, *ops, lse=lse)
    K.inside(got[:3], K.reference(ops[0], ops[1], idx, lse, R.SCALE4, ops[4], grad_scale=K.GRAD_SCALE))
    outside = idx < 0
    assert outside[3].all() and not bits(got[0])[3] and not bits(got[1])[outside].any() and not bits(got[2])[outside].any() and np.isnan(got[3][3]).all()


@pytest.mark.parametrize("kind", ("full", "windows"))
@pytest.mark.parametrize("h", (16, 64, 128))
def test_bounds_with_the_computed_lse(dga, h, kind):
    ops, idx, fwd = dense_case(h, kind)
    _computed(_run(dga, *ops), ops, idx, fwd, R.SCALE4, empty=(3,))


@pytest.mark.parametrize("h", R.PEAK_HEADS)
def test_peaked_scores(dga, h):
    """PEAK times the scale, logits over +-40, full ranges: the online maximum rises along the walk and the rescale matters"""
    scale = R.PEAK * R.SCALE4
    ops, idx, fwd = dense_case(h, "full", scale, True)
    assert R.score_spread(ops[0], ops[1], idx, scale) < R.SPREAD_MAX
    got = _run(dga, *ops, scale=scale)
    assert all(np.isfinite(g).all() for g in got)
    _computed(got, ops, idx, fwd, scale)


def _framed(rows, cols, pad=0):
    """a NaN-filled allocation, a float32 view [rows, cols] inside it whose rows are cols + pad apart, and where that view's elements lie"""
    whole = torch.full((rows * (cols + pad) + 16,), NAN_FILL, dtype=torch.int32, device="cuda")
    inside = torch.zeros(whole.shape, dtype=torch.bool, device="cuda")
    inside[8:-8].view(rows, cols + pad)[:, :cols] = True
    return whole, whole[8:-8].view(rows, cols + pad)[:, :cols].view(torch.float32), inside


def test_layouts_and_untouched_bytes(dga):
    """kv rows 640 apart with NaN between them, logits a column slice of a wider NaN buffer, the four outputs inside NaN-framed allocations,
    d_logits and target with stride(0) > N: inside the bounds, every element of the views written, not a byte outside them changed"""
    ops, idx, fwd = dense_case(48, "windows")
    q, kv, ks, ke, logits = ops
    wide_kv = _bf16(np.concatenate([kv, np.full((N, 64), np.nan, np.float32)], axis=1))[:, None, :R.D_QK]
    wide_lg = raw(np.concatenate([np.full((M, 3), np.nan, np.float32), logits, np.full((M, 6), np.nan, np.float32)], axis=1))[:, 3:3 + N]
    frames = dict(loss=_framed(1, M), d_logits=_framed(M, N, 12), target=_framed(M, N, 5), lse_out=_framed(M, 48))
    views = {name: f[1][0] if name == "loss" else f[1] for name, f in frames.items()}
    assert views["d_logits"].stride(0) > N
    _computed(_run(dga, q, wide_kv, ks, ke, wide_lg, **views), ops, idx, fwd, R.SCALE4, empty=(3,))
    for whole, _, inside in frames.values():
        assert (whole[~inside] == NAN_FILL).all() and not (whole[inside] == NAN_FILL).any()


def test_reproducibility_and_graph_replay(dga):
    """two calls give the same bytes of all four outputs; one captured graph (both launches) replayed after the ranges, q and logits were
    overwritten in place gives the eager bytes, three times over"""
    a, b = dense_case(128, "windows")[0], dense_case(128, "shifted")[0]
    b = (b[0][::-1], b[1], b[2], b[3], -0.5 * np.nan_to_num(b[4]))                        # (the tokens' q reversed, other logits)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(_run(dga, *a), _run(dga, *a)))
    tq, tkv, tks, tke, tlg = _bf16(a[0]), _bf16(a[1]), raw(a[2].copy()), raw(a[3].copy()), raw(a[4].copy())
    call = lambda: dga.indexer_kl_loss_dense(tq, tkv, tks, tke, R.SCALE4, tlg, want_target=True)
    call()
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = call()
    for case in (b, a, b):
        tq.copy_(_bf16(np.ascontiguousarray(case[0]))), tks.copy_(raw(case[2])), tke.copy_(raw(case[3])), tlg.copy_(raw(np.ascontiguousarray(case[4])))
        want = [x.clone() for x in call()]
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o.view(torch.int32), x.view(torch.int32)) for o, x in zip(outs, want)) and want[1].abs().max() > 0


def test_it_closes_the_dense_chain(dga):
    """fp8_mqa_logits -> indexer_kl_loss_dense -> fp8_mqa_logits_bwd_dense on one set of ranges: the loss inside its bounds for the logits
    it was given, the indexer's backward inside mqa_logits_bwd_ref's for the d_logits it was given"""
    h = 64
    (q, kv, ks, ke, _), idx, fwd = dense_case(h, "windows")
    gen = torch.Generator(device="cpu").manual_seed(h)

    def quantised(*shape):
        x = torch.randn(shape, generator=gen)
        s = x.abs().amax(-1, keepdim=True) / 448.0
        return (x / s).to(torch.float8_e4m3fn).view(torch.uint8).numpy(), s.squeeze(-1).numpy()

    (q8, qs), (k8, kscale) = quantised(M, 32, B.D), quantised(N, B.D)
    w = torch.randn((M, 32), generator=gen).numpy() * qs
    ind, span = (raw(q8), (raw(k8), raw(kscale)), raw(w)), (raw(ks), raw(ke))
    logits = dga.fp8_mqa_logits(*ind, *span)
    loss, dl, lse = dga.indexer_kl_loss_dense(_bf16(q), _bf16(kv), *span, R.SCALE4, logits, grad_scale=K.GRAD_SCALE)
    grads = dga.fp8_mqa_logits_bwd_dense(*ind, dl, *span, sync=True)
    lg, dl = logits.cpu().numpy(), dl.cpu().numpy()
    _computed((loss.cpu().numpy(), dl, None, lse.cpu().numpy()), (q, kv, ks, ke, lg), idx, fwd, R.SCALE4, empty=(3,))
    ref = B.reference(q8, k8, kscale, w, lists(ks, ke), dl)
    for got, want, bar in zip(grads, ("dq", "dk", "dw"), (ref["err_dq"], B.bound_dk(ref, 32), ref["err_dw"])):
        assert (np.abs(got.cpu().numpy() - ref[want]) <= bar).all(), want
