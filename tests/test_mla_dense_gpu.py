"""GPU: mla_fwd_dense against sparse_mla_ref.reference (float64) on test_indexer_kl_dense.dense_case, the ranges written out as [M, N]
lists: 5 tokens over 700 keys, 80 .. 640 flat rows -- at Hq = 16 four tokens share a workgroup and the second has one live wave, at 48
and 80 a workgroup straddles two tokens, `windows` leaves dead tiles between and around the ranges, `mixed` puts disjoint ranges in one
workgroup, token 3 is empty.  out is held to sparse_mla_ref.bound_out at N + 32 keys (an unaligned range of n keys meets at most
ceil(n / 32) + 1 tiles), lse to test_indexer_kl_dense.bound_lse.
Measured on an MI355X, worst error / bound over all cases: see DESIGN.md, "Dense MLA attention"."""
import numpy as np
import pytest
import torch

import sparse_mla_ref as R
from sparse_mla_support import NAN_FILL, NAN_FILL16, _bf16
from test_indexer_kl_dense import KINDS, M, N, bound_lse, dense_case
from test_indexer_kl_dense_gpu import _computed, _run as _run_loss, raw

pytestmark = pytest.mark.gpu


def _run(dga, q, kv, ks, ke, scale=R.SCALE4, **kw):
    """the operator on host arrays (tensors pass through): (out as float32, out's bits, lse) on the host"""
    dev = lambda x: x if isinstance(x, torch.Tensor) else _bf16(x)
    out, lse = dga.mla_fwd_dense(dev(q), dev(kv), raw(ks), raw(ke), scale, sync=True, **kw)
    return out.float().cpu().numpy(), out.view(torch.int16).cpu().numpy().view(np.uint16), lse.cpu().numpy()


def _inside(got, fwd, scale, empty=()):
    """every element of out and lse inside its bound of the float64 reference; an empty token +0 as bits and -inf"""
    out, obits, lse = got
    keep = fwd["count"] > 0
    assert list(np.flatnonzero(~keep)) == list(empty) and not obits[~keep].any() and np.isneginf(lse[~keep]).all()
    err, bar = np.abs(out - fwd["out"]), R.bound_out(fwd, scale, N + 32)
    lerr, lbar = np.abs(lse[keep] - fwd["lse"][keep]), bound_lse(fwd, scale)[keep]
    print("out: worst error / bound %.4f, lse: %.4f" % (float((err[keep] / bar[keep]).max()), float((lerr / lbar).max())))
    assert np.isfinite(out).all() and (err <= bar).all() and (lerr <= lbar).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h", R.ALL_HEADS)
def test_bounds(dga, h, kind):
    ops, _, fwd = dense_case(h, kind)
    _inside(_run(dga, *ops[:4]), fwd, R.SCALE4, empty=(3,))


@pytest.mark.parametrize("h", R.PEAK_HEADS)
def test_peaked_scores(dga, h):
    """PEAK times the scale over full ranges: the online maximum rises along the walk and the rescale matters"""
    scale = R.PEAK * R.SCALE4
    ops, idx, fwd = dense_case(h, "full", scale, True)
    assert R.score_spread(ops[0], ops[1], idx, scale) < R.SPREAD_MAX
    got = _run(dga, *ops[:4], scale=scale)
    assert np.isfinite(got[2]).all()
    _inside(got, fwd, scale)


def test_layouts_nan_and_untouched_bytes(dga):
    """kv a [S, 1, 576] view of rows 640 apart, NaN between the rows and in every row outside the call's span [5, 277); out= and lse= inside
    NaN-framed allocations: inside the bounds, every element of the views written, not a byte outside them changed"""
    h = 48
    (q, kv, ks, ke, _), _, fwd = dense_case(h, "windows")
    wide = np.concatenate([kv, np.full((N, 64), np.nan, np.float32)], axis=1)
    wide[:5], wide[277:] = np.nan, np.nan
    whole_o = torch.full((M * h * R.D_V + 16,), NAN_FILL16, dtype=torch.int16, device="cuda")
    whole_l = torch.full((M * h + 8,), NAN_FILL, dtype=torch.int32, device="cuda")
    out, lse = whole_o[8:-8].view(M, h, R.D_V).view(torch.bfloat16), whole_l[4:-4].view(M, h).view(torch.float32)
    _inside(_run(dga, q, _bf16(wide)[:, None, :R.D_QK], ks, ke, out=out, lse=lse), fwd, R.SCALE4, empty=(3,))
    for whole, pad, fill in ((whole_o, 8, NAN_FILL16), (whole_l, 4, NAN_FILL)):
        assert (whole[:pad] == fill).all() and (whole[-pad:] == fill).all() and not (whole[pad:-pad] == fill).any()


def test_reproducibility_and_graph_replay(dga):
    """two calls give the same bytes; one captured graph replayed after the ranges and q were overwritten in place gives the eager bytes,
    three times over"""
    a, b = dense_case(128, "windows")[0][:4], dense_case(128, "shifted")[0][:4]
    b = (b[0][::-1],) + b[1:]                                                              # (the tokens' q reversed)
    assert all(np.array_equal(x, y) for x, y in zip(_run(dga, *a)[1:], _run(dga, *a)[1:]))
    tq, tkv, tks, tke = _bf16(a[0]), _bf16(a[1]), raw(a[2].copy()), raw(a[3].copy())
    call = lambda: dga.mla_fwd_dense(tq, tkv, tks, tke, R.SCALE4)
    call()
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = call()
    for case in (b, a, b):
        tq.copy_(_bf16(np.ascontiguousarray(case[0]))), tks.copy_(raw(case[2])), tke.copy_(raw(case[3]))
        want = [x.clone() for x in call()]
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[0].view(torch.int16), want[0].view(torch.int16)) and torch.equal(outs[1].view(torch.int32), want[1].view(torch.int32))
        assert want[0].float().abs().max() > 0


@pytest.mark.parametrize("h", (16, 128))
def test_both_grid_orders_give_the_same_bytes(dga, h):
    ops = dense_case(h, "mixed")[0][:4]
    assert all(np.array_equal(x, y) for x, y in zip(_run(dga, *ops)[1:], _run(dga, *ops, _flags=1)[1:]))


def test_its_lse_feeds_the_dense_loss(dga):
    """mla_fwd_dense's lse given to indexer_kl_loss_dense(lse=...): the loss, d_logits and target inside indexer_kl_ref's bounds for an
    lse known to bound_lse"""
    ops, idx, fwd = dense_case(64, "shifted")
    lse = _run(dga, *ops[:4])[2]
    _computed(_run_loss(dga, *ops, lse=lse), ops, idx, fwd, R.SCALE4, empty=(3,))
