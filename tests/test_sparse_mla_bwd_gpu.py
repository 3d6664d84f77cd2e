"""GPU: sparse_mla_bwd against tests/sparse_mla_bwd_ref.py.  out and lse are given from the float64 forward reference (out rounded to bf16,
lse to fp32) everywhere but in the end-to-end test, so that these tests do not hang on the forward kernel."""
import numpy as np
import pytest
import torch

import sparse_mla_bwd_ref as B
import sparse_mla_ref as R
from sparse_mla_support import _bf16

pytestmark = pytest.mark.gpu


def _run(dga, q, kv, idx, out, lse, d_out, scale, **kw):
    """the operator on host arrays (tensors pass through): (dq float64, dq bits, dkv float32) on the host"""
    dev = lambda x, make=_bf16: x if isinstance(x, torch.Tensor) else make(x)
    raw = lambda a: torch.from_numpy(np.array(a, dtype=np.float32 if a.dtype.kind == "f" else a.dtype)).cuda()
    dq, dkv = dga.sparse_mla_bwd(dev(q), dev(kv), dev(out), dev(d_out), dev(idx, raw), dev(lse, raw), scale, sync=True, **kw)
    return dq.float().cpu().numpy().astype(np.float64), dq.view(torch.int16).cpu().numpy().view(np.uint16), dkv.cpu().numpy()


def _inside(dq, dkv, ref, topk, h, prior=0.0):
    """every element of dq and of dkv[:, :576] inside its bound; the worst error / bound of each"""
    assert np.isfinite(dq).all() and np.isfinite(dkv).all()
    worst = []
    for err, bar in ((np.abs(dq - ref["dq"]), B.bound_dq(ref, topk)), (np.abs(dkv.astype(np.float64) - prior - ref["dkv"]), B.bound_dkv(ref, h, prior))):
        assert (err <= bar).all(), (int((err > bar).sum()), np.argwhere(err > bar)[:4])
        worst.append(float((err / np.maximum(bar, 1e-300)).max()))
    print("worst error / bound: dq %.3f dkv %.3f" % tuple(worst))


@pytest.mark.parametrize("h", (16, 32, 48, 128))
def test_derived_bounds_on_random_data(dga, h):
    """half a block of heads, one, a half-filled second, four; topk = 320 with invalid positions, an out-of-range row and a duplicate"""
    dq, _, dkv = _run(dga, *B.operands(h))
    _inside(dq, dkv, B.expected(h), R.TOPK4, h)


@pytest.mark.parametrize("layout", ("plain", "wide"))
@pytest.mark.parametrize("topk", (1, 33, 100))
def test_ragged_lists_and_layouts(dga, topk, layout):
    """wide: kv rows 640 apart with NaN between them, dkv rows 640 apart, indices a slice of a wider tensor, offsets given.  dkv starts as
    a finite pattern: rows nobody names and the padding keep their bytes; token 3, whose list is all -1, gets dq = +0."""
    h, pad = 48, 64 if layout == "wide" else 0
    q, kv, idx, out, lse, d_out, scale = B.operands(h, topk)
    s = kv.shape[0]
    prior = ((np.arange(s * (R.D_QK + pad)) % 251 - 125) * 0.25).astype(np.float32).reshape(s, -1)
    dkv, kw = torch.from_numpy(prior.copy()).cuda()[:, :R.D_QK], {}
    if pad:
        kv = _bf16(np.concatenate([kv, np.full((s, pad), np.nan, np.float32)], axis=1))[:, :R.D_QK]
        off = -np.arange(1, 6, dtype=np.int32)
        shifted = np.where(idx >= 0, idx - off[:, None], idx).astype(np.int32)
        idx = torch.from_numpy(np.concatenate([shifted, np.full((5, 7), 3, np.int32)], axis=1)).cuda()[:, :topk]
        kw = dict(index_offsets=torch.from_numpy(off).cuda())
    dq, bits, got = _run(dga, q, kv, idx, out, lse, d_out, scale, dkv=dkv, **kw)
    ref = B.expected(h, topk)
    _inside(dq, got, ref, topk, h, prior[:, :R.D_QK].astype(np.float64))
    full = dkv.as_strided((s, R.D_QK + pad), (R.D_QK + pad, 1)).cpu().numpy().view(np.uint32)
    assert np.array_equal(full[ref["count"] == 0], prior.view(np.uint32)[ref["count"] == 0]) and np.array_equal(full[:, R.D_QK:], prior.view(np.uint32)[:, R.D_QK:])
    assert (ref["count"] > 0).any() and not bits[3].any() and bits[0].any()


@pytest.mark.parametrize("h", (16, 48, 128))
def test_every_head_finds_its_own_row_exactly(dga, h):
    """p is exactly 1 on a head's winner and underflows to 0 elsewhere, out is the winner's row and dP = delta as exact integers: dq is
    all zero bits and dkv[r, :512] the integer sum of d_out over the (t, h) that win row r, bit for bit (exactly summable: the atomics'
    order cannot show); everything else of dkv is 0"""
    q, kv, idx, scale, win = R.winners_case(h)
    d_out = np.random.default_rng(h).integers(-4, 5, size=(R.WIN_M, h, R.D_V)).astype(np.float32)
    _, bits, dkv = _run(dga, q, kv, idx, kv[win][:, :, :R.D_V], np.full((R.WIN_M, h), 512.0), d_out, scale)
    want = np.zeros((R.WIN_S, R.D_QK), np.float32)
    np.add.at(want, win.ravel(), np.pad(d_out.reshape(-1, R.D_V), ((0, 0), (0, R.D_QK - R.D_V))))
    assert not bits.any()
    assert np.array_equal(dkv, want), np.argwhere(dkv != want)[:4]


def test_reproducibility_as_documented(dga):
    """dq: the same bytes from two runs.  dkv: the same bytes where every element has a single contribution -- 32 heads (one workgroup
    a token) and lists that name every row at most once over all tokens, onto zeros -- and a second call doubles it exactly."""
    ops = B.operands(48)
    assert np.array_equal(_run(dga, *ops)[1], _run(dga, *ops)[1])
    q, kv, _, out, lse, d_out, scale = B.operands(32)
    idx = np.random.default_rng(1).permutation(R.S4)[:R.M4 * 100].reshape(R.M4, 100).astype(np.int32)
    idx[2, 50] = -1
    dkv = torch.zeros((R.S4, R.D_QK), dtype=torch.float32, device="cuda")
    _, _, a = _run(dga, q, kv, idx, out, lse, d_out, scale, dkv=dkv)
    _, _, twice = _run(dga, q, kv, idx, out, lse, d_out, scale, dkv=dkv)
    _, _, b = _run(dga, q, kv, idx, out, lse, d_out, scale)
    assert a.any() and np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(twice, 2 * a)


def _autograd(q, kv, idx, d_out, scale):
    """float64 autograd of the dense masked definition: every row of kv weighted by how often the list names it"""
    rows, valid = R.rows_of(idx, kv.shape[0])
    count = torch.zeros((len(rows), kv.shape[0]), dtype=torch.float64)
    for t in range(len(rows)):
        count[t].index_add_(0, torch.from_numpy(rows[t][valid[t]]), torch.ones(int(valid[t].sum()), dtype=torch.float64))
    qt, kt = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (q, kv))
    p = torch.softmax(scale * torch.einsum("thd,sd->ths", qt, kt) + count.log()[:, None, :], dim=2)
    (torch.einsum("ths,sc->thc", p, kt[:, :R.D_V]) * torch.tensor(d_out, dtype=torch.float64)).sum().backward()
    return qt.grad.numpy(), kt.grad.numpy()


def test_forward_feeds_backward_and_a_graph_replays_both(dga):
    """h = 64: sparse_mla_fwd's out and lse feed sparse_mla_bwd, against float64 autograd.  The widening: the kernel is given out + eo and
    lse + el with |eo| <= bound_out and |el| <= bound_lse of the forward; then p' = p e^-el and delta' = delta + sum_c eo d_out, so dS
    moves by at most sm_scale p (w (|dP - delta| + e_delta) + e_delta) with w = expm1(bound_lse), e_delta = sum_c bound_out |d_out|, and
    p by w p; these enter err(dS) and the error of p in the bounds of case 1 (sparse_mla_bwd_ref.reference(out_err=, lse_err=)).
    The pair is then captured in a graph and replayed on new d_out and indices: dq the eager bytes, dkv inside the same bounds."""
    h = 64
    q, kv, idx, out, lse, d_out, scale = B.operands(h)
    cases = [(idx, d_out), (np.ascontiguousarray(idx[::-1]), -d_out[::-1] * 0.5)]
    tq, tkv, tidx, tdo = _bf16(q), _bf16(kv), torch.from_numpy(idx.copy()).cuda(), _bf16(d_out)
    dkv = torch.zeros((R.S4, R.D_QK), dtype=torch.float32, device="cuda")

    def both():
        o, l = dga.sparse_mla_fwd(tq, tkv, tidx, scale)
        return dga.sparse_mla_bwd(tq, tkv, o, tdo, tidx, l, scale, dkv=dkv)[0]

    def check(dq, i, d):
        fwd = R.reference(q, kv, i, scale)
        ref = B.reference(q, kv, fwd["out"], d, i, fwd["lse"], scale, out_err=R.bound_out(fwd, scale, R.TOPK4), lse_err=R.bound_lse(fwd, scale, R.TOPK4))
        ref["dq"], ref["dkv"] = _autograd(q, kv, i, d, scale)
        _inside(dq.float().cpu().numpy().astype(np.float64), dkv.cpu().numpy(), ref, R.TOPK4, h)

    eager = both()
    torch.cuda.synchronize()
    check(eager, *cases[0])
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            dq = both()
    for i, d in cases[::-1] + cases[:1]:                            # (dkv is cleared outside the graph: the operator adds into it)
        tidx.copy_(torch.from_numpy(np.array(i))), tdo.copy_(_bf16(d)), dkv.zero_()
        want = both().clone()
        dkv.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dq.view(torch.int16), want.view(torch.int16))
        check(dq, i, d)
