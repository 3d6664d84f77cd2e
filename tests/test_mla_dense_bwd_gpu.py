"""GPU: mla_bwd_dense against sparse_mla_bwd_ref.reference (float64) on test_mla_dense_bwd.operands, the ranges written out as [M, N] lists:
5 tokens over 700 keys (21 full tiles and one of 28 rows), 3 .. 20 blocks of 32 flat rows in more than one chunk, token 3 empty.  out and
lse come from the float64 forward reference everywhere but in the chain test, so these tests do not hang on the forward kernel.  The
bounds are sparse_mla_bwd_ref's at N + 32 positions, with no added term (tests/test_mla_dense_bwd.py says why).
Measured on an MI355X, worst error / bound over all cases: see DESIGN.md, "Dense MLA attention, backward"."""
import numpy as np
import pytest
import torch

import mqa_logits_ref as Q
import sparse_mla_bwd_ref as B
import sparse_mla_ref as R
from sparse_mla_support import NAN_FILL16, _bf16
from test_indexer_kl_dense import KINDS, M, N, bound_lse, dense_case
from test_indexer_kl_dense_gpu import raw
from test_mla_dense_bwd import expected, operands

pytestmark = pytest.mark.gpu


def _run(dga, q, kv, ks, ke, out, lse, d_out, **kw):
    """the operator on host arrays (tensors pass through): (dq float64, dq bits, dkv float32) on the host"""
    dev = lambda x: x if isinstance(x, torch.Tensor) else _bf16(x)
    dq, dkv = dga.mla_bwd_dense(dev(q), dev(kv), dev(out), dev(d_out), raw(ks), raw(ke), raw(lse), R.SCALE4, sync=True, **kw)
    return dq.float().cpu().numpy().astype(np.float64), dq.view(torch.int16).cpu().numpy().view(np.uint16), dkv.cpu().numpy()


def _inside(dq, dkv, ref, h, prior=0.0):
    """every element of dq and of dkv[:, :576] inside its bound; the worst error / bound of each"""
    assert np.isfinite(dq).all() and np.isfinite(dkv).all()
    worst = []
    for err, bar in ((np.abs(dq - ref["dq"]), B.bound_dq(ref, N + 32)), (np.abs(dkv.astype(np.float64) - prior - ref["dkv"]), B.bound_dkv(ref, h, prior))):
        worst.append(float((err / np.maximum(bar, 1e-300)).max()))
        assert (err <= bar).all(), (int((err > bar).sum()), np.argwhere(err > bar)[:4], worst)
    print("worst error / bound: dq %.3f dkv %.3f" % tuple(worst))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h", R.ALL_HEADS)
def test_bounds(dga, h, kind):
    dq, bits, dkv = _run(dga, *operands(h, kind)[0])
    _inside(dq, dkv, expected(h, kind), h)
    assert not bits[3].any() and bits[0].any()


def test_layouts_nan_and_untouched_bytes(dga):
    """kv a [S, 1, 576] view of rows 640 apart, NaN between the rows and in every row outside the call's span [5, 277); dkv rows 640 apart
    over a finite pattern; dq inside a NaN-framed allocation: inside the bounds, rows no range names and all padding keep their bytes,
    every element of dq written, not a byte outside it changed"""
    h, pad = 48, 64
    (q, kv, ks, ke, out, lse, d_out), _ = operands(h, "windows")
    ref = expected(h, "windows")
    wide = np.concatenate([kv, np.full((N, pad), np.nan, np.float32)], axis=1)
    wide[:5], wide[277:] = np.nan, np.nan
    prior = ((np.arange(N * (R.D_QK + pad)) % 251 - 125) * 0.25).astype(np.float32).reshape(N, -1)
    dkv = torch.from_numpy(prior.copy()).cuda()[:, :R.D_QK]
    whole = torch.full((M * h * R.D_QK + 16,), NAN_FILL16, dtype=torch.int16, device="cuda")
    dq, _, got = _run(dga, q, _bf16(wide)[:, None, :R.D_QK], ks, ke, out, lse, d_out, dkv=dkv, dq=whole[8:-8].view(M, h, R.D_QK).view(torch.bfloat16))
    _inside(dq, got, ref, h, prior[:, :R.D_QK].astype(np.float64))
    full = dkv.as_strided((N, R.D_QK + pad), (R.D_QK + pad, 1)).cpu().numpy().view(np.uint32)
    assert (ref["count"] == 0).any() and np.array_equal(full[ref["count"] == 0], prior.view(np.uint32)[ref["count"] == 0])
    assert np.array_equal(full[:, R.D_QK:], prior.view(np.uint32)[:, R.D_QK:])
    assert (whole[:8] == NAN_FILL16).all() and (whole[-8:] == NAN_FILL16).all() and not (whole[8:-8] == NAN_FILL16).any()


def test_reproducibility_and_graph_replay(dga):
    """two calls give the same bytes of dq and of dkv; one captured graph replayed after the ranges, q, d_out, out and lse were overwritten
    in place (dkv zeroed outside the graph: the operator adds into it) gives the eager bytes of both, three times over"""
    a, b = operands(128, "windows")[0], operands(128, "shifted")[0]
    first, again = _run(dga, *a), _run(dga, *a)
    assert np.array_equal(first[1], again[1]) and np.array_equal(first[2].view(np.uint32), again[2].view(np.uint32)) and first[2].any()
    ts = [_bf16(a[0]), _bf16(a[1]), raw(a[2].copy()), raw(a[3].copy()), _bf16(a[4]), raw(a[5].copy()), _bf16(a[6])]
    dkv = torch.zeros((N, R.D_QK), dtype=torch.float32, device="cuda")
    call = lambda: dga.mla_bwd_dense(ts[0], ts[1], ts[4], ts[6], ts[2], ts[3], ts[5], R.SCALE4, dkv=dkv)[0]
    call()
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            dq = call()
    for case in (b, a, b):
        for t, x in zip(ts, case):
            t.copy_(_bf16(x) if t.dtype == torch.bfloat16 else raw(x))
        dkv.zero_()
        want_dq, want_dkv = call().clone(), dkv.clone()
        dkv.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dq.view(torch.int16), want_dq.view(torch.int16)) and torch.equal(dkv.view(torch.int32), want_dkv.view(torch.int32))
        assert want_dq.float().abs().max() > 0 and want_dkv.abs().max() > 0


def test_forward_feeds_backward(dga):
    """h = 64, shifted: mla_fwd_dense's out and lse feed mla_bwd_dense, against float64 autograd of the masked definition inside the bounds
    widened for an out and an lse that lie within the forward's bounds of the exact ones (sparse_mla_bwd_ref.reference(out_err=, lse_err=),
    derived at test_sparse_mla_bwd_gpu.test_forward_feeds_backward_and_a_graph_replays_both)"""
    h = 64
    (q, kv, ks, ke, _, _, d_out), idx = operands(h, "shifted")
    fwd = dense_case(h, "shifted")[2]
    tq, tkv, tdo, tks, tke = _bf16(q), _bf16(kv), _bf16(d_out), raw(ks), raw(ke)
    out, lse = dga.mla_fwd_dense(tq, tkv, tks, tke, R.SCALE4)
    dq, _, dkv = _run(dga, tq, tkv, tks, tke, out, lse, tdo)
    ref = B.reference(q, kv, fwd["out"], d_out, idx, fwd["lse"], R.SCALE4, out_err=R.bound_out(fwd, R.SCALE4, N + 32), lse_err=bound_lse(fwd, R.SCALE4))
    mask = torch.from_numpy(Q.in_range(ks, ke, N))
    live = mask.any(1)                                                                   # (the empty token has no softmax; its gradients are 0)
    qt, kt = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (q, kv))
    s = R.SCALE4 * torch.einsum("thd,sd->ths", qt[live], kt) + torch.where(mask[live], 0.0, -np.inf)[:, None, :]
    (torch.einsum("ths,sc->thc", torch.softmax(s, 2), kt[:, :R.D_V]) * torch.tensor(d_out, dtype=torch.float64)[live]).sum().backward()
    ref["dq"], ref["dkv"] = qt.grad.numpy(), kt.grad.numpy()
    _inside(dq, dkv, ref, h)
