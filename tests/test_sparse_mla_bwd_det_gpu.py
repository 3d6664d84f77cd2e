"""GPU: sparse_mla_bwd(deterministic=True) against tests/sparse_mla_bwd_ref.py, on the cases and with the helpers of
test_sparse_mla_bwd_gpu.py (its bounds unchanged), and byte for byte where the atomic path could not promise bytes."""
import numpy as np
import pytest
import torch

import sparse_mla_bwd_ref as B
import sparse_mla_ref as R
from sparse_mla_support import _bf16
from test_sparse_mla_bwd_gpu import _autograd, _inside, _run

pytestmark = pytest.mark.gpu

DET = dict(deterministic=True)


@pytest.mark.parametrize("h", (16, 32, 48, 128))
def test_derived_bounds_and_the_atomic_paths_dq(dga, h):
    dq, bits, dkv = _run(dga, *B.operands(h), **DET)
    _inside(dq, dkv, B.expected(h), R.TOPK4, h)
    assert np.array_equal(bits, _run(dga, *B.operands(h))[1])


@pytest.mark.parametrize("layout", ("plain", "wide"))
@pytest.mark.parametrize("topk", (1, 33, 100))
def test_ragged_lists_and_layouts(dga, topk, layout):
    """test_sparse_mla_bwd_gpu's case: wide = kv and dkv rows 640 apart with NaN between kv rows, indices a slice, offsets given; a finite
    prior in dkv; token 3 all -1.  Rows nobody names and the padding keep their bits."""
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
    dq, bits, got = _run(dga, q, kv, idx, out, lse, d_out, scale, dkv=dkv, **kw, **DET)
    ref = B.expected(h, topk)
    _inside(dq, got, ref, topk, h, prior[:, :R.D_QK].astype(np.float64))
    full = dkv.as_strided((s, R.D_QK + pad), (R.D_QK + pad, 1)).cpu().numpy().view(np.uint32)
    assert np.array_equal(full[ref["count"] == 0], prior.view(np.uint32)[ref["count"] == 0]) and np.array_equal(full[:, R.D_QK:], prior.view(np.uint32)[:, R.D_QK:])
    assert (ref["count"] > 0).any() and not bits[3].any() and bits[0].any()


def test_the_same_bytes_where_the_atomics_gave_other_bytes(dga):
    """M = 32, S = 96, Hq = 16, topk = 130: random rows with duplicates, some -1, the first 64 positions of every token naming row 5 (a
    segment of 2048 in one chunk, dozens elsewhere), onto a nonzero prior.  One chunk and seven (the last ragged): each inside the bounds,
    each the same bytes from two calls."""
    m, s, h, topk = 32, 96, 16, 130
    g = torch.Generator(device="cpu").manual_seed(7)
    q = torch.randn((m, h, R.D_QK), generator=g).to(torch.bfloat16).float().numpy()
    kv = torch.randn((s, R.D_QK), generator=g).to(torch.bfloat16).float().numpy()
    d_out = torch.randn((m, h, R.D_V), generator=g).to(torch.bfloat16).float().numpy()
    rng = np.random.default_rng(7)
    idx = rng.integers(0, s, size=(m, topk)).astype(np.int32)
    idx[rng.random((m, topk)) < 0.05] = -1
    idx[:, :64] = 5
    fwd = R.reference(q, kv, idx, R.SCALE4)
    out, lse = R.bf16_round(fwd["out"].astype(np.float32)).astype(np.float32), fwd["lse"].astype(np.float32)
    ref = B.reference(q, kv, out, d_out, idx, lse, R.SCALE4)
    assert ref["count"][5] >= 2048 and 12 <= np.median(ref["count"]) <= 100
    prior = ((np.arange(s * R.D_QK) % 241 - 120) * 0.125).astype(np.float32).reshape(s, R.D_QK)
    for chunk in (None, 5):
        run = lambda: _run(dga, q, kv, idx, out, lse, d_out, R.SCALE4, dkv=torch.from_numpy(prior.copy()).cuda(), _chunk_tokens=chunk, **DET)
        (dq, bits, dkv), (_, again_bits, again) = run(), run()
        _inside(dq, dkv, ref, topk, h, prior.astype(np.float64))
        assert np.array_equal(dkv.view(np.uint32), again.view(np.uint32)) and np.array_equal(bits, again_bits)


@pytest.mark.parametrize("h", (16, 48, 128))
def test_every_head_finds_its_own_row_exactly(dga, h):
    """test_sparse_mla_bwd_gpu's exact case: dq all zero bits, dkv the integer sum of d_out over the winners of a row, bit for bit"""
    q, kv, idx, scale, win = R.winners_case(h)
    d_out = np.random.default_rng(h).integers(-4, 5, size=(R.WIN_M, h, R.D_V)).astype(np.float32)
    _, bits, dkv = _run(dga, q, kv, idx, kv[win][:, :, :R.D_V], np.full((R.WIN_M, h), 512.0), d_out, scale, **DET)
    want = np.zeros((R.WIN_S, R.D_QK), np.float32)
    np.add.at(want, win.ravel(), np.pad(d_out.reshape(-1, R.D_V), ((0, 0), (0, R.D_QK - R.D_V))))
    assert not bits.any()
    assert np.array_equal(dkv, want), np.argwhere(dkv != want)[:4]


def test_a_graph_replays_forward_and_backward_to_the_eager_bytes(dga):
    """h = 64: sparse_mla_fwd feeding the deterministic backward, captured once and replayed on new indices and d_out (dkv zeroed outside
    the graph): dq AND dkv the eager bytes, inside test_sparse_mla_bwd_gpu's end-to-end bounds against float64 autograd."""
    h = 64
    q, kv, idx, out, lse, d_out, scale = B.operands(h)
    cases = [(idx, d_out), (np.ascontiguousarray(idx[::-1]), -d_out[::-1] * 0.5)]
    tq, tkv, tidx, tdo = _bf16(q), _bf16(kv), torch.from_numpy(idx.copy()).cuda(), _bf16(d_out)
    dkv = torch.zeros((R.S4, R.D_QK), dtype=torch.float32, device="cuda")

    def both():
        o, l = dga.sparse_mla_fwd(tq, tkv, tidx, scale)
        return dga.sparse_mla_bwd(tq, tkv, o, tdo, tidx, l, scale, dkv=dkv, **DET)[0]

    both()                                                              # (the scratch of the eager stream exists before the capture)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            dq = both()
    for i, d in cases[::-1] + cases[:1]:
        tidx.copy_(torch.from_numpy(np.array(i))), tdo.copy_(_bf16(d)), dkv.zero_()
        want_dq, want_dkv = both().clone(), dkv.clone()
        dkv.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dq.view(torch.int16), want_dq.view(torch.int16)) and torch.equal(dkv.view(torch.int32), want_dkv.view(torch.int32))
        fwd = R.reference(q, kv, i, scale)
        ref = B.reference(q, kv, fwd["out"], d, i, fwd["lse"], scale, out_err=R.bound_out(fwd, scale, R.TOPK4), lse_err=R.bound_lse(fwd, scale, R.TOPK4))
        ref["dq"], ref["dkv"] = _autograd(q, kv, i, d, scale)
        _inside(dq.float().cpu().numpy().astype(np.float64), dkv.cpu().numpy(), ref, R.TOPK4, h)
