"""GPU: fp8_mqa_logits_bwd against tests/mqa_logits_bwd_ref.py, M = 5 tokens over N = 300 keys."""
import numpy as np
import pytest
import torch

import mqa_logits_bwd_ref as B
import mqa_logits_ref as Q
import sparse_mla_ref as R

pytestmark = pytest.mark.gpu
dev = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).cuda()


def _run(dga, q, k, ks, w, idx, dl, **kw):
    return tuple(x.cpu().numpy() for x in dga.fp8_mqa_logits_bwd(dev(q), (dev(k), dev(ks)), dev(w), dev(idx), dev(dl), sync=True, **{n: dev(v) for n, v in kw.items()}))


def _inside(got, ref, h, prior=0.0, dk_only=False):
    dq, dk, dw = got
    pairs = [("dk", np.abs(dk.astype(np.float64) - prior - ref["dk"]), B.bound_dk(ref, h, prior))]
    pairs += [] if dk_only else [("dq", np.abs(dq - ref["dq"]), ref["err_dq"]), ("d_weights", np.abs(dw - ref["dw"]), ref["err_dw"])]
    print("worst error / bound: " + " ".join("%s %.3f" % (name, float((err / np.maximum(bar, 1e-300)).max())) for name, err, bar in pairs))
    for name, err, bar in pairs:
        assert np.isfinite(err).all() and (err <= bar).all(), (name, int((err > bar).sum()), np.argwhere(err > bar)[:4])


@pytest.mark.parametrize("topk", (1, 63, 64, 65, 200))
@pytest.mark.parametrize("h", Q.HEADS)
def test_exactly_summable_operands_bit_for_bit(dga, h, topk):
    """every G is exact in bf16 and every sum exact in fp32 in any order: all three outputs equal the reference as values, dk's atomics
    notwithstanding; d_logits is NaN at every invalid position; token 3, whose list is all invalid, gets all-zero bits"""
    ops, ref = B.exact_case(h, topk)
    dq, dk, dw = _run(dga, *ops)
    for got, want in ((dq, ref["dq"]), (dk, ref["dk"]), (dw, ref["dw"])):
        assert np.array_equal(got.astype(np.float64), want), np.argwhere(got != want)[:4]
    assert not dq[3].view(np.uint32).any() and not dw[3].view(np.uint32).any() and np.abs(ref["dk"]).max() > 0


@pytest.mark.parametrize("h", Q.HEADS)
def test_derived_bounds_on_random_data(dga, h):
    """amax-quantised normal data, topk = 200: three full tiles and a ragged fourth"""
    ops, ref = B.random_case(h)
    _inside(_run(dga, *ops), ref, h)


def test_layouts_and_untouched_bytes(dga):
    """indices and d_logits slices of wider tensors (NaN beside d_logits), offsets given, dk rows 160 apart over a finite pattern: rows
    nobody names and the padding keep their bytes, named rows sit inside the bound with the prior counted"""
    h, (q, k, ks, w, idx, dl), ref = 32, *B.random_case(32)
    off = -np.arange(1, 6, dtype=np.int32)
    wide_idx = dev(np.concatenate([np.where(idx >= 0, idx - off[:, None], idx).astype(np.int32), np.full((B.M, 7), 3, np.int32)], axis=1))[:, :idx.shape[1]]
    wide_dl = dev(np.concatenate([dl, np.full((B.M, 9), np.nan, np.float32)], axis=1))[:, :idx.shape[1]]
    prior = ((np.arange(B.N * 160) % 251 - 125) * 0.25).astype(np.float32).reshape(B.N, 160)
    dk = dev(prior.copy())[:, :B.D]
    got = _run(dga, q, k, ks, w, wide_idx, wide_dl, index_offsets=off, dk=dk)
    _inside(got, ref, h, prior[:, :B.D].astype(np.float64))
    full = dk.as_strided((B.N, 160), (160, 1)).cpu().numpy().view(np.uint32)
    assert np.array_equal(full[ref["count"] == 0], prior.view(np.uint32)[ref["count"] == 0]) and np.array_equal(full[:, B.D:], prior.view(np.uint32)[:, B.D:])


@pytest.mark.parametrize("h", Q.HEADS)
def test_forward_and_backward_agree_on_the_scores(dga, h):
    """d_logits one-hot at a valid position j per token: sum_h weights d_weights = logits[m, r_j] of fp8_mqa_logits, within the forward's
    documented bound plus the reference's d_weights bound (times |weights|)"""
    q, k, ks, w, idx, _ = B.random_case(h)[0]
    rows, valid = R.rows_of(idx, B.N)
    tok = np.flatnonzero(valid.any(1))
    pos = np.array([np.flatnonzero(valid[t])[-1] for t in tok])
    dl = np.zeros(idx.shape, np.float32)
    dl[tok, pos] = 1.0
    ref = B.reference(q, k, ks, w, idx, dl)
    full = torch.zeros(B.M, dtype=torch.int32, device="cuda"), torch.full((B.M,), B.N, dtype=torch.int32, device="cuda")
    logits = dga.fp8_mqa_logits(dev(q), (dev(k), dev(ks)), dev(w), *full, sync=True).cpu().numpy().astype(np.float64)[tok, rows[tok, pos]]
    _, mag = Q.reference(q, k, ks, w, *(x.cpu().numpy() for x in full))
    tied = (w.astype(np.float64) * _run(dga, q, k, ks, w, idx, dl)[2]).sum(1)[tok]
    assert (np.abs(tied - logits) <= Q.bound(h) * mag[tok, rows[tok, pos]] + (np.abs(w) * ref["err_dw"]).sum(1)[tok]).all()
    assert np.abs(logits).min() > 0


def test_reproducibility_and_graph_replay(dga):
    """two runs give the same bytes of dq and d_weights; a captured graph replayed on new indices and d_logits gives the eager bytes of
    both, and a dk (cleared outside the graph: the operator adds into it) inside the bounds"""
    h, (q, k, ks, w, idx, dl), ref = 64, *B.random_case(64)
    a, b = _run(dga, q, k, ks, w, idx, dl), _run(dga, q, k, ks, w, idx, dl)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    tq, tk, tks, tw, tidx, tdl = (dev(x) for x in (q, k, ks, w, idx.copy(), dl.copy()))
    dk = torch.zeros((B.N, B.D), dtype=torch.float32, device="cuda")
    both = lambda: dga.fp8_mqa_logits_bwd(tq, (tk, tks), tw, tidx, tdl, dk=dk)
    both()
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = both()
    for i, d in ((np.ascontiguousarray(idx[::-1]), -0.5 * dl[::-1]), (idx, dl)):
        tidx.copy_(dev(i)), tdl.copy_(dev(np.ascontiguousarray(d)))
        want = [x.clone() for x in both()]
        dk.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(out[2].view(torch.int32), want[2].view(torch.int32))
        _inside((None, dk.cpu().numpy(), None), ref if i is idx else B.reference(q, k, ks, w, i, d), h, dk_only=True)
