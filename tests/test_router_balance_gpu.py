"""GPU: router_balance_loss, router_balance_loss_backward and router_bias_update against tests/balance_ref.py.  B = 3 segments of L = 1, 37
or 50 tokens (at 50 a segment spans four stage-one chunks, the last of two tokens: asserted from the workspace query), every (E, k) of
router_ref.EK, both score functions, with and without normalisation, on router_topk's own scores and ids from bfloat16 logits and on
synthetic scores with arbitrary ids (-1 and E among them).  Every output is pre-filled with sentinels.  counts equal the host's exactly;
psum, loss and the backward lie under their bars against float64; two runs give the same bits; add_to (also as out itself) gives
fl32(add_to + aux) bit for bit; the 16-bit outputs are the RNE of the float32 one; a NaN poisons its own segment only; the bias update
matches numpy bit for bit."""
import numpy as np
import pytest
import torch

import balance_ref as B
import router_ref as R

pytestmark = pytest.mark.gpu

ALPHA = B.ALPHA


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _f32_sentinels(*shape):
    return torch.full(shape, R.SENTINEL_F32, dtype=torch.int32, device="cuda").view(torch.float32)


def _forward(dga, scores, ids, seq_len, normalize):
    """-> (loss, counts, psum) as numpy, from pre-filled outputs."""
    b_n, e = scores.shape[0] // seq_len, scores.shape[1]
    out = (_f32_sentinels(b_n), torch.full((b_n, e), R.SENTINEL_ID, dtype=torch.int32, device="cuda"), _f32_sentinels(b_n, e))
    got = dga.router_balance_loss(_dev(scores), _dev(ids), seq_len=seq_len, alpha=ALPHA, normalize=normalize, out=out, sync=True)
    assert all(g is o for g, o in zip(got, out))
    return tuple(t.cpu().numpy() for t in out)


def _case(dga, scores, ids, seq_len, func, normalize, where):
    """scores float32 [T, e], ids int32 [T, k] on the host -> every check of the forward and of the backward."""
    t_n, e = scores.shape
    k, b_n = ids.shape[1], t_n // seq_len
    loss, counts, psum = _forward(dga, scores, ids, seq_len, normalize)
    assert (loss.view(np.uint32) != R.SENTINEL_F32).all() and (psum.view(np.uint32) != R.SENTINEL_F32).all() and (counts >= 0).all(), where
    rl, rc, rp = B.forward_ref(scores, ids, seq_len, ALPHA, normalize)
    assert np.array_equal(counts, rc), where                                       # exact
    perr, pbar = np.abs(psum.astype(np.float64) - rp), B.psum_bar(seq_len, e) * rp
    lerr, lbar = np.abs(loss.astype(np.float64) - rl), B.loss_bar(seq_len, e) * rl
    worst_p, worst_l = float((perr / pbar).max()), float((lerr[rl > 0] / lbar[rl > 0]).max()) if (rl > 0).any() else 0.0
    print(f"{where} psum: worst error = {worst_p:.3f} of the bar; loss: {worst_l:.3f} of the bar")
    assert (perr <= pbar).all() and (lerr <= lbar).all(), (where, worst_p, worst_l)
    again = _forward(dga, scores, ids, seq_len, normalize)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again, (loss, counts, psum))), where   # the same bits twice

    # the backward, on the counts the device wrote
    rng = np.random.default_rng([13, e, k, seq_len])
    dloss = rng.standard_normal(b_n).astype(np.float32)
    args = dict(seq_len=seq_len, alpha=ALPHA, normalize=normalize)
    d_dloss, d_counts, d_scores = _dev(dloss), _dev(counts), _dev(scores)
    out = _f32_sentinels(t_n, e)
    got = dga.router_balance_loss_backward(d_dloss, d_counts, d_scores, k, func, out=out, sync=True, **args)
    assert got is out
    aux = out.cpu().numpy()
    assert (aux.view(np.uint32) != R.SENTINEL_F32).all(), where
    ref, m = B.backward_ref(dloss, counts, scores, k, func, seq_len, ALPHA, normalize)
    err, bar = np.abs(aux.astype(np.float64) - ref), B.backward_bar(e) * m
    worst = float((err[m > 0] / bar[m > 0]).max()) if (m > 0).any() else 0.0
    print(f"{where} backward: worst error = {worst:.3f} of the bar")
    assert (err <= bar).all(), (where, worst)
    again = dga.router_balance_loss_backward(d_dloss, d_counts, d_scores, k, func, sync=True, **args).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), aux.view(np.uint32)), where      # two runs, the same bits
    # add_to: fl32(add_to + aux), into another tensor and into add_to itself
    add = rng.standard_normal((t_n, e)).astype(np.float32) * np.float32(np.abs(aux).max() + 1e-3)
    want = np.add(add, aux, dtype=np.float32).view(np.uint32)
    summed = dga.router_balance_loss_backward(d_dloss, d_counts, d_scores, k, func, add_to=_dev(add), sync=True, **args).cpu().numpy()
    assert np.array_equal(summed.view(np.uint32), want), where
    buf = _dev(add)
    assert dga.router_balance_loss_backward(d_dloss, d_counts, d_scores, k, func, add_to=buf, out=buf, sync=True, **args) is buf
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), want), where
    for dtype in ("bf16", "fp16"):
        o16 = torch.full((t_n, e), 0x7FC1, dtype=torch.int16, device="cuda").view(R.TORCH_DT[dtype])
        dga.router_balance_loss_backward(d_dloss, d_counts, d_scores, k, func, out=o16, sync=True, **args)
        assert np.array_equal(o16.view(torch.int16).cpu().numpy().view(np.uint16), R.round_to(aux, dtype)), (where, dtype)


def test_the_longest_case_spans_three_chunks_with_a_ragged_last_one(dga):
    seq_len = max(B.SEQ_LENS)
    t_n = B.SEGMENTS * seq_len
    for e, _ in R.EK:
        chunks, rest = divmod(dga.router_balance_loss_workspace_bytes(t_n, e, seq_len), 8 * B.SEGMENTS * e)
        assert rest == 0 and chunks >= 3 and chunks == -(-seq_len // B.chunk_tokens(t_n)) and seq_len % B.chunk_tokens(t_n) != 0


@pytest.mark.parametrize("normalize", (True, False), ids=("normalize", "plain"))
@pytest.mark.parametrize("func", R.FUNCS)
@pytest.mark.parametrize("seq_len", B.SEQ_LENS)
@pytest.mark.parametrize("e,k", R.EK)
def test_on_router_topk_outputs(dga, e, k, seq_len, func, normalize):
    x = B.logits_case(e, seq_len)
    ids, _, scores = dga.router_topk(_dev(x).to(torch.bfloat16), k, score_func=func, bias=_dev(R.tie_bias(e)), sync=True)
    _case(dga, scores.cpu().numpy(), ids.cpu().numpy(), seq_len, func, normalize, f"[{e},{k},L={seq_len},{func},{normalize}]")


@pytest.mark.parametrize("normalize", (True, False), ids=("normalize", "plain"))
@pytest.mark.parametrize("func", R.FUNCS)
@pytest.mark.parametrize("seq_len", B.SEQ_LENS)
@pytest.mark.parametrize("e,k", R.EK)
def test_on_synthetic_scores_and_arbitrary_ids(dga, e, k, seq_len, func, normalize):
    scores, ids = B.synthetic_case(e, k, seq_len)
    _case(dga, scores, ids, seq_len, func, normalize, f"[{e},{k},L={seq_len},{func},{normalize}] synthetic")


@pytest.mark.parametrize("e,k", [(60, 6), (160, 8)])
def test_more_chunks_than_stage_two_has_slices(dga, e, k):
    """L = 643: 41 chunks of 16 tokens, the last of three; stage two adds them in 16 runs (E = 60) or in 5 with idle threads (E = 160)."""
    seq_len = 643
    assert dga.router_balance_loss_workspace_bytes(B.SEGMENTS * seq_len, e, seq_len) == 8 * B.SEGMENTS * 41 * e
    scores, ids = B.synthetic_case(e, k, seq_len)
    _case(dga, scores, ids, seq_len, "sigmoid", True, f"[{e},{k},L={seq_len}] synthetic")


@pytest.mark.parametrize("normalize", (True, False), ids=("normalize", "plain"))
@pytest.mark.parametrize("e,k", [(60, 6), (256, 8)])
def test_a_nan_row_poisons_only_its_own_segment(dga, e, k, normalize):
    seq_len = 37
    scores, ids = B.synthetic_case(e, k, seq_len)
    clean = _forward(dga, scores, ids, seq_len, normalize)
    scores[seq_len + 20, e // 2] = np.nan                                       # a token of segment 1
    loss, counts, psum = _forward(dga, scores, ids, seq_len, normalize)
    assert np.isnan(loss[1]) and np.isnan(psum[1, e // 2]) and np.isnan(psum[1]).all() == normalize
    assert np.array_equal(counts, clean[1])
    for b in (0, 2):
        assert loss.view(np.uint32)[b] == clean[0].view(np.uint32)[b] and np.array_equal(psum.view(np.uint32)[b], clean[2].view(np.uint32)[b])
    if not normalize:
        keep = np.arange(e) != e // 2
        assert np.array_equal(psum.view(np.uint32)[1, keep], clean[2].view(np.uint32)[1, keep])


@pytest.mark.parametrize("e", [4, 60, 1024])
def test_the_bias_update_bit_for_bit(dga, e):
    rng = np.random.default_rng([17, e])
    d = rng.integers(1, 7, size=e // 2)
    d[0] = 0                                                                    # experts 0 and 1 sit exactly at the mean, 12: sgn = 0
    n = 12 + np.stack([d, -d], axis=1).reshape(-1)                              # the others in pairs 12 + d, 12 - d
    counts = np.stack([n // 3, n // 3, n - 2 * (n // 3)]).astype(np.int32)
    sgn = np.sign(n.sum() - e * n)
    assert n.sum() == 12 * e and set(sgn.tolist()) == {-1, 0, 1} and sgn[0] == 0 and sgn[1] == 0
    bias = (rng.standard_normal(e) * 0.1).astype(np.float32)
    bias[1] = -0.0                                                              # (-0) + (+0) is +0 on both sides
    for rate in (0.001, 0.125):
        want = B.bias_update_ref(bias, counts, rate)
        d_bias = _dev(bias)
        assert dga.router_bias_update(d_bias, _dev(counts), rate, sync=True) is d_bias
        got = d_bias.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (got[:2] == bias[:2]).all() and (got[2::2] < bias[2::2]).all() and (got[3::2] > bias[3::2]).all()
