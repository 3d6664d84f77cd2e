"""GPU: router_topk and router_topk_backward against tests/router_ref.py.  T = 37 tokens (no multiple of the 4 a workgroup takes), every
output pre-filled with sentinels.  Forward, on every case: the scores lie under their bar against float64; ids and weights equal the numpy
float32 reference on the device's own scores bit for bit; ids are distinct and in range; every element is written.  The inputs make ties
(router_ref.tie_logits).  On continuous logits the ids, as sets, are torch.topk's of the float64 scores.  Backward: under its bar against
float64 on the same scores, +0 off the selection for sigmoid, the same bits twice, the 16-bit output the RNE of the float32 one."""
import numpy as np
import pytest
import torch

import router_ref as R

pytestmark = pytest.mark.gpu

T = R.T


def _outputs(e, k):
    return (torch.full((T, k), R.SENTINEL_ID, dtype=torch.int32, device="cuda"),
            torch.full((T, k), R.SENTINEL_F32, dtype=torch.int32, device="cuda").view(torch.float32),
            torch.full((T, e), R.SENTINEL_F32, dtype=torch.int32, device="cuda").view(torch.float32))


def _run(dga, x, dtype, k, func, bias, n_groups, topk_groups, renormalize, scale):
    """-> (ids, weights, scores) as numpy, from pre-filled outputs."""
    e = x.shape[1]
    out = _outputs(e, k)
    got = dga.router_topk(torch.from_numpy(x).to(R.TORCH_DT[dtype]).cuda(), k, score_func=func,
                          bias=torch.from_numpy(bias).cuda() if bias is not None else None, n_groups=n_groups, topk_groups=topk_groups,
                          renormalize=renormalize, scale=scale, out=out, sync=True)
    assert all(g is o for g, o in zip(got, out))
    return tuple(t.cpu().numpy() for t in out)


def _check_forward(x, k, func, bias, n_groups, topk_groups, renormalize, scale, ids, w, s, where=""):
    e = x.shape[1]
    clean = ~np.isnan(x).any(axis=1)
    # every element written
    assert (ids != R.SENTINEL_ID).all() and (w.view(np.uint32) != R.SENTINEL_F32).all() and (s.view(np.uint32) != R.SENTINEL_F32).all(), where
    # (1) the scores against float64, where the bar applies; finite and inside [0, 1] on every row without a NaN
    p64 = R.scores64(x, func)
    checked = R.score_checked(x, func) & clean[:, None]
    err = np.abs(s.astype(np.float64) - p64)
    worst = float((err[checked] / p64[checked]).max() / R.score_bar(e, func))
    print(f"{where} scores: worst error = {worst:.3f} of the bar")
    assert (err[checked] <= R.score_bar(e, func) * p64[checked]).all(), (where, worst)
    assert np.isfinite(s[clean]).all() and (s[clean] >= 0).all() and (s[clean] <= 1).all()
    assert not s[clean][np.isneginf(x[clean])].any()                      # exp(-inf) and sigmoid(-inf) are +0
    # (2) ids and weights from the device's own scores, bit for bit; the row with a NaN: the ids contract only
    rid, rw = R.select_ref(s, k, bias, n_groups, topk_groups, renormalize, scale)
    assert np.array_equal(ids, rid), (where, np.nonzero((ids != rid).any(axis=1))[0])
    assert np.array_equal(w[clean].view(np.uint32), rw[clean].view(np.uint32)), where
    assert ((ids >= 0) & (ids < e)).all() and all(len(set(row)) == k for row in ids.tolist()), where
    assert np.isfinite(w[clean]).all()
    if bias is None and n_groups == 1:
        assert ids[R.ROW_ZEROS].tolist() == list(range(k))
        if func == "softmax":                                              # an all-NaN row of scores: every sel is -inf
            assert ids[R.ROW_NAN].tolist() == list(range(k))
        if k >= 2:
            assert ids[R.ROW_TWO_MAXIMA, :2].tolist() == [e // 3, e - 1]


@pytest.mark.parametrize("with_bias", (False, True), ids=("nobias", "bias"))
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("func", R.FUNCS)
@pytest.mark.parametrize("e,k", R.EK)
def test_forward_on_inputs_full_of_ties(dga, e, k, func, dtype, with_bias):
    x = R.tie_logits(e, k, dtype)
    bias = R.tie_bias(e) if with_bias else None
    for renormalize in (True, False):
        for scale in (1.0, 2.5):
            ids, w, s = _run(dga, x, dtype, k, func, bias, 1, 1, renormalize, scale)
            _check_forward(x, k, func, bias, 1, 1, renormalize, scale, ids, w, s, f"[{e},{k},{func},{dtype},{renormalize},{scale}]")


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("func", R.FUNCS)
@pytest.mark.parametrize("e,k,n_groups,topk_groups", R.GROUPED + R.GROUPED_OTHER)
def test_forward_group_limited(dga, e, k, n_groups, topk_groups, func, dtype):
    x = R.tie_logits(e, k, dtype)
    gs = e // n_groups
    for bias in (R.tie_bias(e), None):
        ids, w, s = _run(dga, x, dtype, k, func, bias, n_groups, topk_groups, True, 2.5)
        _check_forward(x, k, func, bias, n_groups, topk_groups, True, 2.5, ids, w, s, f"[{e},{k},{n_groups},{topk_groups},{func},{dtype}]")
        assert all(len(set(g // gs for g in row)) <= topk_groups for row in ids.tolist())
        if topk_groups * gs == k:                                          # the kept groups hold exactly k experts: all of them are chosen
            _, ok = R.selectable(s, bias, n_groups, topk_groups)
            assert all(sorted(row) == np.nonzero(ok[t])[0].tolist() for t, row in enumerate(ids.tolist()))


@pytest.mark.parametrize("with_bias", (False, True), ids=("nobias", "bias"))
@pytest.mark.parametrize("func", R.FUNCS)
@pytest.mark.parametrize("e,k,dtype", [(ek[0], ek[1], "fp32") for ek in R.EK] + [(256, 8, "bf16"), (60, 6, "fp16")])
def test_ids_are_torch_topk_of_the_float64_scores(dga, e, k, func, with_bias, dtype):
    """Independent of the numpy selection: on continuous logits the chosen set is torch.topk's on float64.  The seed is chosen (by the
    reference alone) so that every row separates its k-th from its (k+1)-th value by more than the scores' bar allows to close."""
    x, bias, want = R.continuous_case(e, k, func, with_bias, dtype)
    assert R.margin_ok(x, bias, k, func).all()                            # on the host: no row is left out
    ids, w, s = _run(dga, x, dtype, k, func, bias, 1, 1, True, 1.0)
    assert np.array_equal(np.sort(ids, axis=1), want)
    sel = s + bias[None, :] if with_bias else s
    picked = np.take_along_axis(sel, ids.astype(np.int64), axis=1)
    assert (np.diff(picked, axis=1) <= 0).all()                           # descending
    assert np.allclose(w.sum(axis=1), 1.0, atol=1e-5)


def _backward_case(dga, scores, ids, func, renormalize, scale, seed, where):
    """scores float32 [T, e], ids int32 [T, k] on the host -> the checks of the backward."""
    e, k = scores.shape[1], ids.shape[1]
    dw = np.random.default_rng([seed, e, k]).standard_normal((T, k)).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).cuda()
    out = torch.full((T, e), R.SENTINEL_F32, dtype=torch.int32, device="cuda").view(torch.float32)
    got = dga.router_topk_backward(dev(dw), dev(scores), dev(ids), func, renormalize=renormalize, scale=scale, out=out, sync=True)
    assert got is out
    d = out.cpu().numpy()
    assert (d.view(np.uint32) != R.SENTINEL_F32).all()
    ref, m = R.backward_ref(dw, scores, ids, func, renormalize, scale)
    err, bar = np.abs(d.astype(np.float64) - ref), R.backward_bar(e, k) * m
    worst = float((err[m > 0] / bar[m > 0]).max())
    print(f"{where} backward: worst error = {worst:.3f} of the bar")
    assert (err <= bar).all(), (where, worst)
    if func == "sigmoid":
        off = np.ones((T, e), bool)
        off[np.arange(T)[:, None], ids] = False
        assert not d.view(np.uint32)[off].any()                           # exactly +0 off the selection
        if not (renormalize and k == 1):                                      # (one renormalised weight is the constant `scale`)
            assert d[~off].all()
    again = dga.router_topk_backward(dev(dw), dev(scores), dev(ids), func, renormalize=renormalize, scale=scale, sync=True).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), d.view(np.uint32))       # two runs, the same bits
    for dtype in ("bf16", "fp16"):
        o16 = torch.full((T, e), 0x7FC1, dtype=torch.int16, device="cuda").view(R.TORCH_DT[dtype])
        dga.router_topk_backward(dev(dw), dev(scores), dev(ids), func, renormalize=renormalize, scale=scale, out=o16, sync=True)
        assert np.array_equal(o16.view(torch.int16).cpu().numpy().view(np.uint16), R.round_to(d, dtype)), (where, dtype)


@pytest.mark.parametrize("renormalize", (True, False), ids=("renorm", "plain"))
@pytest.mark.parametrize("func", R.FUNCS)
@pytest.mark.parametrize("e,k", R.EK)
def test_backward_on_the_forwards_outputs(dga, e, k, func, renormalize):
    x = R.to_dtype(np.random.default_rng([5, e, k]).standard_normal((T, e)) * 2.0, "bf16")
    ids, w, s = _run(dga, x, "bf16", k, func, R.tie_bias(e), 1, 1, renormalize, 2.5)
    _backward_case(dga, s, ids, func, renormalize, 2.5, 11, f"[{e},{k},{func},{renormalize}]")


@pytest.mark.parametrize("renormalize", (True, False), ids=("renorm", "plain"))
@pytest.mark.parametrize("func", R.FUNCS)
@pytest.mark.parametrize("e,k", [(8, 8), (60, 6), (160, 8), (384, 8), (1024, 64)])
def test_backward_on_synthetic_scores_and_arbitrary_ids(dga, e, k, func, renormalize):
    rng = np.random.default_rng([6, e, k])
    scores = (rng.random((T, e)) * 0.98 + 0.01).astype(np.float32)
    ids = np.stack([rng.permutation(e)[:k] for _ in range(T)]).astype(np.int32)       # distinct, in no order
    _backward_case(dga, scores, ids, func, renormalize, 1.0, 12, f"[{e},{k},{func},{renormalize}] synthetic")
