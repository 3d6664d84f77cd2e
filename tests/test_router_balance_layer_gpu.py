"""GPU: a router's whole training step at tests/test_router_layer_gpu.py's sizes (T = 96 tokens, k = 3 of E = 4 experts, sequences of
L = 32 tokens):
  router_topk(logits, k, "sigmoid", bias)                                              ids, weights, scores
  router_balance_loss(scores, ids, seq_len=L, normalize=True)                          loss [3], counts [3, E], psum
  router_topk_backward(dw, scores, ids)                                                dlogits of the layer's own loss
  router_balance_loss_backward(dloss, counts, scores, k, add_to=that)                  the step's whole dlogits
  router_bias_update(bias, counts, rate)                                               the bias the next step selects with
eagerly, then as one captured single-stream graph that is replayed after the logits are rewritten.  Every link is checked against the
references on what the run itself produced; the replay's counts differ from the first run's, and the bias moved."""
import numpy as np
import pytest
import torch

import balance_ref as B
import router_ref as R

pytestmark = pytest.mark.gpu

T, E, K, L = 96, 4, 3, 32
SEGMENTS, FUNC, SCALE, ALPHA, RATE = T // L, "sigmoid", 2.5, 0.01, 2.0 ** -6


def _buffers():
    f32 = lambda *s: torch.full(s, R.SENTINEL_F32, dtype=torch.int32, device="cuda").view(torch.float32)
    ints = lambda *s: torch.full(s, R.SENTINEL_ID, dtype=torch.int32, device="cuda")
    return {"ids": ints(T, K), "w": f32(T, K), "scores": f32(T, E), "loss": f32(SEGMENTS), "counts": ints(SEGMENTS, E), "psum": f32(SEGMENTS, E),
            "dl_topk": f32(T, E), "dlogits": f32(T, E)}


def _step(dga, logits, bias, dw, dloss, b):
    dga.router_topk(logits, K, score_func=FUNC, bias=bias, scale=SCALE, out=(b["ids"], b["w"], b["scores"]))
    dga.router_balance_loss(b["scores"], b["ids"], seq_len=L, alpha=ALPHA, normalize=True, out=(b["loss"], b["counts"], b["psum"]))
    dga.router_topk_backward(dw, b["scores"], b["ids"], FUNC, scale=SCALE, out=b["dl_topk"])
    dga.router_balance_loss_backward(dloss, b["counts"], b["scores"], K, FUNC, seq_len=L, alpha=ALPHA, normalize=True, add_to=b["dl_topk"],
                                     out=b["dlogits"])
    dga.router_bias_update(bias, b["counts"], RATE)


def _logits(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, E, generator=g) * 2.0
    x[:, 1] += 1.5                                                            # expert 1 is loaded above the mean: its bias goes down
    return x.to(torch.bfloat16).cuda()


def _check(dga, b, logits, bias_before, bias_after, dw, dloss):
    """What one run left in b, every link against its reference on what the run itself produced.  Returns the counts."""
    n = {name: t.cpu().numpy() for name, t in b.items()}
    s, ids = n["scores"], n["ids"]
    for name in ("w", "scores", "loss", "psum", "dl_topk", "dlogits"):
        assert (n[name].view(np.uint32) != R.SENTINEL_F32).all(), name
    p64 = R.scores64(logits.float().cpu().numpy(), FUNC)
    assert (np.abs(s - p64) <= R.score_bar(E, FUNC) * p64).all()
    rid, rw = R.select_ref(s, K, bias_before, scale=SCALE)
    assert np.array_equal(ids, rid) and np.array_equal(n["w"].view(np.uint32), rw.view(np.uint32))
    rl, rc, rp = B.forward_ref(s, ids, L, ALPHA, True)
    assert np.array_equal(n["counts"], rc) and rc.sum() == T * K
    assert (np.abs(n["psum"] - rp) <= B.psum_bar(L, E) * rp).all() and (np.abs(n["loss"] - rl) <= B.loss_bar(L, E) * rl).all()
    assert (n["loss"] > 0).all()
    ref, m = R.backward_ref(dw.cpu().numpy(), s, ids, FUNC, True, SCALE)
    assert (np.abs(n["dl_topk"].astype(np.float64) - ref) <= R.backward_bar(E, K) * m).all()
    # the balance term alone, run again on what the step left, then the step's sum bit for bit
    aux = dga.router_balance_loss_backward(dloss, b["counts"], b["scores"], K, FUNC, seq_len=L, alpha=ALPHA, normalize=True, sync=True).cpu().numpy()
    ref, m = B.backward_ref(dloss.cpu().numpy(), rc, s, K, FUNC, L, ALPHA, True)
    assert (np.abs(aux.astype(np.float64) - ref) <= B.backward_bar(E) * m).all() and aux.any()
    assert np.array_equal(n["dlogits"].view(np.uint32), np.add(n["dl_topk"], aux, dtype=np.float32).view(np.uint32))
    assert np.array_equal(bias_after.view(np.uint32), B.bias_update_ref(bias_before, rc, RATE).view(np.uint32))
    return rc


def test_the_training_step_eager_then_one_graph(dga):
    bias = torch.zeros(E, device="cuda")
    logits = _logits(1)
    g = torch.Generator().manual_seed(2)
    dw, dloss = torch.randn(T, K, generator=g).cuda(), torch.randn(SEGMENTS, generator=g).cuda()
    b = _buffers()
    run = lambda: _step(dga, logits, bias, dw, dloss, b)
    host = lambda: bias.cpu().numpy().copy()

    bias0 = host()
    run(); torch.cuda.synchronize()
    bias1 = host()
    first = _check(dga, b, logits, bias0, bias1, dw, dloss)
    assert not np.array_equal(bias1, bias0) and bias1[1] == -RATE              # the bias moved: down for the loaded expert
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run()
    torch.cuda.synchronize()

    logits.copy_(_logits(8))
    fresh = _buffers()
    for name in b:
        b[name].copy_(fresh[name])
    torch.cuda.synchronize()
    before = host()
    graph.replay()
    torch.cuda.synchronize()
    after = host()
    counts = _check(dga, b, logits, before, after, dw, dloss)                  # every link on what the replay itself produced
    assert not np.array_equal(counts, first) and not np.array_equal(after, before)
    assert after[1] == before[1] - RATE
