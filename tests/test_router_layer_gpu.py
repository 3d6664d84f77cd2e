"""GPU: an MoE layer from the gate's logits to y, tests/test_moe_permute_gpu.py's sizes (G = 4 experts, Mmax = 256 slots each, D = 384,
N = 256, T = 96 tokens, k = 3 of E = G experts):
  router_topk(logits, k, "sigmoid", bias)                                                   ids int32 [T, k], weights, scores
  route_slots(ids, 4, T * k, ...)                                                           counts, dest, inverse
  gather_per_token_cast_to_fp8_transposed(x, inverse, index_div=k, masked_m=counts, ...)    (X^T q, ..), (Xq, sX)
  m_grouped_gemm_fp8_fp8_bf16_nt_masked((Xq, sX), Wq)                                       Out bf16 [G, Mmax, N]
  combine_tokens(Out, dest, weights)                                                        y bf16 [T, N]
eagerly, then as one captured single-stream graph that is replayed after the logits and x are rewritten: the graph follows the routing from
the logits on.  The bias leaves one expert empty.  Then the backward link, combine_tokens_weight_grad -> router_topk_backward."""
import numpy as np
import pytest
import torch

import combine_ref as C
import router_ref as R

pytestmark = pytest.mark.gpu

G, MMAX, D, N, T, K = 4, 256, 384, 256, 96, 3
E, SLOTS, FUNC, SCALE = G, G * MMAX, "sigmoid", 2.5
EMPTY = 2                                    # the expert the bias keeps every token away from (k = 3 of 4: the other three are chosen)
SENTINEL_Q, SENTINEL_SF, NAN16 = 0xA5, 0x7FC0A5A5, 0x7FC1


def _buffers():
    byt = lambda *s: torch.full(s, SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sfs = lambda *s: torch.full(s, SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    nan16 = lambda *s: torch.full(s, NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return {"ids": torch.full((T, K), R.SENTINEL_ID, dtype=torch.int32, device="cuda"), "w": sfs(T, K), "scores": sfs(T, E),
            "xt": (byt(D, SLOTS), sfs(D, SLOTS // 128)), "x": (byt(G, MMAX, D), sfs(G, MMAX, D // 128)), "out": nan16(G, MMAX, N), "y": nan16(T, N),
            "counts": torch.full((G,), 77, dtype=torch.int32, device="cuda"), "dest": torch.full((T * K,), 12345, dtype=torch.int64, device="cuda"),
            "inverse": torch.full((SLOTS,), 1 << 62, dtype=torch.int64, device="cuda"), "overflow": torch.zeros(1, dtype=torch.int32, device="cuda")}


def _layer(dga, logits, bias, x, wq, b):
    dga.router_topk(logits, K, score_func=FUNC, bias=bias, scale=SCALE, out=(b["ids"], b["w"], b["scores"]))
    b["overflow"].zero_()
    dga.route_slots(b["ids"], 4, T * K, G, MMAX, b["counts"], b["dest"], b["overflow"], inverse=b["inverse"])
    dga.gather_per_token_cast_to_fp8_transposed(x, b["inverse"].view(G, MMAX), index_div=K, masked_m=b["counts"], rowwise=True,
                                                out=(b["xt"], b["x"]))
    dga.m_grouped_gemm_fp8_fp8_bf16_nt_masked(b["x"], wq, b["out"], b["counts"], MMAX)
    dga.combine_tokens(b["out"].view(SLOTS, N), b["dest"].view(T, K), b["w"], out=b["y"])


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(T, E, generator=g) * 2.0).to(torch.bfloat16).cuda()
    x = torch.randn(T, D, generator=g).to(torch.bfloat16).cuda()
    return logits, x


def _expert_weights(dga):
    g = torch.Generator().manual_seed(99)
    pairs = [dga.per_block_cast_to_fp8((torch.randn(N, D, generator=g) * 0.05).cuda()) for _ in range(G)]
    return torch.stack([q.view(torch.uint8) for q, _ in pairs]), torch.stack([sf for _, sf in pairs])


def _bf16(t):
    return (t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def _check(b, logits, bias):
    """What one run left in b, against the references on what the run itself produced.  Returns (ids, weights, scores, out, dest)."""
    ids, w, s = b["ids"].cpu().numpy(), b["w"].cpu().numpy(), b["scores"].cpu().numpy()
    p64 = R.scores64(logits.float().cpu().numpy(), FUNC)
    assert (np.abs(s - p64) <= R.score_bar(E, FUNC) * p64).all()
    rid, rw = R.select_ref(s, K, bias.cpu().numpy(), scale=SCALE)
    assert np.array_equal(ids, rid) and np.array_equal(w.view(np.uint32), rw.view(np.uint32))
    counts, dest = b["counts"].cpu().numpy(), b["dest"].cpu().numpy()
    assert np.array_equal(counts, np.bincount(ids.reshape(-1), minlength=G)) and counts[EMPTY] == 0 and b["overflow"].item() == 0
    assert (dest >= 0).all() and np.array_equal(dest // MMAX, ids.reshape(-1))          # pair t * k + j sits in a slot of expert ids[t, j]
    assert np.array_equal(b["inverse"].cpu().numpy()[dest], np.arange(T * K))
    out = _bf16(b["out"]).reshape(SLOTS, N)
    y_bits = b["y"].view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(y_bits, C.round_to(C.combine_ref(out, dest.reshape(T, K), w), "bf16"))
    y = _bf16(b["y"])
    assert np.isfinite(y).all() and y.any()
    return ids, w, s, out, dest


def test_the_layer_from_logits_eager_then_one_graph_then_backward(dga):
    bias = torch.zeros(E)
    bias[EMPTY] = -4.0                                                       # sigmoid <= 1: expert EMPTY is below every other
    bias = bias.cuda()
    logits, x = _inputs(1)
    wq = _expert_weights(dga)
    b = _buffers()
    run = lambda: _layer(dga, logits, bias, x, wq, b)

    run(); torch.cuda.synchronize()
    first = _check(b, logits, bias)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run()
    torch.cuda.synchronize()

    logits2, x2 = _inputs(8)
    logits.copy_(logits2); x.copy_(x2)
    fresh = _buffers()
    for name in ("ids", "w", "scores", "out", "y"):
        b[name].copy_(fresh[name])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    ids, w, s, out, dest = _check(b, logits2, bias)                          # y is the numpy combine of what the replay itself produced
    assert not np.array_equal(ids, first[0])                                 # ... under another routing

    # the backward link: dw from the combine's weight gradient, then to the logits
    dy = torch.randn(T, N, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).cuda()
    dw = dga.combine_tokens_weight_grad(b["out"].view(SLOTS, N), dy, b["dest"].view(T, K))
    dlogits = dga.router_topk_backward(dw, b["scores"], b["ids"], FUNC, scale=SCALE, sync=True).cpu().numpy()
    refw, barw = C.weight_grad_ref(out, dy.float().cpu().numpy(), dest.reshape(T, K))
    dw_np = dw.cpu().numpy()
    assert (np.abs(dw_np.astype(np.float64) - refw) <= barw).all()
    ref, m = R.backward_ref(dw_np, s, ids, FUNC, True, SCALE)
    assert (np.abs(dlogits.astype(np.float64) - ref) <= R.backward_bar(E, K) * m).all()
    assert not dlogits.view(np.uint32)[:, EMPTY].any() and dlogits[:, [g for g in range(G) if g != EMPTY]].any()
