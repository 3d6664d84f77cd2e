"""GPU: the dispatch and combine around one grouped GEMM of a MoE layer, masked layout, driven by route_slots' tables as they are.

G = 4 experts, Mmax = 256 slots each, D = 384, N = 256, T = 96 tokens, k = 3 choices.  The 288 keys leave expert 1 empty and send 270 to
expert 0, which overflows its 256 slots: dest holds -1 for the dropped pairs.
  forward    gather_per_token_cast_to_fp8_transposed(x, inverse, index_div=k, masked_m=counts, rowwise=True)   (X^T q, ..), (Xq, sX)
             m_grouped_gemm_fp8_fp8_bf16_nt_masked((Xq, sX), Wq)                                               Out bf16 [G, Mmax, N]
             combine_tokens(Out, dest, w)                                                                      y bf16 [T, N]
  backward   gather_per_token_cast_to_fp8_transposed(dY, inverse, index_div=k, row_scale=w, ...)               dOut = w dY[token], never written
             combine_tokens_weight_grad(Out, dY, dest)                                                         dw fp32 [T, k]
             combine_tokens(dX_slots, dest)                                                                    dX bf16 [T, D]
Every link is compared with the same entry on the gather torch materialises; y with the numpy combine of the GEMM output the device made.
Then the forward, route_slots included, runs as one captured graph under another routing."""
import numpy as np
import pytest
import torch

import combine_ref as C

pytestmark = pytest.mark.gpu

G, MMAX, D, N, T, K = 4, 256, 384, 256, 96, 3
SLOTS = G * MMAX
SENTINEL_Q, SENTINEL_SF, NAN16 = 0xA5, 0x7FC0A5A5, 0x7FC1
STALE = 1 << 62


def _keys(seed, per_expert):
    """int32 [T * K]: per_expert[g] keys of expert g, shuffled."""
    keys = np.concatenate([np.full(n, g, np.int32) for g, n in enumerate(per_expert)])
    assert keys.size == T * K
    return np.random.default_rng(seed).permutation(keys)


def _buffers():
    """Every output of the forward, pre-filled: sentinels in codes and scales, NaN in the bf16 tensors, stale values in the tables."""
    byt = lambda *s: torch.full(s, SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sfs = lambda *s: torch.full(s, SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    nan16 = lambda *s: torch.full(s, NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return {"xt": (byt(D, SLOTS), sfs(D, SLOTS // 128)), "x": (byt(G, MMAX, D), sfs(G, MMAX, D // 128)), "out": nan16(G, MMAX, N), "y": nan16(T, N),
            "counts": torch.full((G,), 77, dtype=torch.int32, device="cuda"), "dest": torch.full((T * K,), 12345, dtype=torch.int64, device="cuda"),
            "inverse": torch.full((SLOTS,), STALE, dtype=torch.int64, device="cuda"), "overflow": torch.zeros(1, dtype=torch.int32, device="cuda")}


def _route(dga, keys, b):
    b["overflow"].zero_()
    dga.route_slots(keys, 4, T * K, G, MMAX, b["counts"], b["dest"], b["overflow"], inverse=b["inverse"])


def _forward(dga, x, wq, w, b, tables=None):
    """The three entries on the current stream; tables = (counts, dest, inverse) other than b's own."""
    counts, dest, inverse = tables if tables is not None else (b["counts"], b["dest"], b["inverse"])
    dga.gather_per_token_cast_to_fp8_transposed(x, inverse.view(G, MMAX), index_div=K, masked_m=counts, rowwise=True, out=(b["xt"], b["x"]))
    dga.m_grouped_gemm_fp8_fp8_bf16_nt_masked(b["x"], wq, b["out"], counts, MMAX)
    dga.combine_tokens(b["out"].view(SLOTS, N), dest.view(T, K), w, out=b["y"])


def _bits(t):
    if isinstance(t, tuple):
        return tuple(_bits(v) for v in t)
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return (t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.uint8) if t.dtype != torch.uint8 else t).cpu().numpy()


def _inputs(dga, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, D, generator=g).to(torch.bfloat16).cuda()
    w = torch.rand(T, K, generator=g).add_(0.05).cuda()
    return x, w


def _expert_weights(dga):
    g = torch.Generator().manual_seed(99)
    pairs = [dga.per_block_cast_to_fp8((torch.randn(N, D, generator=g) * 0.05).cuda()) for _ in range(G)]
    return torch.stack([q.view(torch.uint8) for q, _ in pairs]), torch.stack([sf for _, sf in pairs])


def _valid_slots(counts):
    return (np.arange(MMAX)[None, :] < counts[:, None]).reshape(-1)


def _check_tables(counts, dest, inverse, overflow, per_expert):
    """route_slots' contract on the host: counts, the overflow, dest and inverse inverse to each other on the placed pairs."""
    want = np.minimum(np.array(per_expert), MMAX)
    assert np.array_equal(counts, want) and int(overflow) == int(sum(per_expert) - want.sum())
    placed = dest >= 0
    assert int(placed.sum()) == int(want.sum()) and (dest[~placed] == -1).all()
    assert np.array_equal(inverse[dest[placed]], np.nonzero(placed)[0])
    assert np.array_equal(np.sort(dest[placed]), np.nonzero(_valid_slots(counts))[0])


def test_the_layer_on_route_slots_tables_link_by_link(dga):
    per_expert = (270, 0, 10, 8)
    keys = torch.from_numpy(_keys(0, per_expert)).cuda()
    x, w = _inputs(dga, 1)
    wq = _expert_weights(dga)
    b = _buffers()
    _route(dga, keys, b)
    _forward(dga, x, wq, w, b)
    torch.cuda.synchronize()
    counts, dest, inverse = b["counts"].cpu().numpy(), b["dest"].cpu().numpy(), b["inverse"].cpu().numpy()
    _check_tables(counts, dest, inverse, b["overflow"].item(), per_expert)
    assert (dest == -1).sum() == 14 and counts[1] == 0
    valid = _valid_slots(counts)
    assert (inverse[~valid] == STALE).all()                                   # route_slots writes the placed slots only

    # F1: the materialised gather, NaN on the slots beyond counts, through per_token_cast_to_fp8_transposed with the same mask
    token = torch.from_numpy(np.where(valid, inverse, 0) // K).cuda()
    ok = torch.from_numpy(valid).cuda()
    nan_rows = lambda rows: torch.where(ok[:, None], rows, torch.full_like(rows, float("nan"))).view(G, MMAX, -1).contiguous()
    ref = _buffers()
    dga.per_token_cast_to_fp8_transposed(nan_rows(x[token]), masked_m=b["counts"], rowwise=True, out=(ref["xt"], ref["x"]))
    dga.m_grouped_gemm_fp8_fp8_bf16_nt_masked(ref["x"], wq, ref["out"], b["counts"], MMAX)
    torch.cuda.synchronize()
    tup = lambda v: v if isinstance(v, tuple) else (v,)
    for name in ("xt", "x", "out"):                                           # (the excluded rows hold the same sentinels on both sides)
        for got, want in zip(tup(_bits(b[name])), tup(_bits(ref[name]))):
            assert np.array_equal(got, want), name
    out_bits = _bits(b["out"]).reshape(SLOTS, N)
    assert (out_bits[~valid] == NAN16).all() and (_bits(b["x"][0]).reshape(SLOTS, D)[~valid] == SENTINEL_Q).all()
    out_np = (out_bits.astype(np.uint32) << 16).view(np.float32)
    assert np.isfinite(out_np[valid]).all() and out_np[valid].any()

    # F3: y is the numpy combine of the GEMM output the device made
    w_np, dest2 = w.cpu().numpy(), dest.reshape(T, K)
    assert np.array_equal(_bits(b["y"]), C.round_to(C.combine_ref(out_np, dest2, w_np), "bf16"))

    # B1: dOut[slot] = w[pair] dY[token], quantised both ways without being written
    dy = torch.randn(T, N, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).cuda()
    pair = torch.from_numpy(np.where(valid, inverse, 0)).cuda()
    dout = nan_rows(w.view(-1)[pair][:, None] * dy[token].float())
    byt = lambda *s: torch.full(s, SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sfs = lambda *s: torch.full(s, SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    outs = [((byt(N, SLOTS), sfs(N, SLOTS // 128)), (byt(G, MMAX, N), sfs(G, MMAX, N // 128))) for _ in range(2)]
    dga.gather_per_token_cast_to_fp8_transposed(dy, b["inverse"].view(G, MMAX), index_div=K, row_scale=w.view(-1), masked_m=b["counts"],
                                                rowwise=True, out=outs[0])
    dga.per_token_cast_to_fp8_transposed(dout, masked_m=b["counts"], rowwise=True, out=outs[1])
    torch.cuda.synchronize()
    for got, want in zip(_bits(outs[0][0]) + _bits(outs[0][1]), _bits(outs[1][0]) + _bits(outs[1][1])):
        assert np.array_equal(got, want)

    # the router's gradient, under combine_tokens_weight_grad's own bar, and the backward of the dispatch
    dw = dga.combine_tokens_weight_grad(b["out"].view(SLOTS, N), dy, b["dest"].view(T, K), sync=True).cpu().numpy()
    refw, bar = C.weight_grad_ref(out_np, dy.float().cpu().numpy(), dest2)
    assert (np.abs(dw.astype(np.float64) - refw) <= bar).all() and not dw.view(np.uint32)[dest2 < 0].any() and dw[dest2 >= 0].all()
    dx_slots = nan_rows(torch.randn(SLOTS, D, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda()).view(SLOTS, D)
    dx = dga.combine_tokens(dx_slots, b["dest"].view(T, K), sync=True)
    assert np.array_equal(_bits(dx), C.round_to(C.combine_ref(dx_slots.float().cpu().numpy(), dest2), "bf16"))


def test_one_captured_graph_follows_the_routing(dga):
    """route_slots, the gathering quantiser, the grouped GEMM and the combine captured as one single-stream graph (eager once on the capture
    stream first).  keys, x and the routing weights are rewritten and the graph replayed: every output equals the eager forward under the new
    routing bit for bit -- qt / sft whole, (q, sf) and Out on the valid slots, y whole.  The slot order inside an expert is unspecified, so
    the eager run takes the replay's own tables, copied out; the slots beyond the new counts still hold the first routing's entries."""
    first, second = (270, 0, 10, 8), (3, 200, 0, 85)
    keys = torch.from_numpy(_keys(0, first)).cuda()
    x, w = _inputs(dga, 1)
    wq = _expert_weights(dga)
    b, fresh = _buffers(), _buffers()

    def run():
        _route(dga, keys, b)
        _forward(dga, x, wq, w, b)

    run(); torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run()
    torch.cuda.synchronize()
    old_inverse = b["inverse"].clone()

    keys.copy_(torch.from_numpy(_keys(7, second)).cuda())
    x2, w2 = _inputs(dga, 8)
    x.copy_(x2); w.copy_(w2)
    for name in ("xt", "x"):
        for t, f in zip(b[name], fresh[name]):
            t.copy_(f)
    b["out"].copy_(fresh["out"]); b["y"].copy_(fresh["y"])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()

    counts, dest, inverse = b["counts"].cpu().numpy(), b["dest"].cpu().numpy(), b["inverse"].cpu().numpy()
    _check_tables(counts, dest, inverse, b["overflow"].item(), second)
    valid = _valid_slots(counts)
    assert np.array_equal(inverse[~valid], old_inverse.cpu().numpy()[~valid]) and (inverse[~valid] != STALE).any()   # stale, valid-looking entries
    eager = _buffers()
    _forward(dga, x2, wq, w2, eager, tables=(b["counts"].clone(), b["dest"].clone(), b["inverse"].clone()))
    torch.cuda.synchronize()
    got, want = {k: _bits(b[k]) for k in ("xt", "x", "out", "y")}, {k: _bits(eager[k]) for k in ("xt", "x", "out", "y")}
    assert np.array_equal(got["xt"][0], want["xt"][0]) and np.array_equal(got["xt"][1], want["xt"][1])
    for i in range(2):
        g2, w2_ = got["x"][i].reshape(SLOTS, -1), want["x"][i].reshape(SLOTS, -1)
        assert np.array_equal(g2[valid], w2_[valid])
        assert (g2[~valid] == (SENTINEL_Q, SENTINEL_SF)[i]).all()
    go, wo = got["out"].reshape(SLOTS, N), want["out"].reshape(SLOTS, N)
    assert np.array_equal(go[valid], wo[valid]) and (go[~valid] == NAN16).all()
    assert np.array_equal(got["y"], want["y"])
    y = (got["y"].astype(np.uint32) << 16).view(np.float32)
    assert np.isfinite(y).all() and y.any()
    # ... and y is still the definition on what the replay itself produced
    out_np = (go.astype(np.uint32) << 16).view(np.float32)
    assert np.array_equal(got["y"], C.round_to(C.combine_ref(out_np, dest.reshape(T, K), w2.cpu().numpy()), "bf16"))
