"""GPU: indexer_prepare_q / indexer_prepare_k / indexer_prepare_backward against tests/indexer_prepare_ref.py.  Every output is pre-filled
with sentinels; codes, scales, folded weights and float32 gradients equal the float32 definition bit for bit (the k outputs on the RETURNED
mean and rstd, which are held to their derived bounds against float64); tokens with position -1 and position P keep their sentinels."""
import numpy as np
import pytest
import torch

import indexer_prepare_ref as P
import paged_mqa_logits_ref as PG

pytestmark = pytest.mark.gpu

TABLE, EPS, PAD, SENT16, WS = P.table(50), 1e-6, 0xA5, 0x7FC1, 0.37
STRIDE = PG.BLOCK_BYTES + 16


def _dev(a, dtype="fp32"):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(P.TORCH_DT[dtype]).cuda()      # (converted on the host: exact values)


def _sent(dtype, *shape):
    if dtype == "u8":
        return torch.full(shape, PAD, dtype=torch.uint8, device="cuda")
    if dtype == "fp32":
        return torch.full(shape, P.SENTINEL_F32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, SENT16, dtype=torch.int16, device="cuda").view(P.TORCH_DT[dtype])


def _positions(tokens, seed, torch_dtype=torch.int64):
    """positions inside the table, token 1 at -1 and the last at P when there are three or more -> (numpy, device, live mask)"""
    pos = np.random.default_rng(seed).integers(0, len(TABLE), tokens)
    if tokens >= 3:
        pos[1], pos[-1] = -1, len(TABLE)
    return pos, torch.from_numpy(pos).to(torch_dtype).cuda(), (pos >= 0) & (pos < len(TABLE))


def _expect(live, fill, values, dtype):
    want = np.full((len(live),) + values.shape[1:], fill, dtype)
    want[live] = values
    return want


def _quantised(oracle, y, ue8m0):
    codes, sf = oracle.quant_1x128(np.ascontiguousarray(y, np.float32), ue8m0)
    return codes, sf.reshape(-1)


@pytest.mark.parametrize("m,h,dtype,interleaved,ue8m0,w_dtype,pos_dtype", [(1, 1, "fp32", False, False, "fp32", torch.int64),
                         (5, 3, "bf16", True, True, "bf16", torch.int32), (3, 32, "fp16", False, True, "fp32", torch.int64),
                         (33, 64, "bf16", True, False, "bf16", torch.int32), (33, 64, "bf16", False, False, "fp32", torch.int32)])
def test_q_codes_scales_and_weights_bit_for_bit(dga, oracle, m, h, dtype, interleaved, ue8m0, w_dtype, pos_dtype):
    x, w = P.rows(m * h, dtype, 1), P.rows(m, w_dtype, 2)[:, :h].reshape(-1)
    pos, pos_d, live = _positions(m, 3, pos_dtype)
    live, cs = np.repeat(live, h), TABLE[np.repeat(pos, h).clip(0, len(TABLE) - 1)]
    out = (_sent("u8", m, h, P.D), _sent("fp32", m, h), _sent("fp32", m, h))
    got = dga.indexer_prepare_q(_dev(x, dtype).view(m, h, P.D), pos_d, _dev(TABLE), weights=_dev(w, w_dtype).view(m, h), weight_scale=WS,
                                interleaved=interleaved, use_ue8m0=ue8m0, out=out, sync=True)
    assert got[0].dtype == torch.float8_e4m3fn and all(a.data_ptr() == b.data_ptr() for a, b in zip(got, out))
    codes, sf = _quantised(oracle, P.prepared32(x[live], cs[live], interleaved), ue8m0)
    assert np.array_equal(P.bits_of(out[0]).reshape(-1, P.D), _expect(live, PAD, codes, np.uint8))
    assert np.array_equal(P.bits_of(out[1]).reshape(-1), _expect(live, P.SENTINEL_F32, sf.view(np.uint32), np.uint32))
    folded = (w[live] * np.float32(WS)) * sf
    assert np.array_equal(P.bits_of(out[2]).reshape(-1), _expect(live, P.SENTINEL_F32, folded.view(np.uint32), np.uint32))
    assert dga.indexer_prepare_q(_dev(x, dtype).view(m, h, P.D), pos_d, _dev(TABLE), sync=True)[2] is None


@pytest.mark.parametrize("norm", [None, "fp32", "same"])
@pytest.mark.parametrize("n", [1, 17, 130])
def test_k_statistics_codes_and_paged_cache(dga, oracle, n, norm):
    dtype, interleaved, ue8m0 = P.DTYPES[n % 3], n == 17, n == 130
    x = P.to_dtype(P.rows(n, dtype, 4, 2.0) + np.linspace(-3, 3, n, dtype=np.float32)[:, None], dtype)
    pos, pos_d, live = _positions(n, 5)
    w_dtype = dtype if norm == "same" else "fp32"
    gamma, beta = (None, None) if norm is None else (P.to_dtype(P.rows(1, w_dtype, 6)[0] + 1, w_dtype), None if n == 17 else P.rows(1, w_dtype, 7)[0])
    nb = (n + 63) // 64 + 1
    slots = np.random.default_rng(8).permutation(64 * nb)[:n].astype(np.int64)
    if n >= 3:
        slots[0], slots[2] = -1, 64 * nb
    kw = dict(norm_weight=None if norm is None else _dev(gamma, w_dtype), norm_bias=None if beta is None else _dev(beta, w_dtype), eps=EPS,
              slot_mapping=torch.from_numpy(slots).cuda(), interleaved=interleaved, use_ue8m0=ue8m0, sync=True)
    out = {"k_fp8": _sent("u8", n, P.D), "kscale": _sent("fp32", n)}
    if norm is not None:
        out.update(mean=_sent("fp32", n), rstd=_sent("fp32", n))
    caches = [_sent("u8", nb, STRIDE), _sent("u8", nb, STRIDE)]
    got = dga.indexer_prepare_k(_dev(x, dtype), pos_d, _dev(TABLE), kv_cache=caches[0][:, :PG.BLOCK_BYTES], out=out, **kw)
    alone = dga.indexer_prepare_k(_dev(x, dtype), pos_d, _dev(TABLE), kv_cache=caches[1][:, :PG.BLOCK_BYTES], contiguous=False, **kw)
    assert alone.k_fp8 is None and alone.kscale is None and (got.mean is None) == (norm is None) and got.k_fp8.dtype == torch.float8_e4m3fn
    stats = None
    if norm is not None:
        mean, rstd = (P.bits_of(out[name]).view(np.float32)[live] for name in ("mean", "rstd"))
        assert np.array_equal(P.bits_of(out["mean"])[~live], np.full((~live).sum(), P.SENTINEL_F32, np.uint32))
        assert np.array_equal(P.bits_of(alone.mean)[live], mean.view(np.uint32)) and np.array_equal(P.bits_of(alone.rstd)[live], rstd.view(np.uint32))
        mu, _ = P.stats64(x[live], EPS)
        _, want = P.stats64(x[live], EPS, mean)
        e_mean, e_rstd = np.abs(mean - mu) / (P.MEAN_BAR * np.abs(x[live]).mean(axis=1)), np.abs(rstd / want - 1) / P.RSTD_BAR
        print(f"[{n},{norm}] worst error / bound: mean {e_mean.max():.3f}, rstd {e_rstd.max():.3f}")
        assert (e_mean <= 1).all() and (e_rstd <= 1).all()
        stats = (mean, rstd, gamma, beta)
    codes, sf = _quantised(oracle, P.prepared32(x[live], TABLE[pos[live]], interleaved, stats), ue8m0)
    assert np.array_equal(P.bits_of(out["k_fp8"]), _expect(live, PAD, codes, np.uint8))
    assert np.array_equal(P.bits_of(out["kscale"]), _expect(live, P.SENTINEL_F32, sf.view(np.uint32), np.uint32))
    want = np.full((nb, STRIDE), PAD, np.uint8)
    for i, slot in enumerate(slots[live]):
        if 0 <= slot < 64 * nb:
            want[slot // 64, 128 * (slot % 64):128 * (slot % 64 + 1)] = codes[i]
            want[slot // 64, PG.SCALES_AT + 4 * (slot % 64):PG.SCALES_AT + 4 * (slot % 64 + 1)] = sf[i:i + 1].view(np.uint8)
    for cache in caches:
        assert np.array_equal(cache.cpu().numpy(), want)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_special_rows_touch_no_other_row(dga, bad):
    x = P.rows(20, "fp32", 9)
    x[3] = 0
    pos_d, cs, gamma = torch.arange(20, device="cuda"), _dev(TABLE), _dev(P.rows(1, "fp32", 6)[0] + 1)
    for kw in (dict(), dict(norm_weight=gamma, norm_bias=gamma)):
        clean = dga.indexer_prepare_k(_dev(x), pos_d, cs, sync=True, **kw)
        if not kw:   # an all-zero row: scale 1 and zero codes
            assert float(clean.kscale[3]) == 1.0 and not P.bits_of(clean.k_fp8)[3].any()
        y = x.copy()
        y[7, 5] = bad
        dirty = dga.indexer_prepare_k(_dev(y), pos_d, cs, sync=True, **kw)
        others = np.arange(20) != 7
        for a, b in zip(clean, dirty):
            assert a is None or np.array_equal(P.bits_of(a)[others], P.bits_of(b)[others])


@pytest.mark.parametrize("lead,interleaved", [((5, 3), False), ((33, 64), True), ((17,), True), ((130,), False)])
def test_backward_bit_for_bit_and_rounded(dga, lead, interleaved):
    rows, tokens, is_q = int(np.prod(lead)), lead[0], len(lead) == 2
    g = P.rows(rows, "fp32", 10)
    pos, pos_d, live = _positions(tokens, 11, torch.int32)
    live, cs = np.repeat(live, rows // tokens), TABLE[np.repeat(pos, rows // tokens).clip(0, len(TABLE) - 1)]
    div = np.abs(P.rows(rows, "fp32", 12)[:, 0]) + np.float32(0.01) if is_q else None
    dw = P.rows(rows, "fp32", 13)[:, 0] if is_q else None
    grad = _dev(g).view(*lead, P.D) if is_q else torch.cat((_dev(g), _sent("fp32", rows, 4)), dim=1)[:, :P.D]
    kw = dict(interleaved=interleaved)
    if is_q:
        kw.update(row_div=_dev(div).view(lead), d_weights=_dev(dw).view(lead), weight_scale=WS)
    out = (_sent("fp32", *lead, P.D), _sent("fp32", *lead)) if is_q else (_sent("fp32", *lead, P.D),)
    got = dga.indexer_prepare_backward(grad, pos_d, _dev(TABLE), out_dtype=torch.float32, out=out, sync=True, **kw)
    want = P.backward32(g[live], cs[live], interleaved, None if div is None else div[live])
    got32 = P.bits_of(got[0]).reshape(-1, P.D)
    assert np.array_equal(got32, _expect(live, P.SENTINEL_F32, want.view(np.uint32), np.uint32))
    if is_q:
        raw = (dw[live] * np.float32(WS)) * div[live]
        assert np.array_equal(P.bits_of(got[1]).reshape(-1), _expect(live, P.SENTINEL_F32, raw.view(np.uint32), np.uint32))
    else:
        assert got[1] is None
    out16 = (_sent("bf16", *lead, P.D),) + out[1:]
    got16 = dga.indexer_prepare_backward(grad, pos_d, _dev(TABLE), out=out16, sync=True, **kw)       # (out_dtype: bfloat16, the default)
    assert got16[0].dtype == torch.bfloat16
    assert np.array_equal(P.bits_of(got16[0]).reshape(-1, P.D), _expect(live, SENT16, P.round_to(want, "bf16"), np.uint16))


def test_one_graph_prepares_and_scores_and_follows_new_inputs(dga, oracle):
    b, h, n, nb = 3, 32, 70, 3
    lens, tables = torch.tensor([70, 33, 64], dtype=torch.int32).cuda(), torch.tensor([[0, 2], [1, 0], [2, 1]], dtype=torch.int32).cuda()
    k, q, w = torch.empty((n, P.D), dtype=torch.bfloat16).cuda(), torch.empty((b, h, P.D), dtype=torch.bfloat16).cuda(), torch.empty((b, h)).cuda()
    kpos, qpos, slots = torch.zeros(n, dtype=torch.int64).cuda(), torch.zeros(b, dtype=torch.int64).cuda(), torch.zeros(n, dtype=torch.int64).cuda()
    cs, cache = _dev(TABLE), _sent("u8", nb, PG.BLOCK_BYTES)
    qo, logits = (_sent("u8", b, h, P.D), _sent("fp32", b, h), _sent("fp32", b, h)), _sent("fp32", b, 128)

    def fill(seed):
        rng = np.random.default_rng(seed)
        vals = P.rows(n, "bf16", seed), P.rows(b * h, "bf16", seed + 1), P.rows(b, "fp32", seed + 2)[:, :h].copy()
        ints = rng.integers(0, len(TABLE), n), rng.integers(0, len(TABLE), b), rng.permutation(64 * nb)[:n]
        for t, a in zip((k, q, w), vals):
            t.copy_(_dev(a, "bf16" if t.dtype == torch.bfloat16 else "fp32").view(t.shape))
        for t, a in zip((kpos, qpos, slots), ints):
            t.copy_(torch.from_numpy(a).cuda())
        return vals + ints

    def layer():
        dga.indexer_prepare_k(k, kpos, cs, kv_cache=cache, slot_mapping=slots, contiguous=False)
        q8, _, wf = dga.indexer_prepare_q(q, qpos, cs, weights=w, weight_scale=WS, out=qo)
        dga.fp8_paged_mqa_logits(q8.view(b, 1, h, P.D), cache, wf, lens, tables, None, 128, True, out=logits)

    fill(20)
    layer(); torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        layer()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        layer()
    kv, qv, wv, kp, qp, sl = fill(30)                             # positions, slots and inputs overwritten after the capture
    cache.fill_(PAD); logits.copy_(_sent("fp32", b, 128)); torch.cuda.synchronize()
    graph.replay(); torch.cuda.synchronize()
    first = P.bits_of(logits).copy()
    graph.replay(); torch.cuda.synchronize()
    assert np.array_equal(P.bits_of(logits), first)
    kc, ks = _quantised(oracle, P.prepared32(kv, TABLE[kp], False), False)
    qc, qs = _quantised(oracle, P.prepared32(qv, TABLE[np.repeat(qp, h)], False), False)
    codes, scales = np.full((64 * nb, P.D), PAD, np.uint8), np.frombuffer(bytes([PAD]) * (256 * nb), np.float32).copy()
    codes[sl], scales[sl] = kc, ks
    ref_cache = torch.from_numpy(PG.pack(codes.reshape(nb, 64, P.D), scales.reshape(nb, 64))).cuda()
    assert np.array_equal(cache.cpu().numpy(), ref_cache.cpu().numpy())
    folded = torch.from_numpy(((wv.reshape(-1) * np.float32(WS)) * qs).reshape(b, h)).cuda()
    want = dga.fp8_paged_mqa_logits(torch.from_numpy(qc).cuda().view(b, 1, h, P.D), ref_cache, folded, lens, tables, None, 128, True, sync=True)
    assert np.array_equal(first, P.bits_of(want))
