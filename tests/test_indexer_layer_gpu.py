"""GPU: the indexer end to end -- keys written, scored, selected -- with nothing decided on the host.  The reference selection
(tests/indexer_topk_ref.py) runs on the logits tensor the scoring kernel produced, read back: on float64 logits near-ties would flip.
Prefill: fp8_mqa_logits -> indexer_topk(row_starts, row_ends, relative=True).  Decode: per_token_cast_to_fp8_paged ->
fp8_paged_mqa_logits(clean_logits=False) into a buffer of NaN -> indexer_topk(context_lens, next_n=2, block_tables=...): no fill is
needed, and the NaN beyond each sequence's last page is still there afterwards.  Step by step first, then as one captured graph replayed
after the lengths, the tables and the slots were overwritten in place."""
import numpy as np
import pytest
import torch

import indexer_topk_ref as R
import paged_mqa_logits_ref as P
from test_mqa_logits_gpu import NAN_FILL, _dev, _filled

pytestmark = pytest.mark.gpu

KV, D = P.BLOCK_KV, P.D


@pytest.mark.parametrize("k", (2048, 64))
def test_prefill_scores_then_selects(dga, k):
    m, n, h = 96, 2300, 32
    g = torch.Generator(device="cpu").manual_seed(7)
    q, _ = dga.per_token_cast_to_fp8(torch.randn((m * h, D), generator=g).cuda())
    keys, sfk = dga.per_token_cast_to_fp8(torch.randn((n, D), generator=g).cuda())
    weights = torch.randn((m, h), generator=g).cuda()
    ks = np.zeros(m, np.int32)
    ks[[3, 40, 41, 95]] = 1, 130, 2290, 517
    ke = (n - m + np.arange(m) + 1).astype(np.int32)                      # causal: token m sees the keys up to its own
    ks_d, ke_d = _dev(ks), _dev(ke)
    logits = dga.fp8_mqa_logits(q.view(m, h, D), (keys, sfk.reshape(n).contiguous()), weights, ks_d, ke_d, sync=True)
    got = dga.indexer_topk(logits, k, row_starts=ks_d, row_ends=ke_d, relative=True, sync=True)
    host = logits.cpu().numpy()
    want = R.reference(host, k, row_starts=ks, row_ends=ke, relative=True)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert np.isneginf(host[0, ke[0]:]).all() and (want[0, :k] >= 0).all() and (want[41, 10:] == -1).all()
    # the selected scores are the row's largest
    for r in (0, 40, 95):
        inside = host[r, ks[r]:ke[r]]
        picked = inside[want[r][want[r] >= 0]]
        assert len(picked) == min(k, len(inside)) and picked.min() >= np.sort(inside)[-len(picked)]


def _decode_case(seed, lens, n, max_blocks, longest):
    """(slots int64 [B longest], tables, num_blocks): where the writer puts key p of sequence i (-1 beyond its length)"""
    tables, nb = P.make_tables(tuple(lens), n, max_blocks, seed)
    slots = np.full((len(lens), longest), -1, np.int64)
    for i, ctx in enumerate(lens):
        pos = np.arange(ctx)
        slots[i, :ctx] = tables[i, pos // KV].astype(np.int64) * KV + pos % KV
    return slots.reshape(-1), tables, nb


def test_decode_writes_scores_and_selects_without_a_fill(dga):
    h, nn, k = 64, 2, 2048
    lens_a, lens_b = (0, 1, 65, 2049, 2200), (2200, 65, 0, 1, 2049)
    b, longest = len(lens_a), 2200
    max_blocks = (longest + KV - 1) // KV + 1
    n = KV * max_blocks                                                   # 2304
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn((b * longest, D), generator=g).to(torch.bfloat16).cuda()            # the history of each sequence, 2200 keys
    q = dga.per_token_cast_to_fp8(torch.randn((b * nn * h, D), generator=g).cuda())[0].view(b, nn, h, D)
    weights = torch.randn((b * nn, h), generator=g).cuda()
    slots_a, tables_a, nb_a = _decode_case(1, lens_a, n, max_blocks, longest)
    slots_b, tables_b, nb_b = _decode_case(2, lens_b, n, max_blocks, longest)
    nb = max(nb_a, nb_b)
    cache = torch.full((nb, KV, 1, D + 4), 0x5A, dtype=torch.uint8, device="cuda")
    slots, lens, tables = _dev(slots_a), _dev(np.asarray(lens_a, np.int32)), _dev(tables_a)
    buf = _filled(b * nn, n)
    out = torch.full((b * nn, k), 7, dtype=torch.int32, device="cuda")

    def layer():
        dga.per_token_cast_to_fp8_paged(x, cache, slots)
        dga.fp8_paged_mqa_logits(q, cache, weights, lens, tables, None, n, False, out=buf)
        dga.indexer_topk(buf, k, context_lens=lens, next_n=nn, block_tables=tables, page_size=KV, num_blocks=nb, out=out)

    def verify(lens_h, tables_h):
        torch.cuda.synchronize()
        host, got = buf.cpu().numpy(), out.cpu()
        lens_np = np.asarray(lens_h, np.int32)
        want = R.reference(host, k, context_lens=lens_np, next_n=nn, block_tables=tables_h, page_size=KV, num_blocks=nb)
        assert torch.equal(got, torch.from_numpy(want))
        columns = R.reference(host, k, context_lens=lens_np, next_n=nn)
        words = host.view(np.uint32)
        for i, ctx in enumerate(lens_h):
            rows = slice(i * nn, (i + 1) * nn)
            pages = (ctx + KV - 1) // KV
            assert (words[rows, pages * KV:] == NAN_FILL).all()                        # nothing was filled beyond the last page
            assert np.isfinite(host[i * nn + 1, :ctx]).all()
            count = [max(min(ctx - nn + j + 1, k), 0) for j in range(nn)]
            assert [(want[i * nn + j] >= 0).sum() for j in range(nn)] == count and (columns[rows] < max(ctx, 1)).all()
        # the same scores behind a fill give the same selection: the fill buys nothing
        clean = dga.fp8_paged_mqa_logits(q, cache, weights, lens, tables, None, n, True, sync=True)
        again = dga.indexer_topk(clean, k, context_lens=lens, next_n=nn, block_tables=tables, page_size=KV, num_blocks=nb, sync=True)
        assert torch.equal(again.cpu(), got)
        return got

    # step by step
    layer()
    first = verify(lens_a, tables_a)
    assert (first[8] >= 0).all() and (first[6] >= 0).sum() == 2048 and (first[:2] == -1).all() and first[3].tolist()[:2] == [tables_a[1, 0] * KV, -1]

    # one captured graph, replayed after lengths, tables and slots were overwritten in place
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        layer()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        layer()
    for lens_h, tables_h, slots_h in ((lens_b, tables_b, slots_b), (lens_a, tables_a, slots_a)):
        lens.copy_(_dev(np.asarray(lens_h, np.int32))); tables.copy_(_dev(tables_h)); slots.copy_(_dev(slots_h))
        cache.fill_(0x5A); buf.copy_(_filled(b * nn, n)); out.fill_(7)
        torch.cuda.synchronize()
        graph.replay()
        got = verify(lens_h, tables_h)
        if lens_h is lens_a:
            assert torch.equal(got, first)
        else:
            assert not torch.equal(got, first) and (got[0] >= 0).sum() == 2048 and (got[4:6] == -1).all()
