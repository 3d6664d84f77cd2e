"""GPU: the paged decode chain with both caches in fp8, on one set of block tables and lengths and with nothing decided on the host:
per_token_cast_to_fp8_paged -> fp8_paged_mqa_logits(clean_logits=False) -> indexer_topk(context_lens, next_n=2, block_tables=...,
page_size=64) -> mla_kv_cast_to_fp8_paged -> sparse_mla_fwd_fp8, the latent cache sharing the key cache's slots.  Step by step first,
then as one captured graph replayed after the lengths, the tables and the slots were overwritten in place.  The attention output is held
to sparse_mla_ref.reference on the dequantised rows of the cache the chain wrote, on the indices the GPU selection produced, under
sparse_mla_fwd's own bounds: sparse_mla_fwd_fp8 is that function on those rows bit for bit, so the bounds need no margin."""
import numpy as np
import pytest
import torch

import indexer_topk_ref as T
import paged_mqa_logits_ref as P
import sparse_mla_fp8_ref as F
import sparse_mla_ref as R
from sparse_mla_support import _check
from sparse_mla_support import _filled as _filled_attention
from test_indexer_layer_gpu import _decode_case
from test_mqa_logits_gpu import _dev, _filled

pytestmark = pytest.mark.gpu

KV, D = P.BLOCK_KV, P.D
SCALE = R.D_QK ** -0.5


def test_decode_chain_with_both_caches_in_fp8(dga):
    h, nn, k, hq = 64, 2, 128, 64
    lens_a, lens_b = (70, 129, 300), (300, 1, 200)                      # partial last pages; shorter and longer than k; 1 seen from n - 2
    b, longest = len(lens_a), 300
    max_blocks = (longest + KV - 1) // KV + 1
    n = KV * max_blocks
    g = torch.Generator(device="cpu").manual_seed(17)
    x = torch.randn((b * longest, D), generator=g).to(torch.bfloat16).cuda()                 # the indexer's keys, per sequence and position
    latent = torch.randn((b * longest, R.D_QK), generator=g).to(torch.bfloat16).cuda()        # the rows of the latent cache, likewise
    kv_c, k_pe = latent[:, :F.LATENT], latent[:, F.LATENT:]                                   # (column slices of one tensor)
    q_index = dga.per_token_cast_to_fp8(torch.randn((b * nn * h, D), generator=g).cuda())[0].view(b, nn, h, D)
    weights = torch.randn((b * nn, h), generator=g).cuda()
    q = torch.randn((b * nn, hq, R.D_QK), generator=g).to(torch.bfloat16).cuda()
    slots_a, tables_a, nb_a = _decode_case(1, lens_a, n, max_blocks, longest)
    slots_b, tables_b, nb_b = _decode_case(2, lens_b, n, max_blocks, longest)
    nb = max(nb_a, nb_b)
    cache = torch.full((nb, KV, 1, D + 4), 0x5A, dtype=torch.uint8, device="cuda")
    stride = KV * F.ROW + 64                                            # a padded block stride
    mla_buf = torch.zeros((nb, stride), dtype=torch.uint8, device="cuda")
    mla_cache = mla_buf[:, :KV * F.ROW].view(nb, KV, 1, F.ROW)
    slots, lens, tables = _dev(slots_a), _dev(np.asarray(lens_a, np.int32)), _dev(tables_a)
    buf = _filled(b * nn, n)
    sel = torch.full((b * nn, k), 7, dtype=torch.int32, device="cuda")
    out, lse = _filled_attention(b * nn, hq)

    def layer():
        dga.per_token_cast_to_fp8_paged(x, cache, slots)
        dga.fp8_paged_mqa_logits(q_index, cache, weights, lens, tables, None, n, False, out=buf)
        dga.indexer_topk(buf, k, context_lens=lens, next_n=nn, block_tables=tables, page_size=KV, num_blocks=nb, out=sel)
        dga.mla_kv_cast_to_fp8_paged(kv_c, k_pe, mla_cache, slots)
        dga.sparse_mla_fwd_fp8(q, mla_cache, sel, SCALE, out=out, lse=lse)

    def verify(lens_h, tables_h, slots_h):
        torch.cuda.synchronize()
        got = sel.cpu().numpy()
        want = T.reference(buf.cpu().numpy(), k, context_lens=np.asarray(lens_h, np.int32), next_n=nn, block_tables=tables_h, page_size=KV,
                           num_blocks=nb)
        assert np.array_equal(got, want)
        host = mla_buf.cpu().numpy()
        codes, scales, rope = F.unpack(host, KV)
        kept = slots_h >= 0                                             # what the writer was to write is what the cache holds
        wq, wsf = dga.per_token_cast_to_fp8(kv_c.contiguous())
        assert np.array_equal(codes[slots_h[kept]], wq.view(torch.uint8).cpu().numpy()[kept])
        assert np.array_equal(scales[slots_h[kept]].view(np.uint32), wsf.cpu().numpy().view(np.uint32)[kept])
        assert np.array_equal(rope[slots_h[kept]], k_pe.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)[kept])
        ref = R.reference(q.float().cpu().numpy(), F.deq(codes, scales, rope), got, SCALE)
        bits = out.view(torch.int16).cpu().numpy().view(np.uint16)
        _check((out.float().cpu().numpy().astype(np.float64), bits, lse.cpu().numpy()), ref, SCALE, k)
        count = [max(min(ctx - nn + j + 1, k), 0) for ctx in lens_h for j in range(nn)]
        assert ref["count"].tolist() == count
        # ... and, bit for bit, the bf16 kernel on the dequantised rows
        deq = torch.from_numpy(F.deq_bits(codes, scales, rope).view(np.int16)).view(torch.bfloat16).cuda()
        o2, l2 = dga.sparse_mla_fwd(q, deq, sel, SCALE, sync=True)
        assert torch.equal(o2.view(torch.int16), out.view(torch.int16)) and torch.equal(l2.view(torch.int32), lse.view(torch.int32))
        return out.clone(), lse.clone()

    layer()
    first = verify(lens_a, tables_a, slots_a)
    assert 0 < min(lens_a) - nn + 1 < k < max(lens_a)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        layer()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        layer()
    for lens_h, tables_h, slots_h in ((lens_b, tables_b, slots_b), (lens_a, tables_a, slots_a)):
        lens.copy_(_dev(np.asarray(lens_h, np.int32))); tables.copy_(_dev(tables_h)); slots.copy_(_dev(slots_h))
        cache.fill_(0x5A); mla_buf.zero_(); buf.copy_(_filled(b * nn, n)); sel.fill_(7)
        fill = _filled_attention(b * nn, hq)
        out.copy_(fill[0]); lse.copy_(fill[1])
        torch.cuda.synchronize()
        graph.replay()
        got = verify(lens_h, tables_h, slots_h)
        same = torch.equal(got[0].view(torch.int16), first[0].view(torch.int16)) and torch.equal(got[1].view(torch.int32), first[1].view(torch.int32))
        assert same == (lens_h is lens_a)
    assert np.isneginf(lse.cpu().numpy()).sum() == 0                    # (the last replay is lens_a's: every token sees a key)
