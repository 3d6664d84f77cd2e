"""GPU: the indexer and what it selects for, end to end, with nothing decided on the host.  Decode: per_token_cast_to_fp8_paged ->
fp8_paged_mqa_logits(clean_logits=False) -> indexer_topk(context_lens, next_n=2, block_tables=...) -> sparse_mla_fwd on a bf16 latent
cache that shares the block table and the slots, whose flat view the physical slots index directly.  Prefill: fp8_mqa_logits ->
indexer_topk(relative=True) -> sparse_mla_fwd(index_offsets=row_starts).  The attention output is held to the reference
(tests/sparse_mla_ref.py) run on the indices the GPU selection produced, read back.  Step by step first, then the decode chain as one
captured graph replayed after the lengths, the tables and the slots were overwritten in place."""
import numpy as np
import pytest
import torch

import indexer_topk_ref as T
import paged_mqa_logits_ref as P
import sparse_mla_ref as R
from sparse_mla_support import _check
from sparse_mla_support import _filled as _filled_attention
from test_indexer_layer_gpu import _decode_case
from test_mqa_logits_gpu import _dev, _filled

pytestmark = pytest.mark.gpu

KV, D = P.BLOCK_KV, P.D
SCALE = R.D_QK ** -0.5


def _attention_inputs(m, hq, rows, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn((m, hq, R.D_QK), generator=g).to(torch.bfloat16).cuda()
    latent = torch.randn((rows, R.D_QK), generator=g).to(torch.bfloat16).cuda()
    return q, latent


def _verify_attention(q, latent, sel, out, lse, topk, offsets=None):
    ref = R.reference(q.float().cpu().numpy(), latent.float().cpu().numpy().reshape(-1, R.D_QK), sel, SCALE, offsets)
    bits = out.view(torch.int16).cpu().numpy().view(np.uint16)
    _check((out.float().cpu().numpy().astype(np.float64), bits, lse.cpu().numpy()), ref, SCALE, topk)
    return ref


def test_decode_chain_selects_then_attends(dga):
    h, nn, k, hq = 64, 2, 256, 64
    lens_a, lens_b = (0, 1, 65, 255, 600), (600, 65, 0, 1, 257)         # 0, 1, shorter than k, longer than k
    b, longest = len(lens_a), 600
    max_blocks = (longest + KV - 1) // KV + 1
    n = KV * max_blocks
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn((b * longest, D), generator=g).to(torch.bfloat16).cuda()
    q_index = dga.per_token_cast_to_fp8(torch.randn((b * nn * h, D), generator=g).cuda())[0].view(b, nn, h, D)
    weights = torch.randn((b * nn, h), generator=g).cuda()
    slots_a, tables_a, nb_a = _decode_case(1, lens_a, n, max_blocks, longest)
    slots_b, tables_b, nb_b = _decode_case(2, lens_b, n, max_blocks, longest)
    nb = max(nb_a, nb_b)
    cache = torch.full((nb, KV, 1, D + 4), 0x5A, dtype=torch.uint8, device="cuda")
    q, latent = _attention_inputs(b * nn, hq, nb * KV, 3)
    latent = latent.view(nb, KV, R.D_QK)                                # the paged bf16 latent cache: block, slot in block, 576
    slots, lens, tables = _dev(slots_a), _dev(np.asarray(lens_a, np.int32)), _dev(tables_a)
    buf = _filled(b * nn, n)
    sel = torch.full((b * nn, k), 7, dtype=torch.int32, device="cuda")
    out, lse = _filled_attention(b * nn, hq)

    def layer():
        dga.per_token_cast_to_fp8_paged(x, cache, slots)
        dga.fp8_paged_mqa_logits(q_index, cache, weights, lens, tables, None, n, False, out=buf)
        dga.indexer_topk(buf, k, context_lens=lens, next_n=nn, block_tables=tables, page_size=KV, num_blocks=nb, out=sel)
        dga.sparse_mla_fwd(q, latent.view(-1, R.D_QK), sel, SCALE, out=out, lse=lse)

    def verify(lens_h, tables_h):
        torch.cuda.synchronize()
        got = sel.cpu().numpy()
        want = T.reference(buf.cpu().numpy(), k, context_lens=np.asarray(lens_h, np.int32), next_n=nn, block_tables=tables_h, page_size=KV,
                           num_blocks=nb)
        assert np.array_equal(got, want)
        ref = _verify_attention(q, latent, got, out, lse, k)
        count = [max(min(ctx - nn + j + 1, k), 0) for ctx in lens_h for j in range(nn)]
        assert ref["count"].tolist() == count
        return out.clone(), lse.clone()

    layer()
    first = verify(lens_a, tables_a)
    assert np.isneginf(first[1][:2].cpu().numpy()).all() and np.isneginf(first[1][2].cpu().numpy()).all()     # context 0, and 1 seen from n - 2

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        layer()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        layer()
    for lens_h, tables_h, slots_h in ((lens_b, tables_b, slots_b), (lens_a, tables_a, slots_a)):
        lens.copy_(_dev(np.asarray(lens_h, np.int32))); tables.copy_(_dev(tables_h)); slots.copy_(_dev(slots_h))
        cache.fill_(0x5A); buf.copy_(_filled(b * nn, n)); sel.fill_(7)
        fill = _filled_attention(b * nn, hq)
        out.copy_(fill[0]); lse.copy_(fill[1])
        torch.cuda.synchronize()
        graph.replay()
        got = verify(lens_h, tables_h)
        same = torch.equal(got[0].view(torch.int16), first[0].view(torch.int16)) and torch.equal(got[1].view(torch.int32), first[1].view(torch.int32))
        assert same == (lens_h is lens_a)


@pytest.mark.parametrize("hq", (16, 128))
def test_prefill_chain_selects_then_attends(dga, hq):
    m, n, h, k = 12, 500, 32, 128
    g = torch.Generator(device="cpu").manual_seed(7)
    q_index, _ = dga.per_token_cast_to_fp8(torch.randn((m * h, D), generator=g).cuda())
    keys, sfk = dga.per_token_cast_to_fp8(torch.randn((n, D), generator=g).cuda())
    weights = torch.randn((m, h), generator=g).cuda()
    ks = np.zeros(m, np.int32)
    ks[[3, 7, 11]] = 1, 130, 480
    ke = (n - m + np.arange(m) + 1).astype(np.int32)
    ke[5] = 100                                                         # a row shorter than k
    ks_d, ke_d = _dev(ks), _dev(ke)
    q, latent = _attention_inputs(m, hq, n, 5)
    logits = dga.fp8_mqa_logits(q_index.view(m, h, D), (keys, sfk.reshape(n).contiguous()), weights, ks_d, ke_d)
    sel = dga.indexer_topk(logits, k, row_starts=ks_d, row_ends=ke_d, relative=True)
    out, lse = _filled_attention(m, hq)
    dga.sparse_mla_fwd(q, latent, sel, SCALE, index_offsets=ks_d, out=out, lse=lse, sync=True)
    got = sel.cpu().numpy()
    assert np.array_equal(got, T.reference(logits.cpu().numpy(), k, row_starts=ks, row_ends=ke, relative=True))
    ref = _verify_attention(q, latent, got, out, lse, k, ks)
    assert ref["count"].tolist() == [int(min(e - s, k)) for s, e in zip(ks, ke)] and ref["count"][11] == 20 and ref["count"][5] == 100
    # relative indices without their offsets name other rows: the offsets are what was consumed
    plain = R.reference(q.float().cpu().numpy(), latent.float().cpu().numpy(), got, SCALE)
    assert not np.allclose(plain["out"][7], ref["out"][7])
