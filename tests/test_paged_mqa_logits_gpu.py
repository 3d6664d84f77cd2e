"""GPU: fp8_paged_mqa_logits and per_token_cast_to_fp8_paged against tests/paged_mqa_logits_ref.py.  C is the kernel's chunk of columns, a
page is 64 keys.  Every output starts as the NaN pattern of test_mqa_logits_gpu.py; the physical blocks are a random permutation, two
sequences share their first block, and the unused table entries hold -1 and 0x7FFFFFFF.  Exactly summable operands must give the float64
reference as values at H = 32 and 64 and next_n = 1 and 2 -- lengths 0, 1, a page, a page and one, a chunk and one and the whole ragged
width; one column; a table shorter than the width -- lengths are clamped and an out-of-range entry costs its page only; amax-quantised
random operands are bit for bit fp8_mqa_logits on the gathered operands and inside its bound; clean_logits=False leaves what it must not
touch; a padded cache changes nothing; every code that is no NaN gives its exact value from either operand, and fp8_mqa_logits' bits; a
NaN code of either sign poisons its column in every sequence that names the block, or its row; a captured graph follows rewritten
operands, lengths, tables and cache bytes; the writer stores the quantiser's bytes at their slots and nothing else; and one captured
graph that writes the new keys and then scores them matches fp8_mqa_logits on the contiguous history."""
import numpy as np
import pytest
import torch

import mqa_logits_ref as M
import paged_mqa_logits_ref as R
from test_mqa_logits_gpu import NAN_FILL, _dev, _filled, _same_values

pytestmark = pytest.mark.gpu

KV, BYTES = R.BLOCK_KV, R.BLOCK_BYTES


def _chunk():
    from deepgemm_ascend_amd import api
    return api.PAGED_MQA_LOGITS_CHUNK_N


def _big():
    """(lens, N, max_blocks, share): six sequences over a ragged width of two chunks and 37"""
    c = _chunk()
    n = 2 * c + 37
    return (0, 1, KV, KV + 1, c + 1, n), n, (n + KV - 1) // KV, (3, 4)


def _cache(buf, padded=False):
    """the device cache of a packed [num_blocks, 8448] array: [num_blocks, 64, 1, 132], or a [num_blocks, 8448] view of rows 8448 + 64 apart"""
    if not padded:
        return _dev(buf).view(buf.shape[0], KV, 1, R.D + 4)
    codes, scales = R.unpack(np.asarray(buf))
    wide = _dev(R.pack(codes, scales, BYTES + 64))
    view = wide[:, :BYTES]
    assert view.stride(0) == BYTES + 64
    return view


def _run(dga, q, buf, weights, lens, tables, n, clean=True, out=None, padded=False):
    rows = q.shape[0] * q.shape[1]
    out = _filled(rows, n) if out is None else out
    got = dga.fp8_paged_mqa_logits(_dev(q).view(torch.float8_e4m3fn), _cache(buf, padded), _dev(weights), _dev(lens), _dev(tables), None, n,
                                   clean, out=out, sync=True)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("nn", (1, 2))
@pytest.mark.parametrize("h", M.HEADS)
def test_exact_values_on_exactly_summable_data(dga, h, nn):
    lens, n, max_blocks, share = _big()
    q, buf, weights, lens_a, tables, want = R.exact_case(h, nn, lens, n, max_blocks, share)
    assert tables[3, 0] == tables[4, 0] and set(tables[0]) == set(R.UNUSED)
    fin = ~np.isneginf(want)
    assert fin.sum() == sum(max(v - nn + j + 1, 0) for v in lens for j in range(nn)) and len(np.unique(want[fin])) > 1000
    if nn == 2:
        assert fin[2].sum() == 0 and fin[3].sum() == 1              # length 1: an empty row and a row of one key
    _same_values(_run(dga, q, buf, weights, lens_a, tables, n), want)
    # one sequence, one column
    q, buf, weights, lens_a, tables, want = R.exact_case(h, nn, (1,), 1, 1)
    assert want.shape == (nn, 1) and np.isfinite(want[nn - 1, 0])
    _same_values(_run(dga, q, buf, weights, lens_a, tables, 1), want)
    # a table of two pages under a width of 300: the lengths stop at 128
    q, buf, weights, lens_a, tables, want = R.exact_case(h, nn, (300, 90, 128), 300, 2)
    assert np.isfinite(want[nn - 1, :128]).all() and np.isneginf(want[:, 128:]).all()
    _same_values(_run(dga, q, buf, weights, lens_a, tables, 300), want)


def test_lengths_are_clamped_and_a_bad_entry_costs_its_page_only(dga):
    h, nn, c = 64, 2, _chunk()
    n = c + 37
    lens = (-5, n + 100, 3 * KV + 9, 2 * KV)
    q, buf, weights, lens_a, tables, want = R.exact_case(h, nn, lens, n, (n + KV - 1) // KV, (1, 2), seed=3)
    assert np.isneginf(want[:2]).all() and np.isfinite(want[3, :n]).all() and np.isfinite(want[2, :n - 1]).all()
    clean = _run(dga, q, buf, weights, lens_a, tables, n)
    _same_values(clean, want)
    nb = buf.shape[0]
    bad = tables.copy()
    bad[1, 2], bad[2, 1], bad[3, 0] = nb, -3, 0x7FFFFFFF             # needed pages: too large by one, negative, huge
    got = _run(dga, q, buf, weights, lens_a, bad, n)
    want_bad, _ = R.reference(q, buf, weights, lens_a, bad, n)
    lost = np.zeros(want.shape, bool)
    lost[2:4, 2 * KV:3 * KV], lost[4:6, KV:2 * KV], lost[6:8, :KV] = True, True, True
    assert np.array_equal(np.isneginf(want_bad), np.isneginf(want) | lost) and (lost & ~np.isneginf(want)).sum() > 5 * KV
    assert np.isneginf(got[lost]).all()
    assert np.array_equal(_bits(got[~lost]), _bits(clean[~lost]))


def _quantised(dga, h, nn, lens, n, max_blocks, share, seed):
    """amax-quantised normal draws: (q fp8 [B, nn, h, 128], packed cache, weights, tables, the codes and scales as numpy)"""
    b = len(lens)
    tables, nb = R.make_tables(lens, n, max_blocks, seed, share)
    g = torch.Generator(device="cpu").manual_seed(seed)
    xq = torch.randn((b * nn * h, R.D), generator=g).cuda()
    xk = torch.randn((nb * KV, R.D), generator=g).cuda()
    weights = torch.randn((b * nn, h), generator=g).cuda()
    q, _ = dga.per_token_cast_to_fp8(xq)                  # q carries no scale: the caller would fold it into weights
    k, sfk = dga.per_token_cast_to_fp8(xk)
    qc = q.view(torch.uint8).cpu().numpy().reshape(b, nn, h, R.D)
    kc, sc = k.view(torch.uint8).cpu().numpy().reshape(nb, KV, R.D), sfk.cpu().numpy().reshape(nb, KV)
    assert int((qc & 0x7F).max()) == 0x7E and int((kc & 0x7F).max()) == 0x7E           # codes up to 448
    return q.view(b, nn, h, R.D), R.pack(kc, sc), weights, tables, qc


@pytest.mark.parametrize("nn", (1, 2))
@pytest.mark.parametrize("h", M.HEADS)
def test_bit_for_bit_fp8_mqa_logits_on_the_gathered_operands(dga, h, nn):
    c = _chunk()
    n = 2 * c + 37
    lens = (c + 70, 1, n, 3 * KV, 2)
    max_blocks = (n + KV - 1) // KV
    q, buf, weights, tables, qc = _quantised(dga, h, nn, lens, n, max_blocks, (0, 2), 29 + h + nn)
    lens_a = np.asarray(lens, np.int32)
    out = _filled(len(lens) * nn, n)
    dga.fp8_paged_mqa_logits(q, _cache(buf), weights, _dev(lens_a), _dev(tables), None, n, True, out=out, sync=True)
    got = out.cpu().numpy()
    hi = R.row_ends(lens_a, nn, n, max_blocks)
    inside = np.arange(n)[None, :] < hi[:, None]
    assert np.array_equal(np.isneginf(got), ~inside) and not np.isnan(got).any()
    for i, ctx in enumerate(lens):
        rows = slice(i * nn, (i + 1) * nn)
        kg, sg, ok = R.gather(buf, tables[i], ctx)
        assert ok.all()
        ke = _dev(hi[rows].astype(np.int32))
        flat = dga.fp8_mqa_logits(q[i], (_dev(kg).view(torch.float8_e4m3fn), _dev(sg)), weights[rows], torch.zeros_like(ke), ke, sync=True)
        assert np.array_equal(_bits(got[rows, :ctx]), _bits(flat.cpu().numpy())), (i, ctx)
    want, mag = R.reference(qc, buf, weights.cpu().numpy(), lens_a, tables, n)
    err, bar = np.abs(got[inside].astype(np.float64) - want[inside]), (M.bound(h) * mag)[inside]
    print("H=%d next_n=%d: worst error / bound = %.4f, worst error / mag = 2^%.2f"
          % (h, nn, (err / bar).max(), np.log2((err / mag[inside]).max())))
    assert (err <= bar).all(), (int((err > bar).sum()), float((err / bar).max()))


@pytest.mark.parametrize("nn", (1, 2))
@pytest.mark.parametrize("h", M.HEADS)
@pytest.mark.parametrize("mirrored", (False, True), ids=("codes_in_k", "codes_in_q"))
def test_every_e4m3_code_gives_its_exact_value_and_fp8_mqa_logits_bits(dga, mirrored, h, nn):
    """mqa_logits_ref.all_codes_operands behind two tables that the even and the odd sequences share: the exact value of every code that
    is no NaN from either operand, and the bits of fp8_mqa_logits on the gathered operands"""
    q, buf, weights, lens, tables, n, want = R.all_codes_case(h, nn, mirrored)
    b = q.shape[0]
    assert len(np.unique(tables, axis=0)) == 2 and np.array_equal(tables[0], tables[2]) and len(np.unique(want[~np.isneginf(want)])) == 127
    hi = R.row_ends(lens, nn, n, tables.shape[1])
    assert np.array_equal(~np.isneginf(want), np.arange(n)[None, :] < hi[:, None]) and hi.min() == n - nn + 1
    got = _run(dga, q, buf, weights, lens, tables, n)
    _same_values(got, want)
    # both tables gather the same keys, so one prefill call holds every row
    kg, sg, ok = R.gather(buf, tables[0], n)
    kg1, sg1, ok1 = R.gather(buf, tables[1], n)
    assert ok.all() and ok1.all() and np.array_equal(kg, kg1) and np.array_equal(sg, sg1) and not np.array_equal(tables[0], tables[1])
    ke = _dev(hi.astype(np.int32))
    flat = dga.fp8_mqa_logits(_dev(q).view(b * nn, h, R.D).view(torch.float8_e4m3fn), (_dev(kg).view(torch.float8_e4m3fn), _dev(sg)),
                              _dev(weights), torch.zeros_like(ke), ke, sync=True)
    assert np.array_equal(_bits(got), _bits(flat.cpu().numpy()))


@pytest.mark.parametrize("h", M.HEADS)
def test_clean_logits_false_touches_nothing_beyond_the_last_page(dga, h):
    nn = 2
    lens, n, max_blocks, share = _big()
    q, buf, weights, lens_a, tables, want = R.exact_case(h, nn, lens, n, max_blocks, share)
    full = _run(dga, q, buf, weights, lens_a, tables, n)
    part = _run(dga, q, buf, weights, lens_a, tables, n, clean=False)
    w = R.written(lens_a, nn, n, max_blocks, clean=False)
    assert list(w.sum(axis=1)) == [0, 0, KV, KV, KV, KV, 2 * KV, 2 * KV, _chunk() + KV, _chunk() + KV, n, n]
    assert (_bits(part[~w]) == NAN_FILL).all()
    assert np.array_equal(_bits(part[w]), _bits(full[w]))
    tail = w & ~(np.arange(n)[None, :] < R.row_ends(lens_a, nn, n, max_blocks)[:, None])
    assert tail.sum() > 4 * KV and np.isneginf(part[tail]).all() and np.isneginf(want[tail]).all()


@pytest.mark.parametrize("clean", (True, False))
def test_a_padded_cache_gives_the_same_bits(dga, clean):
    h, nn = 64, 2
    lens, n, max_blocks, share = _big()
    q, buf, weights, lens_a, tables, _ = R.exact_case(h, nn, lens, n, max_blocks, share)
    dense = _run(dga, q, buf, weights, lens_a, tables, n, clean=clean)
    padded = _run(dga, q, buf, weights, lens_a, tables, n, clean=clean, padded=True)
    assert np.array_equal(_bits(dense), _bits(padded))
    flat = dga.fp8_paged_mqa_logits(_dev(q), _dev(buf), _dev(weights), _dev(lens_a), _dev(tables), max_model_len=n, clean_logits=clean,
                                    out=_filled(len(lens) * nn, n), sync=True)           # [num_blocks, 8448], uint8 q
    assert np.array_equal(_bits(dense), _bits(flat.cpu().numpy()))


# (the first two ids are those the test had before the cache took the negative NaN byte too)
@pytest.mark.parametrize("h,code", [(32, 0x7F), (64, 0x7F), (32, 0xFF), (64, 0xFF)], ids=("32", "64", "32-0xff", "64-0xff"))
def test_a_nan_code_poisons_its_column_in_both_sequences_and_its_row_only(dga, h, code):
    nn = 2
    lens, n, max_blocks, share = _big()
    q, buf, weights, lens_a, tables, want = R.exact_case(h, nn, lens, n, max_blocks, share)
    clean = _run(dga, q, buf, weights, lens_a, tables, n)
    inside = ~np.isneginf(want)
    q2, buf2 = q.copy(), buf.copy()
    shared, key = int(tables[3, 0]), 5
    assert code & 0x7F == M.NAN_CODE
    buf2[shared, key * R.D + 9] = code                                  # key 5 of the block sequences 3 and 4 both name as page 0
    q2[4, 1, h - 3, 77] = code ^ 0x80                                   # row 9: the NaN byte of the other sign
    got = _run(dga, q2, buf2, weights, lens_a, tables, n)
    poisoned = np.zeros_like(inside)
    poisoned[6:10, key], poisoned[9] = True, True
    poisoned &= inside
    assert poisoned.sum() == 3 + _chunk() + 1 and inside[6:10, key].all()
    assert np.isnan(got[poisoned]).all()
    assert np.array_equal(_bits(got[~poisoned]), _bits(clean[~poisoned]))
    assert np.isneginf(got[~inside]).all()


def test_a_captured_graph_follows_new_lengths_tables_operands_and_cache_bytes(dga):
    h, nn, c = 64, 2, _chunk()
    n = c + 100
    max_blocks = (n + KV - 1) // KV
    first = R.exact_case(h, nn, (n, 5, KV + 1, 0), n, max_blocks, (0, 2))
    second = R.exact_case(h, nn, (2 * KV, c + 3, 1, n - 7), n, max_blocks, (1, 3), seed=1)
    nb = max(first[1].shape[0], second[1].shape[0])
    cache = torch.zeros((nb, KV, 1, R.D + 4), dtype=torch.uint8, device="cuda")
    q, weights, lens, tables = (_dev(first[i]) for i in (0, 2, 3, 4))
    cache[:first[1].shape[0]].copy_(_dev(first[1]).view(-1, KV, 1, R.D + 4))
    out = _filled(4 * nn, n)
    call = lambda: dga.fp8_paged_mqa_logits(q.view(torch.float8_e4m3fn), cache, weights, lens, tables, None, n, True, out=out)
    call(); torch.cuda.synchronize()                       # eager once: the library is loaded
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    out.copy_(_filled(4 * nn, n))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    _same_values(out.cpu().numpy(), first[5])
    for dst, i in ((q, 0), (weights, 2), (lens, 3), (tables, 4)):
        dst.copy_(_dev(second[i]))
    cache.zero_()
    cache[:second[1].shape[0]].copy_(_dev(second[1]).view(-1, KV, 1, R.D + 4))
    out.copy_(_filled(4 * nn, n))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert not np.array_equal(np.isneginf(first[5]), np.isneginf(second[5]))
    _same_values(out.cpu().numpy(), second[5])


@pytest.mark.parametrize("h", M.HEADS)
def test_out_determinism_and_an_empty_batch(dga, h):
    nn, c = 2, _chunk()
    n = c + 100
    lens = (n, 77, c + 1)
    max_blocks = (n + KV - 1) // KV
    q, buf, weights, tables, _ = _quantised(dga, h, nn, lens, n, max_blocks, None, 5)
    cache, lens_d, tables_d = _cache(buf), _dev(np.asarray(lens, np.int32)), _dev(tables)
    a = dga.fp8_paged_mqa_logits(q, cache, weights, lens_d, tables_d, None, n, sync=True)
    b = dga.fp8_paged_mqa_logits(q.view(torch.uint8), cache, weights, lens_d, tables_d, max_model_len=n, sync=True)     # uint8 bytes are codes
    o = _filled(3 * nn, n)
    assert dga.fp8_paged_mqa_logits(q, cache, weights, lens_d, tables_d, None, n, out=o, sync=True) is o
    assert a.dtype == torch.float32 and a.shape == (3 * nn, n) and a.data_ptr() != b.data_ptr()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), o.view(torch.int32))
    assert torch.isfinite(a).any() and torch.isneginf(a).any() and not torch.isnan(a).any()
    empty = dga.fp8_paged_mqa_logits(q[:0], cache, weights[:0], lens_d[:0], tables_d[:0], None, n, sync=True)             # B == 0: no launch
    assert empty.shape == (0, n) and empty.dtype == torch.float32


def _slots(t, nb, seed):
    """int64 [t]: a scattered choice of distinct slots of nb blocks, with -1 and 64 nb (both skipped) where t allows"""
    rng = np.random.default_rng([seed, t, nb])
    slots = rng.permutation(nb * KV)[:t].astype(np.int64)
    if t >= 16:
        slots[3], slots[t - 2] = -1, nb * KV
    return slots


@pytest.mark.parametrize("t", (1, 16, 67, 300))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16, torch.float16), ids=("fp32", "bf16", "fp16"))
def test_the_writer_stores_the_quantisers_bytes_at_their_slots_and_nothing_else(dga, dtype, t):
    nb = (t + KV - 1) // KV + 3
    g = torch.Generator(device="cpu").manual_seed(100 + t)
    x = (torch.randn((t, R.D), generator=g) * torch.rand((t, 1), generator=g) * 8).to(dtype).cuda()
    slots = _slots(t, nb, 7)
    valid = (slots >= 0) & (slots < nb * KV)
    assert valid.sum() == (t if t < 16 else t - 2)
    fill = torch.randint(0, 256, (nb, BYTES + 64), generator=g, dtype=torch.uint8).cuda()
    for padded in (False, True):
        for ue8m0 in (False, True):
            qx, sf = dga.per_token_cast_to_fp8(x, use_ue8m0=ue8m0)
            want = fill.clone() if padded else fill[:, :BYTES].contiguous()
            wq, wsf = qx.view(torch.uint8).cpu().numpy(), sf.cpu().numpy().reshape(t)
            host = want.cpu().numpy()
            for i in np.flatnonzero(valid):
                blk, key = divmod(int(slots[i]), KV)
                host[blk, key * R.D:(key + 1) * R.D] = wq[i]
                host[blk, R.SCALES_AT + 4 * key:R.SCALES_AT + 4 * key + 4] = wsf[i:i + 1].view(np.uint8)
            buf = fill.clone() if padded else fill[:, :BYTES].contiguous()
            cache = buf[:, :BYTES] if padded else buf.view(nb, KV, 1, R.D + 4)
            got = dga.per_token_cast_to_fp8_paged(x, cache, _dev(slots), use_ue8m0=ue8m0, sync=True)
            assert got is cache
            assert np.array_equal(buf.cpu().numpy(), host), (padded, ue8m0)
            if ue8m0:
                mant, _ = np.frexp(wsf)
                assert (mant == 0.5).all()


def test_the_writer_gives_the_quantisers_codes_on_nan_and_infinite_input(dga):
    t, nb = 20, 2
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn((t, R.D), generator=g)
    x[2, 5], x[2, 100], x[7, 0], x[9, 64], x[11] = float("nan"), -float("nan"), float("inf"), -float("inf"), 0.0
    x[13, 3] = float("nan")
    x[13, 4] = float("inf")
    x = x.cuda()
    slots = np.random.default_rng(1).permutation(nb * KV)[:t].astype(np.int64)
    qx, sf = dga.per_token_cast_to_fp8(x)
    wq, wsf = qx.view(torch.uint8).cpu().numpy(), sf.cpu().numpy().reshape(t)
    assert (wq[2] & 0x7F == 0x7F).sum() == 2 and np.isinf(wsf[7]) and wsf[11] == 1.0
    cache = torch.full((nb, KV, 1, R.D + 4), 0x5A, dtype=torch.uint8, device="cuda")
    dga.per_token_cast_to_fp8_paged(x, cache, _dev(slots), sync=True)
    codes, scales = R.unpack(cache.view(nb, BYTES).cpu().numpy())
    codes, scales = codes.reshape(nb * KV, R.D), scales.reshape(nb * KV)
    assert np.array_equal(codes[slots], wq) and np.array_equal(scales[slots].view(np.uint32), wsf.view(np.uint32))
    rest = np.setdiff1d(np.arange(nb * KV), slots)
    assert (codes[rest] == 0x5A).all() and (scales[rest].view(np.uint8) == 0x5A).all()


def test_one_graph_writes_the_new_keys_and_scores_them(dga):
    """A decode layer: each step appends next_n keys per sequence to the cache and scores the next_n newest tokens.  Sequence 0 crosses a
    page boundary inside the first step, sequence 1 between the steps."""
    h, nn, b, n, max_blocks = 64, 2, 3, 3 * KV, 3
    start, steps = (KV - 1, 2 * KV - 2, 5), 2
    g = torch.Generator(device="cpu").manual_seed(41)
    hist = [torch.randn((start[i] + steps * nn, R.D), generator=g).to(torch.bfloat16).cuda() for i in range(b)]
    tables, nb = R.make_tables(tuple(s + steps * nn for s in start), n, max_blocks, 9)
    tables_d = _dev(tables)
    cache = torch.full((nb, KV, 1, R.D + 4), 0x5A, dtype=torch.uint8, device="cuda")

    def slots_of(i, lo, hi):
        pos = np.arange(lo, hi)
        return tables[i, pos // KV].astype(np.int64) * KV + pos % KV

    # the history so far, through the writer (eager)
    for i in range(b):
        dga.per_token_cast_to_fp8_paged(hist[i][:start[i]], cache, _dev(slots_of(i, 0, start[i])), sync=True)
    qs = [dga.per_token_cast_to_fp8(torch.randn((b * nn * h, R.D), generator=g).cuda())[0].view(b, nn, h, R.D) for _ in range(steps)]
    ws = [torch.randn((b * nn, h), generator=g).cuda() for _ in range(steps)]

    def step_inputs(s):
        lo = [start[i] + s * nn for i in range(b)]
        x = torch.cat([hist[i][lo[i]:lo[i] + nn] for i in range(b)])
        slots = np.concatenate([slots_of(i, lo[i], lo[i] + nn) for i in range(b)])
        return x, _dev(slots), _dev(np.asarray([v + nn for v in lo], np.int32))

    x, slots, lens = step_inputs(0)
    q, weights = qs[0].clone(), ws[0].clone()
    out = _filled(b * nn, n)

    def layer():
        dga.per_token_cast_to_fp8_paged(x, cache, slots)
        dga.fp8_paged_mqa_logits(q, cache, weights, lens, tables_d, None, n, True, out=out)

    before = cache.clone()
    layer(); torch.cuda.synchronize()                      # eager once: the library is loaded
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        layer()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        layer()
    cache.copy_(before)                                    # the step's keys are written by the replay
    for s in range(steps):
        if s:
            nx, nslots, nlens = step_inputs(s)
            x.copy_(nx); slots.copy_(nslots); lens.copy_(nlens); q.copy_(qs[s]); weights.copy_(ws[s])
        out.copy_(_filled(b * nn, n))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for i in range(b):
            ctx = start[i] + (s + 1) * nn
            rows = slice(i * nn, (i + 1) * nn)
            k, sfk = dga.per_token_cast_to_fp8(hist[i][:ctx])
            ke = _dev(np.asarray([ctx - nn + j + 1 for j in range(nn)], np.int32))
            flat = dga.fp8_mqa_logits(qs[s][i], (k, sfk.reshape(ctx).contiguous()), ws[s][rows], torch.zeros_like(ke), ke, sync=True)
            assert np.array_equal(_bits(got[rows, :ctx]), _bits(flat.cpu().numpy())), (s, i)
            assert np.isneginf(got[rows, ctx:]).all() and np.isfinite(got[i * nn + nn - 1, :ctx]).all()
