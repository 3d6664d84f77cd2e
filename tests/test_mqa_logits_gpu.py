"""GPU: fp8_mqa_logits against tests/mqa_logits_ref.py.  BM = 64 tokens and BN = 256 keys are the kernel's token run and key block.
Exactly summable operands must give the float64 reference as values (a zero of either sign is zero, -inf where the reference has it) at
H = 32 and 64, on a shape of more than one run and block with ragged ends and on shapes below one tile, under every kind of range, into an
output pre-filled with a NaN pattern; amax-quantised random operands must stay inside the derived bound on every in-range element; every
code that is no NaN gives its exact value from either operand; a NaN code of either sign poisons its row or column inside the ranges and
nothing else; a captured graph follows rewritten operands and ranges; two calls give the same bits and out= matches the allocating
call."""
import numpy as np
import pytest
import torch

import mqa_logits_ref as R

pytestmark = pytest.mark.gpu

BIG = (R.BM + 3, 2 * R.BN + 37)
NAN_FILL = 0x7FC12345


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared references are read-only)


def _filled(m, n):
    """float32 [m, n] full of a NaN pattern no result takes"""
    return torch.full((m, n), NAN_FILL, dtype=torch.int32, device="cuda").view(torch.float32)


def _run(dga, q, k, kscale, weights, ks, ke, out=None):
    m, n = q.shape[0], k.shape[0]
    out = _filled(m, n) if out is None else out
    got = dga.fp8_mqa_logits(_dev(q).view(torch.float8_e4m3fn), (_dev(k).view(torch.float8_e4m3fn), _dev(kscale)), _dev(weights), _dev(ks),
                             _dev(ke), out=out, sync=True)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy()


_same_values = R.assert_same_values                                  # (tests/mqa_logits_ref.py; tests/test_mqa_logits.py tests it)


@pytest.mark.parametrize("h", R.HEADS)
@pytest.mark.parametrize("m,n", (BIG, (1, 1), (5, 15)), ids=("runs_blocks", "1x1", "5x15"))
def test_bit_for_bit_on_exactly_summable_data(dga, m, n, h):
    q, k, kscale, weights, ks, ke, want = R.exact_case(m, n, h)
    assert np.isfinite(want).all() and len(np.unique(want)) > min(m * n, 3) // 2
    _same_values(_run(dga, q, k, kscale, weights, ks, ke), want)


@pytest.mark.parametrize("h", R.HEADS)
@pytest.mark.parametrize("kind", R.RANGE_KINDS)
def test_ranges(dga, kind, h):
    m, n = BIG
    q, k, kscale, weights, ks, ke, want = R.exact_case(m, n, h, kind)
    inside = R.in_range(ks, ke, n)
    if kind == "empty":
        assert not inside.any()
    elif kind in ("full", "beyond"):
        assert inside.all()
    elif kind == "mixed":        # in the first run, every key block has rows that exclude it wholly and rows that include it
        for b in range(3):
            touched = inside[:R.BM, b * R.BN:(b + 1) * R.BN].any(axis=1)
            assert touched.any() and not touched.all(), b
    else:
        assert inside.any() and not inside.all()
    _same_values(_run(dga, q, k, kscale, weights, ks, ke), want)


@pytest.mark.parametrize("h", R.HEADS)
def test_derived_bound_on_quantised_random_data(dga, h):
    m, n = 2 * R.BM + 1, R.BN + 100
    g = torch.Generator(device="cpu").manual_seed(17 + h)
    xq = torch.randn((m * h, R.D), generator=g).cuda()
    xk = torch.randn((n, R.D), generator=g).cuda()
    weights = torch.randn((m, h), generator=g).cuda()
    q, _ = dga.per_token_cast_to_fp8(xq)                  # q carries no scale: the caller would fold it into weights
    k, sfk = dga.per_token_cast_to_fp8(xk)
    kscale = sfk.reshape(n).contiguous()
    i = np.arange(m)
    ks, ke = ((i * 7) % 50).astype(np.int32), (n - (i * 5) % 90).astype(np.int32)
    qc, kc = q.view(torch.uint8).cpu().numpy().reshape(m, h, R.D), k.view(torch.uint8).cpu().numpy()
    assert int((qc & 0x7F).max()) == 0x7E and int((kc & 0x7F).max()) == 0x7E           # codes up to 448
    out = _filled(m, n)
    dga.fp8_mqa_logits(q.view(m, h, R.D), (k, kscale), weights, _dev(ks), _dev(ke), out=out, sync=True)
    got = out.cpu().numpy()
    want, mag = R.reference(qc, kc, kscale.cpu().numpy(), weights.cpu().numpy(), ks, ke)
    inside = R.in_range(ks, ke, n)
    assert np.array_equal(np.isneginf(got), ~inside) and not np.isnan(got).any()
    err, bar = np.abs(got[inside].astype(np.float64) - want[inside]), (R.bound(h) * mag)[inside]
    print("H=%d: worst error / bound = %.4f, worst error / mag = 2^%.2f" % (h, (err / bar).max(), np.log2((err / mag[inside]).max())))
    assert (err <= bar).all(), (int((err > bar).sum()), float((err / bar).max()))


@pytest.mark.parametrize("h", R.HEADS)
@pytest.mark.parametrize("mirrored", (False, True), ids=("codes_in_k", "codes_in_q"))
def test_every_e4m3_code_gives_its_exact_value(dga, mirrored, h):
    """All 254 codes that are no NaN -- the subnormals and -0 among them -- opposite a unit code, in every dimension: a logit is relu of
    the code's value or of its negative, exactly, down to 2^-9"""
    q, k, kscale, weights, ks, ke, want = R.all_codes_case(h, mirrored)
    assert len(R.all_codes_seen(h, mirrored)) == 254 and len(np.unique(want)) == 127
    _same_values(_run(dga, q, k, kscale, weights, ks, ke), want)


# (the first two ids are those the test had before the negative NaN byte joined it)
@pytest.mark.parametrize("h,code", [(32, 0x7F), (64, 0x7F), (32, 0xFF), (64, 0xFF)], ids=("32", "64", "32-0xff", "64-0xff"))
def test_a_nan_code_poisons_its_row_and_its_column_only(dga, h, code):
    m, n = BIG
    q, k, kscale, weights, ks, ke, _ = R.exact_case(m, n, h, "windows")
    clean = _run(dga, q, k, kscale, weights, ks, ke)
    inside = R.in_range(ks, ke, n)
    row = int(np.flatnonzero(inside.sum(axis=1) > 40)[3])
    col = int(np.flatnonzero(inside.sum(axis=0) > 2)[-1])
    q2, k2 = q.copy(), k.copy()
    assert code & 0x7F == R.NAN_CODE
    q2[row, h - 3, 77], k2[col, 5] = code, code
    got = _run(dga, q2, k2, kscale, weights, ks, ke)
    poisoned = np.zeros_like(inside)
    poisoned[row], poisoned[:, col] = True, True
    poisoned &= inside
    assert poisoned.sum() > 42
    assert np.isnan(got[poisoned]).all()
    assert np.array_equal(got[~poisoned].view(np.uint32), clean[~poisoned].view(np.uint32))
    assert np.isneginf(got[~inside]).all()


def test_a_captured_graph_follows_new_operands_and_ranges(dga):
    m, n, h = BIG[0], BIG[1], 64
    first = R.exact_case(m, n, h, "causal")
    second = R.exact_case(m, n, h, "mixed", seed=1)
    q, k, kscale, weights, ks, ke = (_dev(a) for a in first[:6])
    q, k = q.view(torch.float8_e4m3fn), k.view(torch.float8_e4m3fn)
    out = _filled(m, n)
    call = lambda: dga.fp8_mqa_logits(q, (k, kscale), weights, ks, ke, out=out)
    call(); torch.cuda.synchronize()                       # eager once: the library is loaded
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    out.copy_(_filled(m, n))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    _same_values(out.cpu().numpy(), first[6])
    for dst, src in zip((q.view(torch.uint8), k.view(torch.uint8), kscale, weights, ks, ke), second[:6]):
        dst.copy_(_dev(src))
    out.copy_(_filled(m, n))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert not np.array_equal(first[6], second[6])
    _same_values(out.cpu().numpy(), second[6])


@pytest.mark.parametrize("h", R.HEADS)
def test_out_and_determinism(dga, h):
    m, n = 2 * R.BM + 1, R.BN + 100
    g = torch.Generator(device="cpu").manual_seed(5)
    q = torch.randint(0, 256, (m, h, R.D), generator=g, dtype=torch.uint8)
    k = torch.randint(0, 256, (n, R.D), generator=g, dtype=torch.uint8)
    q[(q & 0x7F) == 0x7F] = 0x11
    k[(k & 0x7F) == 0x7F] = 0x11
    q, k = q.cuda(), k.cuda()
    kscale = torch.rand(n, generator=g).cuda() + 0.5
    weights = torch.randn((m, h), generator=g).cuda()
    ks, ke = R.ranges("windows", m, n)
    ks, ke = _dev(ks), _dev(ke)
    a = dga.fp8_mqa_logits(q, (k, kscale), weights, ks, ke, sync=True)                 # uint8 bytes are taken as codes
    b = dga.fp8_mqa_logits(q.view(torch.float8_e4m3fn), (k.view(torch.float8_e4m3fn), kscale), weights, ks, ke, sync=True)
    c = _filled(m, n)
    assert dga.fp8_mqa_logits(q, (k, kscale), weights, ks, ke, out=c, sync=True) is c
    assert a.dtype == torch.float32 and a.shape == (m, n) and a.data_ptr() != b.data_ptr()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert torch.isfinite(a).any() and torch.isneginf(a).any() and not torch.isnan(a).any()
    empty = dga.fp8_mqa_logits(q[:0], (k, kscale), weights[:0], ks[:0], ke[:0], sync=True)      # M == 0: no launch
    assert empty.shape == (0, n) and empty.dtype == torch.float32
